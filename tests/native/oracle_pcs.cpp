// Test shim over the CPU oracle (oracle/*.h, the checker): prove and verify under an explicit PcsConfig. The oracle's own C ABI
// (oracle/oracle_capi.cpp) fixes PcsConfig::default(); tests/test_pcs_config_cpu.py and tests/test_gpu_pcs_config.py build this file with g++
// into a temporary directory (next to oracle/simd_port.cpp, which the headers call into) and load it with ctypes.
// The oracle's commitment, sampling, quotient, FRI, proof-of-work and decommitment code is generic in the config. Its compute_composition
// evaluates the constraints on CanonicCoset(log_size + 1): at log_blowup_factor 1 that is the committed LDE, above it the columns are evaluated
// there from the committed polynomials (oracle/prover.h). Whole proofs are the byte-exact reference at every log_blowup_factor.
#include "json.h"
#include <cstdio>

using namespace orc;

static thread_local std::string g_err;

static PcsConfig make_cfg(u32 pow_bits, u32 log_blowup, u32 n_queries) {
    PcsConfig cfg; cfg.pow_bits = pow_bits; cfg.log_blowup = log_blowup; cfg.n_queries = n_queries; cfg.log_last_layer_degree_bound = 0;
    return cfg;
}

extern "C" {

const char* ops_last_error() { return g_err.c_str(); }
void ops_free(void* p) { free(p); }

// this library's copy of the process-wide conventions (same numbering as include/bfhip.h `bfhip_conventions`)
int ops_set_conventions(u32 merkle_node_hash, u32 mix_u64, u32 logup_mask_order, u32 merkle_channel) {
    if (merkle_node_hash > 1 || mix_u64 > 1 || logup_mask_order > 1 || merkle_channel > 1) { g_err = "bad convention value"; return -1; }
    conventions().merkle_node_hash = merkle_node_hash; conventions().mix_u64 = mix_u64; conventions().logup_mask_order = logup_mask_order;
    conventions().merkle_channel = merkle_channel;
    return 0;
}

// The proof (malloc'd JSON) and the transcript taps ("name:hexdigest\n" per tap, malloc'd; optional) under the given config. A proof that
// fails still returns the taps it reached.
int ops_prove(const char* code, const u8* input, size_t n_in, u32 log_max_rows, u32 pow_bits, u32 log_blowup, u32 n_queries,
              char** json_out, size_t* json_len, char** transcript_out) {
    std::string transcript;
    auto give_transcript = [&] {
        if (transcript_out) { *transcript_out = (char*)malloc(transcript.size() + 1); memcpy(*transcript_out, transcript.c_str(), transcript.size() + 1); }
    };
    try {
        std::vector<u32> ins = compile(code);
        Machine m(ins, std::vector<u8>(input, input + n_in));
        m.execute();
        Prover pv; pv.log_max_rows = log_max_rows; pv.cfg = make_cfg(pow_bits, log_blowup, n_queries);
        pv.trace_hook = [&](const char* name, const Channel& ch) {
            char buf[4]; transcript += name; transcript += ":";
            for (int i = 0; i < 32; i++) { snprintf(buf, sizeof buf, "%02x", ch.digest.b[i]); transcript += buf; }
            transcript += "\n";
        };
        BrainfuckProof bp = pv.prove(m.trace, ins);
        std::string js = proof_to_json(bp);
        *json_out = (char*)malloc(js.size() + 1); memcpy(*json_out, js.c_str(), js.size() + 1); *json_len = js.size();
        give_transcript();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); give_transcript(); return -1; } catch (...) { g_err = "unknown"; give_transcript(); return -1; }
}

// 0 = verified; 1 = rejected (reason in err); -1 = internal error
int ops_verify(const char* json, size_t len, u32 log_max_rows, u32 pow_bits, u32 log_blowup, u32 n_queries, char* err, size_t errcap) {
    try {
        BrainfuckProof bp;
        try { bp = proof_from_json(json, len); } catch (const std::exception& e) { if (err) snprintf(err, errcap, "InvalidStructure: %s", e.what()); return 1; }
        Verifier v; v.log_max_rows = log_max_rows; v.cfg = make_cfg(pow_bits, log_blowup, n_queries);
        std::string e = v.verify(bp);
        if (err) snprintf(err, errcap, "%s", e.c_str());
        return e.empty() ? 0 : 1;
    } catch (const std::exception& e) { g_err = e.what(); return -1; } catch (...) { g_err = "unknown"; return -1; }
}

}  // extern "C"
