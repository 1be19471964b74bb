// Test shim over the CPU oracle (oracle/*.h, the checker): its commitment scheme over ARBITRARY columns. oracle/prover.h has the generic half
// of stwo's CommitmentSchemeProver already — interpolate_col, commit_tree and Prover::prove_values take any trees and any points; only
// Prover::prove knows Brainfuck. This file is the C entry to them and restates nothing of the protocol: a channel, a session that commits
// trees and calls Prover::prove_values under the description bfhip_pcs_prove_values takes (points, a sample count per column, point indices in
// sample order), and the serde bytes of the commitment-scheme proof alone. Those bytes are cut out of oracle/json.h's proof_to_json — the
// "proof" member of a BrainfuckProof with an empty claim, as tests/pcs_replay.py proof_member cuts it out of a real one — so the field order
// is json.h's and nobody else's.
// tests/oracle_pcs_generic.py builds this file with g++ into a temporary directory (next to oracle/simd_port.cpp) and loads it with ctypes;
// tests/native/oracle_pcs_generic_sanitize.cpp includes it into a stand-alone program for AddressSanitizer + UBSan.
#include "json.h"
#include <cstdio>
#ifdef _OPENMP
#include <omp.h>
#endif

using namespace orc;

static thread_local std::string g_opg_err;

namespace {

struct OpgSession {
    Prover pv;
    TwiddleTree tw;
    std::vector<CommitmentTree> trees;
    bool proved = false;
};

QM31 opg_q(const u32* w) { return QM31::from_u32(w[0], w[1], w[2], w[3]); }
void opg_words(const QM31& q, u32* out) { auto a = q.to_u32(); for (int k = 0; k < 4; k++) out[k] = a[k]; }
void opg_canonical(const u32* w, size_t n, const char* what) { for (size_t i = 0; i < n; i++) if (w[i] >= P) throw std::runtime_error(std::string(what) + ": a word is not below P"); }

}  // namespace

#define OPG_TRY try {
#define OPG_CATCH } catch (const std::exception& e) { g_opg_err = e.what(); return -1; } catch (...) { g_opg_err = "unknown"; return -1; }

extern "C" {

const char* opg_last_error() { return g_opg_err.c_str(); }
void opg_free(void* p) { free(p); }

// this library's copy of the process-wide conventions (same numbering as include/bfhip.h `bfhip_conventions`); a channel takes its kind
// (Blake2s / Poseidon252) from them when it is created
int opg_set_conventions(u32 merkle_node_hash, u32 mix_u64, u32 logup_mask_order, u32 merkle_channel) {
    if (merkle_node_hash > 1 || mix_u64 > 1 || logup_mask_order > 1 || merkle_channel > 1) { g_opg_err = "bad convention value"; return -1; }
    conventions().merkle_node_hash = merkle_node_hash; conventions().mix_u64 = mix_u64; conventions().logup_mask_order = logup_mask_order;
    conventions().merkle_channel = merkle_channel;
    return 0;
}

void opg_set_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

// ---- channel ------------------------------------------------------------------------------------------------------------------------------
void* opg_channel_new() { return new Channel(); }
void opg_channel_free(void* c) { delete (Channel*)c; }
int opg_channel_mix_root(void* c, const u8 root[32]) { OPG_TRY Hash32 h; memcpy(h.b, root, 32); ((Channel*)c)->mix_root(h); return 0; OPG_CATCH }
int opg_channel_mix_u64(void* c, u64 v) { OPG_TRY ((Channel*)c)->mix_u64(v); return 0; OPG_CATCH }
int opg_channel_mix_felts(void* c, const u32* words, size_t n) {
    OPG_TRY
    opg_canonical(words, 4 * n, "mix_felts");
    std::vector<QM31> v; for (size_t i = 0; i < n; i++) v.push_back(opg_q(words + 4 * i));
    ((Channel*)c)->mix_felts(v.data(), n);
    return 0;
    OPG_CATCH
}
int opg_channel_draw_felts(void* c, size_t n, u32* out) {
    OPG_TRY
    std::vector<QM31> v = ((Channel*)c)->draw_felts(n);
    for (size_t i = 0; i < n; i++) opg_words(v[i], out + 4 * i);
    return 0;
    OPG_CATCH
}
int opg_channel_draw_point(void* c, u32 out[8]) {
    OPG_TRY
    PointQ p = Prover::get_random_point(*(Channel*)c);
    opg_words(p.x, out); opg_words(p.y, out + 4);
    return 0;
    OPG_CATCH
}
void opg_channel_state(void* c, u8 digest[32], u32* n_sent) { memcpy(digest, ((Channel*)c)->digest.b, 32); if (n_sent) *n_sent = ((Channel*)c)->n_sent; }

// ---- session ------------------------------------------------------------------------------------------------------------------------------
// max_log_size: the largest trace-domain log size any tree of this session will hold (sizes the twiddle tree, as Prover::prove sizes its own:
// one level above the largest committed domain).
void* opg_session_new(u32 pow_bits, u32 log_blowup, u32 n_queries, u32 max_log_size) {
    try {
        if (log_blowup < 1 || max_log_size + log_blowup + 1 > 30) throw std::runtime_error("session: domain outside the circle group");
        auto* s = new OpgSession();
        s->pv.cfg.pow_bits = pow_bits; s->pv.cfg.log_blowup = log_blowup; s->pv.cfg.n_queries = n_queries; s->pv.cfg.log_last_layer_degree_bound = 0;
        s->pv.log_max_rows = max_log_size;
        s->tw = precompute_twiddles(CanonicCoset{max_log_size + log_blowup + 1}.circle_domain().half_coset);
        return s;
    } catch (const std::exception& e) { g_opg_err = e.what(); return nullptr; } catch (...) { g_opg_err = "unknown"; return nullptr; }
}
void opg_session_free(void* s) { delete (OpgSession*)s; }

// One tree: column k has 2^log_sizes[k] words, evaluations on the bit-reversed circle domain (form 0, interpolate_col) or coefficients
// (form 1). commit_tree extends, hashes and mixes the root into the channel.
int opg_session_commit(void* sv, void* c, const u32* const* cols, const u32* log_sizes, u32 n_cols, int form, u8 root_out[32]) {
    OPG_TRY
    auto* s = (OpgSession*)sv;
    if (s->proved) throw std::runtime_error("commit: prove_values was already called");
    if (form != 0 && form != 1) throw std::runtime_error("commit: form must be 0 or 1");
    if (n_cols == 0) throw std::runtime_error("commit: a tree has at least one column");
    CommitmentTree t;
    t.polys.resize(n_cols);
    for (u32 k = 0; k < n_cols; k++) {
        if (log_sizes[k] < 1 || log_sizes[k] > s->pv.log_max_rows) throw std::runtime_error("commit: log size outside the session's range");
        opg_canonical(cols[k], size_t(1) << log_sizes[k], "commit");
    }
#pragma omp parallel for schedule(dynamic)
    for (u32 k = 0; k < n_cols; k++) {
        std::vector<u32> v(cols[k], cols[k] + (size_t(1) << log_sizes[k]));
        if (form == 0) t.polys[k] = interpolate_col(v, log_sizes[k], s->tw);
        else t.polys[k] = PolyCol{log_sizes[k], std::move(v)};
    }
    s->trees.push_back(std::move(t));
    commit_tree(s->trees.back(), s->pv.cfg, s->tw, *(Channel*)c);
    memcpy(root_out, s->trees.back().merkle.root().b, 32);
    return 0;
    OPG_CATCH
}

// points: n_points x 8 words (x then y). n_samples: one count per column over all trees in commit order. point_idx: the indices flat, in
// sample order. sampled_out (optional): 4 words per sample, in that order. proof_json: malloc'd, the CommitmentSchemeProof's serde bytes.
int opg_session_prove_values(void* sv, void* c, const u32* points, u32 n_points, const u32* n_samples, const u32* point_idx, u32* sampled_out,
                             char** proof_json, size_t* proof_len) {
    OPG_TRY
    auto* s = (OpgSession*)sv;
    if (s->proved) throw std::runtime_error("prove_values: already called");
    if (s->trees.empty()) throw std::runtime_error("prove_values: nothing was committed");
    opg_canonical(points, 8 * size_t(n_points), "prove_values: point");
    std::vector<PointQ> pts;
    for (u32 p = 0; p < n_points; p++) pts.push_back(PointQ(opg_q(points + 8 * p), opg_q(points + 8 * p + 4)));
    std::vector<std::vector<std::vector<PointQ>>> sample_points(s->trees.size());
    size_t col = 0, at = 0;
    for (size_t t = 0; t < s->trees.size(); t++) {
        sample_points[t].resize(s->trees[t].polys.size());
        for (size_t k = 0; k < s->trees[t].polys.size(); k++, col++)
            for (u32 j = 0; j < n_samples[col]; j++) {
                const u32 i = point_idx[at++];
                if (i >= n_points) throw std::runtime_error("prove_values: point index out of range");
                sample_points[t][k].push_back(pts[i]);
            }
    }
    s->proved = true;
    BrainfuckProof bp;
    for (int k = 0; k < N_COMPONENTS; k++) { bp.log_sizes[k] = 0; bp.claimed_sums[k] = QM31::zero(); }
    bp.proof = s->pv.prove_values(s->trees, sample_points, *(Channel*)c, s->tw);
    if (sampled_out) { size_t i = 0; for (auto& t : bp.proof.sampled_values) for (auto& cv : t) for (auto& v : cv) opg_words(v, sampled_out + 4 * i++); }
    const std::string js = proof_to_json(bp);
    const char key[] = "\"proof\":";
    const size_t from = js.find(key);
    if (from == std::string::npos || js.back() != '}') throw std::runtime_error("prove_values: no proof member");
    const std::string member = js.substr(from + sizeof key - 1, js.size() - 1 - (from + sizeof key - 1));
    *proof_json = (char*)malloc(member.size() + 1);
    if (!*proof_json) throw std::runtime_error("out of memory");
    memcpy(*proof_json, member.c_str(), member.size() + 1);
    *proof_len = member.size();
    return 0;
    OPG_CATCH
}

}  // extern "C"
