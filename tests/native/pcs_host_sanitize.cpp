// CPU sanitizer harness for the host-only half of the commitment-scheme session (stwo-brainfuck_amd/csrc/pcs_host.hip: bfhip_channel_*,
// bfhip_circle_point_offset, bfhip_brainfuck_composition_at_point, bfhip_pcs_verifier_*). tests/test_pcs_session_cpu.py compiles this
// file TOGETHER with pcs_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program
// directly. It replays verify_brainfuck through the C ABI only — the protocol of tests/pcs_replay.py — over a proof file:
//   pcs_host_sanitize <proof.json> <log_max_rows> <node_hash> <mix_u64> <mask_order> <channel> <pow_bits> <log_blowup> <n_queries>
// prints "ok" or the rejection reason, then a line of edge calls (null and non-canonical arguments) that must all be refused.
// The proof's claim and commitments are read with the product's own JSON reader (host/verifier.h), which is under the sanitizers with it.
#include "../../include/bfhip.h"
#include "../../stwo-brainfuck_amd/csrc/host/verifier.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

// what api_ctx.hip provides inside the library
static std::string g_error;
void bfhip_set_error(const std::string& s) { g_error = s; }

using namespace bf;

static void words(const Q31& q, uint32_t* o) { o[0] = q.a.a; o[1] = q.a.b; o[2] = q.b.a; o[3] = q.b.b; }
#define MUST(call) do { if ((call) != 0) { printf("internal: %s: %s\n", #call, g_error.c_str()); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc != 10) { fprintf(stderr, "usage: see the source header\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::stringstream ss; ss << in.rdbuf();
    const std::string raw = ss.str();
    const uint32_t lmr = (uint32_t)atoi(argv[2]);
    bfhip_conventions cv{}; cv.merkle_node_hash = atoi(argv[3]); cv.mix_u64 = atoi(argv[4]); cv.logup_mask_order = atoi(argv[5]); cv.merkle_channel = atoi(argv[6]);
    bfhip_pcs_config pc{}; pc.pow_bits = atoi(argv[7]); pc.log_blowup_factor = atoi(argv[8]); pc.n_queries = atoi(argv[9]);
    BrainfuckProof bp;
    try { bp = proof_from_json(raw.data(), raw.size(), cv.merkle_channel == 1); } catch (const std::exception& e) { printf("InvalidStructure: %s\n", e.what()); return 0; }
    const StarkProof& pf = bp.proof;
    std::string reason;
    bfhip_channel* ch = nullptr; bfhip_pcs_verifier* v = nullptr;
    MUST(bfhip_channel_create(&cv, &ch));
    MUST(bfhip_pcs_verifier_create(&cv, &pc, &v));
    auto replay = [&]() -> int {
        if (pf.commitments.size() != 4 || pf.sampled_values.size() != 4 || pf.decommitments.size() != 4 || pf.queried_values.size() != 4) { reason = "InvalidStructure"; return 0; }
        for (int k = 0; k < N_COMPONENTS; k++) if (bp.log_sizes[k] < LOG_N_LANES || bp.log_sizes[k] > lmr) { reason = "InvalidStructure: log_size"; return 0; }
        std::vector<uint32_t> logs[4];
        uint32_t top = 0;
        for (uint32_t l = lmr; l >= LOG_N_LANES; l--) logs[0].push_back(l);
        for (int k = 0; k < N_COMPONENTS; k++) {
            for (u32 j = 0; j < n_main_cols(k); j++) logs[1].push_back(bp.log_sizes[k]);
            for (u32 j = 0; j < 4 * n_logup_cols(k); j++) logs[2].push_back(bp.log_sizes[k]);
            top = std::max(top, bp.log_sizes[k] + 1);
        }
        logs[3].assign(4, top);
        MUST(bfhip_pcs_verifier_commit(v, ch, pf.commitments[0].b, logs[0].data(), (uint32_t)logs[0].size()));
        for (int k = 0; k < N_COMPONENTS; k++) MUST(bfhip_channel_mix_u64(ch, bp.log_sizes[k]));
        MUST(bfhip_pcs_verifier_commit(v, ch, pf.commitments[1].b, logs[1].data(), (uint32_t)logs[1].size()));
        uint32_t lookup[24];
        for (int k = 0; k < 3; k++) MUST(bfhip_channel_draw_felts(ch, 2, lookup + 8 * k));
        Q31 total = q_zero();
        std::vector<uint32_t> claimed(4 * N_COMPONENTS);
        for (int k = 0; k < N_COMPONENTS; k++) { total = q_add(total, bp.claimed_sums[k]); words(bp.claimed_sums[k], claimed.data() + 4 * k); }
        if (!q_is_zero(total)) { reason = "InvalidLookup: Invalid LogUp sum"; return 0; }
        for (int k = 0; k < N_COMPONENTS; k++) MUST(bfhip_channel_mix_felts(ch, claimed.data() + 4 * k, 1));
        MUST(bfhip_pcs_verifier_commit(v, ch, pf.commitments[2].b, logs[2].data(), (uint32_t)logs[2].size()));
        uint32_t coeff[4], points[8 * (1 + N_COMPONENTS)];
        MUST(bfhip_channel_draw_felts(ch, 1, coeff));
        MUST(bfhip_pcs_verifier_commit(v, ch, pf.commitments[3].b, logs[3].data(), (uint32_t)logs[3].size()));
        MUST(bfhip_channel_draw_point(ch, points));
        for (int k = 0; k < N_COMPONENTS; k++) MUST(bfhip_circle_point_offset(points, bp.log_sizes[k], -1, points + 8 * (1 + k)));
        // the mask: n_samples per column and the point indices, flat over the four trees
        std::vector<std::vector<uint32_t>> mask[4];
        mask[0].assign(logs[0].size(), {});
        for (int k = 0; k < N_COMPONENTS; k++) mask[0][lmr - bp.log_sizes[k]] = {0};
        for (int k = 0; k < N_COMPONENTS; k++) {
            for (u32 j = 0; j < n_main_cols(k); j++) mask[1].push_back({0});
            const u32 ni = 4 * n_logup_cols(k);
            for (u32 j = 0; j < ni; j++) {
                if (j + 4 >= ni) { if (cv.logup_mask_order == 1) mask[2].push_back({(uint32_t)(1 + k), 0}); else mask[2].push_back({0, (uint32_t)(1 + k)}); }
                else mask[2].push_back({0});
            }
        }
        mask[3].assign(4, {0});
        std::vector<uint32_t> counts, idx, n3, sampled3;
        uint32_t n_cols3[3];
        for (int t = 0; t < 4; t++) {
            if (pf.sampled_values[t].size() != mask[t].size()) { reason = "InvalidStructure: sampled_values"; return 0; }
            for (size_t c = 0; c < mask[t].size(); c++) {
                if (pf.sampled_values[t][c].size() != mask[t][c].size()) { reason = "InvalidStructure: sampled_values"; return 0; }
                counts.push_back((uint32_t)mask[t][c].size());
                for (uint32_t i : mask[t][c]) idx.push_back(i);
                if (t < 3) { n3.push_back((uint32_t)mask[t][c].size()); for (const Q31& q : pf.sampled_values[t][c]) { uint32_t w[4]; words(q, w); sampled3.insert(sampled3.end(), w, w + 4); } }
            }
            if (t < 3) n_cols3[t] = (uint32_t)mask[t].size();
        }
        uint32_t want[4], got[4];
        MUST(bfhip_brainfuck_composition_at_point(bp.log_sizes, claimed.data(), lmr, lookup, points, n_cols3, n3.data(), sampled3.data(), coeff, &cv, want));
        {
            Q31 r = pf.sampled_values[3][0][0];
            r = q_add(r, q_mul(pf.sampled_values[3][1][0], q_make(0, 1, 0, 0)));
            r = q_add(r, q_mul(pf.sampled_values[3][2][0], q_make(0, 0, 1, 0)));
            r = q_add(r, q_mul(pf.sampled_values[3][3][0], q_make(0, 0, 0, 1)));
            words(r, got);
        }
        if (memcmp(want, got, sizeof want) != 0) { reason = "OodsNotMatching"; return 0; }
        // the "proof" member's own bytes
        const size_t at = raw.find("\"proof\":");
        if (at == std::string::npos) { reason = "InvalidStructure: no proof member"; return 0; }
        const char* js = raw.data() + at + 8;
        const size_t len = raw.size() - (at + 8) - 1;
        char err[512] = {0};
        const int32_t rc = bfhip_pcs_verifier_verify_values(v, ch, points, 1 + N_COMPONENTS, counts.data(), idx.data(), js, len, err, sizeof err);
        if (rc < 0) { printf("internal: verify_values: %s\n", g_error.c_str()); return 2; }
        reason = err;
        return 0;
    };
    const int rc = replay();
    if (rc) return rc;
    printf("%s\n", reason.empty() ? "ok" : reason.c_str());
    // edge calls: every one must be refused (-1), none may read through a null pointer or accept a non-canonical word
    int refused = 0, tried = 0;
    uint32_t bad[8] = {0x7fffffffu, 0, 0, 0, 0, 0, 0, 0}, out8[8], out4[4];
    uint8_t d[32];
    auto expect = [&](int32_t r) { tried++; if (r == -1) refused++; };
    expect(bfhip_channel_create(&cv, nullptr));
    expect(bfhip_channel_mix_root(nullptr, d));
    expect(bfhip_channel_mix_root(ch, nullptr));
    expect(bfhip_channel_mix_u64(nullptr, 1));
    expect(bfhip_channel_mix_felts(ch, bad, 1));
    expect(bfhip_channel_mix_felts(ch, nullptr, 1));
    expect(bfhip_channel_draw_felts(ch, 1, nullptr));
    expect(bfhip_channel_draw_point(ch, nullptr));
    expect(bfhip_channel_state(nullptr, d, nullptr));
    expect(bfhip_circle_point_offset(bad, 5, -1, out8));
    expect(bfhip_circle_point_offset(out8, 0, -1, out8));
    expect(bfhip_circle_point_offset(nullptr, 5, -1, out8));
    expect(bfhip_pcs_verifier_commit(v, ch, d, nullptr, 1));
    { uint32_t big = 31; expect(bfhip_pcs_verifier_commit(v, ch, d, &big, 1)); }
    expect(bfhip_pcs_verifier_verify_values(nullptr, ch, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0));
    expect(bfhip_brainfuck_composition_at_point(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out4));
    { bfhip_pcs_config z{}; bfhip_pcs_verifier* w = nullptr; expect(bfhip_pcs_verifier_create(nullptr, &z, &w)); }
    { bfhip_conventions z{}; z.merkle_channel = 7; bfhip_channel* c2 = nullptr; expect(bfhip_channel_create(&z, &c2)); }
    printf("edges refused %d of %d\n", refused, tried);
    MUST(bfhip_pcs_verifier_destroy(v));
    MUST(bfhip_channel_destroy(ch));
    return refused == tried ? 0 : 3;
}
