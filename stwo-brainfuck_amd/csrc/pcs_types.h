// The handles of the commitment-scheme session (include/bfhip.h: bfhip_channel, bfhip_pcs_verifier) as pcs_host.hip (host only) and pcs.hip
// (the prover session) share them. Internal to the library.
#pragma once
#include "../../include/bfhip.h"
#include "host/verifier.h"
#include <stdexcept>
#include <string>
#include <vector>

// stwo's `channel` argument of commit / prove_values / verify_values: Blake2sChannel or Poseidon252Channel by the conventions it was created under
struct bfhip_channel { bf::Channel ch; bf::Conventions conv; };

// CommitmentSchemeVerifier: the roots and column log sizes (LDE domain) committed so far
struct bfhip_pcs_verifier {
    bf::Conventions conv; bf::PcsConfig cfg;
    std::vector<bf::Hash32> roots; std::vector<std::vector<bf::u32>> col_logs;
};

namespace bf {

// a bfhip_conventions checked against the known values (NULL = defaults); shared by every entry that takes one
inline Conventions conventions_from(const bfhip_conventions* conv) {
    Conventions cv;
    if (!conv) return cv;
    if (conv->merkle_node_hash > 1 || conv->mix_u64 > 1 || conv->logup_mask_order > 1 || conv->merkle_channel > 1) throw std::runtime_error("unknown convention value");
    for (uint32_t r : conv->reserved) if (r) throw std::runtime_error("bfhip_conventions: reserved fields must be zero");
    cv.merkle_node_hash = conv->merkle_node_hash; cv.mix_u64 = conv->mix_u64; cv.logup_mask_order = conv->logup_mask_order; cv.merkle_channel = conv->merkle_channel;
    return cv;
}
inline Q31 canonical_q31(const uint32_t* w, const char* what) {
    for (int k = 0; k < 4; k++) if (w[k] >= P31) throw std::runtime_error(std::string(what) + ": a word is not a canonical M31");
    return q_make(w[0], w[1], w[2], w[3]);
}
inline PtQ canonical_point(const uint32_t* w, const char* what) { return PtQ{canonical_q31(w, what), canonical_q31(w + 4, what)}; }
inline void q31_words(const Q31& q, uint32_t* out) { out[0] = q.a.a; out[1] = q.a.b; out[2] = q.b.a; out[3] = q.b.b; }

// The sample description shared by bfhip_pcs_prove_values and bfhip_pcs_verifier_verify_values: for every column of every tree, in commit
// order, n_samples_h[] counts its samples and point_idx_h lists them as indices into the points. Returns mask[tree][column] = point indices.
inline std::vector<std::vector<std::vector<u32>>> sample_mask(const std::vector<size_t>& cols_per_tree, uint32_t n_points, const uint32_t* n_samples_h, const uint32_t* point_idx_h) {
    std::vector<std::vector<std::vector<u32>>> mask(cols_per_tree.size());
    size_t ci = 0, si = 0;
    for (size_t t = 0; t < cols_per_tree.size(); t++) {
        mask[t].resize(cols_per_tree[t]);
        for (size_t c = 0; c < cols_per_tree[t]; c++, ci++) {
            const u32 n = n_samples_h[ci];
            if (n > BFHIP_PCS_MAX_SAMPLES_PER_COLUMN) throw std::runtime_error("tree " + std::to_string(t) + " column " + std::to_string(c) + ": " + std::to_string(n) + " samples, at most 2 per column (BFHIP_PCS_MAX_SAMPLES_PER_COLUMN)");
            if (n && !point_idx_h) throw std::runtime_error("null argument");
            for (u32 s = 0; s < n; s++, si++) {
                if (point_idx_h[si] >= n_points) throw std::runtime_error("tree " + std::to_string(t) + " column " + std::to_string(c) + ": point index " + std::to_string(point_idx_h[si]) + " out of range (n_points " + std::to_string(n_points) + ")");
                mask[t][c].push_back(point_idx_h[si]);
            }
        }
    }
    return mask;
}

}  // namespace bf
