// Circle FFT / iFFT over M31 for gfx950 (MI355X) — SURVEY.md §8 rows a1 (twiddles), a2 (interpolate), a3 (evaluate / LDE).
// Replaces stwo `PolyOps::{precompute_twiddles, interpolate_columns, evaluate_polynomials}` as reached from
// crates/brainfuck_prover/src/brainfuck_air/mod.rs:480-484 (twiddles), :497,550-562,690-702 (extend_evals = interpolate),
// :500,583,723 (commit = LDE evaluate).
//
// Layout: a column is a contiguous u32[2^log] in HBM, bit-reversed circle-domain order (the order the reference stores).
// The butterfly network is identical to stwo's CpuBackend (layer 0 = circle layer on adjacent pairs, layer i>=1 = line layer
// at distance 2^i), so results are value-identical. A transform is executed as 1..3 passes; each pass stages a 4096-element
// tile in LDS, runs up to 12 (contiguous tile) or 7 (128-byte-chunk strided tile) layers there, and touches HBM once for read and
// once for write with 16-byte per-lane accesses. Twiddles of the tile are staged in LDS once and reused for every column of
// the batch (grid.y walks column groups), so twiddle traffic is amortised over the batch.
//
// "line mode" (circle = 0) runs the same network without the circle layer: this is exactly what the circle FFT of a column
// whose every value is replicated 16x (the reference broadcasts each table row into 16 SIMD lanes, memory/table.rs:95-104)
// reduces to, on the 16x smaller row-granular column. See DESIGN.md "replicated columns".
#include "kernels.h"
#include <cstdlib>
#include <stdexcept>
#include <mutex>
#include <optional>
#include <set>
#include <string>

namespace bf {

static constexpr int TILE = 1 << TILE_LOG;   // TILE_LOG, CHUNK_LOG, STRIDED_K and the kernel kinds: fft_plan.h
static constexpr int FFT_THREADS = 256;
// PassArgs::scale of an inverse transform is 2^-n = a power of two (m31.h: m_inv_pow2): its exponent, for m_mul_pow2 (uniform: scalar unit)
__device__ __forceinline__ u32 scale_shift(u32 scale) { return (u32)__builtin_ctz(scale); }

// ---------------------------------------------------------------------------------------------------------------------
// Twiddle generation (a1). Layered buffer exactly as stwo's slow_precompute_twiddles(Coset::half_odds(R)):
// layer j (j < R) holds the bit-reversed x-coordinates of the first half of the coset doubled j times; last entry = 1.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void point_of_index(u32 idx, const uint2* __restrict__ tlo, const uint2* __restrict__ thi, u32& x, u32& y) {
    uint2 a = tlo[idx & 0xffffu], b = thi[(idx >> 16) & 0x7fffu];
    x = m_sub(m_mul(a.x, b.x), m_mul(a.y, b.y));
    y = m_add(m_mul(a.x, b.y), m_mul(a.y, b.x));
}

__global__ void k_gen_twiddles(u32* __restrict__ tw, u32* __restrict__ itw, u32 R, const uint2* __restrict__ tlo, const uint2* __restrict__ thi) {
    u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    u32 total = 1u << R;
    if (g >= total) return;
    if (g == total - 1) { tw[g] = 1; itw[g] = 1; return; }
    // layer j starts at offset 2^R - 2^(R-j): j = number of leading ones of g within R bits
    u32 j = __clz(~(g << (32 - R)));
    u32 off = total - (1u << (R - j));
    u32 k = g - off;
    u32 bits = R - 1 - j;
    u32 init = (1u << (31 - R - 2)) << j, step = (1u << (31 - R)) << j;
    u32 idx = (init + step * bit_rev(k, bits)) & 0x7fffffffu;
    u32 x, y;
    point_of_index(idx, tlo, thi, x, y);
    tw[g] = x;
    itw[g] = m_inv(x);
}

// ---------------------------------------------------------------------------------------------------------------------
// Preprocessed columns in closed form: interpolate(gen_is_first(n)) for every n in one launch (mod.rs:495-499: gen_is_first::<SimdBackend>
// then tree_builder.extend_evals = interpolate). IsFirst(n) is the indicator of cell 0; under the inverse butterflies
// (v0, v1) -> (v0 + v1, (v0 - v1) t) a one-hot vector stays a tensor product: after layer i cell (1 << i) | l holds cell l times t_i,
// t_i = the layer's inverse twiddle of butterfly block 0. Hence coefficient j = 2^-n * prod over the set bits i of j of t_i — the values the
// transform of the one-hot column produces, with no column traffic and no 19 x (1 + 3) launches.
// t_0 = the circle layer's twiddle of pair 0 (y of the first entry pair of the first line table), t_i = entry 0 of line layer i.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_is_first_coeffs(IsFirstCols a, const u32* __restrict__ itw, u32 tw_total) {
    // one lane writes 16 consecutive coefficients; lanes are flattened over the columns in ascending size
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x + (1u << (a.log_min - 4));
    if (u >= (1u << (a.log_max - 3))) return;
    const u32 n = 35u - __clz(u);                     // column IsFirst(n): u in [2^(n-4), 2^(n-3))
    u32* __restrict__ dst = a.ptr[n - a.log_min];
    if (!dst) return;                                 // another rank of the shard group owns this column
    const u32 jhi = u - (1u << (n - 4));              // coefficient index >> 4
    auto t = [&](u32 i) -> u32 { return i == 0 ? itw[tw_total - (1u << (n - 1)) + 1] : itw[tw_total - (1u << (n - i))]; };
    u32 v[16];
    v[0] = m_inv_pow2(n);
    for (u32 i = 4; i < n; i++) if ((jhi >> (i - 4)) & 1) v[0] = m_mul(v[0], t(i));
#pragma unroll
    for (u32 b = 0; b < 4; b++) {
        const u32 tb = t(b);
#pragma unroll
        for (u32 e = 0; e < (1u << b); e++) v[e + (1u << b)] = m_mul(v[e], tb);
    }
    uint4* o = reinterpret_cast<uint4*>(dst + 16 * (size_t)jhi);
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
void is_first_coeffs(hipStream_t stream, const IsFirstCols& a, const u32* itw, u32 tw_root_log) {
    if (a.log_min < 4 || a.log_max < a.log_min || a.log_max - a.log_min >= 28 || a.log_max > tw_root_log + 1) throw std::runtime_error("is_first_coeffs: unsupported sizes");
    const u32 lanes = (1u << (a.log_max - 3)) - (1u << (a.log_min - 4));
    hipLaunchKernelGGL(k_is_first_coeffs, dim3((lanes + 255) / 256), dim3(256), 0, stream, a, itw, 1u << tw_root_log);
}

// The LDE of those columns in closed form as well: evaluate(interpolate(gen_is_first(n))) on the 2^N-cell domain, N = n + log_blowup, for every n in
// one launch. The tensor product survives the forward butterflies (v0, v1) -> (v0 + v1 T, v0 - v1 T) too: the layers >= n only duplicate, and going
// down from layer n - 1 the pair of layer i holds (P, P t_i) x (what the layers above made of the cell's block), so layer i multiplies the cell by
// 1 + t_i T_i(cell >> (i + 1)) or, with bit i of the cell set, 1 - t_i T_i(cell >> (i + 1)):
//     e(cell) = 2^-n * prod_{i < n} (1 +- t_i T_i(cell >> (i + 1)))
// T_i(h) = the forward twiddle of pair block h in layer i of the 2^N-cell transform, read exactly as fft_pass_body stages it (layer_table; the circle
// layer takes [y, -y, -x, x][h & 3] of entry pair h >> 2 of the first line table), t_i as in k_is_first_coeffs. Exact field arithmetic on canonical
// values: the words are those the general transform writes. One lane owns 16 consecutive cells: the factors of the layers >= 4 are common to them
// (two products per layer; those of the layers >= 10 are common to the whole wave and computed once for it), the four low layers take 11 products for
// their 15 distinct factors and 30 to spread them over the cells. No column is read.
__global__ void __launch_bounds__(256) k_is_first_lde(IsFirstCols a, u32 log_blowup, const u32* __restrict__ tw, const u32* __restrict__ itw, u32 tw_total) {
    // lanes flattened over the columns in ascending size, lane u = 2^(N-4) + (cell >> 4) of the 2^N-cell column: a wave (64 lanes, 1024 cells) of u >= 64
    // lies inside one column of >= 2^10 cells (the lanes below 2^(log_min + log_blowup - 4) have no column)
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < (1u << (a.log_min + log_blowup - 4)) || u >= (1u << (a.log_max + log_blowup - 3))) return;
    const u32 N = 35u - __clz(u), n = N - log_blowup;  // column IsFirst(n) on 2^N cells: u in [2^(N-4), 2^(N-3))
    u32* __restrict__ dst = a.ptr[n - a.log_min];
    if (!dst) return;                                 // another rank of the shard group owns this column
    const u32 chi = u - (1u << (N - 4));              // cell >> 4
    auto t = [&](u32 i) -> u32 { return i == 0 ? itw[tw_total - (1u << (n - 1)) + 1] : itw[tw_total - (1u << (n - i))]; };
    u32 pre = m_inv_pow2(n), lane_layers = n;         // the layers [4, lane_layers) are this lane's own
    if (u >= 64u) {
        // the factors of the layers >= 10 are the same for the wave's 1024 cells: wave-uniform operands, so once per wave (scalar unit) and not per lane
        const u32 cw = __builtin_amdgcn_readfirstlane(chi >> 6), nw = __builtin_amdgcn_readfirstlane(n), Nw = nw + log_blowup;
        u32 pw = m_inv_pow2(nw);
        for (u32 i = 10; i < nw; i++) {
            const u32 f = m_mul(itw[tw_total - (1u << (nw - i))], tw[tw_total - (1u << (Nw - i)) + (cw >> (i - 9))]);
            pw = m_mul(pw, (cw >> (i - 10)) & 1 ? m_sub(1u, f) : m_add(1u, f));
        }
        pre = pw; lane_layers = min(n, 10u);
    }
    for (u32 i = 4; i < lane_layers; i++) {
        const u32 f = m_mul(t(i), tw[tw_total - (1u << (N - i)) + (chi >> (i - 3))]);
        pre = m_mul(pre, (chi >> (i - 4)) & 1 ? m_sub(1u, f) : m_add(1u, f));
    }
    // layers 1 and 0 share the four entries 4 chi .. 4 chi + 3 of the first line table: T_1 of the cell quads, (x, y) of the two circle-layer chunks
    const uint4 l0 = *reinterpret_cast<const uint4*>(tw + (tw_total - (1u << (N - 1))) + 4 * (size_t)chi);
    const u32 l0w[4] = {l0.x, l0.y, l0.z, l0.w};
    const u32 t0 = t(0), t1 = t(1), t2 = t(2), t3 = t(3);
    const u32 f3 = m_mul(t3, tw[tw_total - (1u << (N - 3)) + chi]);
    u32 w3[2] = {m_mul(pre, m_add(1u, f3)), m_mul(pre, m_sub(1u, f3))};
    u32 v[16];
#pragma unroll
    for (u32 b3 = 0; b3 < 2; b3++) {
        const u32 f2 = m_mul(t2, tw[tw_total - (1u << (N - 2)) + 2 * chi + b3]);
        const u32 w2[2] = {m_mul(w3[b3], m_add(1u, f2)), m_mul(w3[b3], m_sub(1u, f2))};
        // circle layer of this half: pairs (y, -y, -x, x) of chunk 2 chi + b3
        const u32 gx = m_mul(t0, l0w[2 * b3]), gy = m_mul(t0, l0w[2 * b3 + 1]);
        const u32 py = m_add(1u, gy), ny = m_sub(1u, gy), px = m_add(1u, gx), nx = m_sub(1u, gx);
        const u32 f0[8] = {py, ny, ny, py, nx, px, px, nx};
#pragma unroll
        for (u32 b2 = 0; b2 < 2; b2++) {
            const u32 f1 = m_mul(t1, l0w[2 * b3 + b2]);
            const u32 w1[2] = {m_mul(w2[b2], m_add(1u, f1)), m_mul(w2[b2], m_sub(1u, f1))};
#pragma unroll
            for (u32 e = 0; e < 4; e++) v[8 * b3 + 4 * b2 + e] = m_mul(w1[e >> 1], f0[4 * b2 + e]);
        }
    }
    g_u32p o = as_global(dst) + 16 * (size_t)chi;
#pragma unroll
    for (int q = 0; q < 4; q++) st16(o + 4 * q, make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]));
}
// The same product at a point outside the domain (PolyOps::eval_at_point of these columns): sum_j c_j prod_{bit b of j} F[b] with c_j = 2^-n prod t_b
// factors into 2^-n prod_{b < n} (1 + t_b F[b]). One wave per (size, point): lane b holds the factor of bit b (n <= 31), five exchange steps multiply them
// up (exact field arithmetic: the order does not matter). F as eval_at_points takes it (32 QM31 entries per point).
__global__ void __launch_bounds__(64) k_is_first_samples(const IsFirstSample* __restrict__ jobs, const uint4* __restrict__ factors, uint4* __restrict__ out,
                                                         const u32* __restrict__ itw, u32 tw_total) {
    const IsFirstSample job = jobs[blockIdx.x];
    const u32 n = job.log_n, b = threadIdx.x;
    Q31 acc = q_one();
    if (b < n) {
        const u32 tb = b == 0 ? itw[tw_total - (1u << (n - 1)) + 1] : itw[tw_total - (1u << (n - b))];
        const uint4 f = factors[(size_t)job.point * 32 + b];
        acc = q_addm(q_mulm(q_make(f.x, f.y, f.z, f.w), tb), 1u);
    }
    for (int s = 1; s < 32; s <<= 1) {      // every lane of the wave takes part (the lanes >= n carry ones)
        const Q31 o = q_make((u32)__shfl_xor((int)acc.a.a, s), (u32)__shfl_xor((int)acc.a.b, s), (u32)__shfl_xor((int)acc.b.a, s), (u32)__shfl_xor((int)acc.b.b, s));
        acc = q_mul(acc, o);
    }
    if (b == 0) { acc = q_mulm(acc, m_inv_pow2(n)); out[job.out_idx] = make_uint4(acc.a.a, acc.a.b, acc.b.a, acc.b.b); }
}
void is_first_samples(hipStream_t stream, const IsFirstSample* d_jobs, u32 n_jobs, const void* d_factors, void* d_out, const u32* itw, u32 tw_root_log) {
    if (!n_jobs) return;
    hipLaunchKernelGGL(k_is_first_samples, dim3(n_jobs), dim3(64), 0, stream, d_jobs, (const uint4*)d_factors, (uint4*)d_out, itw, 1u << tw_root_log);
}
void is_first_lde(hipStream_t stream, const IsFirstCols& a, u32 log_blowup, const u32* tw, const u32* itw, u32 tw_root_log) {
    if (a.log_min < 4 || a.log_max < a.log_min || a.log_max - a.log_min >= 28 || a.log_max + log_blowup > tw_root_log + 1 || a.log_max + log_blowup > 31)
        throw std::runtime_error("is_first_lde: unsupported sizes");
    const u32 lanes = 1u << (a.log_max + log_blowup - 3);
    double bytes = 0;
    for (u32 n = a.log_min; n <= a.log_max; n++) if (a.ptr[n - a.log_min]) bytes += 4.0 * (double)(1ull << (n + log_blowup));
    ProfScope ps(stream, "k_is_first_lde", bytes, bytes);
    hipLaunchKernelGGL(k_is_first_lde, dim3((lanes + 255) / 256), dim3(256), 0, stream, a, log_blowup, tw, itw, 1u << tw_root_log);
}

// ---------------------------------------------------------------------------------------------------------------------
// One pass = layers [lo, lo+k) of a size-2^log transform, for the columns cols[by * cpb .. +cpb) of one GROUP (columns of one size and
// storage). A launch covers several groups (PassArgs table in HBM, fft_plan.h): workgroup b belongs to the group g with
// groups[g].block0 <= b < groups[g + 1].block0 and is its (tile, column block) = ((b - block0) % grid_x, (b - block0) / grid_x). The 13
// components of a proof have ~10 distinct sizes: one launch per pass and kernel kind instead of one per size.
// ---------------------------------------------------------------------------------------------------------------------
struct BlockOfGroup { u32 g, tile, by; };
template <bool INV> __device__ __forceinline__ void fft_tiny_body(const PassArgs& a, const BlockOfGroup& bg);      // defined with k_fft_tiny below
__device__ __forceinline__ BlockOfGroup find_group(const PassArgs* __restrict__ groups, u32 ngroups) {
    u32 g = 0;
    while (g + 1 < ngroups && groups[g + 1].block0 <= blockIdx.x) g++;      // uniform: scalar loads
    const u32 local = blockIdx.x - groups[g].block0, gx = groups[g].grid_x;
    return {g, local % gx, local / gx};
}
__device__ __forceinline__ const u32* layer_table(const PassArgs& a, u32 layer) {
    // line layer `layer` (>= 1 in circle mode, >= 0 in line mode): len = 2^(log-1-layer), table at tw_total - 2*len.
    // In line mode local layer j plays the role of circle-mode layer j+1 of a transform twice the size.
    u32 eff = a.circle ? layer : layer + 1;
    u32 lg = a.circle ? a.log : a.log + 1;
    u32 len = 1u << (lg - 1 - eff);
    return a.tw + (a.tw_total - 2 * len);
}

// s_val, s_tw: TILE words each (s_tw: per-layer twiddle segments of this tile, packed)
template <bool INV>
__device__ __forceinline__ void fft_pass_body(const PassArgs& a, const BlockOfGroup& bg, u32* __restrict__ s_val, u32* __restrict__ s_tw) {
    const u32 t = threadIdx.x;
    const u32 lo = a.lo, k = a.k;
    const u32 c = lo == 0 ? 0 : CHUNK_LOG;
    const u32 tile_log = lo == 0 ? a.tile_log : k + c;
    const u32 tile_n = 1u << tile_log;
    const u32 kt = tile_log - c;   // twiddle span: local layer j needs 2^(kt-1-j) entries, staged at offset 2^kt - 2^(kt-j)
    const u32 tile = bg.tile;
    // element (m, l) of the tile -> global index
    // contiguous: idx = tile * tile_n + m
    // strided   : idx = (H << (lo+k)) | (m << lo) | (Lhi << c) | l   with tile = H * 2^(lo-c) + Lhi
    const u32 n_lhi_log = lo - c;  // only used when lo > 0
    const u32 H = lo ? (tile >> n_lhi_log) : 0, Lhi = lo ? (tile & ((1u << n_lhi_log) - 1)) : 0;
    const u32 base = lo ? ((H << (lo + k)) | (Lhi << c)) : (tile << tile_log);

    // ---- stage twiddles: for local layer j (global lo+j) the tile needs 2^(k-1-j) entries -----------------------------
    // s_tw offset of local layer j: sum_{q<j} 2^(k-1-q) = 2^k - 2^(k-j)
    for (u32 e = t; e < (1u << kt) - (1u << (kt - k)); e += FFT_THREADS) {
        // find layer j with offset <= e
        u32 j = __clz(~((e) << (32 - kt)));  // leading ones of e in kt bits
        u32 off = (1u << kt) - (1u << (kt - j));
        u32 q = e - off;                     // q < 2^(kt-1-j): index of the h-block inside the tile
        u32 gl = lo + j;
        u32 hbase = lo ? (H << (kt - 1 - j)) : (tile << (kt - 1 - j));
        u32 v;
        if (a.circle && gl == 0) {
            // circle layer: pair h uses [y, -y, -x, x][h & 3] of chunk (h >> 2) of the first line table
            const u32* l0 = layer_table(a, 1);
            u32 h = hbase + q;
            u32 x = l0[(h >> 2) * 2], y = l0[(h >> 2) * 2 + 1];
            u32 sel = h & 3;
            v = sel == 0 ? y : sel == 1 ? m_neg(y) : sel == 2 ? m_neg(x) : x;
        } else {
            v = layer_table(a, gl)[hbase + q];
        }
        s_tw[e] = v;
    }

    const u32 col0 = bg.by * a.cols_per_block;
    const u32 col1 = min(a.ncols, col0 + a.cols_per_block);
    for (u32 col = col0; col < col1; col++) {
        g_cu32p src = as_global(a.src[col]);
        g_u32p dst = as_global(a.dst[col]);
        __syncthreads();  // s_tw ready / previous column's stores done reading s_val
        // ---- load tile (16 B per lane) -----------------------------------------------------------------------------
        for (u32 e4 = t * 4; e4 < tile_n; e4 += 4 * FFT_THREADS) {
            u32 gidx = lo ? (base | ((e4 >> c) << lo) | (e4 & ((1u << c) - 1))) : (base + e4);
            // src_mask < 3 (uniform): 1 or 2 coefficients, zero-padded to the 4 cells of every load (fft_plan)
            uint4 v = a.src_mask < 3u ? make_uint4(src[0], a.src_mask ? src[1] : 0u, 0u, 0u) : ld16(src + (gidx & a.src_mask));
            *reinterpret_cast<uint4*>(&s_val[e4]) = v;
        }
        __syncthreads();
        // ---- butterflies -------------------------------------------------------------------------------------------
        const u32 nb = tile_n >> 1;
        if (INV) {
            for (u32 j = 0; j < k; j++) {
                u32 dist = 1u << (j + c);
                u32 toff = (1u << kt) - (1u << (kt - j));
                for (u32 b = t; b < nb; b += FFT_THREADS) {
                    u32 i0 = ((b >> (j + c)) << (j + c + 1)) | (b & (dist - 1));
                    u32 tw = s_tw[toff + (b >> (j + c))];
                    u32 v0 = s_val[i0], v1 = s_val[i0 + dist];
                    s_val[i0] = m_add(v0, v1);
                    s_val[i0 + dist] = m_mul(m_sub(v0, v1), tw);
                }
                __syncthreads();
            }
        } else {
            for (int j = (int)k - 1; j >= 0; j--) {
                u32 dist = 1u << (j + c);
                u32 toff = (1u << kt) - (1u << (kt - j));
                for (u32 b = t; b < nb; b += FFT_THREADS) {
                    u32 i0 = ((b >> (j + c)) << (j + c + 1)) | (b & (dist - 1));
                    u32 tw = s_tw[toff + (b >> (j + c))];
                    u32 v0 = s_val[i0], v1 = m_mul(s_val[i0 + dist], tw);
                    s_val[i0] = m_add(v0, v1);
                    s_val[i0 + dist] = m_sub(v0, v1);
                }
                __syncthreads();
            }
        }
        // ---- store tile --------------------------------------------------------------------------------------------
        for (u32 e4 = t * 4; e4 < tile_n; e4 += 4 * FFT_THREADS) {
            u32 gidx = lo ? (base | ((e4 >> c) << lo) | (e4 & ((1u << c) - 1))) : (base + e4);
            uint4 v = *reinterpret_cast<uint4*>(&s_val[e4]);
            if (INV && a.scale != 1) { const u32 sk = scale_shift(a.scale); v.x = m_mul_pow2(v.x, sk); v.y = m_mul_pow2(v.y, sk); v.z = m_mul_pow2(v.z, sk); v.w = m_mul_pow2(v.w, sk); }
            st16(dst + gidx, v);
        }
    }
}

template <bool INV>
__global__ void __launch_bounds__(FFT_THREADS) k_fft_pass(const PassArgs* __restrict__ groups, u32 ngroups) {
    const BlockOfGroup bg = find_group(groups, ngroups);
    const PassArgs a = groups[bg.g];
    __shared__ u32 s_val[TILE];
    __shared__ u32 s_tw[TILE];
    fft_pass_body<INV>(a, bg, s_val, s_tw);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fast path (transforms of >= 2^12 cells): register-radix butterflies, one LDS round trip per 4 layers.
//   k_fft_tile12 : contiguous 4096-cell tile, layers [0, k), 6 <= k <= 12. 256 lanes x 16 cells. Layers 0,1 and 10,11 are done
//                  in registers on the 16-byte global accesses; layers 2..5 and 6..9 are two radix-16 rounds through LDS.
//   k_fft_strided7: 128 rows x 32 or 64 cells (128- or 256-byte rows at stride 2^lo), layers [lo, lo+7). 32 cells per lane. Layers lo..lo+2 in
//                  registers on the 16-byte accesses, layers lo+3..lo+6 as one radix-16 round with 4-byte coalesced row accesses.
// LDS index padding p(i) = i + 4*(i >> 6) keeps the stride-4 round conflict-free and the 16-byte accesses aligned.
// ---------------------------------------------------------------------------------------------------------------------
// t2 = TWICE the twiddle (the kernels below stage their twiddles doubled in LDS, once per workgroup and batch of columns): m31.h m_mul_pre2
// 11 VALU per butterfly (product 5, a + t 3, a - t 3), and no lazily reduced form is shorter in 32-bit lanes (r05): p = 2^31 - 1
// leaves one spare bit, so (i) m_mul_pre2 needs its multiplicand < 2^31 — for b < 2^32 the fold high + (low >> 1) of b * 2w can reach
// 2^32 + 2^31 and loses the carry —, (ii) a lazy sum a + t <= 2p may be added to once more at most (3p > 2^32) while half of a layer's outputs are the
// next layer's multiplicands, and (iii) folding the addition into the multiply-add (b * 2w + 2a in 64 bits) saves an add but costs a second
// v_mad_u64_u32 (1.6 issue slots) for the subtracted output.
template <bool INV> __device__ __forceinline__ void bfly(u32& x, u32& y, u32 t2) {
    if (INV) { u32 s = m_add(x, y); y = m_mul_pre2(m_sub(x, y), t2); x = s; }
    else { u32 w = m_mul_pre2(y, t2); y = m_sub(x, w); x = m_add(x, w); }
}
// radix-16 over the 4 local bits of v[16]; tw(jl, idx) returns the twiddle of local layer jl for pair index (e >> (jl+1)).
template <bool INV, class TW> __device__ __forceinline__ void radix16(u32 (&v)[16], u32 nlayers, TW tw) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int jl = INV ? s : 3 - s;
        if ((u32)jl < nlayers) {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int e0 = ((b >> jl) << (jl + 1)) | (b & ((1 << jl) - 1));
                bfly<INV>(v[e0], v[e0 | (1 << jl)], tw(jl, e0 >> (jl + 1)));
            }
        }
    }
}
__device__ __forceinline__ u32 lds_pad(u32 i) { return i + 4 * (i >> 6); }

// KC != 0: k == KC is a compile-time fact (KC = 9, 10, 11, 12: k0 = layers - 7 x strided passes; the contiguous pass of the three-pass transforms of 2^24 / 2^25 / >= 2^26 cells and of
// every two-pass size): every "layer < k" test folds away, and with them the phi copies the compiler otherwise keeps for the skipped-layer paths
// (r05: profiles/r05_fft_isa_mix.txt). KC = 0: k read from the pass descriptor. One kernel, a uniform branch at its top picks the body.
template <bool INV, int KC>
__device__ __forceinline__ void fft_tile12_body(const PassArgs& a, const BlockOfGroup& bg, u32* __restrict__ s_val, u32* __restrict__ s_tw) {
    const u32 t = threadIdx.x, k = KC ? (u32)KC : a.k, tile = bg.tile;
    const u32 base = tile << 12;
    const u32 col0 = bg.by * a.cols_per_block, col1 = min(a.ncols, col0 + a.cols_per_block);
    // The tile of the next column is fetched while the current one is transformed (16 more registers, same occupancy): without it
    // every column starts with an exposed HBM round trip, which costs ~25 % when a block has only a few columns.
    uint4 nxt[4];
    if (col0 < col1) {
        g_cu32p src0 = as_global(a.src[col0]);
#pragma unroll
        for (int q = 0; q < 4; q++) nxt[q] = ld16(src0 + ((base + 1024 * q + 4 * t) & a.src_mask));
    }
    // stage twiddles of local layers j < k: entry (j, q) at 4096 - 2^(12-j) + q, q < 2^(11-j); global h = (tile << (11-j)) + q.
    // 16 entries per lane with a compile-time layer for each slot (8 of layer 0, 4 of layer 1, 2 of layer 2, 1 of layer 3, 1 of the
    // layers 4..11), so that the 16 loads are issued back to back and waited for once — a rolled loop serialises 16 memory round
    // trips per block, which dominates when a batch has only a few columns per block.
    {
        u32 tw_r[16];
        g_cu32p tw = as_global(a.tw);
        auto table = [&](u32 j) -> g_cu32p { return tw + (layer_table(a, j) - a.tw); };
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const u32 j = s < 8 ? 0u : s < 12 ? 1u : s < 14 ? 2u : s < 15 ? 3u : 4u;            // slot -> layer (4 = "4 and above")
            const u32 e = 256u * s + t;
            u32 v = 0;
            if (j < 4) {
                if (j < k) {
                    const u32 q = e - (4096u - (4096u >> j));
                    const u32 h = (tile << (11 - j)) + q;
                    if (j == 0 && a.circle) {
                        g_cu32p l0 = table(1);
                        const u32 x = l0[(h >> 2) * 2], y = l0[(h >> 2) * 2 + 1], sel = h & 3;
                        v = sel == 0 ? y : sel == 1 ? m_neg(y) : sel == 2 ? m_neg(x) : x;
                    } else v = table(j)[h];
                }
            } else if (e < 4096u - (4096u >> k)) {
                const u32 jj = __clz(~(e << 20));
                const u32 q = e - (4096u - (4096u >> jj));
                v = table(jj)[(tile << (11 - jj)) + q];
            }
            tw_r[s] = v;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) s_tw[256u * s + t] = 2u * tw_r[s];     // doubled: bfly
    }
    auto TW = [&](u32 layer, u32 idx) -> u32 { return s_tw[4096u - (4096u >> layer) + idx]; };
    for (u32 col = col0; col < col1; col++) {
        g_u32p dst = as_global(a.dst[col]);
        __syncthreads();
        u32 r[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++) { r[q][0] = nxt[q].x; r[q][1] = nxt[q].y; r[q][2] = nxt[q].z; r[q][3] = nxt[q].w; }
        if (col + 1 < col1) {
            g_cu32p srcn = as_global(a.src[col + 1]);
#pragma unroll
            for (int q = 0; q < 4; q++) nxt[q] = ld16(srcn + ((base + 1024 * q + 4 * t) & a.src_mask));
        }
        // ---- register stage on the 16-byte groups: layers 0,1 (cells 4t..4t+3 of each quarter q) and 10,11 (across q) --------
        auto stage_low = [&]() {
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int L = INV ? s : 1 - s;
                if ((u32)L < k) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        u32 i = 1024 * q + 4 * t;
                        if (L == 0) { bfly<INV>(r[q][0], r[q][1], TW(0, i >> 1)); bfly<INV>(r[q][2], r[q][3], TW(0, (i >> 1) + 1)); }
                        else { u32 w = TW(1, i >> 2); bfly<INV>(r[q][0], r[q][2], w); bfly<INV>(r[q][1], r[q][3], w); }
                    }
                }
            }
        };
        auto stage_high = [&]() {
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int L = INV ? 10 + s : 11 - s;
                if ((u32)L < k) {
                    if (L == 10) { u32 w0 = TW(10, 0), w1 = TW(10, 1);
#pragma unroll
                        for (int j = 0; j < 4; j++) { bfly<INV>(r[0][j], r[1][j], w0); bfly<INV>(r[2][j], r[3][j], w1); } }
                    else { u32 w = TW(11, 0);
#pragma unroll
                        for (int j = 0; j < 4; j++) { bfly<INV>(r[0][j], r[2][j], w); bfly<INV>(r[1][j], r[3][j], w); } }
                }
            }
        };
        auto round_lds = [&](u32 first_layer) {
            // 16 cells per lane with tile-index bits [first_layer, first_layer+4) = e
            u32 lo_bits = first_layer;                       // 2 or 6
            u32 lo = t & ((1u << lo_bits) - 1), hi = t >> lo_bits;
            u32 idx0 = (hi << (lo_bits + 4)) | lo;
            u32 v[16];
#pragma unroll
            for (int e = 0; e < 16; e++) v[e] = s_val[lds_pad(idx0 | ((u32)e << lo_bits))];
            u32 nl = k > first_layer ? k - first_layer : 0;
            radix16<INV>(v, nl, [&](int jl, int pe) -> u32 { return TW(first_layer + jl, ((hi << 4) >> (jl + 1)) + pe); });
#pragma unroll
            for (int e = 0; e < 16; e++) s_val[lds_pad(idx0 | ((u32)e << lo_bits))] = v[e];
        };
        auto put = [&]() {
#pragma unroll
            for (int q = 0; q < 4; q++) *reinterpret_cast<uint4*>(&s_val[lds_pad(1024 * q + 4 * t)]) = make_uint4(r[q][0], r[q][1], r[q][2], r[q][3]);
        };
        auto get = [&]() {
#pragma unroll
            for (int q = 0; q < 4; q++) { uint4 v = *reinterpret_cast<uint4*>(&s_val[lds_pad(1024 * q + 4 * t)]); r[q][0] = v.x; r[q][1] = v.y; r[q][2] = v.z; r[q][3] = v.w; }
        };
        if (INV) {
            stage_low(); put(); __syncthreads();
            round_lds(2); __syncthreads();
            round_lds(6); __syncthreads();
            get(); stage_high();
        } else {
            stage_high(); put(); __syncthreads();
            round_lds(6); __syncthreads();
            round_lds(2); __syncthreads();
            get(); stage_low();
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint4 v = make_uint4(r[q][0], r[q][1], r[q][2], r[q][3]);
            if (INV && a.scale != 1) { const u32 sk = scale_shift(a.scale); v.x = m_mul_pow2(v.x, sk); v.y = m_mul_pow2(v.y, sk); v.z = m_mul_pow2(v.z, sk); v.w = m_mul_pow2(v.w, sk); }
            st16(dst + base + 1024 * q + 4 * t, v);
        }
    }
}

template <bool INV>
__global__ void __launch_bounds__(256) k_fft_tile12(const PassArgs* __restrict__ groups, u32 ngroups, u32 generic) {
    const BlockOfGroup bg = find_group(groups, ngroups);
    const PassArgs a = groups[bg.g];
    __shared__ __attribute__((aligned(16))) u32 s_val[4096 + 4 * 64];
    __shared__ u32 s_tw[4096];
    // guests of this launch (fft_plan): small single-pass transforms and tiny ones, in the same LDS (4096 words each suffice)
    if (a.kind == K_PASS) { fft_pass_body<INV>(a, bg, s_val, s_tw); return; }
    if (a.kind == K_TINY) { fft_tiny_body<INV>(a, bg); return; }
    const u32 k = generic ? 0u : a.k;                  // generic: A/B knob (BFHIP_FFT_TILE12_GENERIC=1), same bytes
    if (k == 12) fft_tile12_body<INV, 12>(a, bg, s_val, s_tw);
    else if (k == 11) fft_tile12_body<INV, 11>(a, bg, s_val, s_tw);
    else if (k == 10) fft_tile12_body<INV, 10>(a, bg, s_val, s_tw);
    else if (k == 9) fft_tile12_body<INV, 9>(a, bg, s_val, s_tw);
    else fft_tile12_body<INV, 0>(a, bg, s_val, s_tw);
}

// CL = log2 of the cells per row: 5 (128-byte rows, 128 lanes) or 6 (256-byte rows, 256 lanes: longer contiguous bursts per DRAM page at
// the same per-lane work; needs lo >= 6). Per lane always 32 cells: 8 rows x 4 cells in the 16-byte phase, 2 x 16 in the 4-byte phase.
template <bool INV, int CL>
__global__ void __launch_bounds__(4 << CL, 3) k_fft_strided7(const PassArgs* __restrict__ groups, u32 ngroups) {
    const BlockOfGroup bg = find_group(groups, ngroups);
    const PassArgs a = groups[bg.g];
    constexpr u32 C = 1u << CL, NT = 4u << CL;
    __shared__ __attribute__((aligned(16))) u32 s_val[128 * C];
    __shared__ u32 s_tw[128];
    const u32 t = threadIdx.x, lo = a.lo, tile = bg.tile;
    const u32 n_lhi_log = lo - CL;
    const u32 H = tile >> n_lhi_log, Lhi = tile & ((1u << n_lhi_log) - 1);
    const u32 base = (H << (lo + 7)) | (Lhi << CL);
    // twiddles: local layer j (global lo + j) entry q < 2^(6-j) at 128 - 2^(7-j) + q; global h = (H << (6-j)) + q
    if (t < 127) {
        u32 j = __clz(~(t << 25));
        u32 q = t - (128u - (128u >> j));
        s_tw[t] = 2u * layer_table(a, lo + j)[(H << (6 - j)) + q];          // doubled: bfly
    }
    auto TW = [&](u32 layer, u32 idx) -> u32 { return s_tw[128u - (128u >> layer) + idx]; };
    const u32 col0 = bg.by * a.cols_per_block, col1 = min(a.ncols, col0 + a.cols_per_block);
    const u32 l4 = 4 * (t & (C / 4 - 1)), r4 = t >> (CL - 2);      // 16-byte phase: rows m = 8*r4 + q (q = 0..7), cells l4..l4+3
    for (u32 col = col0; col < col1; col++) {
        g_cu32p src = as_global(a.src[col]);
        g_u32p dst = as_global(a.dst[col]);
        __syncthreads();
        auto wide_stage = [&](u32 (&r)[8][4]) {   // layers 0..2 over q
#pragma unroll
            for (int s = 0; s < 3; s++) {
                const int jl = INV ? s : 2 - s;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int q0 = ((b >> jl) << (jl + 1)) | (b & ((1 << jl) - 1));
                    u32 w = TW(jl, (8 * r4 + q0) >> (jl + 1));
#pragma unroll
                    for (int j = 0; j < 4; j++) bfly<INV>(r[q0][j], r[q0 | (1 << jl)][j], w);
                }
            }
        };
        auto narrow_task = [&](u32 id, bool from_global, bool to_global) {   // layers 3..6 over e for fixed (mlow3, l)
            u32 l = id & (C - 1), mlow = id >> CL;
            u32 v[16];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                u32 m = 8 * e + mlow;
                v[e] = from_global ? __builtin_nontemporal_load(src + ((base | (m << lo) | l) & a.src_mask)) : s_val[C * m + l];
            }
            radix16<INV>(v, 4, [&](int jl, int pe) -> u32 { return TW(3 + jl, pe); });
#pragma unroll
            for (int e = 0; e < 16; e++) {
                u32 m = 8 * e + mlow;
                if (to_global) __builtin_nontemporal_store((INV && a.scale != 1) ? m_mul_pow2(v[e], scale_shift(a.scale)) : v[e], dst + (base | (m << lo) | l));   // streamed: +2 %
                else s_val[C * m + l] = v[e];
            }
        };
        if (INV) {
            u32 r[8][4];
#pragma unroll
            for (int q = 0; q < 8; q++) { uint4 v = ld16_stream(src + ((base | ((8 * r4 + q) << lo) | l4) & a.src_mask)); r[q][0] = v.x; r[q][1] = v.y; r[q][2] = v.z; r[q][3] = v.w; }
            wide_stage(r);
#pragma unroll
            for (int q = 0; q < 8; q++) *reinterpret_cast<uint4*>(&s_val[C * (8 * r4 + q) + l4]) = make_uint4(r[q][0], r[q][1], r[q][2], r[q][3]);
            __syncthreads();
            narrow_task(t, false, true);
            narrow_task(t + NT, false, true);
        } else {
            narrow_task(t, true, false);
            // r04 ISA audit (tools/isa_mix.py): left to itself the scheduler hoists the 32 loads of both tasks to the top and the forward
            // kernel needs 168 VGPRs + 20 bytes of scratch inside the column loop; with the two tasks kept apart it takes 142 and no scratch
            // (128 x 2^24: 5.17-5.25 -> 5.10-5.14 ms per launch, profiles/r04_fft_isa_audit.txt). Two waves per SIMD instead: slower.
            __builtin_amdgcn_sched_barrier(0);
            narrow_task(t + NT, true, false);
            __syncthreads();
            u32 r[8][4];
#pragma unroll
            for (int q = 0; q < 8; q++) { uint4 v = *reinterpret_cast<uint4*>(&s_val[C * (8 * r4 + q) + l4]); r[q][0] = v.x; r[q][1] = v.y; r[q][2] = v.z; r[q][3] = v.w; }
            wide_stage(r);
#pragma unroll
            for (int q = 0; q < 8; q++) st16(dst + (base | ((8 * r4 + q) << lo) | l4), make_uint4(r[q][0], r[q][1], r[q][2], r[q][3]));
        }
    }
}

// Strided pass of K = 8, 9 or 10 layers (2^20 .. 2^22-cell transforms in TWO passes: 12 contiguous + K strided, instead of 6..8 + 7 + 7):
// 2^K rows of 2^CL cells (rows at stride 2^lo) staged in LDS — 32 KiB for K = 8, 64 KiB for K = 9 (128-byte rows) and K = 10 (64-byte rows) —
// read and written with 16-byte accesses, 32 cells per lane. The layers run as radix-16 rounds over 4 row bits each (16 values per lane
// in registers, lanes of a wave on consecutive cells: conflict-free LDS accesses); the last round covers the top 4 row bits and applies
// only the layers the earlier rounds have not. At 8-10 layers such a pass is as much butterfly work as HBM time (fft.hip header).
template <bool INV, class TW> __device__ __forceinline__ void radix16_range(u32 (&v)[16], int jl_lo, TW tw) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int jl = INV ? s : 3 - s;
        if (jl >= jl_lo) {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int e0 = ((b >> jl) << (jl + 1)) | (b & ((1 << jl) - 1));
                bfly<INV>(v[e0], v[e0 | (1 << jl)], tw(jl, e0 >> (jl + 1)));
            }
        }
    }
}
template <bool INV, int K, int CL>
__global__ void __launch_bounds__((1 << (K + CL)) / 32) k_fft_stridedK(const PassArgs* __restrict__ groups, u32 ngroups) {
    constexpr u32 C = 1u << CL, ROWS = 1u << K, CELLS = ROWS * C, NT = CELLS / 32;
    constexpr int NR = (K + 3) / 4;                 // rounds
    const BlockOfGroup bg = find_group(groups, ngroups);
    const PassArgs a = groups[bg.g];
    __shared__ __attribute__((aligned(16))) u32 s_val[CELLS];
    __shared__ u32 s_tw[ROWS];
    const u32 t = threadIdx.x, lo = a.lo, tile = bg.tile;
    const u32 n_lhi_log = lo - CL;
    const u32 H = tile >> n_lhi_log, Lhi = tile & ((1u << n_lhi_log) - 1);
    const u32 base = (H << (lo + K)) | (Lhi << CL);
    // twiddles: local layer j (global lo + j), entry q < 2^(K-1-j) at ROWS - (ROWS >> j) + q; global h = (H << (K-1-j)) + q
    for (u32 e = t; e < ROWS - 1; e += NT) {
        const u32 j = __clz(~(e << (32 - K)));
        const u32 q = e - (ROWS - (ROWS >> j));
        s_tw[e] = 2u * layer_table(a, lo + j)[(H << (K - 1 - j)) + q];      // doubled: bfly
    }
    auto TW = [&](u32 layer, u32 idx) -> u32 { return s_tw[ROWS - (ROWS >> layer) + idx]; };
    const u32 col0 = bg.by * a.cols_per_block, col1 = min(a.ncols, col0 + a.cols_per_block);
    for (u32 col = col0; col < col1; col++) {
        g_cu32p src = as_global(a.src[col]);
        g_u32p dst = as_global(a.dst[col]);
        __syncthreads();      // twiddles staged / the previous column's stores have read s_val
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            const u32 idx = 4 * (t + NT * i), m = idx >> CL, l = idx & (C - 1);
            const uint4 v = ld16_stream(src + ((base | (m << lo) | l) & a.src_mask));
            *reinterpret_cast<uint4*>(&s_val[idx]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
            const int r = INV ? rr : NR - 1 - rr;
            // window of 4 row bits [b, b + 4); the last round is shifted down to the top 4 bits and skips the layers already done
            const int b = (4 * r + 4 <= K) ? 4 * r : K - 4;
            const int jl_lo = 4 * r - b;
#pragma unroll
            for (u32 g2 = 0; g2 < 2; g2++) {
                const u32 id = t + NT * g2, l = id & (C - 1), rest = id >> CL;      // rest: the K - 4 row bits outside the window
                const u32 rest_lo = rest & ((1u << b) - 1), rest_hi = rest >> b;
                const u32 m0 = (rest_hi << (b + 4)) | rest_lo;
                u32 v[16];
#pragma unroll
                for (int e = 0; e < 16; e++) v[e] = s_val[((m0 | ((u32)e << b)) << CL) | l];
                radix16_range<INV>(v, jl_lo, [&](int jl, int pe) -> u32 { return TW(b + jl, (rest_hi << (3 - jl)) + pe); });
#pragma unroll
                for (int e = 0; e < 16; e++) s_val[((m0 | ((u32)e << b)) << CL) | l] = v[e];
            }
            __syncthreads();
        }
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            const u32 idx = 4 * (t + NT * i), m = idx >> CL, l = idx & (C - 1);
            uint4 v = *reinterpret_cast<uint4*>(&s_val[idx]);
            if (INV && a.scale != 1) { const u32 sk = scale_shift(a.scale); v.x = m_mul_pow2(v.x, sk); v.y = m_mul_pow2(v.y, sk); v.z = m_mul_pow2(v.z, sk); v.w = m_mul_pow2(v.w, sk); }
            st16(dst + (base | (m << lo) | l), v);
        }
    }
}

// Tiny transforms (log <= 5: the 16..32-cell columns of empty sub-component tables, end_of_execution, and their row-granular forms down to ONE cell): one LANE per
// cell, 64 >> log columns per wave, the butterflies as lane exchanges (__shfl_xor) — a launch of six such kernels per proof used to cost 13-15 us each (one thread
// per column looping over a 32-word array in scratch memory: a latency chain), r06: the whole transform is five dependent exchanges behind one round of loads.
template <bool INV>
__device__ __forceinline__ void fft_tiny_body(const PassArgs& a, const BlockOfGroup& bg) {
    const u32 n = 1u << a.log, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, i = lane & (n - 1);
    const u32 col = (bg.tile * (blockDim.x >> 6) + wave) * (64u >> a.log) + (lane >> a.log);
    const bool act = col < a.ncols;
    u32 v = act ? a.src[col][i & a.src_mask] : 0u;
    // this cell's twiddle in every layer (pair block h = i >> (j + 1)): independent loads, one round trip
    u32 tw[5];
#pragma unroll
    for (u32 j = 0; j < 5; j++) {
        tw[j] = 1u;
        if (j < a.k) {
            const u32 h = i >> (j + 1);
            if (a.circle && j == 0) {
                const u32* l0 = layer_table(a, 1);
                const u32 x = l0[(h >> 2) * 2], y = l0[(h >> 2) * 2 + 1], sel = h & 3;
                tw[j] = sel == 0 ? y : sel == 1 ? m_neg(y) : sel == 2 ? m_neg(x) : x;
            } else tw[j] = layer_table(a, j)[h];
        }
    }
#pragma unroll
    for (u32 jj = 0; jj < 5; jj++) {
        if (jj >= a.k) break;                                         // uniform
        const u32 j = INV ? jj : a.k - 1 - jj;
        const u32 other = (u32)__shfl_xor((int)v, 1 << j);           // every lane of the wave takes part (inactive columns carry zeros)
        const bool hi = (i >> j) & 1u;
        const u32 x = hi ? other : v, y = hi ? v : other;            // (v0, v1) of this cell's butterfly; both lanes of a pair compute the product
        u32 t = 0;
#pragma unroll
        for (u32 q = 0; q < 5; q++) if (q == j) t = tw[q];
        if (INV) v = hi ? m_mul(m_sub(x, y), t) : m_add(x, y);
        else { const u32 w = m_mul(y, t); v = hi ? m_sub(x, w) : m_add(x, w); }
    }
    if (act) a.dst[col][i] = INV ? m_mul(v, a.scale) : v;
}
template <bool INV>
__global__ void __launch_bounds__(256) k_fft_tiny(const PassArgs* __restrict__ groups, u32 ngroups) {
    const BlockOfGroup bg = find_group(groups, ngroups);
    const PassArgs a = groups[bg.g];
    fft_tiny_body<INV>(a, bg);
}

// BFHIP_FFT_PROF_DETAIL=1 (tools/fft_inproof.py): the profiler's record of an FFT launch carries its shape — "name/b<workgroups>/g<size groups>" — so that
// the in-proof launches can be priced one by one (butterflies and bytes per launch against its time) instead of per kernel name.
static const char* fft_prof_name(const char* base, const FftLaunch& L) {
    static const bool detail = [] { const char* v = getenv("BFHIP_FFT_PROF_DETAIL"); return v && v[0] == '1'; }();
    if (!detail) return base;
    static std::mutex mu; static std::set<std::string> names;
    std::lock_guard<std::mutex> g(mu);
    return names.insert(std::string(base) + "/b" + std::to_string(L.total_blocks) + "/g" + std::to_string(L.ngroups)).first->c_str();
}

// The kernel of every launch kind: forward and inverse entry point, workgroup size (what the kernel's __launch_bounds__ says, from the same template
// arguments) and the profiler's names. k_fft_tile12 takes one argument more (generic); k_fft_tiny is launched without a profiler record.
using FftKernel = void (*)(const PassArgs*, u32); using FftKernelTile12 = void (*)(const PassArgs*, u32, u32);
struct FftKernelEntry { FftKernel fn[2]; FftKernelTile12 tile12[2]; u32 threads; const char* name[2]; };      // [inverse]
template <int CL> constexpr FftKernelEntry strided7_entry() { return {{k_fft_strided7<false, CL>, k_fft_strided7<true, CL>}, {}, 4u << CL, {"k_fft_strided7<false>", "k_fft_strided7<true>"}}; }
template <int K, int CL> constexpr FftKernelEntry stridedK_entry() { return {{k_fft_stridedK<false, K, CL>, k_fft_stridedK<true, K, CL>}, {}, (1u << (K + CL)) / 32, {"k_fft_stridedK<false>", "k_fft_stridedK<true>"}}; }
static constexpr FftKernelEntry FFT_KERNELS[K_KINDS] = {
    /* K_TILE12      */ {{}, {k_fft_tile12<false>, k_fft_tile12<true>}, 256, {"k_fft_tile12<false>", "k_fft_tile12<true>"}},
    /* K_STRIDED5    */ strided7_entry<5>(),
    /* K_STRIDED6    */ strided7_entry<6>(),
    /* K_PASS        */ {{k_fft_pass<false>, k_fft_pass<true>}, {}, FFT_THREADS, {"k_fft_pass<false>", "k_fft_pass<true>"}},
    /* K_TINY        */ {{k_fft_tiny<false>, k_fft_tiny<true>}, {}, 256, {nullptr, nullptr}},
    /* K_STRIDED_K8  */ stridedK_entry<8, FFT_STRIDED_K_CHUNK_LOG>(),
    /* K_STRIDED_K9  */ stridedK_entry<9, FFT_STRIDED_K_CHUNK_LOG>(),
    /* K_STRIDED_K10 */ stridedK_entry<10, FFT_STRIDED_K10_CHUNK_LOG>(),
};
void fft_run(hipStream_t stream, const FftPlan& plan) {
    if (plan.launches.empty()) return;
    if (!plan.d_groups) throw std::runtime_error("fft_run: the plan's group table has not been staged");
    static const u32 generic = [] { const char* v = getenv("BFHIP_FFT_TILE12_GENERIC"); return (v && v[0] == '1') ? 1u : 0u; }();
    const int inv = plan.inverse ? 1 : 0;
    for (const FftLaunch& L : plan.launches) {
        const FftKernelEntry& e = FFT_KERNELS[L.kind];
        const PassArgs* g = plan.d_groups + L.first_group;
        const dim3 grid(L.total_blocks), block(e.threads);
        std::optional<ProfScope> ps;
        if (e.name[inv]) ps.emplace(stream, fft_prof_name(e.name[inv], L), L.bytes, L.alg, false, L.bfly);
        if (e.tile12[inv]) hipLaunchKernelGGL(e.tile12[inv], grid, block, 0, stream, g, L.ngroups, generic);
        else hipLaunchKernelGGL(e.fn[inv], grid, block, 0, stream, g, L.ngroups);
    }
}

void gen_twiddles(hipStream_t stream, u32* d_tw, u32* d_itw, u32 R, const uint2* d_tlo, const uint2* d_thi) {
    u32 total = 1u << R;
    hipLaunchKernelGGL(k_gen_twiddles, dim3((total + 255) / 256), dim3(256), 0, stream, d_tw, d_itw, R, d_tlo, d_thi);
}

}  // namespace bf
