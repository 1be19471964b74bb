// The lookup tuples that do not cancel: every relation entry of the row-granular tables with its multiplicity, and the tuples whose
// multiplicities do not sum to zero (include/bfhip.h: bfhip_relation_summary, bfhip_trace_relations).
//
// Replaces stwo's relation tracker, the debugging tool it ships beside `assert_constraints` (check.hip): where `lookup_sum_valid`
// (brainfuck_air/mod.rs:207-226) only says that the 13 claimed sums do not add up to zero, this pass names the tuples. Who adds what to
// which relation restates the `add_to_relation` calls of components/<name>/component.rs as air.h has them: air_memory (numerator d - 1),
// air_instruction (d - 1), air_program (1 - d), air_processor (1 - d, into all three relations), air_jump / air_instr (d - 1),
// air_eoe (-1).
//
// Per relation: (1) one lane per table row computes the numerator, non-zero rows are compacted in (table, row) order; (2) an index
// permutation is sorted by the tuple, least significant pair of words first, with rocPRIM's stable radix sort on 64-bit keys (as
// tables.hip sorts); (3) segment heads by comparing each tuple with its predecessor; (4) per tuple, net (mod p) and the yield / use /
// other counts are differences of one four-channel inclusive scan at the segment's ends — a segment may span any number of workgroups
// (an instruction inside a loop repeats its (ip, ci, ni) once per iteration) —, first yield and first use are 64-bit atomicMin;
// (5) the tuples with net != 0 are compacted in sorted order, up to the caller's cap. Integers only: nothing depends on the schedule.
// Steps (2) to (5) are relation_aggregate (ctx.h), which the relation programs of any AIR share (relation_program.hip): they bring their own
// step (1), an interpreter instead of k_rel_flags / k_rel_emit. relation_multiplicities (ctx.h) shares steps (2) and (3) (relation_sort) and
// the scan, and writes each tuple's net into the looked-up table's column instead of reporting it.
#include "../../include/bfhip.h"
#include <cstring>
#include <optional>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "kernels.h"
#include "api_guard.h"
#include "api_args.h"
#include "air.h"

namespace bf {

enum : u32 { REL_YIELD = 0, REL_USE = 1, REL_USE_ALWAYS = 2 };      // numerator 1 - d, d - 1, -1
// One table's part in one relation: the columns of the tuple's words, the dummy column, and where its rows lie in the relation's row stream
struct RelSource { const u32* w[7]; const u32* d; u32 row0, rows, table, kind; };
struct RelSources { u32 n, n_words, pad_[2]; RelSource src[64]; };
// RelEntries (ctx.h): SoA tuple words, numerator, (table << 32 | row)

static constexpr u32 ST_TILE = 2048;   // 256 lanes x 8, the tile of exclusive_scan_u32

__device__ __forceinline__ const RelSource& rel_source_of(const RelSources& S, u32 i) {
    u32 lo = 0, hi = S.n;              // largest k with src[k].row0 <= i
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (S.src[mid].row0 <= i) lo = mid; else hi = mid; }
    return S.src[lo];
}
__device__ __forceinline__ u32 rel_numerator(const RelSource& q, u32 row) {
    if (q.kind == REL_USE_ALWAYS) return P31 - 1;
    const u32 d = q.d[row] % P31;
    return q.kind == REL_YIELD ? m_sub(1, d) : m_sub(d, 1);
}

// ---- (1) entries: rows with a non-zero numerator, in (table, row) order ----------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rel_flags(const RelSources* __restrict__ Sp, u32 N, u32* __restrict__ flags) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const RelSource& q = rel_source_of(*Sp, i);
    flags[i] = rel_numerator(q, i - q.row0) != 0 ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_rel_emit(const RelSources* __restrict__ Sp, u32 N, const u32* __restrict__ flags, const u32* __restrict__ pos, RelEntries e) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || !flags[i]) return;
    const RelSources& S = *Sp;
    const RelSource& q = rel_source_of(S, i);
    const u32 row = i - q.row0, j = pos[i];
    for (u32 k = 0; k < S.n_words; k++) e.w[k][j] = q.w[k][row];
    e.num[j] = rel_numerator(q, row);
    e.origin[j] = ((u64)q.table << 32) | row;
}

// ---- (2) the sort's key gather: two words of the tuple per pass, read through the permutation so far -------------------------------------
__global__ void __launch_bounds__(256) k_rel_iota(u32* __restrict__ perm, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) perm[i] = i;
}
__global__ void __launch_bounds__(256) k_rel_keys(const u32* __restrict__ hi, const u32* __restrict__ lo, const u32* __restrict__ perm, u64* __restrict__ keys, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 j = perm[i];
    keys[i] = ((u64)(hi ? hi[j] : 0u) << 32) | lo[j];
}

// ---- (3) segment heads ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rel_heads(RelEntries e, u32 n_words, const u32* __restrict__ perm, u32 n, u32* __restrict__ heads) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u32 differs = i == 0;
    if (i) {
        const u32 a = perm[i], b = perm[i - 1];
        for (u32 k = 0; k < n_words; k++) differs |= e.w[k][a] != e.w[k][b];
    }
    heads[i] = differs ? 1u : 0u;
}
// start[s] = sorted position of tuple s's first entry; start[n_tuples] = n. Tuple of position i: segx[i] + heads[i] - 1 (segx = exclusive scan of heads)
__global__ void __launch_bounds__(256) k_rel_starts(const u32* __restrict__ heads, const u32* __restrict__ segx, u32 n, u32* __restrict__ start) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (heads[i]) start[segx[i]] = i;
    if (i == n - 1) start[segx[i] + heads[i]] = n;
}

// ---- (4) one inclusive scan of (numerator mod p, is yield, is use, is other) in sorted order ---------------------------------------------
__device__ __forceinline__ uint4 st_add(uint4 a, uint4 b) { return make_uint4(m_add(a.x, b.x), a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ uint4 st_of(u32 num) { return make_uint4(num, num == 1u, num == P31 - 1, num != 1u && num != P31 - 1); }
// Hillis-Steele over the 256 lane sums in LDS; returns the lane's exclusive prefix, *total = the workgroup's sum
__device__ __forceinline__ uint4 st_block_scan(uint4* s, uint4 sum, uint4* total) {
    s[threadIdx.x] = sum;
    __syncthreads();
    for (u32 off = 1; off < 256; off <<= 1) {
        const uint4 t = threadIdx.x >= off ? s[threadIdx.x - off] : make_uint4(0, 0, 0, 0);
        __syncthreads();
        s[threadIdx.x] = st_add(s[threadIdx.x], t);
        __syncthreads();
    }
    const uint4 excl = threadIdx.x ? s[threadIdx.x - 1] : make_uint4(0, 0, 0, 0);
    *total = s[255];
    __syncthreads();
    return excl;
}
// MARKED (relation_multiplicities): an entry whose origin carries REL_TABLE_SIDE contributes nothing to any channel — masked, not given
// multiplicity 0, which st_of would count as "other"
template <bool MARKED>
__global__ void __launch_bounds__(256) k_rel_stats_local(const u32* __restrict__ num, const u64* __restrict__ origin, const u32* __restrict__ perm, uint4* __restrict__ out,
                                                         uint4* __restrict__ totals, u32 n) {
    __shared__ uint4 s[256];
    const u32 base = blockIdx.x * ST_TILE + threadIdx.x * 8;
    uint4 v[8], sum = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (u32 k = 0; k < 8; k++) {
        v[k] = make_uint4(0, 0, 0, 0);
        if (base + k < n) {
            const u32 j = perm[base + k];
            if (!MARKED || !(origin[j] & REL_TABLE_SIDE)) v[k] = st_of(num[j]);
        }
        sum = st_add(sum, v[k]);
    }
    uint4 total, run = st_block_scan(s, sum, &total);
#pragma unroll
    for (u32 k = 0; k < 8; k++) { run = st_add(run, v[k]); if (base + k < n) out[base + k] = run; }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) k_rel_stats_totals(uint4* __restrict__ totals, u32 nb) {      // exclusive, in place, one workgroup
    __shared__ uint4 s[256];
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (u32 b0 = 0; b0 < nb; b0 += 256) {
        const u32 i = b0 + threadIdx.x;
        uint4 total;
        const uint4 excl = st_block_scan(s, i < nb ? totals[i] : make_uint4(0, 0, 0, 0), &total);
        if (i < nb) totals[i] = st_add(carry, excl);
        carry = st_add(carry, total);
    }
}
__global__ void __launch_bounds__(256) k_rel_stats_add(uint4* __restrict__ out, const uint4* __restrict__ totals, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = st_add(out[i], totals[i / ST_TILE]);
}
// First yield and first use of every tuple: the lowest (table, row) among its entries with numerator 1 / p - 1. A lane whose left
// neighbour in the wave offers a lower origin for the same tuple and kind leaves the atomic to it (a chain of such lanes ends at one that
// issues): a long segment costs about one atomic per wave, and the minimum is the same. MARKED (relation_multiplicities): an entry whose
// origin carries REL_TABLE_SIDE is a third kind whatever its multiplicity word, and its minimum goes to first_side — the mark is the top bit
// of every such origin, so the minimum is still the lowest row.
template <bool MARKED>
__global__ void __launch_bounds__(256) k_rel_first(const u32* __restrict__ num, const u64* __restrict__ origin, const u32* __restrict__ perm, const u32* __restrict__ heads,
                                                   const u32* __restrict__ segx, u32 n, u64* __restrict__ first_yield, u64* __restrict__ first_use, u64* __restrict__ first_side) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    u32 seg = 0xffffffffu, kind = 0;
    u64 org = ~u64(0);
    if (i < n) {
        const u32 j = perm[i], v = num[j];
        seg = segx[i] + heads[i] - 1;
        kind = v == 1u ? 1u : v == P31 - 1 ? 2u : 0u;
        org = origin[j];
        if (MARKED && (org & REL_TABLE_SIDE)) kind = 3u;
    }
    const u32 pseg = __shfl_up(seg, 1, 64), pkind = __shfl_up(kind, 1, 64);
    const u64 porg = __shfl_up((unsigned long long)org, 1, 64);
    const bool covered = (threadIdx.x & 63u) != 0 && pseg == seg && pkind == kind && porg < org;
    if (kind && !covered) atomicMin(reinterpret_cast<unsigned long long*>(kind == 1 ? first_yield + seg : kind == 2 ? first_use + seg : first_side + seg), (unsigned long long)org);
}
__device__ __forceinline__ uint4 rel_segment_stats(const uint4* __restrict__ scan, const u32* __restrict__ start, u32 s) {
    const u32 a = start[s], b = start[s + 1];
    const uint4 hi = scan[b - 1], lo = a ? scan[a - 1] : make_uint4(0, 0, 0, 0);
    return make_uint4(m_sub(hi.x, lo.x), hi.y - lo.y, hi.z - lo.z, hi.w - lo.w);
}
__global__ void __launch_bounds__(256) k_rel_unbalanced(const uint4* __restrict__ scan, const u32* __restrict__ start, u32 n_tuples, u32* __restrict__ unb) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s < n_tuples) unb[s] = rel_segment_stats(scan, start, s).x != 0 ? 1u : 0u;
}

// ---- (5) the unbalanced tuples, in sorted order, up to the cap ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rel_report(RelEntries e, u32 n_words, u32 relation, const u32* __restrict__ perm, const uint4* __restrict__ scan,
                                                    const u32* __restrict__ start, u32 n_tuples, const u32* __restrict__ unb, const u32* __restrict__ upos,
                                                    const u64* __restrict__ first_yield, const u64* __restrict__ first_use, u32 cap, bfhip_relation_entry* __restrict__ out) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_tuples || !unb[s] || upos[s] >= cap) return;
    const uint4 st = rel_segment_stats(scan, start, s);
    const u32 j = perm[start[s]];
    bfhip_relation_entry& r = out[upos[s]];      // every field is written: the arena is not zeroed
    r.relation = relation; r.n_words = n_words;
#pragma unroll
    for (u32 k = 0; k < 7; k++) r.tuple[k] = k < n_words ? e.w[k][j] : 0u;
    r.net = st.x; r.n_yield = st.y; r.n_use = st.z; r.n_other = st.w;
    const u64 fy = first_yield[s], fu = first_use[s];
    r.first_yield_table = fy == ~u64(0) ? -1 : (int32_t)(fy >> 32); r.first_yield_row = fy == ~u64(0) ? fy : (fy & 0xffffffffu);
    r.first_use_table = fu == ~u64(0) ? -1 : (int32_t)(fu >> 32); r.first_use_row = fu == ~u64(0) ? fu : (fu & 0xffffffffu);
    r.reserved[0] = 0; r.reserved[1] = 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static dim3 grid256(u32 n) { return dim3((n + 255) / 256); }
static u32 scan_total(Ctx& c, const u32* d_total) { u32 v = 0; c.read_back(&v, d_total, sizeof v); return v; }

// One relation over its sources (N rows in all). Arena memory only; every launch has a non-zero size.
static void relation_run(Ctx& c, u32 relation, const RelSources& S, u32 N, u32 cap, bfhip_relation_report& rep, bfhip_relation_entry* entries_h) {
    hipStream_t s = c.stream;
    rep = bfhip_relation_report{};
    rep.relation = relation; rep.n_words = S.n_words;
    if (N == 0) return;
    // (1)
    const RelSources* d_S = c.stage(&S, 1);
    u32* flags = c.alloc_u32(N); u32* pos = c.alloc_u32(N); u32* tot = c.alloc_u32(N / ST_TILE + 3);
    const u32* d_n;
    {
        ProfScope ps(s, "relations_extract", 0);
        hipLaunchKernelGGL(k_rel_flags, grid256(N), dim3(256), 0, s, d_S, N, flags);
        d_n = exclusive_scan_u32(s, flags, pos, tot, N);
    }
    const u32 n = scan_total(c, d_n);
    rep.n_entries = n;
    if (n == 0) return;
    relation_aggregate(c, relation, S.n_words, n, cap, rep, entries_h,
                       [&](const RelEntries& e) { hipLaunchKernelGGL(k_rel_emit, grid256(N), dim3(256), 0, s, d_S, N, flags, pos, e); });
}

// Steps (2) and (3) over the n >= 1 entries that `emit` writes: the entries, their sorted order, the segment heads and their exclusive scan.
// Shared by relation_aggregate and relation_multiplicities; arena memory only.
struct RelSorted { RelEntries e; const u32* order; u32* heads; u32* segx; u32 n_tuples; };
static RelSorted relation_sort(Ctx& c, u32 n_words, u32 n, const std::function<void(const RelEntries&)>& emit, const char* emit_scope, const char* sort_scope) {
    hipStream_t s = c.stream;
    RelEntries e{};
    for (u32 k = 0; k < n_words; k++) e.w[k] = c.alloc_u32(n);
    e.num = c.alloc_u32(n);
    e.origin = (u64*)c.arena.alloc(sizeof(u64) * n);
    // (2) + (3)
    u32* perm[2] = {c.alloc_u32(n), c.alloc_u32(n)};
    u64* keys = (u64*)c.arena.alloc(sizeof(u64) * n); u64* keys_sorted = (u64*)c.arena.alloc(sizeof(u64) * n);
    size_t sort_tmp_bytes = 0;
    BF_HIP(rocprim::radix_sort_pairs(nullptr, sort_tmp_bytes, keys, keys_sorted, perm[0], perm[1], n, 0, 64, s));
    void* sort_tmp = c.arena.alloc(sort_tmp_bytes + 256);
    u32* heads = c.alloc_u32(n); u32* segx = c.alloc_u32(n); u32* seg_tot = c.alloc_u32(n / ST_TILE + 3);
    const u32* d_n_tuples;
    int cur = 0;
    if (emit_scope) { ProfScope ps(s, emit_scope, 0); emit(e); }
    {
        ProfScope ps(s, sort_scope, 0);
        if (!emit_scope) emit(e);
        hipLaunchKernelGGL(k_rel_iota, grid256(n), dim3(256), 0, s, perm[0], n);
        // stable LSD passes over (w[k-1], w[k]) pairs from the last word down; word 0 of an odd tuple goes alone (32 key bits)
        for (int k = (int)n_words - 1; k >= 0; k -= 2) {
            const u32* hi = k >= 1 ? e.w[k - 1] : nullptr;
            hipLaunchKernelGGL(k_rel_keys, grid256(n), dim3(256), 0, s, hi, (const u32*)e.w[k], (const u32*)perm[cur], keys, n);
            BF_HIP(rocprim::radix_sort_pairs(sort_tmp, sort_tmp_bytes, keys, keys_sorted, perm[cur], perm[cur ^ 1], n, 0, hi ? 64 : 32, s));
            cur ^= 1;
        }
        hipLaunchKernelGGL(k_rel_heads, grid256(n), dim3(256), 0, s, e, n_words, (const u32*)perm[cur], n, heads);
        d_n_tuples = exclusive_scan_u32(s, heads, segx, seg_tot, n);
    }
    return RelSorted{e, perm[cur], heads, segx, scan_total(c, d_n_tuples)};
}

// Steps (2) to (5) over the n >= 1 entries that `emit` writes (ctx.h). Arena memory only; every launch has a non-zero size.
void relation_aggregate(Ctx& c, u32 relation, u32 n_words, u32 n, u32 cap, bfhip_relation_report& rep, bfhip_relation_entry* entries_h,
                        const std::function<void(const RelEntries&)>& emit, const char* emit_scope) {
    hipStream_t s = c.stream;
    const RelSorted sorted = relation_sort(c, n_words, n, emit, emit_scope, "relations_sort");
    const RelEntries& e = sorted.e;
    const u32* order = sorted.order;
    const u32* heads = sorted.heads; const u32* segx = sorted.segx;
    const u32 n_tuples = sorted.n_tuples;
    rep.n_tuples = n_tuples;
    // (4)
    const u32 nb = (n + ST_TILE - 1) / ST_TILE;
    uint4* scan = (uint4*)c.arena.alloc(sizeof(uint4) * n); uint4* scan_tot = (uint4*)c.arena.alloc(sizeof(uint4) * nb);
    u32* start = c.alloc_u32(size_t(n_tuples) + 1);
    u64* first = (u64*)c.arena.alloc(sizeof(u64) * 2 * n_tuples);
    u32* unb = c.alloc_u32(n_tuples); u32* upos = c.alloc_u32(n_tuples); u32* unb_tot = c.alloc_u32(n_tuples / ST_TILE + 3);
    const u32* d_n_unb;
    {
        ProfScope ps(s, "relations_reduce", 0);
        hipLaunchKernelGGL(k_rel_stats_local<false>, dim3(nb), dim3(256), 0, s, (const u32*)e.num, (const u64*)nullptr, order, scan, scan_tot, n);
        hipLaunchKernelGGL(k_rel_stats_totals, dim3(1), dim3(256), 0, s, scan_tot, nb);
        hipLaunchKernelGGL(k_rel_stats_add, grid256(n), dim3(256), 0, s, scan, (const uint4*)scan_tot, n);
        hipLaunchKernelGGL(k_rel_starts, grid256(n), dim3(256), 0, s, (const u32*)heads, (const u32*)segx, n, start);
        BF_HIP(hipMemsetAsync(first, 0xff, sizeof(u64) * 2 * n_tuples, s));
        hipLaunchKernelGGL(k_rel_first<false>, grid256(n), dim3(256), 0, s, (const u32*)e.num, (const u64*)e.origin, order, (const u32*)heads, (const u32*)segx, n, first, first + n_tuples,
                           (u64*)nullptr);
        hipLaunchKernelGGL(k_rel_unbalanced, grid256(n_tuples), dim3(256), 0, s, (const uint4*)scan, (const u32*)start, n_tuples, unb);
        d_n_unb = exclusive_scan_u32(s, unb, upos, unb_tot, n_tuples);
    }
    const u32 n_unb = scan_total(c, d_n_unb);
    rep.n_unbalanced = n_unb;
    const u32 n_rep = n_unb < cap ? n_unb : cap;
    rep.n_reported = n_rep;
    if (n_rep == 0) return;
    // (5)
    bfhip_relation_entry* d_out = (bfhip_relation_entry*)c.arena.alloc(sizeof(bfhip_relation_entry) * n_rep);
    {
        ProfScope ps(s, "relations_report", 0);
        hipLaunchKernelGGL(k_rel_report, grid256(n_tuples), dim3(256), 0, s, e, n_words, relation, order, (const uint4*)scan, (const u32*)start, n_tuples, (const u32*)unb,
                           (const u32*)upos, (const u64*)first, (const u64*)(first + n_tuples), n_rep, d_out);
    }
    BF_HIP(hipGetLastError());
    c.read_back(entries_h, d_out, sizeof(bfhip_relation_entry) * n_rep);
}

// ---- the other direction: the nets go INTO the looked-up table's multiplicity column (ctx.h: relation_multiplicities) -----------------------
// One lane per tuple. The scan was taken with the table-side entries masked, so st is the net and the counts of the OTHER entries; side =
// the lowest table-side origin of the segment (k_rel_first<true>) or ~0. A tuple some row holds: that row's word of out (zeroed before) gets
// the net. A tuple no row holds with net != 0 is missing. counts = {tuples some row holds, tuples with another entry, rows given a non-zero
// word}: one integer atomicAdd per wave and counter, of a ballot's population count — the sums do not depend on the order.
__global__ void __launch_bounds__(256) k_rel_mult_scatter(const uint4* __restrict__ scan, const u32* __restrict__ start, const u64* __restrict__ first_side, u32 n_tuples,
                                                          u32 n_rows, u32* __restrict__ out, u32* __restrict__ missing, u32* __restrict__ counts) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    bool held = false, used = false, filled = false;
    if (s < n_tuples) {
        const uint4 st = rel_segment_stats(scan, start, s);
        const u64 side = first_side[s];
        held = side != ~u64(0);
        used = (st.y | st.z | st.w) != 0;
        filled = held && st.x != 0;
        missing[s] = !held && st.x != 0 ? 1u : 0u;
        const u32 row = (u32)side;                                // origin = mark | table << 32 | row
        if (filled && row < n_rows) out[row] = st.x;
    }
    const u32 n_held = __popcll(__ballot(held)), n_used = __popcll(__ballot(used)), n_filled = __popcll(__ballot(filled));
    if ((threadIdx.x & 63u) == 0) {
        if (n_held) atomicAdd(counts + 0, n_held);
        if (n_used) atomicAdd(counts + 1, n_used);
        if (n_filled) atomicAdd(counts + 2, n_filled);
    }
}

void relation_multiplicities(Ctx& c, u32 relation, u32 n_words, u32 n, u32 n_rows, u32* out_d, u32 cap, bfhip_multiplicity_report& rep,
                             bfhip_relation_entry* missing_h, const std::function<void(const RelEntries&)>& emit) {
    hipStream_t s = c.stream;
    // (2) + (3): the stable sort keeps (table, row, program order) inside a segment
    const RelSorted sorted = relation_sort(c, n_words, n, emit, "relation_multiplicities_extract", "relation_multiplicities_sort");
    const RelEntries& e = sorted.e;
    const u32* order = sorted.order;
    const u32 n_tuples = sorted.n_tuples;
    const u32 nb = (n + ST_TILE - 1) / ST_TILE;
    uint4* scan = (uint4*)c.arena.alloc(sizeof(uint4) * n); uint4* scan_tot = (uint4*)c.arena.alloc(sizeof(uint4) * nb);
    u32* start = c.alloc_u32(size_t(n_tuples) + 1);
    u64* first = (u64*)c.arena.alloc(sizeof(u64) * 3 * n_tuples);      // first yield, first use, lowest table-side row
    u32* miss = c.alloc_u32(n_tuples); u32* mpos = c.alloc_u32(n_tuples); u32* miss_tot = c.alloc_u32(n_tuples / ST_TILE + 3);
    u32* counts = c.alloc_u32(4);
    const u32* d_n_miss;
    {
        ProfScope ps(s, "relation_multiplicities_scatter", 0);
        hipLaunchKernelGGL(k_rel_stats_local<true>, dim3(nb), dim3(256), 0, s, (const u32*)e.num, (const u64*)e.origin, order, scan, scan_tot, n);
        hipLaunchKernelGGL(k_rel_stats_totals, dim3(1), dim3(256), 0, s, scan_tot, nb);
        hipLaunchKernelGGL(k_rel_stats_add, grid256(n), dim3(256), 0, s, scan, (const uint4*)scan_tot, n);
        hipLaunchKernelGGL(k_rel_starts, grid256(n), dim3(256), 0, s, (const u32*)sorted.heads, (const u32*)sorted.segx, n, start);
        BF_HIP(hipMemsetAsync(first, 0xff, sizeof(u64) * 3 * n_tuples, s));
        BF_HIP(hipMemsetAsync(counts, 0, sizeof(u32) * 4, s));
        hipLaunchKernelGGL(k_rel_first<true>, grid256(n), dim3(256), 0, s, (const u32*)e.num, (const u64*)e.origin, order, (const u32*)sorted.heads, (const u32*)sorted.segx, n, first,
                           first + n_tuples, first + 2 * size_t(n_tuples));
        // out_d may be a column the extraction read: every launch that reads columns is ahead of these two on the stream
        BF_HIP(hipMemsetAsync(out_d, 0, sizeof(u32) * size_t(n_rows), s));
        hipLaunchKernelGGL(k_rel_mult_scatter, grid256(n_tuples), dim3(256), 0, s, (const uint4*)scan, (const u32*)start, (const u64*)(first + 2 * size_t(n_tuples)), n_tuples, n_rows,
                           out_d, miss, counts);
        d_n_miss = exclusive_scan_u32(s, miss, mpos, miss_tot, n_tuples);
    }
    const u32 n_miss = scan_total(c, d_n_miss);
    u32 h_counts[4] = {};
    c.read_back(h_counts, counts, sizeof h_counts);
    rep.n_row_tuples = h_counts[0]; rep.n_entries = u64(n) - n_rows; rep.n_tuples = h_counts[1]; rep.n_filled = h_counts[2];
    rep.n_missing = n_miss;
    const u32 n_rep = n_miss < cap ? n_miss : cap;
    rep.n_reported = n_rep;
    if (n_rep == 0) return;
    bfhip_relation_entry* d_out = (bfhip_relation_entry*)c.arena.alloc(sizeof(bfhip_relation_entry) * n_rep);
    {
        ProfScope ps(s, "relation_multiplicities_report", 0);
        hipLaunchKernelGGL(k_rel_report, grid256(n_tuples), dim3(256), 0, s, e, n_words, relation, order, (const uint4*)scan, (const u32*)start, n_tuples, (const u32*)miss,
                           (const u32*)mpos, (const u64*)first, (const u64*)(first + n_tuples), n_rep, d_out);
    }
    BF_HIP(hipGetLastError());
    c.read_back(missing_h, d_out, sizeof(bfhip_relation_entry) * n_rep);
}

struct RelTable { int component; u32 log_size; const u32* const* cols; };

// in_proof: called from inside a proof (its preflight) — the arena holds the proof's tables, so each relation's scratch is taken above a mark
// and given back instead of resetting the arena, and the staging ring is left alone
static void relations_run(Ctx& c, const RelTable* tables, u32 n_tables, bfhip_relation_report out[3], bfhip_relation_entry* entries_h, u32 cap, bool in_proof = false) {
    if (c.shard.count > 1) throw HipError("relation summary: a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    u64 total_rows = 0;
    for (u32 t = 0; t < n_tables; t++) {
        const RelTable& T = tables[t];
        check_component(T.component, T.log_size);
        if (!T.cols) throw HipError("null main column array");
        for (u32 j = 0; j < n_main_cols(T.component); j++) if (!T.cols[j]) throw HipError("null main column pointer");
        total_rows += u64(1) << (T.log_size - LOG_N_LANES);
    }
    if (total_rows > (u64(1) << 31)) throw HipError("more than 2^31 table rows in total");
    static const u32 N_WORDS[3] = {3, 3, 7};
    if (!in_proof) c.refuse_in_session("relation summary");
    // in a proof each relation's scratch is borrowed and given back on every path; outside one the arena is reset and left as it is
    std::optional<ArenaBorrow> borrow;
    if (in_proof) borrow.emplace(c);
    for (u32 r = 0; r < 3; r++) {
        RelSources S{};
        S.n_words = N_WORDS[r];
        u32 N = 0;
        for (u32 t = 0; t < n_tables; t++) {
            const RelTable& T = tables[t];
            const int k = T.component;
            RelSource q{};
            // word columns and dummy column of component k in relation r; -1 = takes no part
            int w0 = -1, d = -1;
            int wc[7] = {0, 1, 2, 3, 4, 5, 6};
            if (k == C_PROCESSOR) {
                q.kind = REL_YIELD; d = 7; w0 = 0;
                if (r == 0) { wc[1] = 4; wc[2] = 5; }
                if (r == 1) { wc[0] = 1; wc[1] = 2; wc[2] = 3; }
            } else if (k == C_MEMORY && r == 0) { q.kind = REL_USE; d = 3; w0 = 0; }
            else if (k == C_INSTRUCTION && r == 1) { q.kind = REL_USE; d = 3; w0 = 0; }
            else if (k == C_PROGRAM && r == 1) { q.kind = REL_YIELD; d = 3; w0 = 0; }
            else if ((k == C_JNZ || k == C_JZ) && r == 2) { q.kind = REL_USE; d = 11; w0 = 0; }
            else if (k >= C_INPUT && k <= C_RIGHT && r == 2) { q.kind = REL_USE; d = 7; w0 = 0; }
            else if (k == C_EOE && r == 2) { q.kind = REL_USE_ALWAYS; w0 = 0; }
            if (w0 < 0) continue;
            for (u32 j = 0; j < S.n_words; j++) q.w[j] = T.cols[wc[j]];
            q.d = d >= 0 ? T.cols[d] : nullptr;
            q.row0 = N; q.rows = 1u << (T.log_size - LOG_N_LANES); q.table = t;
            N += q.rows;
            S.src[S.n++] = q;
        }
        // like a proof: nothing of this context is in flight, and its per-proof memory starts empty
        c.sync();
        if (borrow) borrow->rewind_now();
        else { c.arena.reset(); c.stage_checkpoint(); }
        relation_run(c, r, S, N, cap, out[r], entries_h ? entries_h + size_t(r) * cap : nullptr);
    }
    if (borrow) { c.sync(); borrow->end(); }
    BF_HIP(hipGetLastError());
}

void relations_in_proof(Ctx& c, const u32* const* const cols[N_COMPONENTS], const u32 log_sizes[N_COMPONENTS], bfhip_relation_report* out,
                        bfhip_relation_entry* entries_h, u32 cap) {
    RelTable t[N_COMPONENTS];
    for (int k = 0; k < N_COMPONENTS; k++) t[k] = RelTable{k, log_sizes[k], cols[k]};
    relations_run(c, t, N_COMPONENTS, out, entries_h, cap, /*in_proof=*/true);
}

}  // namespace bf

using namespace bf;

int32_t bfhip_relation_summary(bfhip_ctx* ctx, const bfhip_relation_table* tables, uint32_t n_tables, bfhip_relation_report out[3],
                               bfhip_relation_entry* entries_h, uint32_t cap_per_relation) {
    API_CTX(ctx)
    if (!tables || !out || (!entries_h && cap_per_relation)) throw HipError("null argument");
    if (n_tables < 1 || n_tables > 64) throw HipError("relation summary: 1 to 64 tables");
    RelTable t[64];
    for (u32 i = 0; i < n_tables; i++) t[i] = RelTable{tables[i].component, tables[i].log_size, tables[i].main_rows_h};
    relations_run(ctx->c, t, n_tables, out, entries_h, cap_per_relation);
    return 0;
    API_CATCH
}

int32_t bfhip_trace_relations(bfhip_ctx* ctx, const bfhip_trace* trace, bfhip_relation_report out[3], bfhip_relation_entry* entries_h, uint32_t cap_per_relation) {
    API_CTX(ctx)
    if (!trace || !out || (!entries_h && cap_per_relation)) throw HipError("null argument");
    const u32* rows[N_COMPONENTS][13] = {};
    u32 log_sizes[N_COMPONENTS];
    trace_columns(trace, rows, log_sizes);
    RelTable t[N_COMPONENTS];
    for (int k = 0; k < N_COMPONENTS; k++) t[k] = RelTable{k, log_sizes[k], rows[k]};
    relations_run(ctx->c, t, N_COMPONENTS, out, entries_h, cap_per_relation);
    return 0;
    API_CATCH
}
