// Register rows as the caller holds them -> the seven SoA columns the table builders read (tables.hip: TraceSoA).
// prove_brainfuck(&Machine) receives an executed machine whose trace is a Vec<Registers> (mod.rs:471-473, :508): n rows of 7 u32
// (clk, ip, ci, ni, mp, mv, mvi), row-major. The rows cross PCIe in ONE copy into arena scratch; one launch transposes them through LDS and
// checks every word for canonicity on the way, so the host neither walks the rows nor builds per-column vectors.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ctx.h"

namespace bf {

static constexpr u32 IN_TILE = 256;               // rows per workgroup = lanes per workgroup
static constexpr u32 IN_WORDS = 7 * IN_TILE;      // 1792 words = 7168 B = 448 x 16 B: tile bases stay 16-byte aligned when the buffer is

struct IngestCols { u32* c[7]; };

// first_bad: min over the non-canonical words of row * 8 + register (UINT64_MAX when every word is canonical).
__global__ void __launch_bounds__(256) k_ingest_registers(const u32* __restrict__ rows7, u32 n, IngestCols out, unsigned long long* __restrict__ first_bad) {
    __shared__ u32 s[IN_WORDS];
    const u32 tid = threadIdx.x;
    const u64 row0 = (u64)blockIdx.x * IN_TILE;
    const u64 base = row0 * 7;                     // 64-bit word offset: 7 n exceeds 2^32 long before n does
    const u32 tile_rows = n - row0 < IN_TILE ? (u32)(n - row0) : IN_TILE;
    const u32 words = 7 * tile_rows;
    unsigned long long bad = ~0ull;
    auto note = [&](u32 v, u32 w) { if (v >= P31) { unsigned long long key = (row0 + w / 7) * 8 + w % 7; if (key < bad) bad = key; } };
    g_cu32p src = as_global(rows7) + base;
    if (tile_rows == IN_TILE) {
        // consecutive 16-byte pieces of the tile: 448 of them over 256 lanes
        for (u32 q = tid; q < IN_WORDS / 4; q += 256) {
            uint4 v = ld16_stream(src + 4 * q);
            s[4 * q] = v.x; s[4 * q + 1] = v.y; s[4 * q + 2] = v.z; s[4 * q + 3] = v.w;
            note(v.x, 4 * q); note(v.y, 4 * q + 1); note(v.z, 4 * q + 2); note(v.w, 4 * q + 3);
        }
    } else {
        for (u32 w = tid; w < words; w += 256) { u32 v = src[w]; s[w] = v; note(v, w); }      // the last, partial tile: word by word, bounded
    }
    __syncthreads();
    if (tid < tile_rows) {
        // lane r reads words 7 r .. 7 r + 6: a stride of 7 words between lanes. 7 is odd, so the lanes of a group that the LDS serves in one
        // cycle (32 lanes over 32 or 64 banks) land on distinct banks — no padding needed.
        const u64 r = row0 + tid;
#pragma unroll
        for (int k = 0; k < 7; k++) as_global(out.c[k])[r] = s[7 * tid + k];      // seven coalesced column stores
    }
    // one atomic per wave, and only from a wave that saw a non-canonical word
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { unsigned long long o = __shfl_down(bad, off, 64); if (o < bad) bad = o; }
    if ((tid & 63) == 0 && bad != ~0ull) atomicMin(first_bad, bad);
}

// Uploads n rows of 7 u32 (one transfer), transposes them into arena scratch and returns the columns. *first_bad = row * 8 + register of the
// lowest non-canonical word, UINT64_MAX if there is none (the host has waited for the launch when this returns).
TraceSoA ingest_registers(Ctx& c, const u32* trace7_h, size_t n_rows, u64* first_bad) {
    if (n_rows == 0) throw HipError("EmptyTrace");
    if (n_rows >= (size_t(1) << 31)) throw HipError("register trace of 2^31 rows or more");
    const u32 n = (u32)n_rows;
    hipStream_t s = c.stream;
    u32* d_rows = c.alloc_u32(7 * n_rows);        // arena allocations are 256-byte aligned
    BF_HIP(hipMemcpyAsync(d_rows, trace7_h, 7 * n_rows * sizeof(u32), hipMemcpyHostToDevice, s));
    IngestCols cols;
    for (auto& p : cols.c) p = c.alloc_u32(n);
    unsigned long long* d_bad = (unsigned long long*)c.arena.alloc(256);
    BF_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), s));
    {
        ProfScope ps(s, "k_ingest_registers", 56.0 * n);
        hipLaunchKernelGGL(k_ingest_registers, dim3((n + IN_TILE - 1) / IN_TILE), dim3(256), 0, s, d_rows, n, cols, d_bad);
    }
    BF_HIP(hipGetLastError());
    unsigned long long h_bad = ~0ull;
    c.read_back(&h_bad, d_bad, sizeof h_bad);
    *first_bad = h_bad;
    return TraceSoA{cols.c[0], cols.c[1], cols.c[2], cols.c[3], cols.c[4], cols.c[5], cols.c[6], n};
}

}  // namespace bf
