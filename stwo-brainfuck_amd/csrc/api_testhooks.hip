// Test entries of libbfhip_testhooks.so only (Makefile: HOOKED); not declared in include/bfhip.h. The default library compiles this file to nothing.
#ifdef BFHIP_TEST_HOOKS
#include "../../include/bfhip.h"
#include "api_guard.h"
#include "prover.h"

using namespace bf;

// m31.h is compiled twice (x86 and gfx950) and the host-side sanitizer run sees the x86 half only: this entry runs ONE primitive of m31.h per
// element on the device, so that tests/test_gpu_field_edges.py can compare the gfx950 half with exact integers at the edge values. a, b, out: n elements of 4 words each (a QM31, or a scalar in word 0; a 64-bit operand = word 0 + 2^32 word 1).
// op: 0 m_add  1 m_sub  2 m_mul  3 m_mul_pre2(a, 2 b)  4 m_mul_pow2(a, b % 31)  5 m_inv  6 m_red4(a64)  7 m_canon(a64)  8 q_mul  9 q_mul_const(a, q_const(b))  10 q_inv
__global__ void __launch_bounds__(256) k_test_field_op(u32 op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 a0 = a[4 * i], a1 = a[4 * i + 1], a2 = a[4 * i + 2], a3 = a[4 * i + 3];
    const u32 b0 = b[4 * i], b1 = b[4 * i + 1], b2 = b[4 * i + 2], b3 = b[4 * i + 3];
    const u64 a64 = ((u64)a1 << 32) | a0;
    const Q31 x = q_make(a0, a1, a2, a3), y = q_make(b0, b1, b2, b3);
    Q31 r = q_zero();
    switch (op) {
        case 0: r.a.a = m_add(a0, b0); break;
        case 1: r.a.a = m_sub(a0, b0); break;
        case 2: r.a.a = m_mul(a0, b0); break;
        case 3: r.a.a = m_mul_pre2(a0, 2u * b0); break;
        case 4: r.a.a = m_mul_pow2(a0, b0 % 31u); break;
        case 5: r.a.a = m_inv(a0); break;
        case 6: r.a.a = m_red4(a64); break;
        case 7: r.a.a = m_canon(a64); break;
        case 8: r = q_mul(x, y); break;
        case 9: r = q_mul_const(x, q_const(y)); break;
        default: r = q_inv(x); break;
    }
    out[4 * i] = r.a.a; out[4 * i + 1] = r.a.b; out[4 * i + 2] = r.b.a; out[4 * i + 3] = r.b.b;
}
extern "C" int32_t bfhip_test_field_op(bfhip_ctx* ctx, uint32_t op, const uint32_t* a_d, const uint32_t* b_d, uint32_t* out_d, size_t n) {
    API_CTX(ctx)
    if (op > 10) throw HipError("bfhip_test_field_op: unknown op");
    if (!a_d || !b_d || !out_d) throw HipError("null argument");
    if (n == 0 || n > (size_t(1) << 28)) throw HipError("bfhip_test_field_op: n out of range");
    hipLaunchKernelGGL(k_test_field_op, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->c.stream, op, a_d, b_d, out_d, (u32)n);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
// Which constraint kernel bfhip_eval_constraints would launch for this storage layout under the current BFHIP_CONSTRAINT_GROUP_MIN_LOG: 0 = one lane per
// row, 16 = row-group kernel, 32 = paired row-group kernel. main_shift: shift of every main column and of every logUp column but the last (the last is full size).
extern "C" int32_t bfhip_test_constraint_group_rows(int32_t component, uint32_t log_size, uint32_t main_shift) {
    API_TRY
    if (component < 0 || component >= N_COMPONENTS) throw HipError("unknown component");
    ConstraintLaunch L{};
    for (u32 j = 0; j < n_main_cols(component); j++) L.trace[j].shift = main_shift;
    for (u32 j = 0; j + 4 < 4 * n_logup_cols(component); j++) L.inter[j].shift = main_shift;
    L.log_size = log_size;
    return (int32_t)constraint_group_rows(L, component);
    API_CATCH
}
// Overwrites one row-granular main column of a resident trace with n_rows host words (n_rows = the column's stored rows): the tests of the trace
// checks and of a proof's preflight build tables no register trace produces — one component corrupted alone, a chosen cell of a chosen table.
extern "C" int32_t bfhip_test_trace_set_column(bfhip_ctx* ctx, bfhip_trace* trace, uint32_t component, uint32_t column, const uint32_t* src_h, size_t n_rows) {
    API_CTX(ctx)
    if (!trace || !src_h) throw HipError("null argument");
    if (component >= (uint32_t)N_COMPONENTS || column >= trace->in.rows[component].size()) throw HipError("bad component/column");
    const DCol& col = trace->in.rows[component][column];
    if (n_rows != col.stored()) throw HipError("bfhip_test_trace_set_column: n_rows differs from the column's stored rows");
    ctx->c.sync();
    BF_HIP(hipMemcpyAsync(col.ptr, src_h, n_rows * sizeof(u32), hipMemcpyHostToDevice, ctx->c.stream));
    ctx->c.sync();
    return 0;
    API_CATCH
}
#endif
