// Test shim over the CPU oracle (oracle/*.h, the checker): the FULL report of an AIR assertion on the trace domain — what
// bfhip_check_constraints / bfhip_trace_check (include/bfhip.h) return — for a caller-supplied table. The oracle's own C ABI
// (oracle_capi.cpp: orc_assert_constraints_table) stops at the first failing cell; tests/test_trace_check_cpu.py and
// tests/test_gpu_trace_check.py build this file with g++ into a temporary directory and load it with ctypes (tests/oracle_air_check.py).
// The definition stays the oracle's: every cell is evaluated by air.h's AssertEvaluator (first failing constraint and its value), and the
// per-constraint counts come from an evaluator that reads its masks THROUGH an AssertEvaluator (same columns, same previous-row map) and
// differs only in remembering every non-zero constraint instead of the first; the two are cross-checked cell by cell.
#include "json.h"
#include <cstdio>

using namespace orc;

static thread_local std::string g_err;

struct MaskEvaluator : EvalBase<MaskEvaluator, M31> {
    AssertEvaluator ae;   // mask reads only
    int ci = 0; u32 mask = 0;
    M31 is_first_mask() { return ae.is_first_mask(); }
    M31 next_trace_mask() { return ae.next_trace_mask(); }
    QM31 next_ext_mask0() { return ae.next_ext_mask0(); }
    void next_ext_mask0m1(QM31& c, QM31& p) { ae.next_ext_mask0m1(c, p); }
    void add_constraint(M31 c) { if (!c.is_zero()) mask |= 1u << ci; ci++; }
    void add_constraint(QM31 c) { if (!c.is_zero()) mask |= 1u << ci; ci++; }
    M31 cst(u32 k) { return M31(k); }
};

extern "C" {

const char* oac_last_error() { return g_err.c_str(); }

// rows: n_main row-granular columns of n_rows (a power of two) values, column-major. elems24: (z, alpha) of Memory, Instruction, Processor.
// inter: NULL = generate the logUp columns from `rows` (gen_interaction_trace), else 4 * n_logup full-size columns of 16 * n_rows cells,
// column-major. claimed_in: NULL = the generated claimed sum, else the total the last logUp column is closed on.
// Out: cells with a violation, the smallest violating storage index (UINT64_MAX: none), the lowest failing constraint there (-1) and its
// value, cells violating each constraint, the claimed sum used. Returns 0 (the verdict is in the outputs) or -1 (oac_last_error).
int oac_check(int component, const u32* rows, size_t n_rows, const u32* elems24, const u32* inter, const u32* claimed_in,
              u64* n_bad_cells, u64* first_bad_cell, int* first_bad_constraint, u32 first_bad_value[4], u64 bad_per_constraint[16], u32 claimed_out[4]) {
    try {
        if (component < 0 || component >= N_COMPONENTS) throw std::runtime_error("unknown component");
        if (n_rows == 0 || (n_rows & (n_rows - 1))) throw std::runtime_error("n_rows must be a power of two");
        Table t; t.init(N_MAIN_COLS[component], n_rows);
        for (size_t c = 0; c < t.cols.size(); c++) memcpy(t.cols[c].data(), rows + c * n_rows, n_rows * sizeof(u32));
        InteractionElements el;
        auto q = [&](int i) { return QM31::from_u32(elems24[4 * i], elems24[4 * i + 1], elems24[4 * i + 2], elems24[4 * i + 3]); };
        el.memory = LookupElements::make(q(0), q(1)); el.instruction = LookupElements::make(q(2), q(3)); el.processor = LookupElements::make(q(4), q(5));
        const u32 log = t.log_size();
        const size_t n = size_t(1) << log;
        std::vector<std::vector<u32>> main_cols;
        for (auto& c : t.cols) main_cols.push_back(broadcast16(c));
        QM31 claimed = QM31::zero();
        std::vector<std::vector<u32>> gen;
        std::vector<const u32*> tc, ic;
        if (inter) for (u32 k = 0; k < 4 * N_LOGUP_COLS[component]; k++) ic.push_back(inter + k * n);
        else { gen = gen_interaction_trace(component, t, el, &claimed); for (auto& c : gen) ic.push_back(c.data()); }
        if (claimed_in) claimed = QM31::from_u32(claimed_in[0], claimed_in[1], claimed_in[2], claimed_in[3]);
        else if (inter) throw std::runtime_error("caller-supplied logUp columns need a claimed sum");
        std::vector<u32> isf(n, 0); isf[0] = 1;
        for (auto& c : main_cols) tc.push_back(c.data());
        u64 bad = 0, first = ~u64(0), per[16] = {0};
        int first_con = -1; QM31 first_val = QM31::zero();
        bool inconsistent = false;
#pragma omp parallel
        {
            u64 l_bad = 0, l_first = ~u64(0), l_per[16] = {0};
            int l_con = -1; QM31 l_val = QM31::zero();
            bool l_inc = false;
#pragma omp for schedule(static)
            for (long long cell = 0; cell < (long long)n; cell++) {
                AssertEvaluator ae;
                ae.is_first_col = isf.data(); ae.trace_cols = tc.data(); ae.inter_cols = ic.data(); ae.row = (size_t)cell; ae.log_size = log; ae.total_sum = claimed;
                eval_component(component, ae, el);
                MaskEvaluator me;
                me.ae.is_first_col = isf.data(); me.ae.trace_cols = tc.data(); me.ae.inter_cols = ic.data(); me.ae.row = (size_t)cell; me.ae.log_size = log; me.total_sum = claimed;
                eval_component(component, me, el);
                if ((me.mask != 0) != (ae.failed >= 0) || (me.mask && __builtin_ctz(me.mask) != ae.failed) || me.ci != ae.ci) l_inc = true;
                if (ae.failed < 0) continue;
                l_bad++;
                for (int j = 0; j < 16; j++) l_per[j] += (me.mask >> j) & 1u;
                if ((u64)cell < l_first) { l_first = (u64)cell; l_con = ae.failed; l_val = ae.failed_value; }
            }
#pragma omp critical
            {
                bad += l_bad; inconsistent = inconsistent || l_inc;
                for (int j = 0; j < 16; j++) per[j] += l_per[j];
                if (l_first < first) { first = l_first; first_con = l_con; first_val = l_val; }
            }
        }
        if (inconsistent) throw std::runtime_error("the mask evaluator and AssertEvaluator disagree");
        *n_bad_cells = bad; *first_bad_cell = first; *first_bad_constraint = first_con;
        auto v = first_val.to_u32(); for (int k = 0; k < 4; k++) first_bad_value[k] = v[k];
        for (int j = 0; j < 16; j++) bad_per_constraint[j] = per[j];
        auto a = claimed.to_u32(); for (int k = 0; k < 4; k++) claimed_out[k] = a[k];
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; } catch (...) { g_err = "unknown"; return -1; }
}

}  // extern "C"
