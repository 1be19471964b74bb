// The relation program over a component's cells (include/bfhip.h "Relation programs": bfhip_relation_program_summary) — the front half of
// stwo's relation tracker for any AIR: every `add_to_relation(relation, multiplicity, values)` of a component, read from a program instead
// of one compiled branch per Brainfuck table (relations.hip: k_rel_flags, k_rel_emit). The back half — sort, segment, net, first yield and
// first use, report — is relations.hip's relation_aggregate, unchanged.
//
// Interpreter (k_relation_program<EMIT>): the core of program_interp.h, which k_air_program and k_logup_program run too, without its q
// half: one lane per evaluated row, one wave per workgroup, one register file. WORD does not copy a value: the pending tuple is seven register
// INDICES packed into one wave-uniform 64-bit scalar (8 bits each, newest lowest), taken from the instruction stream. ENTRY of another
// relation than the launch's only empties it.
// Per relation r, over the tables whose program has an ENTRY for r, rows concatenated in table order:
//   (1) EMIT = false: counts[row] = entries of r with a non-zero multiplicity at that row;
//   (2) exclusive_scan_u32: pos[row], and the total n;
//   (3) EMIT = true: the row's entries go to pos[row], pos[row] + 1, ... in program order — words, multiplicity, origin (table << 32 | row).
// So the entries stand in (table, row, program order) whatever the schedule: no atomics, integers only.
// bfhip_relation_program_multiplicities (include/bfhip.h "Lookup multiplicities") runs the same three steps for one relation with the looked-up
// table's launches in TARGET mode and hands the entries to relations.hip's relation_multiplicities instead.
#include "api_guard.h"
#include "relation_program.h"
#include "program_interp.h"
#include "../../include/bfhip.h"

namespace bf {

static constexpr u32 RP_SCAN_TILE = 2048;   // the tile of exclusive_scan_u32

// Staged in HBM, one per (relation, table). Addresses are kept as integers: read from address space 4 they arrive in SGPRs and are cast to
// global pointers.
struct RelProgLaunch {
    u64 code;            // bf_u32x4[n_instr]
    u64 cols;            // bf_u32x4[n_cols]: {pointer low, pointer high, read shift (row r reads word (r << row_shift) >> s_k), left shift}
    u64 counts;          // u32[rows] of this table inside the relation's row stream: written by EMIT = false
    u64 pos;             // u32[rows], the same place in the scanned stream: read by EMIT = true
    u64 w[REL_PROG_MAX_WORDS], num, origin;      // RelEntries
    u32 n_instr, rows, relation, n_words, table, n_m;      // n_m: host side only, the LDS size of the launch
    u32 target, pad_;    // TARGET launches only: which ENTRY of `relation`, in program order from 0, is the table side
};

// An evaluated row r, read at offset 0 only (bfhip_relation_program_create refuses offsets): column k holds it at (r << row_shift) >> s_k,
// the common part of the two shifts cancelled on the host
struct RelRow {
    static constexpr bool OFFSETS = false;
    u32 self;
    __device__ __forceinline__ u64 at0(const bf_u32x4 col) const { return (self << col.w) >> col.z; }
};

// m[r] of this lane, r taken from byte `k` of the packed pending tuple
__device__ __forceinline__ u32 rp_pending_reg(u64 pending, u32 k) { return (u32)(pending >> (8u * k)) & 0xffu; }

// WORD / ENTRY. TARGET (bfhip_relation_program_multiplicities, the looked-up table's launch): the a->target-th ENTRY of the relation is the
// table side. It gives an entry at EVERY row, whatever its multiplicity operand holds, with REL_TABLE_SIDE in the origin and multiplicity
// word 0; the ordinal is a wave-uniform counter. Every other ENTRY, and every launch with TARGET = false, is as the file header says.
template <bool EMIT, bool TARGET>
struct RelSink {
    static constexpr bool HAS_Q = false;
    const BF_CONSTANT RelProgLaunch* a;
    u32 row, relation, n_words, target;
    u32 at;                                                       // EMIT: where the row's entries start
    u64 pending = 0;                                              // wave-uniform: register indices, the newest in the low byte
    u32 count = 0;                                                // entries of `relation` with a non-zero multiplicity so far
    u32 ordinal = 0;                                              // TARGET: ENTRYs of `relation` so far
    static constexpr u32 OP = REL_WORD;
    __device__ __forceinline__ void op(const bf_u32x4 ins, const u32*, const u32*) { pending = (pending << 8) | ins.z; }
    __device__ __forceinline__ void other(const bf_u32x4 ins, const u32* m, const u32*) {      // REL_ENTRY: the validator admits nothing else
        if (ins.y == relation) {
            u32 mult = m[ins.z * PROGRAM_LANES];
            const bool side = TARGET && ordinal++ == target;
            if (side) mult = 0;
            if (mult != 0 || side) {
                if (EMIT) {
                    const u32 j = at + count;
#pragma unroll 1
                    for (u32 k = 0; k < n_words; k++)     // word k was pushed n_words - k WORDs ago
                        ((g_u32p)a->w[k])[j] = m[rp_pending_reg(pending, n_words - 1 - k) * PROGRAM_LANES];
                    ((g_u32p)a->num)[j] = mult;
                    ((BF_GLOBAL u64*)a->origin)[j] = (side ? REL_TABLE_SIDE : u64(0)) | ((u64)a->table << 32) | row;
                }
                count++;
            }
        }
        pending = 0;
    }
};

template <bool EMIT, bool TARGET>
__global__ void __launch_bounds__(PROGRAM_LANES) k_relation_program(const RelProgLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT RelProgLaunch* a = (const BF_CONSTANT RelProgLaunch*)(unsigned long long)ap;
    const u32 row = blockIdx.x * PROGRAM_LANES + threadIdx.x;
    if (row >= a->rows) return;
    RelSink<EMIT, TARGET> sink{a, row, a->relation, a->n_words, TARGET ? a->target : 0u, EMIT ? ((g_cu32p)a->pos)[row] : 0u};
    program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, nullptr, s_regs + threadIdx.x, nullptr, RelRow{row}, sink);
    if (!EMIT) ((g_u32p)a->counts)[row] = sink.count;
}

// What bfhip_relation_program_summary and bfhip_relation_program_multiplicities refuse about the list of tables, in the caller's name
static void rp_validate_tables(Ctx& c, const std::string& me, const bfhip_relation_program_table* tables, u32 n_tables, u32 n_relations) {
    if (n_tables < 1 || n_tables > 64) throw HipError(me + "1 to 64 tables, got " + std::to_string(n_tables));
    if (n_relations < 1 || n_relations > REL_PROG_MAX_RELATIONS) throw HipError(me + "1 to 16 relations, got " + std::to_string(n_relations));
    if (c.shard.count > 1) throw HipError(me + "a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    const u32 max_log = c.tw_root_log + 1 < 29 ? c.tw_root_log + 1 : 29;
    for (u32 t = 0; t < n_tables; t++) {
        const bfhip_relation_program_table& T = tables[t];
        const std::string at = me + "table " + std::to_string(t) + ": ";
        if (!T.program) throw HipError(at + "null program");
        const bfhip_relation_program& p = *T.program;
        if (p.n_relations != n_relations) throw HipError(at + "its program was created with " + std::to_string(p.n_relations) + " relations, the call names " + std::to_string(n_relations));
        for (u32 r = 0; r < n_relations; r++)
            if (p.relation_words[r] != tables[0].program->relation_words[r])
                throw HipError(at + "its program gives relation " + std::to_string(r) + " " + std::to_string(p.relation_words[r]) + " words, table 0's " + std::to_string(tables[0].program->relation_words[r]));
        if (T.log_size < 1 || T.log_size > max_log) throw HipError(at + "log_size must be in [1, max_log_domain = " + std::to_string(max_log) + "], got " + std::to_string(T.log_size));
        if (T.row_shift > T.log_size) throw HipError(at + "row_shift " + std::to_string(T.row_shift) + " above log_size " + std::to_string(T.log_size));
        if (!T.cols_h && p.n_cols) throw HipError(at + "null column array");
        for (u32 k = 0; k < p.n_cols; k++) {
            if (!T.cols_h[k]) throw HipError(at + "null column pointer (column " + std::to_string(k) + ")");
            if (T.col_shifts_h && T.col_shifts_h[k] > T.log_size) throw HipError(at + "column " + std::to_string(k) + " has shift " + std::to_string(T.col_shifts_h[k]) + " above log_size " + std::to_string(T.log_size));
        }
    }
    for (u32 r = 0; r < n_relations; r++) {
        u64 total = 0;
        for (u32 t = 0; t < n_tables; t++) total += (u64(1) << (tables[t].log_size - tables[t].row_shift)) * tables[t].program->entries_of[r];
        if (total > (u64(1) << 31)) throw HipError(me + "more than 2^31 entries (rows x ENTRY instructions) of relation " + std::to_string(r) + " in total");
    }
}

// Every distinct program's code once and every table's column descriptors, into the staging ring
struct RpStaged { const bf_u32x4* code[64] = {}; const bf_u32x4* cols[64] = {}; };
static void rp_stage_tables(Ctx& c, const bfhip_relation_program_table* tables, u32 n_tables, u32 n_relations, RpStaged& st) {
    const bf_u32x4** d_code = st.code;
    const bf_u32x4** d_cols = st.cols;
    // At the caps (64 programs of 4096 instructions) one call stages more than half the ring, so "recycle when half full" is not enough:
    // count what this call stages — the code of every distinct program, a descriptor block per table, two launch blocks per relation —
    // and recycle when it would not fit. At most 64 x 64 KiB + 64 x 4 KiB + 16 x 2 x 8 KiB = 4.5 MiB of the ring's 8.
    size_t need = 0;
    for (u32 t = 0; t < n_tables; t++) {
        const bfhip_relation_program& p = *tables[t].program;
        bool seen = false;
        for (u32 u = 0; u < t && !seen; u++) seen = tables[u].program == tables[t].program;
        if (!seen) need += Ctx::stage_round(p.code.size() * sizeof(u32));
        need += Ctx::stage_round((p.n_cols ? p.n_cols : 1) * sizeof(bf_u32x4));
    }
    need += size_t(n_relations) * 2 * Ctx::stage_round(n_tables * sizeof(RelProgLaunch));
    c.stage_checkpoint(need);
    {
        StageBatch sb(c);
        for (u32 t = 0; t < n_tables; t++) {
            const bfhip_relation_program_table& T = tables[t];
            const bfhip_relation_program& p = *T.program;
            for (u32 u = 0; u < t && !d_code[t]; u++) if (tables[u].program == T.program) d_code[t] = d_code[u];
            if (!d_code[t]) d_code[t] = reinterpret_cast<const bf_u32x4*>(c.stage(p.code.data(), p.code.size()));
            std::vector<bf_u32x4> cols(p.n_cols ? p.n_cols : 1, bf_u32x4{0, 0, 0, 0});
            for (u32 k = 0; k < p.n_cols; k++) {
                const u32 sk = T.col_shifts_h ? T.col_shifts_h[k] : T.row_shift;
                const unsigned long long ptr = (unsigned long long)T.cols_h[k];
                // (r << row_shift) >> s_k: one of the two shifts is left after cancelling
                cols[k] = bf_u32x4{(u32)ptr, (u32)(ptr >> 32), sk > T.row_shift ? sk - T.row_shift : 0u, T.row_shift > sk ? T.row_shift - sk : 0u};
            }
            d_cols[t] = c.stage(cols.data(), cols.size());
        }
        sb.end();
    }
}

}  // namespace bf

using namespace bf;

extern "C" int32_t bfhip_relation_program_summary(bfhip_ctx* ctx, const bfhip_relation_program_table* tables, uint32_t n_tables, uint32_t n_relations,
                                                  bfhip_relation_report* out, bfhip_relation_entry* entries_h, uint32_t cap_per_relation) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_relation_program_summary: ";
    if (!tables || !out || (!entries_h && cap_per_relation)) throw HipError(me + "null argument");
    rp_validate_tables(c, me, tables, n_tables, n_relations);
    const bfhip_relation_program& first = *tables[0].program;
    c.refuse_in_session("bfhip_relation_program_summary");
    hipStream_t s = c.stream;
    // like a proof: nothing of this context is in flight, and its per-proof memory starts empty; the bookkeeping is put back at the end
    c.sync();
    ArenaBorrow borrow(c);
    RpStaged staged;
    rp_stage_tables(c, tables, n_tables, n_relations, staged);
    const bf_u32x4* const* d_code = staged.code;
    const bf_u32x4* const* d_cols = staged.cols;
    for (u32 r = 0; r < n_relations; r++) {
        bfhip_relation_report& rep = out[r];
        rep = bfhip_relation_report{};
        rep.relation = r; rep.n_words = first.relation_words[r];
        u32 N = 0, row0[64] = {};
        for (u32 t = 0; t < n_tables; t++) if (tables[t].program->entries_of[r]) { row0[t] = N; N += 1u << (tables[t].log_size - tables[t].row_shift); }
        if (N == 0) continue;
        c.sync();
        c.arena.reset();
        u32* counts = c.alloc_u32(N); u32* pos = c.alloc_u32(N); u32* tot = c.alloc_u32(N / RP_SCAN_TILE + 3);
        RelProgLaunch L[64];
        u32 n_part = 0;
        for (u32 t = 0; t < n_tables; t++) {
            const bfhip_relation_program& p = *tables[t].program;
            if (!p.entries_of[r]) continue;
            RelProgLaunch& l = L[n_part++];
            l = RelProgLaunch{};
            l.code = (u64)d_code[t]; l.cols = (u64)d_cols[t]; l.counts = (u64)(counts + row0[t]); l.pos = (u64)(pos + row0[t]);
            l.n_instr = p.n_instr; l.rows = 1u << (tables[t].log_size - tables[t].row_shift); l.relation = r; l.n_words = rep.n_words; l.table = t;
            l.n_m = p.n_m;
        }
        const u32* d_n;
        {
            ProfScope ps(s, "relation_program_count", 0);
            const RelProgLaunch* d_L = c.stage(L, n_part);
            for (u32 i = 0; i < n_part; i++)
                hipLaunchKernelGGL((k_relation_program<false, false>), dim3((L[i].rows + PROGRAM_LANES - 1) / PROGRAM_LANES), dim3(PROGRAM_LANES), sizeof(u32) * PROGRAM_LANES * L[i].n_m, s, d_L + i);
            d_n = exclusive_scan_u32(s, counts, pos, tot, N);
        }
        u32 n = 0;
        c.read_back(&n, d_n, sizeof n);
        rep.n_entries = n;
        if (n == 0) continue;
        relation_aggregate(c, r, rep.n_words, n, cap_per_relation, rep, entries_h ? entries_h + size_t(r) * cap_per_relation : nullptr,
                           [&](const RelEntries& e) {
                               for (u32 i = 0; i < n_part; i++) {
                                   for (u32 k = 0; k < rep.n_words; k++) L[i].w[k] = (u64)e.w[k];
                                   L[i].num = (u64)e.num; L[i].origin = (u64)e.origin;
                               }
                               const RelProgLaunch* d_L = c.stage(L, n_part);
                               for (u32 i = 0; i < n_part; i++)
                                   hipLaunchKernelGGL((k_relation_program<true, false>), dim3((L[i].rows + PROGRAM_LANES - 1) / PROGRAM_LANES), dim3(PROGRAM_LANES), sizeof(u32) * PROGRAM_LANES * L[i].n_m, s, d_L + i);
                           },
                           "relation_program_emit");
    }
    c.sync();
    BF_HIP(hipGetLastError());
    borrow.end();
    return 0;
    API_CATCH
}

// The other direction (include/bfhip.h "Lookup multiplicities"): the same extraction with the looked-up table's launch in TARGET mode, then
// relations.hip's relation_multiplicities. One relation, so one pass over the arena.
extern "C" int32_t bfhip_relation_program_multiplicities(bfhip_ctx* ctx, const bfhip_relation_program_table* tables, uint32_t n_tables, uint32_t n_relations,
                                                         uint32_t relation, uint32_t target_table, uint32_t target_entry, uint32_t* out_d,
                                                         bfhip_multiplicity_report* report, bfhip_relation_entry* missing_h, uint32_t cap) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_relation_program_multiplicities: ";
    if (!tables || !out_d || !report || (!missing_h && cap)) throw HipError(me + "null argument");
    rp_validate_tables(c, me, tables, n_tables, n_relations);
    if (relation >= n_relations) throw HipError(me + "relation " + std::to_string(relation) + " out of range (the call names " + std::to_string(n_relations) + " relations)");
    if (target_table >= n_tables) throw HipError(me + "target table " + std::to_string(target_table) + " out of range (the call names " + std::to_string(n_tables) + " tables)");
    const u32 target_entries = tables[target_table].program->entries_of[relation];
    if (target_entry >= target_entries)
        throw HipError(me + "target entry " + std::to_string(target_entry) + ": the program of table " + std::to_string(target_table) + " has " + std::to_string(target_entries) +
                       " ENTRY instructions of relation " + std::to_string(relation));
    c.refuse_in_session("bfhip_relation_program_multiplicities");
    hipStream_t s = c.stream;
    const u32 r = relation, n_words = tables[0].program->relation_words[r];
    const u32 n_rows = 1u << (tables[target_table].log_size - tables[target_table].row_shift);
    // like a proof: nothing of this context is in flight, and its per-proof memory starts empty; the bookkeeping is put back at the end
    c.sync();
    ArenaBorrow borrow(c);
    RpStaged staged;
    rp_stage_tables(c, tables, n_tables, n_relations, staged);
    bfhip_multiplicity_report rep{};
    rep.relation = r; rep.n_words = n_words; rep.target_table = target_table; rep.target_entry = target_entry; rep.n_rows = n_rows;
    u32 N = 0, row0[64] = {};
    for (u32 t = 0; t < n_tables; t++) if (tables[t].program->entries_of[r]) { row0[t] = N; N += 1u << (tables[t].log_size - tables[t].row_shift); }
    c.arena.reset();
    u32* counts = c.alloc_u32(N); u32* pos = c.alloc_u32(N); u32* tot = c.alloc_u32(N / RP_SCAN_TILE + 3);
    RelProgLaunch L[64];
    u32 n_part = 0, target_part = 0;
    for (u32 t = 0; t < n_tables; t++) {
        const bfhip_relation_program& p = *tables[t].program;
        if (!p.entries_of[r]) continue;
        if (t == target_table) target_part = n_part;
        RelProgLaunch& l = L[n_part++];
        l = RelProgLaunch{};
        l.code = (u64)staged.code[t]; l.cols = (u64)staged.cols[t]; l.counts = (u64)(counts + row0[t]); l.pos = (u64)(pos + row0[t]);
        l.n_instr = p.n_instr; l.rows = 1u << (tables[t].log_size - tables[t].row_shift); l.relation = r; l.n_words = n_words; l.table = t;
        l.n_m = p.n_m; l.target = target_entry;
    }
    auto launch = [&](bool emit) {
        const RelProgLaunch* d_L = c.stage(L, n_part);
        for (u32 i = 0; i < n_part; i++) {
            const dim3 grid((L[i].rows + PROGRAM_LANES - 1) / PROGRAM_LANES);
            const size_t lds = sizeof(u32) * PROGRAM_LANES * L[i].n_m;
            if (i == target_part) {
                if (emit) hipLaunchKernelGGL((k_relation_program<true, true>), grid, dim3(PROGRAM_LANES), lds, s, d_L + i);
                else hipLaunchKernelGGL((k_relation_program<false, true>), grid, dim3(PROGRAM_LANES), lds, s, d_L + i);
            } else {
                if (emit) hipLaunchKernelGGL((k_relation_program<true, false>), grid, dim3(PROGRAM_LANES), lds, s, d_L + i);
                else hipLaunchKernelGGL((k_relation_program<false, false>), grid, dim3(PROGRAM_LANES), lds, s, d_L + i);
            }
        }
    };
    const u32* d_n;
    {
        ProfScope ps(s, "relation_multiplicities_count", 0);
        launch(false);
        d_n = exclusive_scan_u32(s, counts, pos, tot, N);
    }
    u32 n = 0;
    c.read_back(&n, d_n, sizeof n);      // n >= n_rows >= 1: the table side gives an entry at every row
    relation_multiplicities(c, r, n_words, n, n_rows, out_d, cap, rep, missing_h, [&](const RelEntries& e) {
        for (u32 i = 0; i < n_part; i++) {
            for (u32 k = 0; k < n_words; k++) L[i].w[k] = (u64)e.w[k];
            L[i].num = (u64)e.num; L[i].origin = (u64)e.origin;
        }
        launch(true);
    });
    c.sync();
    BF_HIP(hipGetLastError());
    borrow.end();
    *report = rep;
    return 0;
    API_CATCH
}
