// C ABI (include/bfhip.h) of the prover (prover.h): resident traces, the proving and verifying entry points, the host-only compiler / VM /
// table builders and the per-context profiler. The error boundary is api_guard.h's, like every other entry point's.
#include "prover.h"
#include "api_guard.h"
#include "host/verifier.h"
#include <cstdio>

using namespace bf;

// Selects where bfhip_trace_create / bfhip_prove_brainfuck of THIS context build the 13 component tables: 1 = gfx950 kernels (default), 0 = host builders.
extern "C" int32_t bfhip_ctx_set_table_builder(bfhip_ctx* ctx, int32_t on_gpu) { API_TRY if (!ctx) throw HipError("null context"); ctx->c.tables_on_gpu = on_gpu != 0; return 0; API_CATCH }
// Downloads one row-granular column of a resident trace (tests: GPU tables == host tables).
extern "C" int32_t bfhip_trace_column(bfhip_ctx* ctx, const bfhip_trace* t, uint32_t component, uint32_t column, uint32_t* out_h, size_t cap, size_t* n_rows) {
    API_TRY
    if (!ctx || !t || !n_rows) { bfhip_set_error("null argument"); return -1; }
    if (component >= N_COMPONENTS || column >= t->in.rows[component].size()) { bfhip_set_error("bad component/column"); return -1; }
    const DCol& col = t->in.rows[component][column];
    *n_rows = col.stored();
    if (out_h) {
        if (cap < col.stored()) { bfhip_set_error("capacity"); return -2; }
        ctx->c.bind();
        BF_HIP(hipMemcpyAsync(out_h, col.ptr, col.stored() * sizeof(u32), hipMemcpyDeviceToHost, ctx->c.stream));
        ctx->c.sync();
    }
    return 0;
    API_CATCH
}

// A proof that fails on one rank of a shard group must not leave the others waiting for its next collective: the transport is told to give
// up (in-process: the rendezvous object is marked failed and every waiting rank throws; RCCL: ncclCommAbort). The group is unusable afterwards.
static void release_group_after_failure(bfhip_ctx* ctx) {
    if (ctx && ctx->c.shard.count > 1 && ctx->c.shard.comm) {
        try { ctx->c.shard.comm->abort(); } catch (...) {}
        // every stream of the context may still carry work of the failed proof (the main stream's handle, the side stream, both partners)
        Ctx& c = ctx->c;
        for (hipStream_t st : {c.stream, c.id_main, c.stream2, c.aux[0], c.aux[1]}) if (st) (void)hipStreamSynchronize(st);
    }
}

static void fill_outputs(HipProver& pv, const BrainfuckProof& bp, char** proof_json, size_t* proof_len, char** transcript, double* phase_seconds) {
    if (proof_json) {
        std::string js = proof_to_json(bp, pv.c.conv.merkle_channel == 1);
        *proof_json = (char*)malloc(js.size() + 1);
        memcpy(*proof_json, js.c_str(), js.size() + 1);
        if (proof_len) *proof_len = js.size();
    }
    if (transcript) { *transcript = (char*)malloc(pv.transcript.size() + 1); memcpy(*transcript, pv.transcript.c_str(), pv.transcript.size() + 1); }
    if (phase_seconds) {
        const PhaseTimes& t = pv.tm;
        double v[10] = {t.preprocessed, t.tables, t.main_trace, t.interaction, t.composition, t.oods, t.quotients, t.fri, t.decommit, t.total};
        memcpy(phase_seconds, v, sizeof v);
    }
}

static int32_t trace_create_common(bfhip_ctx* ctx, const std::vector<Registers>& vm_trace, const std::vector<u32>& ins, bfhip_trace** out,
                                   uint32_t log_sizes[13], uint64_t* n_steps, uint64_t* main_cells, uint64_t* interaction_cells) {
    if (vm_trace.empty()) throw HipError("EmptyTrace");   // TraceError::EmptyTrace (memory/table.rs:83-86)
    auto* t = new bfhip_trace();
    try { HipProver::upload_trace(ctx->c, vm_trace, ins, t->in, /*use_arena=*/false, /*on_gpu=*/ctx->c.tables_on_gpu); } catch (...) { t->in.release(); delete t; throw; }
    if (log_sizes) memcpy(log_sizes, t->in.log_sizes, sizeof(u32) * N_COMPONENTS);
    if (n_steps) *n_steps = t->in.n_steps;
    if (main_cells) *main_cells = t->in.main_cells;
    if (interaction_cells) *interaction_cells = t->in.interaction_cells;
    *out = t;
    return 0;
}
extern "C" int32_t bfhip_trace_create_ram(bfhip_ctx* ctx, const char* code, const uint8_t* input, size_t n_input, size_t ram_size, bfhip_trace** out,
                                           uint32_t log_sizes[13], uint64_t* n_steps, uint64_t* main_cells, uint64_t* interaction_cells) {
    API_TRY
    if (!ctx) throw HipError("null context");
    if (!code || !out || (!input && n_input)) throw HipError("null argument");
    ctx->c.bind();
    std::vector<u32> ins = compile(code);
    Machine m(ins, input ? std::vector<u8>(input, input + n_input) : std::vector<u8>(), ram_size ? ram_size : Machine::DEFAULT_RAM_SIZE);
    m.execute();
    return trace_create_common(ctx, m.trace, ins, out, log_sizes, n_steps, main_cells, interaction_cells);
    API_CATCH
}
extern "C" int32_t bfhip_trace_create(bfhip_ctx* ctx, const char* code, const uint8_t* input, size_t n_input, bfhip_trace** out,
                                       uint32_t log_sizes[13], uint64_t* n_steps, uint64_t* main_cells, uint64_t* interaction_cells) {
    return bfhip_trace_create_ram(ctx, code, input, n_input, 0, out, log_sizes, n_steps, main_cells, interaction_cells);
}
// prove_brainfuck(&Machine) receives an executed machine (mod.rs:471-473): its register trace (mod.rs:508) and its program.
extern "C" int32_t bfhip_trace_create_from_registers(bfhip_ctx* ctx, const uint32_t* trace7, size_t n_rows, const uint32_t* code_words, size_t n_code,
                                                      bfhip_trace** out, uint32_t log_sizes[13], uint64_t* main_cells, uint64_t* interaction_cells) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    if (!trace7 || n_rows == 0) throw HipError("EmptyTrace");
    if (!code_words || n_code == 0) throw HipError("empty program");
    // GPU table builder (default): the rows are transposed and checked on the device (ingest.hip); otherwise the host path as it was
    auto* t = new bfhip_trace();
    try { HipProver::upload_registers(ctx->c, trace7, n_rows, code_words, n_code, t->in, /*use_arena=*/false, /*with_place=*/false); } catch (...) { t->in.release(); delete t; throw; }
    if (log_sizes) memcpy(log_sizes, t->in.log_sizes, sizeof(u32) * N_COMPONENTS);
    if (main_cells) *main_cells = t->in.main_cells;
    if (interaction_cells) *interaction_cells = t->in.interaction_cells;
    *out = t;
    return 0;
    API_CATCH
}
extern "C" int32_t bfhip_trace_destroy(bfhip_ctx* ctx, bfhip_trace* t) { API_TRY (void)ctx; if (t) { t->in.release(); delete t; } return 0; API_CATCH }

extern "C" int32_t bfhip_prove_trace(bfhip_ctx* ctx, const bfhip_trace* trace, uint32_t log_max_rows, char** proof_json, size_t* proof_len,
                                      char** transcript, double* phase_seconds) {
    API_TRY
    try {
        if (!ctx) throw HipError("null context");
        if (!trace) throw HipError("null trace");
        ctx->c.bind();
        HipProver pv(ctx->c, log_max_rows);
        pv.want_transcript = transcript != nullptr;
        BrainfuckProof bp = pv.prove(trace->in);
        fill_outputs(pv, bp, proof_json, proof_len, transcript, phase_seconds);
        return 0;
    } catch (...) { release_group_after_failure(ctx); throw; }
    API_CATCH
}

extern "C" int32_t bfhip_prove_brainfuck(bfhip_ctx* ctx, const char* code, const uint8_t* input, size_t n_input, uint32_t log_max_rows,
                                          char** proof_json, size_t* proof_len, char** transcript, double* phase_seconds) {
    API_TRY
    TraceInput in;
    try {
        if (!ctx) throw HipError("null context");
        if (!code) throw HipError("null program text");
        if (!input && n_input) throw HipError("null argument");
        ctx->c.bind();
        HipProver pv(ctx->c, log_max_rows);
        pv.want_transcript = transcript != nullptr;
        // VM run + table build + upload happen while the GPU already works on the preprocessed commitment
        BrainfuckProof bp = pv.prove([&]() -> const TraceInput& {
            std::vector<u32> ins = compile(code);
            Machine m(ins, std::vector<u8>(input, input + n_input));
            m.execute();
            HipProver::upload_trace(ctx->c, m.trace, ins, in, /*use_arena=*/true, /*on_gpu=*/ctx->c.tables_on_gpu);
            return in;
        });
        fill_outputs(pv, bp, proof_json, proof_len, transcript, phase_seconds);
        in.release();
        return 0;
    } catch (...) { release_group_after_failure(ctx); in.release(); throw; }
    API_CATCH
}
// prove_brainfuck(&Machine) in one call: the executed machine's register rows and program words in, the proof out. Ingestion and table build
// are enqueued by the lazy producer, i.e. behind the preprocessed commitment the GPU is already working on; the tables live in the proof's arena.
extern "C" int32_t bfhip_prove_registers(bfhip_ctx* ctx, const uint32_t* trace7_h, size_t n_rows, const uint32_t* code_words_h, size_t n_code,
                                          uint32_t log_max_rows, char** proof_json, size_t* proof_len, char** transcript, double* phase_seconds) {
    API_TRY
    TraceInput in;
    try {
        if (!ctx) throw HipError("null context");
        if (!trace7_h || n_rows == 0) throw HipError("EmptyTrace");
        if (n_rows >= (size_t(1) << 31)) throw HipError("bfhip_prove_registers: n_rows >= 2^31");
        if (!code_words_h || n_code == 0) throw HipError("empty program");
        ctx->c.bind();
        HipProver pv(ctx->c, log_max_rows);
        pv.want_transcript = transcript != nullptr;
        BrainfuckProof bp = pv.prove([&]() -> const TraceInput& {
            HipProver::upload_registers(ctx->c, trace7_h, n_rows, code_words_h, n_code, in, /*use_arena=*/true, /*with_place=*/true);
            return in;
        });
        fill_outputs(pv, bp, proof_json, proof_len, transcript, phase_seconds);
        in.release();
        return 0;
    } catch (...) { release_group_after_failure(ctx); in.release(); throw; }
    API_CATCH
}
extern "C" void bfhip_free_host(void* p) { free(p); }
extern "C" int32_t bfhip_ctx_last_proof_flags(bfhip_ctx* ctx, uint32_t* flags) {
    API_TRY
    if (!ctx || !flags) throw HipError("null argument");
    *flags = ctx->c.last_proof_flags;
    return 0;
    API_CATCH
}
// on: keep the preprocessed tree of this context's next proof and reuse it while it matches (prover.h: PreprocessedCache). off: free the kept tree.
extern "C" int32_t bfhip_ctx_reuse_preprocessed(bfhip_ctx* ctx, int32_t on) {
    API_TRY
    if (!ctx) throw HipError("null context");
    if (on) { preprocessed_cache_of(ctx->c).enabled = true; return 0; }
    if (ctx->c.pre_cache) { if (ctx->c.stream) (void)hipStreamSynchronize(ctx->c.stream); preprocessed_cache_drop(ctx->c); }
    return 0;
    API_CATCH
}

// verify_brainfuck (mod.rs:738-797). Host only. 0 = accepted, 1 = rejected (reason in err), -1 = internal error.
extern "C" int32_t bfhip_verify_brainfuck_pcs(const char* proof_json, size_t proof_len, uint32_t log_max_rows, const bfhip_conventions* conv,
                                              const bfhip_pcs_config* pcs, char* err, size_t err_cap) {
    API_TRY
    PcsConfig cfg = pcs_config_from(pcs);
    Conventions cv;
    if (conv) {
        if (conv->merkle_node_hash > 1 || conv->mix_u64 > 1 || conv->logup_mask_order > 1 || conv->merkle_channel > 1) throw HipError("unknown convention value");
        cv.merkle_node_hash = conv->merkle_node_hash; cv.mix_u64 = conv->mix_u64; cv.logup_mask_order = conv->logup_mask_order; cv.merkle_channel = conv->merkle_channel;
    }
    std::string reason;
    try { BrainfuckProof bp = proof_from_json(proof_json, proof_len, cv.merkle_channel == 1); reason = verify_brainfuck(bp, log_max_rows, cv, cfg); }
    catch (const std::exception& e) { reason = std::string("InvalidStructure: ") + e.what(); }
    if (err && err_cap) snprintf(err, err_cap, "%s", reason.c_str());
    return reason.empty() ? 0 : 1;
    API_CATCH
}
extern "C" int32_t bfhip_verify_brainfuck_conv(const char* proof_json, size_t proof_len, uint32_t log_max_rows, const bfhip_conventions* conv, char* err, size_t err_cap) {
    return bfhip_verify_brainfuck_pcs(proof_json, proof_len, log_max_rows, conv, nullptr, err, err_cap);
}

extern "C" int32_t bfhip_verify_brainfuck(const char* proof_json, size_t proof_len, uint32_t log_max_rows, char* err, size_t err_cap) {
    return bfhip_verify_brainfuck_conv(proof_json, proof_len, log_max_rows, nullptr, err, err_cap);
}

// ---- host-only entry points (no GPU needed): compiler, VM and table builders of the drop-in's host side ---------------------------
extern "C" int32_t bfhip_host_compile(const char* code, uint32_t* out, size_t cap, size_t* n) {
    API_TRY
    if (!n || (!out && cap)) throw HipError("null argument");
    auto ins = compile(code); *n = ins.size(); if (ins.size() > cap) { bfhip_set_error("capacity"); return -2; } memcpy(out, ins.data(), 4 * ins.size()); return 0;
    API_CATCH
}
extern "C" int32_t bfhip_host_run_ram(const char* code, const uint8_t* input, size_t n_input, size_t ram_size, uint8_t* out, size_t out_cap, size_t* n_out,
                                       uint32_t* trace7, size_t trace_cap_rows, size_t* n_rows) {
    API_TRY
    if (!input && n_input) throw HipError("null argument");
    Machine m(compile(code), std::vector<u8>(input, input + n_input), ram_size ? ram_size : Machine::DEFAULT_RAM_SIZE);
    m.execute();
    if (n_out) *n_out = m.output.size();
    if (out && m.output.size() <= out_cap) memcpy(out, m.output.data(), m.output.size());
    if (n_rows) *n_rows = m.trace.size();
    if (trace7 && m.trace.size() <= trace_cap_rows)
        for (size_t i = 0; i < m.trace.size(); i++) { const Registers& r = m.trace[i]; u32 v[7] = {r.clk, r.ip, r.ci, r.ni, r.mp, r.mv, r.mvi}; memcpy(trace7 + 7 * i, v, 28); }
    return 0;
    API_CATCH
}
extern "C" int32_t bfhip_host_run(const char* code, const uint8_t* input, size_t n_input, uint8_t* out, size_t out_cap, size_t* n_out,
                                   uint32_t* trace7, size_t trace_cap_rows, size_t* n_rows) {
    return bfhip_host_run_ram(code, input, n_input, 0, out, out_cap, n_out, trace7, trace_cap_rows, n_rows);
}
// Table of `component` (0..12, claim order of mod.rs:85-99) built from an explicit register trace (7 u32 per row) and compiled program.
extern "C" int32_t bfhip_host_table(const uint32_t* trace7, size_t n_trace, const uint32_t* code, size_t n_code, int32_t component,
                                     uint32_t* out_row_major, size_t cap, size_t* n_rows, size_t* n_cols) {
    API_TRY
    if (!n_rows || !n_cols) throw HipError("null argument");
    std::vector<Registers> tr(n_trace);
    for (size_t i = 0; i < n_trace; i++) { const u32* v = trace7 + 7 * i; tr[i] = Registers{v[0], v[1], v[2], v[3], v[4], v[5], v[6]}; }
    std::vector<u32> ins(code, code + n_code);
    Table t;
    switch (component) {
        case C_MEMORY: t = memory_table(tr); break;
        case C_INSTRUCTION: t = instruction_table(tr, ins); break;
        case C_PROGRAM: t = program_table(ins); break;
        case C_PROCESSOR: t = processor_table(tr); break;
        case C_JNZ: t = jump_table(tr, OP_JNZ); break;
        case C_JZ: t = jump_table(tr, OP_JZ); break;
        case C_INPUT: t = instruction_sub_table(tr, OP_READCHAR); break;
        case C_LEFT: t = instruction_sub_table(tr, OP_LEFT); break;
        case C_MINUS: t = instruction_sub_table(tr, OP_MINUS); break;
        case C_OUTPUT: t = instruction_sub_table(tr, OP_PUTCHAR); break;
        case C_PLUS: t = instruction_sub_table(tr, OP_PLUS); break;
        case C_RIGHT: t = instruction_sub_table(tr, OP_RIGHT); break;
        case C_EOE: t = eoe_table(tr); break;
        default: bfhip_set_error("bad component"); return -1;
    }
    if (t.n_rows == 0) throw HipError("EmptyTrace");      // TraceError::EmptyTrace (memory/table.rs:83-86 and the six analogues)
    *n_rows = t.n_rows; *n_cols = t.cols.size();
    if (out_row_major) {
        if (t.n_rows * t.cols.size() > cap) { bfhip_set_error("capacity"); return -2; }
        for (size_t r = 0; r < t.n_rows; r++) for (size_t c = 0; c < t.cols.size(); c++) out_row_major[r * t.cols.size() + c] = t.cols[c][r];
    }
    return 0;
    API_CATCH
}
// Profiler state is per stream, i.e. per context: contexts on other threads are not affected (prof.hip).
extern "C" int32_t bfhip_profile_enable(bfhip_ctx* ctx, int32_t mode) {
    API_TRY if (!ctx) throw HipError("null context"); if (mode < 0 || mode > 2) throw HipError("bad profile mode"); ctx->c.bind(); ctx->c.ensure_side(); sync_both(ctx->c); prof_enable(ctx->c.stream, mode); prof_enable(ctx->c.stream2, mode); for (auto a : ctx->c.aux) if (a) prof_enable(a, mode); return 0;
    API_CATCH
}
extern "C" int32_t bfhip_profile_reset(bfhip_ctx* ctx) {
    API_CTX(ctx) sync_both(ctx->c); prof_reset(ctx->c.stream); if (ctx->c.stream2) prof_reset(ctx->c.stream2); for (auto a : ctx->c.aux) if (a) prof_reset(a); return 0;
    API_CATCH
}
extern "C" int32_t bfhip_profile_report(bfhip_ctx* ctx, char** json) {
    API_CTX(ctx) if (!json) throw HipError("null argument"); sync_both(ctx->c); hipStream_t ss[4] = {ctx->c.stream, ctx->c.stream2, ctx->c.aux[0], ctx->c.aux[1]}; std::string s = prof_report_json(ss, 4); *json = (char*)malloc(s.size() + 1); memcpy(*json, s.c_str(), s.size() + 1); return 0;
    API_CATCH
}
