// Between the interaction commitment and FRI (prover.h): the composition polynomial (ComponentProvers::compute_composition_polynomial),
// the out-of-domain samples (PolyOps::eval_at_point for every column and mask point) and the FRI quotients (compute_fri_quotients).
#include "prover.h"
#include <algorithm>

namespace bf {

HipProver::CompositionPlan HipProver::composition_prepare(std::vector<DTree>& trees, const BrainfuckProof& bp, const size_t* main_off, const size_t* inter_off, const Lookups& el) {
    CompositionPlan cp;
    for (int k = 0; k < N_COMPONENTS; k++) { cp.total += n_constraints(k); cp.max_log = std::max(cp.max_log, bp.log_sizes[k] + 1); }
    // The constraints are evaluated on CanonicCoset(log + 1) (stwo's component prover). At log_blowup_factor 1 that domain IS the trace LDE
    // domain and the kernels read the committed evaluations. Above 1 the LDE lives on CanonicCoset(log + b), which does not contain
    // CanonicCoset(log + 1) (odd powers of another generator): the main, interaction and IsFirst polynomials are evaluated on exactly that
    // coset by one extra batch of forward transforms, into arena memory that only the constraint kernels read.
    const bool own_domain = cfg.log_blowup != 1;
    std::vector<DCol> cd_src, cd_dst;
    IsFirstCols cd_is_first{}; cd_is_first.log_min = LOG_N_LANES; cd_is_first.log_max = log_max_rows;
    auto on_constraint_domain = [&](const DCol& poly) {
        if (poly.sliced()) throw HipError("composition: a row-sharded polynomial on the constraint domain");
        DCol e; e.log_size = poly.log_size + 1; e.shift = poly.shift; e.ptr = c.alloc_u32(e.stored());
        cd_src.push_back(poly); cd_dst.push_back(e);
        return e;
    };
    cp.acc.resize(cp.max_log + 1); cp.have.assign(cp.max_log + 1, false); cp.launches.resize(N_COMPONENTS);
    for (int k = 0; k < N_COMPONENTS; k++) {
        u32 log = bp.log_sizes[k], eval_log = log + 1;
        // shard group: an accumulator of a row-sharded size holds this rank's row range only (its components' interaction LDE columns
        // have the same size and are row-sharded too)
        const bool sl = slice_log(eval_log) && !replicate();      // replicate policy: every rank evaluates every row (0.7 ms of a fib19 proof) instead of exchanging rows -> columns
        if (!cp.have[eval_log]) {
            cp.acc[eval_log].log_size = eval_log; cp.acc[eval_log].lc = sl ? lc() : 0;
            for (int w = 0; w < 4; w++) cp.acc[eval_log].c[w] = sl ? alloc_slice(eval_log) : c.alloc_u32(size_t(1) << eval_log);
        }
        ConstraintLaunch L{};
        L.overwrite = cp.have[eval_log] ? 0u : 1u;      // the first component of a size writes the accumulator (no zero fill)
        cp.have[eval_log] = true;
        const u32 ni = 4 * n_logup_cols(k);
        if (!own_domain) {
            L.is_first = trees[0].evals[log_max_rows - log].ptr;
            for (u32 j = 0; j < n_main_cols(k); j++) L.trace[j] = trees[1].evals[main_off[k] + j].desc();
            for (u32 j = 0; j < ni; j++) L.inter[j] = trees[2].evals[inter_off[k] + j].desc();
        } else {
            const DCol& isf = trees[0].polys[log_max_rows - log];
            if (isf.shift != 0 || isf.log_size != log) throw HipError("composition: unexpected IsFirst polynomial layout");
            if (trees[0].is_first_closed) {
                // no coefficients to transform: IsFirst(log) on CanonicCoset(log + 1) in closed form, one column per size, one launch for all below
                u32*& e = cd_is_first.ptr[log - LOG_N_LANES];
                if (!e) e = c.alloc_u32(size_t(1) << eval_log);
                L.is_first = e;
            } else L.is_first = on_constraint_domain(isf).ptr;
            for (u32 j = 0; j < n_main_cols(k); j++) L.trace[j] = on_constraint_domain(trees[1].polys[main_off[k] + j]).desc();
            for (u32 j = 0; j < ni; j++) L.inter[j] = on_constraint_domain(trees[2].polys[inter_off[k] + j]).desc();
        }
        for (int w = 0; w < 4; w++) { const DCol& pv = trees[2].prev[inter_off[k] + ni - 4 + w]; L.inter_prev[w] = pv.ptr; }   // nullptr unless row-sharded
        if (sl) { L.row0 = (u32)slice_first(eval_log); L.n_rows = (u32)slice_cells(eval_log); }
        for (int w = 0; w < 4; w++) L.acc[w] = cp.acc[eval_log].c[w];
        L.el = el; L.log_size = log;
        // denom_inv[i] = 1 / coset_vanishing(CanonicCoset(log).coset, eval_domain.at(i)), i in {0, 1} (bit-reversal of 2 entries = identity)
        for (u32 i = 0; i < 2; i++) L.denom_inv[i] = m_inv(coset_vanishing_m(log, canonic_domain_at(eval_log, i)));
        cp.launches[k] = L;
    }
    if (own_domain) fft_cols(false, cd_src, cd_dst);      // on the stream behind the interaction tree (its polynomials), before the constraints
    if (own_domain && trees[0].is_first_closed) is_first_lde(c.stream, cd_is_first, 1, c.d_tw, c.d_itw, c.tw_root_log);
    return cp;
}
// the challenge-side fields of the 13 launches: coefficient powers and claimed sums
void HipProver::composition_challenge_fields(const BrainfuckProof& bp, u32 total, Q31 random_coeff, ConstraintLaunch* launches) {
    std::vector<Q31> powers(total);
    { Q31 cur = q_one(); for (u32 i = 0; i < total; i++) { powers[i] = cur; cur = q_mul(cur, random_coeff); } }
    u32 remaining = total;
    for (int k = 0; k < N_COMPONENTS; k++) {
        const u32 nc = n_constraints(k);
        // accum.columns(): this component takes the LAST nc remaining powers and uses them reversed (constraint 0 <-> highest)
        for (u32 j = 0; j < nc; j++) launches[k].coeff[j] = powers[remaining - 1 - j];
        remaining -= nc;
        launches[k].total_sum = bp.claimed_sums[k];
    }
}
// mailbox mode: the launch table is already in the ring and the kernels are on the stream; complete it (the caller posts)
void HipProver::composition_fill(const BrainfuckProof& bp, CompositionPlan& cp, Q31 random_coeff) {
    if (!cp.h_staged) throw HipError("composition_fill without a staged launch table");
    composition_challenge_fields(bp, cp.total, random_coeff, cp.h_staged);
}
// mbx != nullptr: the launches go onto the stream behind that mailbox with their challenge-side fields empty (composition_fill completes them)
void HipProver::compute_composition(std::vector<DTree>& trees, const BrainfuckProof& bp, CompositionPlan& cp, Q31 random_coeff, Mailbox* mbx) {
    const u32 max_log = cp.max_log;
    std::vector<DSecure>& acc = cp.acc;
    std::vector<bool>& have = cp.have;
    std::vector<ConstraintLaunch>& launches = cp.launches;
    if (!mbx) composition_challenge_fields(bp, cp.total, random_coeff, launches.data());
    c.stage_checkpoint();
    {   // the 13 evaluate_constraint_quotients_on_domain calls as ONE launch (air.hip: k_constraints_batch), one staging copy
        ConstraintBatch cb;
        constraint_batch_init(cb, launches.data(), N_COMPONENTS);
        const ConstraintLaunch* d_launches = nullptr; const ConstraintBatch* d_cb = nullptr;
        stage_blocks(mbx, [&] {
            d_launches = c.stage(launches.data(), launches.size());
            d_cb = c.stage(&cb, 1);
        });
        if (mbx) cp.h_staged = mbx->host(d_launches);
        eval_constraints_batch(c.stream, d_cb, cb, d_launches);
    }
    BF_HIP(hipGetLastError());
    // finalize (DomainEvaluationAccumulator::finalize): ascending sizes; the reference evaluates the running polynomial on the next
    // populated size, adds the evaluations and interpolates the sum. Interpolation is linear and evaluating a polynomial on a larger
    // domain is zero-extension of its coefficients (CirclePoly::extend), so interpolate(values + evaluate(prev)) =
    // interpolate(values) + extend(prev): one inverse transform per size and an addition over the *smaller* size — no forward
    // transform, no full-size accumulate. Exact field arithmetic: the coefficients are the same.
    // Shard group: the 4 coordinate columns of a row-sharded accumulator are gathered whole on their owners (coordinate w on rank
    // w mod count: rows -> columns, one grouped send-receive per size), which interpolate and merge them; ranks without a coordinate idle.
    if (!sharded() || replicate()) {
        // one process (or a group that replicates the transforms: every accumulator is complete on every rank): every size's accumulator is interpolated by the SAME batch of launches (the transforms are independent), then one
        // launch adds the smaller sizes' coefficients onto the largest size's
        std::vector<DCol> all_vals;
        std::vector<u32> logs;
        for (u32 log = max_log; log >= 1; log--) {
            if (!have[log]) continue;
            logs.push_back(log);
            for (int w = 0; w < 4; w++) { DCol v; v.ptr = acc[log].c[w]; v.log_size = log; v.shift = 0; all_vals.push_back(v); }
        }
        if (logs.size() > 13) throw HipError("composition: too many distinct sizes");
        fft_cols(true, all_vals, all_vals);
        AccumulateSizes as{};
        for (int w = 0; w < 4; w++) as.dst[w] = acc[logs[0]].c[w];
        for (size_t k = 1; k < logs.size(); k++) { for (int w = 0; w < 4; w++) as.src[k - 1][w] = acc[logs[k]].c[w]; as.log[k - 1] = logs[k]; }
        as.n = (u32)logs.size() - 1;
        accumulate_sizes(c.stream, as);
        BF_HIP(hipGetLastError());
        trees[3].polys.assign(all_vals.begin(), all_vals.begin() + 4);
        trees[3].owner.assign(4, OWNER_ALL);
        // replicate policy: the composition LDE is (virtually) row-sharded like every full-size column — commit_tree keys that on an owner entry
        if (replicate() && slice_log(all_vals[0].log_size + cfg.log_blowup)) for (int w = 0; w < 4; w++) trees[3].owner[w] = (u32)w % c.shard.count;
        return;
    }
    bool cur_have = false; std::vector<DCol> cur(4);
    bool cur_owned = false;               // `cur` is complete only on the coordinate's owner
    auto owner_of = [&](int w) { return (u32)w % c.shard.count; };
    for (u32 log = 1; log <= max_log; log++) {
        if (!have[log]) continue;
        std::vector<DCol> vals(4), mine_vals;
        const bool sl = acc[log].lc != 0;
        if (sl) {
            const size_t cells = slice_cells(log), bytes = cells * sizeof(u32), first = slice_first(log);
            std::vector<Xfer> sends, recvs;
            for (int w = 0; w < 4; w++) {
                vals[w].log_size = log; vals[w].shift = 0;
                sends.push_back({owner_of(w), acc[log].c[w] + first, bytes});
                if (owner_of(w) == c.shard.rank) {
                    vals[w].ptr = c.alloc_u32(size_t(1) << log);
                    for (u32 r = 0; r < c.shard.count; r++) recvs.push_back({r, vals[w].ptr + r * cells, bytes});
                    mine_vals.push_back(vals[w]);
                }
            }
            // receive order per peer must follow that peer's send order (coordinate ascending): regroup by coordinate within a peer
            std::stable_sort(recvs.begin(), recvs.end(), [](const Xfer& a, const Xfer& b) { return a.peer < b.peer; });
            c.shard.comm->exchange(c.stream, sends, recvs);
        } else {
            if (cur_owned) throw HipError("composition: a replicated accumulator above a row-sharded one");
            for (int w = 0; w < 4; w++) { vals[w].ptr = acc[log].c[w]; vals[w].log_size = log; vals[w].shift = 0; mine_vals.push_back(vals[w]); }
        }
        fft_cols(true, mine_vals, mine_vals);
        if (cur_have)
            for (int w = 0; w < 4; w++) if (!sl || owner_of(w) == c.shard.rank) accumulate(c.stream, vals[w].ptr, cur[w].ptr, 1u << cur[w].log_size);
        cur = vals; cur_have = true; cur_owned = sl;
    }
    trees[3].polys = cur;
    trees[3].owner.assign(4, OWNER_ALL);
    // The composition LDE is one size above the largest accumulator: it can be row-sharded (quotients, FRI first layer) although no
    // accumulator was. Then every rank holds the complete coefficients and coordinate w's owner alone extends them.
    if (cur_owned || (sharded() && slice_log(cur[0].log_size + cfg.log_blowup))) for (int w = 0; w < 4; w++) trees[3].owner[w] = owner_of(w);
}

HipProver::SamplePlan HipProver::sample_prepare(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask) {
    // Shard group: a sample is evaluated by ONE rank — the owner of the polynomial's coefficients, or for polynomials every rank holds the
    // rank (job index mod count), which splits that work — the others leave a zero and one max-reduce completes the array everywhere.
    SamplePlan sp;
    for (size_t t = 0; t < trees.size(); t++)
        for (size_t col = 0; col < trees[t].polys.size(); col++)
            for (u32 pt : mask[t][col]) {
                const u32 ji = sp.n_all++;
                const u32 owner = trees[t].owner.empty() ? OWNER_ALL : trees[t].owner[col];
                if (sharded() && ((owner == OWNER_ALL || replicate()) ? ji % c.shard.count : owner) != c.shard.rank) continue;
                const DCol& p = trees[t].polys[col];
                if (trees[t].is_first_closed) { sp.isf.push_back({p.log_size, pt, ji}); continue; }      // IsFirst(n) at the point in closed form: no coefficients
                EvalJob j{}; j.coeffs = p.ptr; j.log_n = p.log_size - p.shift; j.point = pt; j.factor_shift = p.shift; j.partial_off = sp.partial_off; j.out_idx = ji;
                sp.partial_off += j.log_n > 12 ? 1u << (j.log_n - 12) : 1u;
                sp.jobs.push_back(j);
            }
    return sp;
}
// factor tables: F[0] = y, F[1] = x, F[b] = double_x^(b-1)(x); 32 entries per point
void HipProver::sample_factors(const std::vector<PtQ>& points, uint4* factors) {
    for (size_t p = 0; p < points.size(); p++) {
        Q31 x = points[p].x;
        auto pk = [](Q31 q) { return make_uint4(q.a.a, q.a.b, q.b.a, q.b.b); };
        factors[p * 32 + 0] = pk(points[p].y);
        for (u32 b = 1; b < 32; b++) { factors[p * 32 + b] = pk(x); x = q_double_x(x); }
    }
}
// The sampling launches. The values go to the pinned bounce buffer (sample_results), or, in a shard group (completed by a max-reduce) or when
// they do not fit it, to d_out in HBM. mbx (mailbox order, one process per proof): the launches go onto the stream before the point is drawn,
// behind that mailbox, with the factor tables staged empty — h_factors is where sample_factors writes them before the host posts.
HipProver::SampleRun HipProver::sample_launch(const SamplePlan& sp, const std::vector<PtQ>& points, Mailbox* mbx) {
    SampleRun sr;
    const bool pinned = !sharded() && sp.n_all * sizeof(uint4) <= c.h_small_bytes - 4096;
    if (mbx && !pinned) throw HipError("sampling: too many samples for the pinned result buffer");
    std::vector<uint4> factors(points.size() * 32, make_uint4(0, 0, 0, 0));
    if (!mbx) sample_factors(points, factors.data());
    c.stage_checkpoint();
    const uint4* d_factors = nullptr; const EvalJob* d_jobs = nullptr; const IsFirstSample* d_isf = nullptr;
    stage_blocks(mbx, [&] {
        d_factors = c.stage(factors.data(), factors.size());     // through the pinned staging ring (no pageable copies)
        d_jobs = sp.jobs.empty() ? nullptr : c.stage(sp.jobs.data(), sp.jobs.size());
        d_isf = sp.isf.empty() ? nullptr : c.stage(sp.isf.data(), sp.isf.size());
    });
    if (mbx) sr.h_factors = mbx->host(d_factors);
    void* d_partials = c.arena.alloc(size_t(sp.partial_off ? sp.partial_off : 1) * sizeof(uint4));
    if (!pinned) {
        sr.d_out = (uint4*)c.arena.alloc(sp.n_all * sizeof(uint4));
        if (sharded()) BF_HIP(hipMemsetAsync(sr.d_out, 0, sp.n_all * sizeof(uint4), c.stream));
    }
    // pinned: the second stage writes the samples into the bounce buffer itself
    void* const d_samples = pinned ? (void*)(c.d_small_alias + 4096) : (void*)sr.d_out;
    eval_at_points(c.stream, d_jobs, (u32)sp.jobs.size(), sp.partial_off, d_factors, d_partials, d_samples);
    is_first_samples(c.stream, d_isf, (u32)sp.isf.size(), d_factors, d_samples, c.d_itw, c.tw_root_log);
    BF_HIP(hipGetLastError());
    if (sharded()) c.shard.comm->all_reduce_max_u32(c.stream, reinterpret_cast<u32*>(sr.d_out), size_t(sp.n_all) * 4);
    return sr;
}
// the values in job order -> pf.sampled_values (per tree, column and mask point)
void HipProver::sample_unpack(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const uint4* out, u32 n_all, StarkProof& pf) {
    pf.sampled_values.resize(trees.size());
    size_t ji = 0;
    for (size_t t = 0; t < trees.size(); t++) {
        pf.sampled_values[t].resize(trees[t].polys.size());
        for (size_t col = 0; col < trees[t].polys.size(); col++)
            for (size_t k = 0; k < mask[t][col].size(); k++, ji++) pf.sampled_values[t][col].push_back(q_make(out[ji].x, out[ji].y, out[ji].z, out[ji].w));
    }
    if (ji != n_all) throw HipError("sampling: job count mismatch");
}
void HipProver::sample(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const std::vector<PtQ>& points, StarkProof& pf, const SamplePlan& sp) {
    const SampleRun sr = sample_launch(sp, points, nullptr);
    std::vector<uint4> out;
    if (sr.d_out) { out.resize(sp.n_all); c.read_back(out.data(), sr.d_out, out.size() * sizeof(uint4)); }
    else c.sync();
    sample_unpack(trees, mask, sr.d_out ? out.data() : sample_results(), sp.n_all, pf);
}

std::vector<HipProver::QuotientGroup> HipProver::quotient_groups(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask) {
    struct FlatCol { DCol col; size_t tree, idx; };
    std::vector<FlatCol> flat;
    for (size_t t = 0; t < trees.size(); t++) for (size_t i = 0; i < trees[t].evals.size(); i++) flat.push_back({trees[t].evals[i], t, i});
    std::stable_sort(flat.begin(), flat.end(), [](const FlatCol& a, const FlatCol& b) { return a.col.log_size > b.col.log_size; });
    std::vector<QuotientGroup> groups;
    for (size_t i = 0; i < flat.size();) {
        size_t j = i; const u32 log = flat[i].col.log_size;
        while (j < flat.size() && flat[j].col.log_size == log) j++;
        QuotientGroup g; g.log = log;
        for (size_t k = i; k < j; k++) {
            const auto& pts = mask[flat[k].tree][flat[k].idx];
            if (pts.size() > 2) throw HipError("quotients: more than two mask points on a column");
            // shard group: a full-size column of the group is row-sharded exactly when the group is; a replicated one may also be complete
            // on every rank
            if (flat[k].col.sliced() != slice_log(log) && (flat[k].col.shift == 0 || flat[k].col.sliced())) throw HipError("quotients: inconsistent row-sharding in a size group");
            g.descs.push_back(flat[k].col.desc());
            ColSamples cs{};
            for (size_t s = 0; s < pts.size(); s++) { cs.point[cs.n] = pts[s]; cs.value[cs.n] = q_zero(); cs.n++; }
            g.cols.push_back(cs); g.src.push_back({flat[k].tree, flat[k].idx});
        }
        groups.push_back(std::move(g));
        i = j;
    }
    return groups;
}
// quotient_constants (host/quotients.h) of one size group. pf == nullptr: the sampled values stay zero — the tables' structure depends on
// the sample points only.
void HipProver::quotient_constants(QuotientGroup& g, const std::vector<PtQ>& points, const StarkProof* pf, Q31 random_coeff,
                                   std::vector<QuotientBatch>& batches, std::vector<QuotientEntry>& entries) {
    if (pf)
        for (size_t k = 0; k < g.cols.size(); k++)
            for (u32 s = 0; s < g.cols[k].n; s++) g.cols[k].value[s] = pf->sampled_values[g.src[k].first][g.src[k].second][s];
    batches.clear(); entries.clear();
    build_quotient_batches_indexed(g.cols.data(), g.cols.size(), points, random_coeff, batches, entries);
    quotient_entries_finish(batches.data(), batches.size(), entries.data(), g.descs.data());
}
// Launches: one per size group of >= 2^19 rows, largest first, each followed by an event (q_waits) — the FRI first-layer tree hashes level L
// as soon as the quotient of size L exists, on the partner stream, while the smaller groups are still being computed — and one launch for all
// the smaller groups together. (Shard group / host channel: one launch, no events.)
// Otherwise the LARGEST group is launched as soon as its own constants exist (four composition columns: a handful of products) and the host
// prepares the constants of the other groups — ~40 us of QM31 arithmetic, with the GPU idle behind the sampled values' round trip — while
// that launch runs; the rest follows as the second launch.
// mb0 / mb1 (mailbox order, one process per proof; pf == nullptr, random_coeff one): the largest group's launch goes behind mailbox mb0, the
// others' behind mb1, with the tables' structure staged (it depends on the sample points, known by now); quotients_fill writes the constants.
HipProver::QuotientRun HipProver::compute_quotients(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const std::vector<PtQ>& points,
                                                    const StarkProof* pf, Q31 random_coeff, std::vector<LevelWait>* q_waits, Mailbox* mb0, Mailbox* mb1) {
    QuotientRun qr;
    qr.groups = quotient_groups(trees, mask);
    mark("quotient columns sorted");
    const bool pipelined = (c.overlap & 2u) && q_waits && !sharded() && c.conv.merkle_channel == 0;
    const bool early_first = !pipelined && !sharded();
    std::vector<QuotientArgs> launches;
    std::vector<QuotientBatch> batches; std::vector<QuotientEntry> entries;
    auto stage_group = [&](QuotientGroup& g, Mailbox* m) {
        quotient_constants(g, points, pf, random_coeff, batches, entries);
        // shard group: the quotient of a row-sharded size is computed for this rank's row range only
        const bool sl = slice_log(g.log);
        DSecure q; q.log_size = g.log; q.lc = sl ? lc() : 0;
        for (int w = 0; w < 4; w++) q.c[w] = sl ? alloc_slice(g.log) : c.alloc_u32(size_t(1) << g.log);
        QuotientArgs a{};
        if (sl) { a.row0 = (u32)slice_first(g.log); a.n_rows = (u32)slice_cells(g.log); }
        a.batches = batches.empty() ? nullptr : c.stage(batches.data(), batches.size());
        a.entries = entries.empty() ? nullptr : c.stage(entries.data(), entries.size());
        if (m) { g.n_batches = batches.size(); g.n_entries = entries.size(); g.h_batches = a.batches ? m->host(a.batches) : nullptr; g.h_entries = a.entries ? m->host(a.entries) : nullptr; }
        a.n_batches = (u32)batches.size(); a.log = g.log; a.tw = c.d_tw; a.tw_total = 1u << c.tw_root_log;
        for (int w = 0; w < 4; w++) a.out[w] = q.c[w];
        launches.push_back(a);
        qr.out.push_back(q);
    };
    c.stage_checkpoint();
    size_t launched = 0;
    if (early_first && !qr.groups.empty()) {
        u32 nblocks = 0; const QuotientArgs* d_first = nullptr;
        stage_blocks(mb0, [&] {
            stage_group(qr.groups[0], mb0);
            nblocks = quotient_groups_layout(&launches[0], 1);
            d_first = c.stage(&launches[0], 1);
        });
        if (mb0) BF_HIP(hipEventRecord(c.ev[4], c.stream));       // the quotient phase's GPU time starts behind the mailbox, not in front of it
        accumulate_quotients(c.stream, d_first, 1, nblocks);
        mark("largest quotient group launched");
        launched = 1;
    }
    if (launched < qr.groups.size()) {
        std::vector<std::pair<u32, u32>> ranges;      // [first group, count)
        std::vector<u32> blocks;
        const QuotientArgs* d_groups = nullptr;
        stage_blocks(mb1, [&] {
            for (size_t g = launched; g < qr.groups.size(); g++) stage_group(qr.groups[g], mb1);
            u32 g = (u32)launched;
            if (pipelined) while (g < launches.size() && launches[g].log >= 19) { ranges.push_back({g, 1u}); g++; }
            if (g < launches.size()) ranges.push_back({g, (u32)launches.size() - g});
            for (auto& r : ranges) blocks.push_back(quotient_groups_layout(launches.data() + r.first, r.second));
            d_groups = c.stage(launches.data(), launches.size());      // one copy for the parameter blocks of every (remaining) size group
        });
        for (size_t k = 0; k < ranges.size(); k++) {
            accumulate_quotients(c.stream, d_groups + ranges[k].first, ranges[k].second, blocks[k]);
            if (pipelined) { hipEvent_t e = c.next_event(); BF_HIP(hipEventRecord(e, c.stream)); q_waits->push_back({(int)launches[ranges[k].first].log, e}); }
        }
    }
    BF_HIP(hipGetLastError());
    return qr;
}
// mailbox order: the constants over the staged tables; mb0 is posted as soon as the largest group's are in place, mb1 after the rest
// (computed while the first launch runs)
void HipProver::quotients_fill(QuotientRun& qr, const std::vector<PtQ>& points, const StarkProof& pf, Q31 random_coeff, Mailbox* mb0, Mailbox* mb1) {
    std::vector<QuotientBatch> batches; std::vector<QuotientEntry> entries;
    for (size_t gi = 0; gi < qr.groups.size(); gi++) {
        QuotientGroup& g = qr.groups[gi];
        quotient_constants(g, points, &pf, random_coeff, batches, entries);
        if (batches.size() != g.n_batches || entries.size() != g.n_entries) throw HipError("quotients: the batch structure changed between enqueue and fill");
        if (g.n_batches) memcpy(g.h_batches, batches.data(), batches.size() * sizeof(QuotientBatch));
        if (g.n_entries) memcpy(g.h_entries, entries.data(), entries.size() * sizeof(QuotientEntry));
        if (gi == 0) mb0->post();
    }
    mb1->post();
}

}  // namespace bf
