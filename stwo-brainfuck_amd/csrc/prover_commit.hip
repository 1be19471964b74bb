// The commit phase of the device prover (prover.h): batched transforms over heterogeneous columns, Merkle planning and launching, which
// columns of a shard group are cut into row ranges, tree commitments (CommitmentTreeProver::new), the trace upload and the preprocessed tree
// with its two ways of being kept: per context (PreprocessedCache) and per pool batch (SharedPreprocessed).
#include "prover.h"
#include <algorithm>

namespace bf {

#ifdef BFHIP_TEST_HOOKS
// libbfhip_testhooks.so only (see the end of this file): with the capture on, every tree commitment of a proof leaves a copy of its
// polynomials on the host, in commit order. The copies are enqueued behind the launches that produce the coefficients; the reader waits.
struct PolyCapture {
    struct Poly { u32 log_size, shift; std::vector<u32> stored; };
    bool on = false; int saved_mailbox_mode = -1;
    std::vector<std::vector<Poly>> trees;
};
static void capture_tree(Ctx& c, const DTree& t) {
    if (!c.capture || !c.capture->on) return;
    c.capture->trees.emplace_back();
    auto& out = c.capture->trees.back();
    out.resize(t.polys.size());
    for (size_t i = 0; i < t.polys.size(); i++) {
        const DCol& p = t.polys[i];
        if (!p.ptr || p.sliced()) throw HipError("bfhip_test_capture_polys: a polynomial this rank does not hold whole");
        out[i].log_size = p.log_size; out[i].shift = p.shift; out[i].stored.resize(p.stored());
        BF_HIP(hipMemcpyAsync(out[i].stored.data(), p.ptr, p.stored() * sizeof(u32), hipMemcpyDeviceToHost, c.stream));
    }
}
#endif

// ---- batched FFT over heterogeneous columns: group by (size, storage) --------------------------------------------------
// Two steps so that a caller can put the plan's staging into a batch shared with what follows (fft_prepare inside a StageBatch,
// fft_launch after its end()): pointer arrays and the pass table of every size group reach the device in one copy.
FftPlan HipProver::fft_prepare(bool inverse, const std::vector<DCol>& src, const std::vector<DCol>& dst) {
    std::map<std::pair<u32, u32>, std::vector<size_t>> groups;   // (dst log_size, shift) -> indices
    for (size_t i = 0; i < dst.size(); i++) groups[{dst[i].log_size, dst[i].shift}].push_back(i);
    struct Job { size_t off, n; u32 log, src_log, sh; };
    std::vector<Job> jobs; std::vector<const u32*> ptrs;
    for (auto it = groups.rbegin(); it != groups.rend(); ++it) {
        const auto& idx = it->second;
        u32 log = it->first.first, sh = it->first.second;
        // split further by source size (forward transforms may extend from different coefficient sizes)
        std::map<u32, std::vector<size_t>> by_src;
        for (size_t i : idx) by_src[src[i].log_size].push_back(i);
        for (auto& kv : by_src) {
            jobs.push_back({ptrs.size(), kv.second.size(), log, kv.first, sh});
            for (size_t i : kv.second) ptrs.push_back(src[i].ptr);
            for (size_t i : kv.second) ptrs.push_back(dst[i].ptr);
        }
    }
    FftPlan plan;
    if (jobs.empty()) return plan;
    StageBatch sb(c);
    const u32* const* d_ptrs = c.stage(ptrs.data(), ptrs.size());
    std::vector<FftJob> fj;
    for (auto& j : jobs) fj.push_back({d_ptrs + j.off, (u32* const*)(d_ptrs + j.off + j.n), (u32)j.n, j.log - j.sh, j.src_log - j.sh, j.sh == 0});
    fft_plan(plan, inverse, fj.data(), fj.size(), c.d_tw, c.d_itw, c.tw_root_log);
    plan.d_groups = c.stage(plan.groups.data(), plan.groups.size());
    sb.end();
    return plan;
}
void HipProver::fft_launch(const FftPlan& plan) { fft_run(c.stream, plan); BF_HIP(hipGetLastError()); }
// ---- batched FFT over heterogeneous columns: one launch per pass and kernel kind, whatever the number of sizes ---------------
void HipProver::fft_cols(bool inverse, const std::vector<DCol>& src, const std::vector<DCol>& dst) {
    c.stage_checkpoint();
    fft_launch(fft_prepare(inverse, src, dst));
}

// folded_leaves: the deepest level is a launch of its own (never part of the subtree kernel), to be issued as the fused fold + leaf kernel
HipProver::MerklePlan HipProver::merkle_plan(const std::vector<DCol>& cols_in, bool folded_leaves) {
    if (cols_in.empty()) throw HipError("merkle_commit: no columns");
    MerklePlan p;
    p.cols = cols_in;
    std::vector<DCol>& cols = p.cols;
    std::stable_sort(cols.begin(), cols.end(), [](const DCol& a, const DCol& b) { return a.log_size > b.log_size; });
    DevMerkle& mk = p.mk;
    mk.cols = cols;
    mk.max_log = cols[0].log_size;
    mk.layers.resize(mk.max_log + 1);
    mk.shifts.assign(mk.max_log + 1, 0);
    u32 min_col_log = cols.back().log_size;
    // one staging copy for the column descriptors of every level; replication shift of every level
    std::vector<ColDesc> all; p.off.assign(mk.max_log + 2, 0); p.bytes.assign(mk.max_log + 1, 0.0);
    {
        size_t ci = 0;
        for (int log = (int)mk.max_log; log >= 0; log--) {
            p.off[log] = all.size();
            u32 sh = log < (int)mk.max_log ? (mk.shifts[log + 1] ? mk.shifts[log + 1] - 1 : 0) : 32;
            while (ci < cols.size() && cols[ci].log_size == (u32)log) { sh = std::min(sh, cols[ci].shift); p.bytes[log] += 4.0 * cols[ci].stored(); all.push_back(cols[ci++].desc()); }
            mk.shifts[log] = std::min<u32>(sh == 32 ? 0 : sh, (u32)log);
        }
    }
    p.n_all = all.size();
    p.poseidon = c.conv.merkle_channel == 1;   // Poseidon252MerkleHasher: layer kernel of poseidon.hip, no fused top, host channel
    (void)min_col_log;
    // The top kernel takes levels [fused_top - 1 .. 0] (<= 512 nodes in its first level, columns included), all un-replicated, and reads
    // the children of its first level from level fused_top (also un-replicated) unless it starts at the leaves.
    u32 fused_top = std::min<u32>(mk.max_log + 1, 10);
    while (fused_top > 0 && mk.shifts[std::min(fused_top, mk.max_log)] != 0) fused_top--;
    if (p.poseidon) fused_top = 0;
    p.fused_top = fused_top;
    // Shard group: the big layers are hashed SHARE-WISE — rank r takes the stored slots [r * stored / count, (r + 1) * stored / count) of
    // every layer with at least 2^SHARE_MIN_LOG_PER_RANK stored nodes per rank, replicated ones included (a slot's children are slots of
    // the same rank in the layer below, whether that layer is stored at the same replication or one step finer). log - shift is
    // non-decreasing in log, so these layers form one band [band_lo, max_log]; the band's lowest layer is completed on every rank by one
    // all-gather and everything below it is hashed by every rank, redundantly, with the same two launches as a one-GPU proof (subtree +
    // top): a share of fewer than 2^14 nodes is a launch that costs more than it computes (r04: 155 of a rank's 217 layer launches per
    // fib19 proof had <= 512 workgroups and took 0.85 ms per rank: profiles/r04_shard_redundancy_before.txt).
    const ShardGroup& sg = c.shard;
    if (sg.count > 1) {
        // (Poseidon252: a node costs ~40x a Blake2s node and there is no multi-level kernel below the band — shares down to 256 nodes)
        const int share_min = p.poseidon ? 8 : (int)SHARE_MIN_LOG_PER_RANK;
        int lo = std::max<int>((int)sg.log_count + share_min, (int)fused_top);
        while (lo <= (int)mk.max_log && (int)lo - (int)mk.shifts[lo] < (int)sg.log_count + share_min) lo++;
        // a tree with fewer than 2^14 stored leaves per rank is hashed whole by every rank: cheaper than the latency of its all-gather
        const bool worth = (int)mk.max_log - (int)mk.shifts[mk.max_log] >= (int)sg.log_count + (int)SLICE_MIN_LOG_PER_RANK;
        if (worth && lo <= (int)mk.max_log) { mk.band_hi = (int)mk.max_log; mk.band_lo = lo; }
        // row-sharded columns can only be hashed share-wise: their layers must lie inside the band
        for (auto& col : cols) if (col.sliced() && ((int)col.log_size < mk.band_lo || (int)col.log_size > mk.band_hi)) throw HipError("shard group: a row-sharded column lies outside the share-wise Merkle band");
    }
    const bool banded = mk.band_hi >= mk.band_lo;
    // Storage of the levels. A share-wise level above the band's lowest holds only this rank's nodes (its children and its decommitment
    // reads are its own), addressed through a virtual base like a row-sharded column: a 2^26-row trace has ~40 GB of hashes, and eight
    // ranks each reserving all of them would not fit one GPU's — or, on eight GPUs, waste seven eighths of — memory.
    for (int log = (int)mk.max_log; log >= 0; log--) {
        const size_t stored = (size_t(1) << log) >> mk.shifts[log];
        if (banded && log > mk.band_lo && log <= mk.band_hi) {
            const size_t per_rank = stored >> sg.log_count;
            mk.layers[log] = reinterpret_cast<u32*>(reinterpret_cast<uintptr_t>(c.arena.alloc(32 * per_rank)) - 32 * per_rank * sg.rank);
        } else mk.layers[log] = (u32*)c.arena.alloc(32 * stored);
    }
    // levels [sub_hi .. 9]: one launch, a workgroup per node of level 9 — over complete, un-replicated levels only (below the band of a
    // shard group's tree); complete levels above sub_hi are single-level launches
    if (fused_top == 10 && mk.max_log >= 11) {
        u32 hi = std::min<u32>(banded ? (u32)mk.band_lo - 1 : mk.max_log, 17);
        if (folded_leaves && hi == mk.max_log) hi--;
        while (hi > 10 && mk.shifts[hi] != 0) hi--;
        if (hi > 10) { p.sub_hi = hi; p.fused_top = fused_top = MERKLE_SUBTREE_ROOT_LEVEL; }     // the top starts below the subtree roots
    }
    auto level_cols = [&](int log) { return (log > 0 ? p.off[log - 1] : all.size()) - p.off[log]; };
    auto level_cost = [&](int log, double& bytes, double& comp) {
        const double nodes = (double)(1u << log), nc = (double)level_cols(log);
        const bool has = log < (int)mk.max_log;
        bytes += nodes * ((has ? 64.0 : 0.0) + 32.0) + p.bytes[log];
        comp += nodes * ((has ? 1.0 : 0.0) + (double)(((u32)nc + 15) / 16) + ((!has && nc == 0) ? 1.0 : 0.0));
    };
    if (banded && !p.poseidon && fused_top > 0 && mk.band_hi > mk.band_lo && c.shard.band_fusion) {
        // The shares of the band's last levels are 2^14..2^17 nodes: 64..512 workgroups each, four launches of ~6-10 us for ~2 us of work
        // each (r04: 50 such launches per rank and fib19 proof, 0.35 ms per rank). Levels band_lo + 3 .. band_lo go into one launch.
        const int hi = std::min(mk.band_hi, mk.band_lo + 3);
        bool plain = true;
        for (int lg = mk.band_lo; lg <= std::min(hi + 1, (int)mk.max_log); lg++) plain = plain && mk.shifts[lg] == 0;
        const u32 r = 8 - (u32)(hi - mk.band_lo);
        if (plain && (u32)mk.band_lo >= sg.log_count + r) {
            p.band_fuse_hi = hi; p.band_fuse_r = r;
            for (int lg = hi; lg >= mk.band_lo; lg--) level_cost(lg, p.band_bytes, p.band_comp);
            p.band_bytes /= sg.count; p.band_comp /= sg.count;
        }
    }
    for (int log = (int)fused_top - 1; log >= 0; log--) level_cost(log, p.top_bytes, p.top_comp);
    if (p.sub_hi) for (int log = (int)p.sub_hi; log >= (int)MERKLE_SUBTREE_ROOT_LEVEL; log--) level_cost(log, p.sub_bytes, p.sub_comp);
    p.d_all = all.empty() ? nullptr : c.stage(all.data(), all.size());
    if (folded_leaves) {
        if (banded || p.poseidon || mk.shifts[mk.max_log] != 0 || level_cols((int)mk.max_log) != 4 || (int)mk.max_log < (p.sub_hi ? (int)p.sub_hi + 1 : (int)fused_top))
            throw HipError("merkle_plan: this tree's deepest level cannot be a fused fold + leaf launch");
        p.folded_leaves = true;
    }
    if (fused_top > 0) {
        MerkleTreeDesc td{};
        if (mk.max_log >= 32) throw HipError("merkle: tree too deep");
        for (u32 lg = 0; lg <= mk.max_log; lg++) { td.layers[lg] = (uint4*)mk.layers[lg]; td.shifts[lg] = mk.shifts[lg]; td.col_off[lg] = (u32)p.off[lg]; }
        td.cols = p.d_all; td.n_cols = (u32)all.size(); td.max_log = mk.max_log;
        p.tree = td;
    }
    return p;
}
// stamp_slot >= 0 (with a pinned root written by the top kernel itself): the top kernel also writes the proof's number into that stamp slot
// behind the root; *stamped tells the caller whether it did (a tree without a fused top needs a k_post_stamp launch instead)
DevMerkle HipProver::merkle_run(MerklePlan& p, Hash32* pinned_root, bool no_readback, const ChannelStep* step, const std::vector<LevelWait>* waits,
                                int stamp_slot, bool* stamped) {
    DevMerkle& mk = p.mk;
    const ShardGroup& sg = c.shard;
    const bool poseidon = p.poseidon;
    const u32 fused_top = p.fused_top;
    if (poseidon && step) throw HipError("the device-side channel step is a Blake2s path");
    const char* layer_kernel = poseidon ? "k_merkle_layer_poseidon" : "k_merkle_layer";
    prof_run_begin(c.stream, layer_kernel);
    const int single_lo = p.sub_hi ? (int)p.sub_hi + 1 : (int)fused_top;
    size_t wi = 0;
    auto apply_waits = [&](int log) { while (waits && wi < waits->size() && (*waits)[wi].level >= log) BF_HIP(hipStreamWaitEvent(c.stream, (*waits)[wi++].ev, 0)); };
    for (int log = (int)mk.max_log; log >= single_lo; log--) {
        apply_waits(log);
        if (log == p.band_fuse_hi) {
            // the rest of the band in one launch over this rank's share, then the all-gather of its lowest level
            prof_run_end(c.stream);
            const u32 n_wg = ((1u << mk.band_lo) >> sg.log_count) >> p.band_fuse_r;
            merkle_subtree_share(c.stream, p.tree, (u32)log, (u32)mk.band_lo, (u32)mk.band_lo - p.band_fuse_r, sg.rank * n_wg, n_wg, c.conv.merkle_node_hash, p.band_bytes, p.band_comp);
            sg.comm->all_gather(c.stream, mk.layers[mk.band_lo], (size_t(32) << mk.band_lo) >> sg.log_count);
            prof_run_begin(c.stream, layer_kernel);
            log = mk.band_lo;
            continue;
        }
        size_t n = (log > 0 ? p.off[log - 1] : p.n_all) - p.off[log];
        if (p.folded_leaves && log == (int)mk.max_log) {
            if (p.fold_mode < 0 || p.fold.log != mk.max_log) throw HipError("merkle_run: the fold of the deepest level was not described");
            fri_fold_leaf(c.stream, mk.layers[log], p.fold, p.fold_mode, c.conv.merkle_node_hash);
            c.last_proof_flags |= 32u;      // bfhip_ctx_last_proof_flags bit 5
            continue;
        }
        const bool share = log >= mk.band_lo && log <= mk.band_hi;
        const u32 per_rank = share ? ((1u << (log - mk.shifts[log])) >> sg.log_count) : 0u;   // in stored slots
        if (poseidon)
            merkle_layer_poseidon(c.stream, mk.layers[log], log < (int)mk.max_log ? mk.layers[log + 1] : nullptr, n ? p.d_all + p.off[log] : nullptr, (u32)n, (u32)log,
                                  mk.shifts[log], log < (int)mk.max_log ? mk.shifts[log + 1] : 0, sg.rank * per_rank, per_rank);
        else
            merkle_layer(c.stream, mk.layers[log], log < (int)mk.max_log ? mk.layers[log + 1] : nullptr, n ? p.d_all + p.off[log] : nullptr, (u32)n, (u32)log, p.bytes[log],
                         mk.shifts[log], log < (int)mk.max_log ? mk.shifts[log + 1] : 0, c.conv.merkle_node_hash, sg.rank * per_rank, per_rank);
        if (share && log == mk.band_lo) {
            // the smallest share-wise layer is completed on every rank by one all-gather on the device buffer (rank r's block = its
            // contiguous node range); the levels below are hashed redundantly, so every rank obtains the same root
            prof_run_end(c.stream);
            sg.comm->all_gather(c.stream, mk.layers[log], ((size_t(32) << log) >> mk.shifts[log]) >> sg.log_count);
            prof_run_begin(c.stream, layer_kernel);
        }
    }
    prof_run_end(c.stream);
    apply_waits(0);
    if (p.sub_hi) merkle_subtree(c.stream, p.tree, p.sub_hi, c.conv.merkle_node_hash, p.sub_bytes, p.sub_comp);
    // a deferred root goes to its pinned slot by the top kernel's own stores (no copy command behind the tree)
    u32* root_direct = (fused_top > 0 && !step && pinned_root) ? reinterpret_cast<u32*>(c.small_alias(pinned_root)) : nullptr;
    const bool stamp_here = root_direct && stamp_slot >= 0;
    if (stamped) *stamped = stamp_here;
    if (fused_top > 0) merkle_top(c.stream, p.tree, fused_top - 1, c.conv.merkle_node_hash, step ? step->chan : nullptr, step ? step->alpha8 : nullptr, step ? step->root_copy : root_direct, p.top_bytes, p.top_comp,
                                  stamp_here ? c.small_alias(c.stamp_host(stamp_slot)) : nullptr, c.proof_seq);
    else if (step) channel_mix_root_draw(c.stream, step->chan, mk.layers[0], step->alpha8, step->root_copy);
    BF_HIP(hipGetLastError());
    if (no_readback) return mk;
    if (pinned_root) { if (!root_direct) BF_HIP(hipMemcpyAsync(pinned_root->b, mk.layers[0], 32, hipMemcpyDeviceToHost, c.stream)); return mk; }
    c.read_back(mk.root.b, mk.layers[0], 32);
    return mk;
}
DevMerkle HipProver::merkle_commit(const std::vector<DCol>& cols_in, Hash32* pinned_root, bool no_readback, const ChannelStep* step) {
    c.stage_checkpoint();
    StageBatch sb(c);
    MerklePlan p = merkle_plan(cols_in);
    sb.end();
    return merkle_run(p, pinned_root, no_readback, step);
}

// storage for this rank's row range of a 2^log column (stored at one word per 2^shift rows), returned as a virtual base (see DCol)
u32* HipProver::alloc_slice(u32 log, u32 shift) {
    return reinterpret_cast<u32*>(reinterpret_cast<uintptr_t>(c.alloc_u32(slice_cells(log) >> shift)) - sizeof(u32) * (slice_first(log) >> shift));
}
// Column-sharding of the transforms: the biggest column goes to the least loaded rank (greedy by 2^log, deterministic on every rank).
std::vector<u32> HipProver::assign_owners(const std::vector<DCol>& polys, u32 log_blowup) const {
    std::vector<u32> owner(polys.size(), OWNER_ALL);
    if (!sharded()) return owner;
    std::vector<size_t> idx;
    for (size_t i = 0; i < polys.size(); i++) if (slice_col(polys[i].log_size + log_blowup, polys[i].shift)) idx.push_back(i);
    // by transform work = stored words (a replicated column is a 16x smaller transform)
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return polys[a].log_size - polys[a].shift > polys[b].log_size - polys[b].shift; });
    std::vector<u64> load(c.shard.count, 0);
    for (size_t i : idx) {
        u32 best = 0;
        for (u32 r = 1; r < c.shard.count; r++) if (load[r] < load[best]) best = r;
        owner[i] = best; load[best] += u64(1) << (polys[i].log_size - polys[i].shift);
    }
    return owner;
}

// CommitmentTreeProver::new: LDE by the blowup factor, Merkle, mix_root.
// Shard group: a polynomial with t.owner[i] != OWNER_ALL is extended by its owner only; one grouped send-receive then hands every rank
// its row range of the LDE column (with_prev: and of the column's previous-row copy, which the constraint kernel needs for the mask
// offset -1 of the last logUp column — that neighbour is a reflection in bit-reversed storage, not a halo).
void HipProver::commit_tree(DTree& t, Hash32* pinned_root, bool with_prev) {
    const size_t n = t.polys.size();
    if (t.owner.size() != n) t.owner.assign(n, OWNER_ALL);
    t.evals.resize(n); t.prev.assign(n, DCol());
    std::vector<DCol> fsrc, fdst, full(n), fullprev(n);
    for (size_t i = 0; i < n; i++) {
        DCol e; e.log_size = t.polys[i].log_size + cfg.log_blowup; e.shift = t.polys[i].shift;
        if (t.owner[i] == OWNER_ALL) { e.ptr = c.alloc_u32(e.stored()); fsrc.push_back(t.polys[i]); fdst.push_back(e); }
        else if (replicate()) {
            // virtually sliced: the whole column is here (virtual base = real base), consumers are restricted to this rank's row range by `lc`;
            // the mask offset -1 of a last logUp column is read from the column itself (prev stays null)
            e.ptr = c.alloc_u32(e.stored()); fsrc.push_back(t.polys[i]); fdst.push_back(e);
            e.lc = lc();
        } else {
            if (t.owner[i] == c.shard.rank) {
                full[i] = e; full[i].ptr = c.alloc_u32(e.stored()); fsrc.push_back(t.polys[i]); fdst.push_back(full[i]);
                if (with_prev && e.shift == 0) { fullprev[i] = e; fullprev[i].ptr = c.alloc_u32(e.stored()); }
            }
            e.lc = lc(); e.ptr = alloc_slice(e.log_size, e.shift);
            // previous-row copies: of the full-size columns only (the last logUp column of each component; a replicated column has no
            // mask offset -1)
            if (with_prev && e.shift == 0) { t.prev[i] = e; t.prev[i].ptr = alloc_slice(e.log_size); }
        }
        t.evals[i] = e;
    }
    // the grouped send-receive that hands every rank its row range of the owned columns `idx` (after the owner's previous-row copies)
    auto exchange_columns = [&](hipStream_t comm_stream, const std::vector<size_t>& idx, hipEvent_t after_copies) {
        std::vector<Xfer> sends, recvs;
        for (size_t i : idx) {
            const u32 el = t.evals[i].log_size, sh = t.evals[i].shift;
            const size_t cells = slice_cells(el) >> sh, bytes = cells * sizeof(u32), first = slice_first(el) >> sh;      // in stored words
            const bool wp = with_prev && sh == 0;
            if (t.owner[i] == c.shard.rank) {
                if (wp) prev_row_copy(c.stream, fullprev[i].ptr, full[i].ptr, t.polys[i].log_size);
                for (u32 r = 0; r < c.shard.count; r++) {
                    sends.push_back({r, full[i].ptr + r * cells, bytes});
                    if (wp) sends.push_back({r, fullprev[i].ptr + r * cells, bytes});
                }
            }
            recvs.push_back({t.owner[i], t.evals[i].ptr + first, bytes});
            if (wp) recvs.push_back({t.owner[i], t.prev[i].ptr + first, bytes});
        }
        if (recvs.empty()) return;
        if (comm_stream != c.stream) { BF_HIP(hipEventRecord(after_copies, c.stream)); BF_HIP(hipStreamWaitEvent(comm_stream, after_copies, 0)); }
        c.shard.comm->exchange(comm_stream, sends, recvs);
    };
    std::vector<size_t> owned;
    u32 big = 0;
    for (size_t i = 0; i < n; i++) if (t.owner[i] != OWNER_ALL && !replicate()) { owned.push_back(i); big = std::max(big, t.evals[i].log_size); }
    std::vector<size_t> first_wave, second_wave;
    for (size_t i : owned) (t.evals[i].log_size == big ? first_wave : second_wave).push_back(i);
    // bfhip_ctx_set_overlap bit 2 (shard groups): the largest size class is transformed first and travels on the partner stream while the
    // remaining columns are being transformed; the second send-receive follows on the same partner stream (every rank issues the group's
    // collectives in one order), and the main stream resumes behind both. Needs at least two size classes among the owned columns.
    if (sharded() && c.exchange_overlapped() && !second_wave.empty() && c.aux[0]) {
        std::vector<DCol> sa, da, sb2, db2;
        {
            size_t k = 0;   // fsrc / fdst hold, in index order, every column this rank transforms
            for (size_t i = 0; i < n; i++) {
                const bool mine = t.owner[i] == OWNER_ALL || t.owner[i] == c.shard.rank;
                if (!mine) continue;
                const bool wave_a = t.owner[i] != OWNER_ALL && t.evals[i].log_size == big;
                (wave_a ? sa : sb2).push_back(fsrc[k]); (wave_a ? da : db2).push_back(fdst[k]);
                k++;
            }
        }
        c.stage_checkpoint();
        FftPlan pa = fft_prepare(false, sa, da), pb = fft_prepare(false, sb2, db2);
        try {
            fft_launch(pa);
            exchange_columns(c.aux[0], first_wave, c.next_event());
            fft_launch(pb);
            exchange_columns(c.aux[0], second_wave, c.next_event());
            hipEvent_t done = c.next_event();
            BF_HIP(hipEventRecord(done, c.aux[0]));
            BF_HIP(hipStreamWaitEvent(c.stream, done, 0));
        } catch (...) {
            // copies and receives still queued on the partner stream write into arena memory the next proof hands out again
            (void)hipStreamSynchronize(c.aux[0]);
            throw;
        }
    } else {
        fft_cols(false, fsrc, fdst);
        if (sharded() && !replicate()) exchange_columns(c.stream, owned, nullptr);
    }
    BF_HIP(hipGetLastError());
    t.mk = merkle_commit(t.evals, pinned_root);
    if (!pinned_root) ch.mix_root(t.mk.root);
#ifdef BFHIP_TEST_HOOKS
    capture_tree(c, t);
#endif
}

// One process per proof: the same commitment with its two bounds overlapped. The transforms are HBM-bound, the Blake2s layers
// VALU-bound, and layer L of a mixed-degree tree needs only the columns of size L and layer L + 1 — so the largest size class is
// transformed first and its layers are hashed on the partner stream while the smaller classes are still being transformed.
// interp_src (optional, one entry per polynomial): evaluations still to be interpolated into t.polys (extend_evals), wave by wave.
// stamp_slot >= 0: behind the root (in its pinned slot) the proof's number is written into that stamp slot (ctx.h: wait_stamp)
void HipProver::commit_tree_overlapped(DTree& t, Hash32* pinned_root, const std::vector<DCol>* interp_src, int stamp_slot, bool evals_ready) {
    const size_t n = t.polys.size();
    t.owner.assign(n, OWNER_ALL);
    if (evals_ready) {
        // the columns are on the stream already: nothing to transform and so nothing to hash beside — one stream
        if (interp_src || t.evals.size() != n) throw HipError("commit_tree_overlapped: ready evaluations do not match the tree");
        t.prev.assign(n, DCol());
        c.stage_checkpoint();
        StageBatch sb(c);
        MerklePlan mp = merkle_plan(t.evals);
        sb.end();
        bool stamped = false;
        t.mk = merkle_run(mp, pinned_root, false, nullptr, nullptr, stamp_slot, &stamped);
        if (stamp_slot >= 0 && !stamped) c.post_stamp(stamp_slot);
        if (!pinned_root) ch.mix_root(t.mk.root);
#ifdef BFHIP_TEST_HOOKS
        capture_tree(c, t);
#endif
        return;
    }
    t.evals.resize(n); t.prev.assign(n, DCol());
    u32 max_log = 0;
    for (size_t i = 0; i < n; i++) {
        DCol e; e.log_size = t.polys[i].log_size + cfg.log_blowup; e.shift = t.polys[i].shift; e.ptr = c.alloc_u32(e.stored());
        t.evals[i] = e; max_log = std::max(max_log, e.log_size);
    }
    std::vector<DCol> src[2], pol[2], ev[2];
    u32 next_log = 0;                       // largest size among the second wave
    for (size_t i = 0; i < n; i++) {
        const int w = t.evals[i].log_size == max_log ? 0 : 1;
        if (interp_src) src[w].push_back((*interp_src)[i]);
        pol[w].push_back(t.polys[i]); ev[w].push_back(t.evals[i]);
        if (w) next_log = std::max(next_log, t.evals[i].log_size);
    }
    // below ~2^18 leaves the whole tree is a latency chain: nothing to hide, one stream
    const bool overlap = (c.overlap & 1u) && !ev[1].empty() && max_log >= 19;
    c.stage_checkpoint();
    FftPlan fi[2], fe[2];
    MerklePlan mp;
    {
        StageBatch sb(c);
        for (int w = 0; w < 2; w++) {
            if (interp_src) fi[w] = fft_prepare(true, src[w], pol[w]);
            fe[w] = fft_prepare(false, pol[w], ev[w]);
        }
        mp = merkle_plan(t.evals);
        sb.end();
    }
    hipStream_t main = c.stream, aux = c.aux_of(main);
    if (interp_src) fft_launch(fi[0]);
    fft_launch(fe[0]);
    if (!overlap) {
        if (interp_src) fft_launch(fi[1]);
        fft_launch(fe[1]);
        bool stamped = false;
        t.mk = merkle_run(mp, pinned_root, false, nullptr, nullptr, stamp_slot, &stamped);
        if (stamp_slot >= 0 && !stamped) c.post_stamp(stamp_slot);
    } else {
        hipEvent_t e1 = c.next_event(), e2 = c.next_event(), e3 = c.next_event();
        BF_HIP(hipEventRecord(e1, main));
        if (interp_src) fft_launch(fi[1]);
        fft_launch(fe[1]);
        BF_HIP(hipEventRecord(e2, main));
        BF_HIP(hipStreamWaitEvent(aux, e1, 0));
        std::vector<LevelWait> waits = {{(int)next_log, e2}};
        c.stream = aux;
        try { t.mk = merkle_run(mp, nullptr, /*no_readback=*/true, nullptr, &waits); } catch (...) { c.stream = main; (void)hipStreamSynchronize(aux); throw; }
        c.stream = main;
        BF_HIP(hipEventRecord(e3, aux));
        BF_HIP(hipStreamWaitEvent(main, e3, 0));      // joined: whatever follows on this stream sees the tree
        if (pinned_root) BF_HIP(hipMemcpyAsync(pinned_root->b, t.mk.layers[0], 32, hipMemcpyDeviceToHost, main));
        else c.read_back(t.mk.root.b, t.mk.layers[0], 32);
        if (stamp_slot >= 0) c.post_stamp(stamp_slot);
    }
    if (!pinned_root) ch.mix_root(t.mk.root);
#ifdef BFHIP_TEST_HOOKS
    capture_tree(c, t);
#endif
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host table build + upload (outside the metric's timed region: "inputs already resident in HBM").
// Prover-input preparation from the VM trace. on_gpu (default): the 13 table builders run on the device (tables.hip);
// otherwise the host builders (host/tables.h) fill the columns and they are uploaded.
// use_arena: take the column storage from the per-proof arena (no hipMalloc, which would synchronise the device) — only valid for
// the duration of the current proof; otherwise the columns live in their own device allocations owned by `in`.
void HipProver::upload_trace(Ctx& c, const std::vector<Registers>& vm_trace, const std::vector<u32>& code, TraceInput& in, bool use_arena, bool on_gpu) {
    c.refuse_in_session("trace upload");      // the GPU table builders take their scratch from the arena
    in.rows.assign(N_COMPONENTS, {});
    in.n_steps = vm_trace.size();
    in.main_cells = in.interaction_cells = 0;
    auto alloc = [&](size_t words) -> u32* {
        if (use_arena) return c.alloc_u32(words);
        u32* p = nullptr; BF_HIP(hipMalloc((void**)&p, (words ? words : 1) * sizeof(u32))); in.owned.push_back(p); return p;
    };
    if (on_gpu) {
        std::vector<u32> soa[7];
        size_t n = vm_trace.size();
        for (auto& v : soa) v.resize(n);
        for (size_t i = 0; i < n; i++) { const Registers& r = vm_trace[i]; soa[0][i] = r.clk; soa[1][i] = r.ip; soa[2][i] = r.ci; soa[3][i] = r.ni; soa[4][i] = r.mp; soa[5][i] = r.mv; soa[6][i] = r.mvi; }
        std::vector<std::vector<u32*>> cols;
        build_tables_device(c, soa, (u32)n, code, alloc, cols, in.log_sizes);
        for (int k = 0; k < N_COMPONENTS; k++)
            for (u32 j = 0; j < n_main_cols(k); j++) { DCol r; r.log_size = in.log_sizes[k]; r.shift = LOG_N_LANES; r.ptr = cols[k][j]; in.rows[k].push_back(r); }
    } else {
        std::vector<Table> tables = build_tables(vm_trace, code);
        for (int k = 0; k < N_COMPONENTS; k++) {
            in.log_sizes[k] = tables[k].log_size();
            for (u32 j = 0; j < n_main_cols(k); j++) {
                DCol r; r.log_size = in.log_sizes[k]; r.shift = LOG_N_LANES;
                r.ptr = alloc(r.stored());
                BF_HIP(hipMemcpyAsync(r.ptr, tables[k].cols[j].data(), r.stored() * sizeof(u32), hipMemcpyHostToDevice, c.stream));
                in.rows[k].push_back(r);
            }
        }
    }
    for (int k = 0; k < N_COMPONENTS; k++) {
        in.main_cells += (u64)n_main_cols(k) << in.log_sizes[k];
        in.interaction_cells += (u64)(4 * n_logup_cols(k)) << in.log_sizes[k];
    }
    c.sync();
}

// Prover-input preparation from the caller's register rows (bfhip_trace_create_from_registers, bfhip_prove_registers, the pool's register
// jobs): the rows go to the device in one copy and are transposed and checked there (ingest.hip); the table kernels read the result.
// Which error wins when several apply: a non-canonical register, then a non-canonical program word, then the table builders' refusals.
void HipProver::upload_registers(Ctx& c, const u32* trace7_h, size_t n_rows, const u32* code_words_h, size_t n_code, TraceInput& in, bool use_arena, bool with_place) {
    auto bad_register = [&](size_t row, int reg) {
        std::string m = "register value is not a canonical M31";
        if (with_place) m += " (row " + std::to_string(row) + ", register " + std::to_string(reg) + ")";
        return HipError(m);
    };
    c.refuse_in_session("trace upload");
    auto check_code = [&]() {
        std::vector<u32> ins(code_words_h, code_words_h + n_code);
        for (u32 w : ins) if (w >= P31) throw HipError("program word is not a canonical M31");
        return ins;
    };
    if (!c.tables_on_gpu) {
        std::vector<Registers> tr(n_rows);
        for (size_t i = 0; i < n_rows; i++) {
            const u32* v = trace7_h + 7 * i;
            for (int k = 0; k < 7; k++) if (v[k] >= P31) throw bad_register(i, k);
            tr[i] = Registers{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
        }
        upload_trace(c, tr, check_code(), in, use_arena, /*on_gpu=*/false);
        return;
    }
    c.stage_checkpoint();
    u64 first_bad = ~u64(0);
    TraceSoA t = ingest_registers(c, trace7_h, n_rows, &first_bad);
    if (first_bad != ~u64(0)) throw bad_register(size_t(first_bad >> 3), int(first_bad & 7));
    std::vector<u32> ins = check_code();
    in.rows.assign(N_COMPONENTS, {});
    in.n_steps = n_rows;
    in.main_cells = in.interaction_cells = 0;
    auto alloc = [&](size_t words) -> u32* {
        if (use_arena) return c.alloc_u32(words);
        u32* p = nullptr; BF_HIP(hipMalloc((void**)&p, (words ? words : 1) * sizeof(u32))); in.owned.push_back(p); return p;
    };
    std::vector<std::vector<u32*>> cols;
    build_tables_device(c, t, ins, alloc, cols, in.log_sizes);
    for (int k = 0; k < N_COMPONENTS; k++) {
        for (u32 j = 0; j < n_main_cols(k); j++) { DCol r; r.log_size = in.log_sizes[k]; r.shift = LOG_N_LANES; r.ptr = cols[k][j]; in.rows[k].push_back(r); }
        in.main_cells += (u64)n_main_cols(k) << in.log_sizes[k];
        in.interaction_cells += (u64)(4 * n_logup_cols(k)) << in.log_sizes[k];
    }
    c.sync();
}

// Phase 0 of prove_brainfuck: the preprocessed tree IsFirst(LOG_MAX_ROWS ..= LOG_N_LANES) (mod.rs:495-500) — polynomials in closed form,
// LDE, Merkle tree; the root goes to *pinned_root behind the tree (no host wait). Storage from the context's current arena.
void HipProver::build_preprocessed(DTree& tree, Hash32* pinned_root) {
    for (u32 log = log_max_rows; log >= LOG_N_LANES; log--) {
        DCol p; p.log_size = log; p.shift = 0; p.ptr = nullptr;
        tree.polys.push_back(p);
    }
    IsFirstCols ifc{}; ifc.log_min = LOG_N_LANES; ifc.log_max = log_max_rows;
    if (log_max_rows - LOG_N_LANES >= 28) throw HipError("log_max_rows too large");
    if (!sharded()) {
        // One process per proof (and the pool's builder): the LDE columns themselves in closed form, one launch (fft.hip: k_is_first_lde) — no coefficient
        // columns, no transforms. The samples and the constraint domain of log_blowup != 1 take the closed form as well (DTree::is_first_closed).
        tree.is_first_closed = true;
        tree.evals.clear();
        for (const DCol& p : tree.polys) {
            DCol e; e.log_size = p.log_size + cfg.log_blowup; e.shift = 0; e.ptr = c.alloc_u32(e.stored());
            tree.evals.push_back(e);
            ifc.ptr[p.log_size - LOG_N_LANES] = e.ptr;
        }
        is_first_lde(c.stream, ifc, cfg.log_blowup, c.d_tw, c.d_itw, c.tw_root_log);
#ifdef BFHIP_TEST_HOOKS
        if (c.capture && c.capture->on) {      // the capture hands out every tree's polynomials: give it the coefficient columns
            IsFirstCols cf{}; cf.log_min = LOG_N_LANES; cf.log_max = log_max_rows;
            for (DCol& p : tree.polys) { p.ptr = c.alloc_u32(p.stored()); cf.ptr[p.log_size - LOG_N_LANES] = p.ptr; }
            is_first_coeffs(c.stream, cf, c.d_itw, c.tw_root_log);
        }
#endif
        commit_tree_overlapped(tree, pinned_root, nullptr, -1, /*evals_ready=*/true);
        return;
    }
    // shard group: the big IsFirst columns are column-sharded like the interaction tree's (owner interpolates and extends,
    // every rank receives its row range of the LDE)
    tree.owner = assign_owners(tree.polys, cfg.log_blowup);
    // interpolate(gen_is_first(log)) for every size in closed form, one launch (fft.hip: k_is_first_coeffs)
    for (size_t i = 0; i < tree.polys.size(); i++) {
        if (!transforms_here(tree.owner[i])) continue;
        DCol& p = tree.polys[i];
        p.ptr = c.alloc_u32(p.stored());
        ifc.ptr[p.log_size - LOG_N_LANES] = p.ptr;
    }
    is_first_coeffs(c.stream, ifc, c.d_itw, c.tw_root_log);
    commit_tree(tree, pinned_root);
}
// The pool's builder (pool.hip): commits the preprocessed tree on this (otherwise idle) context for every proof of a batch and returns
// without waiting — sp.ready is recorded behind the tree and the root's store into pinned memory.
void HipProver::build_shared_preprocessed(SharedPreprocessed& sp) {
    if (sharded()) throw HipError("pool: the builder context must not be a member of a shard group");
    c.refuse_in_session("pool: preprocessed commitment");
    if (log_max_rows < LOG_N_LANES) throw HipError("log_max_rows must be at least LOG_N_LANES (4)");
    check_config();
    sp.valid = false;
    c.sync();                       // nothing of an earlier batch's build is in flight (its readers are done: the pool's batches are serial)
    c.arena.reset(); c.stage_used = 0; c.use_mailbox = false;
    BF_HIP(hipMemsetAsync(c.d_counters, 0, 4 * 64 * sizeof(u32), c.stream));
    sp.tree = DTree();
    Hash32* root = reinterpret_cast<Hash32*>(c.h_small) + sp.root_slot;
    build_preprocessed(sp.tree, root);
    BF_HIP(hipEventRecord(sp.ready, c.stream));
    sp.pinned_root = root; sp.lmr = log_max_rows; sp.node_conv = c.conv.merkle_node_hash; sp.channel = c.conv.merkle_channel; sp.log_blowup = cfg.log_blowup; sp.valid = true;
}

// ---- the preprocessed tree a context keeps across proofs (declared in ctx.h; Ctx::pre_cache owns it) ----------------------------------
// Each context is driven by one thread at a time (the pool relies on the same), so the cache needs no lock.
PreprocessedCache& preprocessed_cache_of(Ctx& c) {
    if (!c.pre_cache) c.pre_cache = new PreprocessedCache();
    return *c.pre_cache;
}
// the caller has waited for whatever may still read the kept tree
void preprocessed_cache_drop(Ctx& c) {
    if (!c.pre_cache) return;
    c.pre_cache->keep.release();
    delete c.pre_cache;
    c.pre_cache = nullptr;
}
// Group membership changes drop the cached tree: the ranks of a group must take the same decision (reuse or rebuild with its exchanges) in
// every proof, and they do when each starts its membership with an empty cache and then issues the group's common sequence of calls. (A cache
// that survived an earlier membership could match on some ranks only — found by tools/fuzz_campaign.py persistent, seed 60806.)
void preprocessed_cache_invalidate(Ctx* c) { if (c->pre_cache) c->pre_cache->valid = false; }

// ---- what pool.hip needs of the prover (declared in ctx.h) ----------------------------------------------------------------------------
SharedPreprocessed* shared_preprocessed_create(Ctx& builder) {
    auto* sp = new SharedPreprocessed();
    try { builder.bind(); BF_HIP(hipEventCreateWithFlags(&sp->ready, hipEventDisableTiming)); } catch (...) { delete sp; throw; }
    return sp;
}
void shared_preprocessed_destroy(SharedPreprocessed* sp) { if (sp) { if (sp->ready) (void)hipEventDestroy(sp->ready); delete sp; } }
bool shared_preprocessed_matches(const SharedPreprocessed* sp, const Ctx& c, u32 log_max_rows) { return sp && sp->matches(c, log_max_rows); }
void shared_preprocessed_build(SharedPreprocessed* sp, Ctx& builder, u32 log_max_rows) {
    builder.bind();
    HipProver pv(builder, log_max_rows);
    try { pv.build_shared_preprocessed(*sp); } catch (...) { sp->valid = false; (void)hipStreamSynchronize(builder.stream); throw; }
}
void shared_preprocessed_invalidate(SharedPreprocessed* sp) { if (sp) sp->valid = false; }

}  // namespace bf

#ifdef BFHIP_TEST_HOOKS
#include "api_guard.h"
// libbfhip_testhooks.so only (Makefile); not declared in include/bfhip.h. What tests/test_gpu_pcs_session.py feeds a commitment-scheme session
// with: the four trees of a Brainfuck proof as plain coefficient columns.
// bfhip_test_capture_polys(ctx, on): on = the proofs of this context from now on copy, behind each tree commitment, every polynomial of the
// tree to host memory (commit order: preprocessed, main trace, interaction, composition); the list starts empty at every call. While the
// capture is on the context proves in the plain launch order (a copy to host memory cannot be enqueued behind a waiting mailbox kernel);
// off restores the mailbox mode and drops the copies.
// bfhip_test_captured_poly(ctx, tree, col, out_h, cap, &log_size): polynomial `col` of captured tree `tree` as a full-size coefficient
// column of 2^log_size words; a row-granular polynomial (stored at one word per 16 cells: its coefficients of index 0 mod 16) is expanded
// with zeros. out_h == NULL: the size only. -2 = cap too small.
extern "C" int32_t bfhip_test_capture_polys(bfhip_ctx* ctx, int32_t on) {
    using namespace bf;
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (c.shard.count > 1) throw HipError("bfhip_test_capture_polys: the context is in a shard group");
    sync_both(c);
    if (!c.capture) { c.capture = new PolyCapture(); c.capture->saved_mailbox_mode = c.mailbox_mode; }
    if (on && !c.capture->on) { c.capture->saved_mailbox_mode = c.mailbox_mode; c.mailbox_mode = 0; }
    if (!on && c.capture->on) c.mailbox_mode = c.capture->saved_mailbox_mode;
    c.capture->on = on != 0;
    c.capture->trees.clear();
    if (!on) { delete c.capture; c.capture = nullptr; }
    return 0;
    API_CATCH
}
extern "C" int32_t bfhip_test_captured_poly(bfhip_ctx* ctx, uint32_t tree, uint32_t col, uint32_t* out_h, size_t cap, uint32_t* log_size) {
    using namespace bf;
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!log_size) throw HipError("null argument");
    if (!c.capture) throw HipError("bfhip_test_captured_poly: the capture is off");
    sync_both(c);
    if (tree >= c.capture->trees.size() || col >= c.capture->trees[tree].size()) throw HipError("bfhip_test_captured_poly: no such captured polynomial");
    const PolyCapture::Poly& p = c.capture->trees[tree][col];
    *log_size = p.log_size;
    if (!out_h) return 0;
    if (cap < (size_t(1) << p.log_size)) { bfhip_set_error("capacity"); return -2; }
    memset(out_h, 0, sizeof(u32) << p.log_size);
    for (size_t i = 0; i < p.stored.size(); i++) out_h[i << p.shift] = p.stored[i];
    return 0;
    API_CATCH
}
#endif
