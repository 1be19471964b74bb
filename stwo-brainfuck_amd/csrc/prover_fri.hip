// The last phase of a proof (prover.h): the FRI commit phase (FriProver::commit), the proof of work (GrindOps) and the decommitment of
// every tree at the query positions — control flow on the host, every read of column or hash data through one gather launch.
#include "prover.h"
#include <algorithm>
#include <set>

namespace bf {

// stamp_slot >= 0 (inside a proof, one process per proof): the host polls a stamp word written behind the gather instead of an event
std::vector<u32> Gather::run(Ctx& c, int stamp_slot) {
    std::vector<u32> out(n_words);
    if (reqs.empty()) return out;
    c.stage_checkpoint();
    if (c.shard.count == 1 && n_words * sizeof(u32) <= c.h_small_bytes - 4096) {
        // One process per proof: the kernel reads the request list where the host wrote it (the pinned side of the staging ring) and
        // writes the words into the pinned bounce buffer — two copy commands and their barriers less on the last round trip of a proof.
        size_t bytes = (reqs.size() * sizeof(GatherReq) + 255) & ~size_t(255);
        if (c.stage_used + bytes > c.stage_bytes) throw HipError("staging buffer exhausted (call stage_checkpoint() between operations)");
        memcpy(c.h_stage + c.stage_used, reqs.data(), reqs.size() * sizeof(GatherReq));
        const GatherReq* d = reinterpret_cast<const GatherReq*>(c.d_hstage_alias + c.stage_used);
        c.stage_used += bytes;
        gather_u32(c.stream, d, (u32)reqs.size(), reinterpret_cast<u32*>(c.d_small_alias + 4096));
        if (stamp_slot >= 0 && c.use_mailbox && c.proof_seq) { c.post_stamp(stamp_slot); c.wait_stamp(stamp_slot); }
        else c.sync();
        memcpy(out.data(), c.h_small + 4096, n_words * sizeof(u32));
        return out;
    }
    u32* dout = c.alloc_u32(n_words);
    // one launch unless the request table outgrows a quarter of the staging ring (many queries at a large LOG_MAX_ROWS): then one launch
    // per quarter, the ring recycled in between
    const size_t per_launch = c.stage_bytes / 4 / sizeof(GatherReq);
    if (reqs.size() > per_launch) c.last_proof_flags |= 16u;      // bfhip_ctx_last_proof_flags bit 4
    for (size_t i = 0; i < reqs.size(); i += per_launch) {
        const size_t n = std::min(per_launch, reqs.size() - i);
        if (i) c.stage_checkpoint();
        GatherReq* d = c.stage(reqs.data() + i, n);
        gather_u32(c.stream, d, (u32)n, dout);
    }
    // shard group: every word is either identical on all ranks (replicated columns, complete layers) or held by one rank and zero
    // elsewhere (rows of sharded columns, hashes of share-wise layers) — an element-wise maximum completes it everywhere
    if (c.shard.count > 1) c.shard.comm->all_reduce_max_u32(c.stream, dout, n_words);
    c.read_back(out.data(), dout, n_words * sizeof(u32));
    return out;
}

HipProver::Finisher HipProver::decommit(Gather& g, const DevMerkle& mk, const std::vector<DCol>& cols_in, const std::map<u32, std::vector<size_t>>& queries_per_log,
                                        std::vector<u32>* queried_values, MerkleDecommitment* dec) {
    // host time matters here (the GPU is idle while the decommitment is planned): no per-layer allocations, no copy when the
    // columns already come in descending size order
    auto by_size = [](const DCol& a, const DCol& b) { return a.log_size > b.log_size; };
    std::vector<DCol> sorted_copy;
    const bool kept = mk.cols.size() == cols_in.size();          // the sorted list of the commitment (same columns, same stable order)
    if (!kept && !std::is_sorted(cols_in.begin(), cols_in.end(), by_size)) { sorted_copy = cols_in; std::stable_sort(sorted_copy.begin(), sorted_copy.end(), by_size); }
    const std::vector<DCol>& cols = kept ? mk.cols : sorted_copy.empty() ? cols_in : sorted_copy;
    struct Slot { int kind; size_t first; };   // kind 0: hash witness (8 words), 1: column witness, 2: queried value
    std::vector<Slot> slots;
    slots.reserve(64 + 4 * cols.size());
    std::vector<DCol> lc;
    lc.reserve(cols.size());
    size_t ci = 0;
    std::vector<size_t> last, total;
    static const std::vector<size_t> empty;
    for (int log = (int)mk.max_log; log >= 0; log--) {
        lc.clear();
        while (ci < cols.size() && cols[ci].log_size == (u32)log) lc.push_back(cols[ci++]);
        const u32* prev_hashes = log < (int)mk.max_log ? mk.layers[log + 1] : nullptr;
        const u32 prev_shift = log < (int)mk.max_log ? mk.shifts[log + 1] : 0;
        auto it = queries_per_log.find((u32)log);
        const std::vector<size_t>& colq = it == queries_per_log.end() ? empty : it->second;
        total.clear();
        size_t pi = 0, qi = 0;
        while (pi < last.size() || qi < colq.size()) {
            size_t node;
            if (pi < last.size() && qi < colq.size()) node = std::min(last[pi] / 2, colq[qi]);
            else if (pi < last.size()) node = last[pi] / 2;
            else node = colq[qi];
            if (prev_hashes) {
                for (size_t child = 2 * node; child <= 2 * node + 1; child++) {
                    if (pi < last.size() && last[pi] == child) pi++;
                    else {
                        // in a shard group a hash of a share-wise layer is held by one rank only; the others request a zero
                        const bool shared_layer = log + 1 > mk.band_lo && log + 1 <= mk.band_hi;
                        const bool mine = !shared_layer || (child >> (log + 1 - c.shard.log_count)) == c.shard.rank;
                        slots.push_back({0, g.add_hash(prev_hashes, child >> prev_shift, mine)});
                    }
                }
            }
            bool queried = qi < colq.size() && colq[qi] == node;
            if (queried) qi++;
            for (auto& col : lc) { size_t f = g.add_col(col, node, c.shard.rank); slots.push_back({queried ? 2 : 1, f}); }
            total.push_back(node);
        }
        std::swap(last, total);
    }
    return [slots = std::move(slots), queried_values, dec](const std::vector<u32>& data) {
        for (auto& s : slots) {
            if (s.kind == 0) { Hash32 h; memcpy(h.b, &data[s.first], 32); dec->hash_witness.push_back(h); }
            else if (s.kind == 1) dec->column_witness.push_back(data[s.first]);
            else if (queried_values) queried_values->push_back(data[s.first]);
        }
    };
}

std::vector<size_t> HipProver::fold_queries(const std::vector<size_t>& q, u32 n) {
    std::vector<size_t> o;
    for (size_t x : q) { size_t y = x >> n; if (o.empty() || o.back() != y) o.push_back(y); }
    return o;
}
// compute_decommitment_positions_and_witness_evals with fold_step = 1; witness values are gathered later.
void HipProver::positions_and_witness(const std::vector<size_t>& queries, std::vector<size_t>& positions, std::vector<size_t>& witness_pos) {
    size_t i = 0;
    while (i < queries.size()) {
        size_t j = i;
        while (j < queries.size() && (queries[j] >> 1) == (queries[i] >> 1)) j++;
        size_t start = (queries[i] >> 1) << 1, qi = i;
        for (size_t pos = start; pos < start + 2; pos++) {
            positions.push_back(pos);
            if (qi < j && queries[qi] == pos) { qi++; continue; }
            witness_pos.push_back(pos);
        }
        i = j;
    }
}
HipProver::Finisher HipProver::gather_secure_deferred(Gather& g, const DSecure& s, const std::vector<size_t>& pos, std::vector<Q31>* out) {
    size_t first = g.n_words;
    for (size_t p : pos) for (int w = 0; w < 4; w++) g.add(s.c[w], p, s.mine(p, c.shard.rank));
    size_t n = pos.size();
    return [first, n, out](const std::vector<u32>& d) { for (size_t k = 0; k < n; k++) out->push_back(q_make(d[first + 4 * k], d[first + 4 * k + 1], d[first + 4 * k + 2], d[first + 4 * k + 3])); };
}
std::vector<DCol> HipProver::secure_cols(const DSecure& s) {
    std::vector<DCol> v(4);
    for (int w = 0; w < 4; w++) { v[w].ptr = s.c[w]; v[w].log_size = s.log_size; v[w].shift = 0; v[w].lc = s.lc; }
    return v;
}

HipProver::FriCommitted HipProver::fri_commit(std::vector<DSecure>& quotients, StarkProof& pf, const std::vector<LevelWait>& q_waits,
                                              const std::function<void()>& while_the_commit_phase_runs, bool last_layer_poly) {
    // FriProver::commit — first layer: one Merkle tree over the coordinate columns of every quotient.
    // The channel is stepped on the device through the whole commit phase (k_channel_mix_root_draw): per layer mix_root(root) and
    // draw_felt() run as a one-lane kernel and the folds read alpha from device memory, so the ~25 layers are enqueued back to back
    // with no host round trip. The roots arrive in pinned memory; the host channel replays the same steps afterwards and must end
    // in the same state.
    FriCommitted out;
    std::vector<DCol>& first_cols = out.first_cols;
    for (auto& q : quotients) for (auto& col : secure_cols(q)) first_cols.push_back(col);
    const size_t max_layers = FRI_MAX_LAYERS;
    Hash32* pinned_roots = reinterpret_cast<Hash32*>(c.h_small + 64);                       // [0] first layer, [1 + i] inner layer i
    u32* pinned_chan = reinterpret_cast<u32*>(c.h_small + 64 + 32 * (max_layers + 1));      // digest[8] || n_sent
    u32* d_chan = c.alloc_u32(16);
    u32* d_alpha = c.alloc_u32(8 * (max_layers + 1));
    u32* d_roots = c.alloc_u32(8 * (max_layers + 1));                                        // root copies, read back once
    memcpy(pinned_chan, ch.digest.b, 32); pinned_chan[8] = ch.n_sent;
    // Pipelined with the quotient launches (q_waits): the channel state, the tree layouts and the first-layer tree go to the PARTNER stream —
    // on the main stream they would queue up behind every quotient kernel.
    hipStream_t main_stream = c.stream;
    const bool first_on_aux = c.conv.merkle_channel == 0 && !q_waits.empty();
    if (first_on_aux) c.stream = c.aux_of(main_stream);
    struct StreamRestore { Ctx& c; hipStream_t s; ~StreamRestore() { c.stream = s; } } restore_stream{c, main_stream};
    BF_HIP(hipMemcpyAsync(d_chan, pinned_chan, 36, hipMemcpyHostToDevice, c.stream));
    // Poseidon252Channel is stepped on the host (one root read-back per layer): two serial Hades permutations by a single lane would
    // cost more than the round trip. commit_step = Merkle tree of a layer + mix_root + draw alpha (alpha || alpha^2 -> d_alpha[idx]).
    const bool host_channel = c.conv.merkle_channel == 1;
    u32 line_log = quotients[0].log_size - 1;
    const u32 last_log = cfg.log_last_layer_degree_bound + cfg.log_blowup;
    if (line_log > last_log + max_layers) throw HipError("FRI: too many layers");
    // Shard group: a layer with >= 2^14 rows per rank is row-sharded like the quotients (a fold maps the sibling pair (2i, 2i+1) to cell
    // i, so a rank's row range of the source folds into its row range of the destination). The first layer below that size is produced
    // range-wise into a complete buffer and finished by one all-gather; everything smaller is folded redundantly on every rank.
    auto new_layer = [&](u32 log) {
        DSecure l; l.log_size = log; l.lc = slice_log(log) ? lc() : 0;
        for (int w = 0; w < 4; w++) l.c[w] = l.lc ? alloc_slice(log) : c.alloc_u32(size_t(1) << log);
        return l;
    };
    // Every layer's storage and (device channel) every tree's layout exist before the first launch: the column descriptors and level
    // tables of all ~26 trees reach the device in ONE staging copy instead of one in front of every layer of the serial chain.
    const u32 n_inner = line_log > last_log ? line_log - last_log : 0;
    std::vector<DSecure>& layers = out.layers;
    layers.resize(n_inner + 1);
    out.path.assign(n_inner + 1, 0u); out.path[n_inner] = FRI_NO_TREE << 4; out.d_alpha = d_alpha; out.d_chan = d_chan;
    auto folded_by = [&](u32 k, u32 who, bool quotient) { out.path[k] |= who | (quotient ? (u32)FRI_QUOTIENT : 0u); };
    auto hashed_by = [&](u32 k, u32 who) { out.path[k] |= who << 4; };
    for (u32 i = 0; i <= n_inner; i++) layers[i] = new_layer(line_log - i);
    std::vector<MerklePlan> plans;                  // [0] first layer, [1 + i] inner layer i
    // Layers of 2^17 rows and above (the ones neither k_fri_layer nor k_fri_tail takes): the fold that produces layer k runs inside the
    // leaf launch of layer k's tree (merkle.hip: k_fri_fold_leaf) instead of as a launch of its own in front of it — device channel, one
    // process, neither the folded layer nor what it is folded from cut into row ranges. Everything else keeps the two launches.
    auto fold_leaf = [&](u32 k) {
        return !host_channel && c.shard.count == 1 && k < n_inner && line_log - k >= 17 && layers[k].lc == 0 && (k == 0 ? quotients[0].lc == 0 : layers[k - 1].lc == 0);
    };
    // what the fused launch of layer k's tree folds: src (2^(log + 1) rows, or nullptr: the first line layer), the circle evaluation of that
    // size (or nullptr), alpha_k. It runs on the main stream behind every quotient launch and behind the channel step that draws alpha_k.
    auto describe_fold = [&](u32 k, const DSecure* src, const DSecure* q) {
        MerklePlan& p = plans[1 + k];
        FriFoldLeafArgs& fa = p.fold;
        for (int w = 0; w < 4; w++) { fa.src[w] = src ? src->c[w] : nullptr; fa.quot[w] = q ? q->c[w] : nullptr; fa.dst[w] = layers[k].c[w]; }
        fa.alpha8 = d_alpha + 8 * k; fa.itw = c.d_itw; fa.tw_total = 1u << c.tw_root_log; fa.log = line_log - k;
        p.fold_mode = !src ? FF_CIRCLE : q ? FF_LINE_CIRCLE : FF_LINE;
    };
    if (!host_channel) {
        c.stage_checkpoint();
        StageBatch sb(c);
        plans.reserve(n_inner + 1);
        plans.push_back(merkle_plan(first_cols));
        for (u32 i = 0; i < n_inner; i++) plans.push_back(merkle_plan(secure_cols(layers[i]), fold_leaf(i)));
        sb.end();
    }
    auto commit_step = [&](size_t plan_idx, const std::vector<DCol>& cols, u32 alpha_idx, u32 root_idx) -> DevMerkle {
        if (!host_channel) { ChannelStep st{d_chan, d_alpha + 8 * alpha_idx, d_roots + 8 * root_idx}; return merkle_run(plans[plan_idx], nullptr, /*no_readback=*/true, &st); }
        DevMerkle t = merkle_commit(cols);
        ch.mix_root(t.root);
        const Q31 a = ch.draw_felt(), sq = q_mul(a, a);
        const u32 w[8] = {a.a.a, a.a.b, a.b.a, a.b.b, sq.a.a, sq.a.b, sq.b.a, sq.b.b};
        c.stage_checkpoint();
        const u32* st = c.stage(w, 8);
        BF_HIP(hipMemcpyAsync(d_alpha + 8 * alpha_idx, st, 32, hipMemcpyDeviceToDevice, c.stream));
        return t;
    };
    DevMerkle& first_tree = out.first_tree;
    if (first_on_aux) {
        // level L of the first-layer tree is hashed as soon as the quotient of size L exists; joined before the first fold
        ChannelStep st{d_chan, d_alpha, d_roots};
        first_tree = merkle_run(plans[0], nullptr, /*no_readback=*/true, &st, &q_waits);
        hipEvent_t e3 = c.next_event();
        BF_HIP(hipEventRecord(e3, c.stream));
        c.stream = main_stream;
        BF_HIP(hipStreamWaitEvent(main_stream, e3, 0));
    } else first_tree = commit_step(0, first_cols, 0, 0);
    typedef FriCommitted::Inner Inner;
    std::vector<Inner>& inner = out.inner;
    // destination range of a fold whose SOURCE has 2^src_log rows: the image of this rank's source range when the source is sharded
    auto fold_range = [&](u32 src_log, bool src_sliced, u32& first, u32& count) {
        if (src_sliced) { first = (u32)(slice_first(src_log) >> 1); count = (u32)(slice_cells(src_log) >> 1); } else { first = 0; count = 0; }
    };
    // a complete (unsharded) buffer of which every rank has filled only its range is finished by one all-gather per coordinate
    auto complete = [&](const DSecure& l) { for (int w = 0; w < 4; w++) c.shard.comm->all_gather(c.stream, l.c[w], sizeof(u32) << (l.log_size - lc())); };
    // circle -> line: the largest quotient opens layer 0 (nothing folded into it yet: no zero fill)
    size_t qi = 0;
    if (quotients[0].log_size - 1 != line_log) throw HipError("FRI: first layer size");
    {
        const DSecure& q = quotients[qi++];
        const u32* src[4] = {q.c[0], q.c[1], q.c[2], q.c[3]};
        u32 first, count; fold_range(q.log_size, q.lc != 0, first, count);
        folded_by(0, fold_leaf(0) ? FRI_BY_FOLD_LEAF : FRI_BY_LAUNCHES, true);
        if (fold_leaf(0)) describe_fold(0, nullptr, &q);
        else {
            fold_circle_into_line(c.stream, layers[0].c, src, d_alpha, c.d_itw, c.tw_root_log, q.log_size, /*fresh=*/true, first, count);
            if (q.lc != 0 && layers[0].lc == 0) complete(layers[0]);
        }
    }
    // inner layers: commit layer k (-> alpha_{k+1}), then ONE launch folds it into layer k + 1 together with the quotient of layer k's
    // size (fold_line, then dst * alpha^2 + fold_circle: both with alpha_{k+1}). Below 2^10 rows the rest of the phase is one launch.
    const u32 TAIL_LOG = 10;
    // layers of 2^11 .. 2^16 rows: fold + tree + channel step in ONE launch (merkle.hip: k_fri_layer) — device channel, one process
    // (in a shard group: layers every rank holds whole, folded from a layer every rank holds whole)
    auto fused = [&](u32 k) { const u32 lg = line_log - k; return !host_channel && k >= 1 && k < n_inner && lg >= 11 && lg <= 16 && layers[k].lc == 0 && layers[k - 1].lc == 0; };
    auto take_quotient = [&](u32 size) -> const DSecure* {
        const DSecure* q = (qi < quotients.size() && quotients[qi].log_size == size) ? &quotients[qi++] : nullptr;
        if (qi < quotients.size() && quotients[qi].log_size == size) throw HipError("FRI: two quotient columns of one size");
        return q;
    };
    u32* d_counter = nullptr;
    u32 li = 0;
    for (; li < n_inner; li++) {
        const u32 log = line_log - li;
        if (!host_channel && log <= TAIL_LOG) break;
        Inner in; in.ev = layers[li];
        if (fused(li)) {
            d_counter = c.merkle_counter();
            const DSecure* q = take_quotient(log + 1);        // the circle evaluation that folds into this layer
            const DevMerkle& mk = plans[1 + li].mk;
            if (mk.max_log != log) throw HipError("FRI layer: tree layout");
            FriLayerArgs fa{};
            for (int w = 0; w < 4; w++) { fa.src[w] = layers[li - 1].c[w]; fa.quot[w] = q ? q->c[w] : nullptr; fa.dst[w] = layers[li].c[w]; }
            for (u32 lg = 0; lg <= log; lg++) { if (mk.shifts[lg] != 0) throw HipError("FRI layer: replicated level"); fa.tree[lg] = (uint4*)mk.layers[lg]; }
            fa.alpha8 = d_alpha + 8 * li; fa.itw = c.d_itw; fa.tw_total = 1u << c.tw_root_log; fa.log = log; fa.rfc = c.conv.merkle_node_hash ? 0xFFFFFFFFu : 0u;
            fa.counter = d_counter; fa.chan = d_chan; fa.alpha_out = d_alpha + 8 * (li + 1); fa.root_out = d_roots + 8 * (1 + li);
            fri_layer(c.stream, fa);
            in.tree = mk;
            folded_by(li, FRI_BY_LAYER_KERNEL, q != nullptr); hashed_by(li, FRI_BY_LAYER_KERNEL);
        } else { in.tree = commit_step(1 + li, secure_cols(layers[li]), li + 1, 1 + li); hashed_by(li, fold_leaf(li) ? FRI_BY_FOLD_LEAF : FRI_BY_LAUNCHES); }
        inner.push_back(in);
        if (fused(li + 1)) continue;                           // the next layer folds this one itself
        const DSecure* q = take_quotient(log);
        DSecure& next = layers[li + 1];
        const u32* src[4] = {layers[li].c[0], layers[li].c[1], layers[li].c[2], layers[li].c[3]};
        const u32* qs[4] = {q ? q->c[0] : nullptr, q ? q->c[1] : nullptr, q ? q->c[2] : nullptr, q ? q->c[3] : nullptr};
        if (q && (q->lc != 0) != (layers[li].lc != 0)) throw HipError("FRI: a layer and the quotient of its size are sharded differently");
        folded_by(li + 1, fold_leaf(li + 1) ? FRI_BY_FOLD_LEAF : FRI_BY_LAUNCHES, q != nullptr);
        if (fold_leaf(li + 1)) { describe_fold(li + 1, &layers[li], q); continue; }      // the next layer's leaf launch folds this one
        u32 first, count; fold_range(log, layers[li].lc != 0, first, count);
        fold_line_circle(c.stream, next.c, src, q ? qs : nullptr, d_alpha + 8 * (li + 1), c.d_itw, c.tw_root_log, log, first, count);
        if (layers[li].lc != 0 && next.lc == 0) complete(next);
    }
    if (li < n_inner) {
        // k_fri_tail: layers li .. n_inner - 1 (2^TAIL_LOG rows and below): trees, channel steps and folds by one workgroup
        FriTailArgs ta{};
        ta.n_layers = n_inner - li; ta.top_log = line_log - li; ta.alpha_idx = li + 1; ta.root_idx = 1 + li;
        ta.chan = d_chan; ta.alpha = d_alpha; ta.roots = d_roots; ta.itw = c.d_itw; ta.tw_total = 1u << c.tw_root_log; ta.rfc = c.conv.merkle_node_hash ? 0xFFFFFFFFu : 0u;
        if (ta.n_layers > 10 || ta.top_log > TAIL_LOG) throw HipError("FRI tail: too many layers");
        for (u32 k = 0; k < ta.n_layers; k++) {
            const u32 log = ta.top_log - k;
            FriTailLayer& L = ta.layer[k];
            for (int w = 0; w < 4; w++) L.ev[w] = layers[li + k].c[w];
            if (qi < quotients.size() && quotients[qi].log_size == log) { for (int w = 0; w < 4; w++) L.quot[w] = quotients[qi].c[w]; qi++; }
            folded_by(li + k + 1, FRI_BY_TAIL, L.quot[0] != nullptr); hashed_by(li + k, FRI_BY_TAIL);
            const DevMerkle& mk = plans[1 + li + k].mk;
            if (mk.max_log != log) throw HipError("FRI tail: tree layout");
            for (u32 lg = 0; lg <= log; lg++) { if (mk.shifts[lg] != 0) throw HipError("FRI tail: replicated level"); L.tree[lg] = (uint4*)mk.layers[lg]; }
            Inner in; in.ev = layers[li + k]; in.tree = mk;
            inner.push_back(in);
        }
        for (int w = 0; w < 4; w++) ta.ev_last[w] = layers[n_inner].c[w];
        double tail_nodes = 0;
        for (u32 k = 0; k < ta.n_layers; k++) tail_nodes += (double)((2u << (ta.top_log - k)) - 1);
        c.stage_checkpoint();
        fri_tail(c.stream, c.stage(&ta, 1), 48.0 * tail_nodes, tail_nodes);
    }
    DSecure layer = layers[n_inner];
    line_log = last_log;
    if (qi != quotients.size()) throw HipError("FRI: not all columns consumed");
    BF_HIP(hipGetLastError());
    if (!host_channel) {
        BF_HIP(hipMemcpyAsync(pinned_chan, d_chan, 36, hipMemcpyDeviceToHost, c.stream));
        BF_HIP(hipMemcpyAsync(pinned_roots, d_roots, 32 * (1 + inner.size()), hipMemcpyDeviceToHost, c.stream));
    }
    // last layer: 2^last_log evaluations -> line polynomial (host; LineEvaluation::interpolate on <= 2 values for the default config)
    {
        if (cfg.log_last_layer_degree_bound != 0) throw HipError("only log_last_layer_degree_bound 0 is supported");
        std::vector<size_t> pos;
        for (size_t p = 0; p < (size_t(1) << last_log); p++) pos.push_back(p);
        mark("FRI commit phase enqueued");
        Gather gl;
        for (size_t p : pos) for (int w = 0; w < 4; w++) gl.add(layer.c[w], p, layer.mine(p, c.shard.rank));
        // the commit phase (~100 launches) is in flight: the host does its own checks now; a failed check waits for the stream before it
        // unwinds (the arena must not be handed out again under running kernels)
        try { while_the_commit_phase_runs(); } catch (...) { (void)hipStreamSynchronize(c.stream); throw; }
        mark("sanity check done");
        static const int last_layer_slot = [] { const char* v = getenv("BFHIP_MB_TAIL"); return v && v[0] == '2' ? -1 : 6; }();
        auto dl = gl.run(c, last_layer_slot);
        std::vector<Q31> v;
        for (size_t k = 0; k < pos.size(); k++) v.push_back(q_make(dl[4 * k], dl[4 * k + 1], dl[4 * k + 2], dl[4 * k + 3]));          // synchronises: roots and the device channel state are on the host now
        mark("FRI last layer arrived");
        if (!host_channel) {
            first_tree.root = pinned_roots[0];
            ch.mix_root(first_tree.root); (void)ch.draw_felt();
            for (size_t li = 0; li < inner.size(); li++) { inner[li].tree.root = pinned_roots[1 + li]; ch.mix_root(inner[li].tree.root); (void)ch.draw_felt(); }
            if (memcmp(pinned_chan, ch.digest.b, 32) != 0 || pinned_chan[8] != ch.n_sent) throw HipError("FRI: device channel diverged from the host channel");
        }
        // bound 0: the 2^b evaluations are those of a constant line polynomial — all equal, and line_ifft's only nonzero coefficient is
        // that value (at b = 1: c0 = (v0 + v1) / 2 = v0, c1 = (v0 - v1) / (2 x0) = 0)
        if (last_layer_poly) {
            for (const Q31& x : v) if (!q_eq(x, v[0])) throw HipError("invalid degree");
            Q31 c0 = v[0];
            pf.fri_proof.last_layer_coeffs = {c0};
            pf.fri_proof.last_layer_log_size = 0;
            ch.mix_felts(&c0, 1);
        }
    }
    tap("fri_commit");
    return out;
}

void HipProver::grind(StarkProof& pf) {
    const bool host_channel = c.conv.merkle_channel == 1;      // Poseidon252Channel: stepped on the host (see fri_commit)
    // proof of work (GrindOps): GPU search in spans, smallest nonce wins. Poseidon252Channel: one Hades permutation per nonce and a
    // 1-in-8 hit rate at pow_bits = 5 (the test reads the top byte of the big-endian digest, which is 0..8) — searched on the host: at the
    // cap of 12 bits that is 128 expected permutations, less than a launch and a read-back of bfhip_grind_poseidon252's kernel.
    if (host_channel) {
        u64 nonce = 0;
        for (;; nonce++) { Channel t = ch; t.mix_u64(nonce); if (t.trailing_zeros() >= cfg.pow_bits) break; if (nonce > (u64(1) << 32)) throw HipError("grind: no nonce found"); }
        pf.proof_of_work = nonce;
        ch.mix_u64(nonce);
    } else if (cfg.pow_bits <= 10 && [&]() {
        // A few bits of work are found faster by the host than by a launch and a read-back (~35 us): 2^pow_bits tries of one compression
        // each on average. GrindOps asks for the SMALLEST nonce: a linear scan from zero finds it. Larger work goes to the GPU search.
        for (u64 nonce = 0; nonce < (u64(64) << cfg.pow_bits); nonce++) {
            Channel t = ch; t.mix_u64(nonce);
            if (t.trailing_zeros() >= cfg.pow_bits) { pf.proof_of_work = nonce; ch.mix_u64(nonce); return true; }
        }
        return false; }()) {
    } else {
        c.stage_checkpoint();
        u32* d_digest = (u32*)c.stage(ch.digest.b, 32);
        unsigned long long init = ~0ull;
        unsigned long long* d_best = (unsigned long long*)c.stage(&init, 1);
        unsigned long long best = ~0ull;
        // one span per launch and read-back: 2^pow_bits nonces (one expected hit), at least 2^16 and at most 2^22 (~0.12 ms of the grid) —
        // pow 26 takes ~16 round trips instead of the ~1024 of fixed 2^16-nonce spans
        const u32 span = 1u << std::min(std::max(cfg.pow_bits, 16u), 22u);
        for (u64 base = 0; best == ~0ull; base += span) {
            if (base >= (u64(1) << 40)) throw HipError("grind: no nonce found below 2^40");
            grind_span(c.stream, d_digest, base, span, cfg.pow_bits, d_best, c.conv.mix_u64);
            c.read_back(&best, d_best, 8);
        }
        pf.proof_of_work = best;
        ch.mix_u64(best);
    }
    mark("nonce found");
}

void HipProver::decommit_queries(std::vector<DTree>& trees, const std::vector<DSecure>& quotients, const FriCommitted& fc, StarkProof& pf) {
    const DevMerkle& first_tree = fc.first_tree;
    const std::vector<DCol>& first_cols = fc.first_cols;
    const std::vector<FriCommitted::Inner>& inner = fc.inner;
    // FRI decommit
    double t0 = now();
    u32 max_log = quotients[0].log_size;
    std::vector<size_t> queries;
    {
        std::set<size_t> qs; u32 cnt = 0; u32 maskq = (u32)((u64(1) << max_log) - 1);
        while (cnt < cfg.n_queries) {   // Queries::generate: chunks_exact(4) of the drawn bytes (32 per draw for Blake2s, 31 for Poseidon252)
            std::vector<u8> r = ch.draw_random_bytes();
            for (size_t k = 0; 4 * k + 4 <= r.size() && cnt < cfg.n_queries; k++) { u32 w; memcpy(&w, r.data() + 4 * k, 4); qs.insert(w & maskq); cnt++; }
        }
        queries.assign(qs.begin(), qs.end());
    }
    std::map<u32, std::vector<size_t>> positions_by_log;
    for (auto& q : quotients) positions_by_log[q.log_size] = fold_queries(queries, max_log - q.log_size);
    // All decommitment reads (FRI witnesses, Merkle witnesses, queried values) are planned first and fetched by ONE gather launch:
    // the control flow depends only on the query positions.
    Gather g;
    g.reqs.reserve(4096);
    std::vector<Finisher> fin;
    fin.reserve(64);
    {
        std::map<u32, std::vector<size_t>> dpos;
        for (auto& q : quotients) {
            std::vector<size_t> pos, wpos;
            positions_and_witness(fold_queries(queries, max_log - q.log_size), pos, wpos);
            dpos[q.log_size] = pos;
            fin.push_back(gather_secure_deferred(g, q, wpos, &pf.fri_proof.first_layer.fri_witness));
        }
        fin.push_back(decommit(g, first_tree, first_cols, dpos, nullptr, &pf.fri_proof.first_layer.decommitment));
        pf.fri_proof.first_layer.commitment = first_tree.root;
    }
    auto lq = fold_queries(queries, 1);
    pf.fri_proof.inner_layers.resize(inner.size());
    for (size_t li = 0; li < inner.size(); li++) {
        auto& in = inner[li];
        FriLayerProof& lp = pf.fri_proof.inner_layers[li];
        std::vector<size_t> pos, wpos;
        positions_and_witness(lq, pos, wpos);
        fin.push_back(gather_secure_deferred(g, in.ev, wpos, &lp.fri_witness));
        std::map<u32, std::vector<size_t>> dpos; dpos[in.ev.log_size] = pos;
        fin.push_back(decommit(g, in.tree, secure_cols(in.ev), dpos, nullptr, &lp.decommitment));
        lp.commitment = in.tree.root;
        lq = fold_queries(lq, 1);
    }
    pf.queried_values.resize(trees.size());
    pf.decommitments.resize(trees.size());
    for (size_t ti = 0; ti < trees.size(); ti++) {
        fin.push_back(decommit(g, trees[ti].mk, trees[ti].evals, positions_by_log, &pf.queried_values[ti], &pf.decommitments[ti]));
        pf.commitments.push_back(trees[ti].mk.root);
    }
    mark("decommitment planned");
    // The proof's LAST wait is an event wait on purpose: with stamps the host never asks the runtime about the stream, and the runtime keeps
    // the bookkeeping of every launch until somebody does — one real synchronisation per proof, at the point where the stream is about to
    // drain anyway, releases it (without it the next proofs' launches slow down: fib19 +0.3 ms in the mean, r04)
    static const int tail_slot = [] { const char* v = getenv("BFHIP_MB_TAIL"); return v && v[0] == '1' ? 7 : -1; }();
    std::vector<u32> data = g.run(c, tail_slot);
    mark("decommitment data arrived");
    for (auto& f : fin) f(data);
    tm.decommit = now() - t0;
}

}  // namespace bf

#ifdef BFHIP_TEST_HOOKS
#include "api_guard.h"
// libbfhip_testhooks.so only (Makefile); not declared in include/bfhip.h. Runs HipProver::fri_commit — the driver above, nothing of it restated — on the
// caller's columns, from a caller-given channel digest (n_sent 0), and hands back everything the commit phase leaves in HBM, so that
// tests/test_gpu_fri_commit.py can compare each fused path with tests/fri_commit_model.py layer by layer: tree nodes no query of a proof opens, layers
// folded without a quotient, the channel's rejected draws. The columns need no low degree: the last layer is returned as it is (last_layer_poly = false).
//   log_sizes[n_cols] distinct and descending, cols_h[4 * n_cols] host arrays of 2^log_sizes[k] words (the 4 coordinates of column k).
//   With line_log = log_sizes[0] - 1 and n_inner = line_log - log_blowup_factor:
//   layers_out  layer 0 .. n_inner, each its 4 coordinate columns of 2^(line_log - k) words
//   trees_out   the first-layer tree, then the tree of layer 0 .. n_inner - 1: every level, deepest first, 8 words per node
//   roots_out, alphas_out   8 words per channel step (first-layer tree, layer 0 .. n_inner - 1): the root mixed, alpha || alpha^2 drawn
//   chan_out    digest[8] || n_sent of the device channel at the end (Poseidon252 channel: of the host channel, the only one there is)
//   paths_out   n_inner + 1 words, HipProver::FriCommitted::path
extern "C" int32_t bfhip_test_fri_commit(bfhip_ctx* ctx, const uint8_t* digest32, uint32_t n_cols, const uint32_t* log_sizes, const uint32_t* const* cols_h,
                                          uint32_t* layers_out, uint32_t* trees_out, uint32_t* roots_out, uint32_t* alphas_out, uint32_t* chan_out, uint32_t* paths_out) {
    using namespace bf;
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!digest32 || !log_sizes || !cols_h || !layers_out || !trees_out || !roots_out || !alphas_out || !chan_out || !paths_out) throw HipError("null argument");
    if (c.shard.count > 1) throw HipError("bfhip_test_fri_commit: the context is in a shard group");
    c.refuse_in_session("bfhip_test_fri_commit");
    if (n_cols == 0) throw HipError("bfhip_test_fri_commit: no columns");
    for (u32 k = 0; k < 4 * n_cols; k++) if (!cols_h[k]) throw HipError("null argument");
    for (u32 k = 1; k < n_cols; k++) if (log_sizes[k] >= log_sizes[k - 1]) throw HipError("bfhip_test_fri_commit: the column sizes must be distinct and descending");
    HipProver pv(c, 0);
    const u32 last_log = pv.cfg.log_last_layer_degree_bound + pv.cfg.log_blowup;
    if (pv.cfg.log_last_layer_degree_bound != 0) throw HipError("only log_last_layer_degree_bound 0 is supported");
    if (log_sizes[n_cols - 1] < last_log + 1) throw HipError("bfhip_test_fri_commit: the smallest column lies below log_blowup_factor + 1");
    if (log_sizes[n_cols - 1] < 3) throw HipError("bfhip_test_fri_commit: a circle evaluation has at least 8 rows");
    if (log_sizes[0] > c.tw_root_log) throw HipError("bfhip_test_fri_commit: context twiddle tree too small for the largest column");
    const u32 line_log = log_sizes[0] - 1;
    if (line_log > last_log + HipProver::FRI_MAX_LAYERS) throw HipError("bfhip_test_fri_commit: more layers than the commit phase allows");
    sync_both(c);
    c.arena.reset();
    c.use_mailbox = false;
    c.stage_checkpoint();
    pv.ch = Channel(c.conv);
    memcpy(pv.ch.digest.b, digest32, 32); pv.ch.n_sent = 0;
    std::vector<DSecure> quotients(n_cols);
    for (u32 k = 0; k < n_cols; k++) {
        quotients[k].log_size = log_sizes[k];
        for (int w = 0; w < 4; w++) {
            quotients[k].c[w] = c.alloc_u32(size_t(1) << log_sizes[k]);
            BF_HIP(hipMemcpyAsync(quotients[k].c[w], cols_h[4 * k + w], sizeof(u32) << log_sizes[k], hipMemcpyHostToDevice, c.stream));
        }
    }
    StarkProof pf;
    HipProver::FriCommitted fc;
    try { fc = pv.fri_commit(quotients, pf, {}, [] {}, /*last_layer_poly=*/false); } catch (...) { (void)hipStreamSynchronize(c.stream); throw; }
    sync_both(c);
    const u32 n_inner = (u32)fc.inner.size();
    if (fc.layers.size() != n_inner + 1 || fc.path.size() != n_inner + 1) throw HipError("bfhip_test_fri_commit: layer count");
    for (u32 k = 0; k <= n_inner; k++) {
        const DSecure& l = fc.layers[k];
        for (int w = 0; w < 4; w++) { BF_HIP(hipMemcpy(layers_out, l.c[w], sizeof(u32) << l.log_size, hipMemcpyDeviceToHost)); layers_out += size_t(1) << l.log_size; }
        paths_out[k] = fc.path[k];
    }
    for (u32 t = 0; t <= n_inner; t++) {
        const DevMerkle& mk = t == 0 ? fc.first_tree : fc.inner[t - 1].tree;
        for (int lg = (int)mk.max_log; lg >= 0; lg--) {
            if (mk.shifts[lg] != 0) throw HipError("bfhip_test_fri_commit: replicated tree level");
            BF_HIP(hipMemcpy(trees_out, mk.layers[lg], size_t(32) << lg, hipMemcpyDeviceToHost));
            trees_out += size_t(8) << lg;
        }
        memcpy(roots_out + 8 * t, mk.root.b, 32);
    }
    BF_HIP(hipMemcpy(alphas_out, fc.d_alpha, 32 * (n_inner + 1), hipMemcpyDeviceToHost));
    if (c.conv.merkle_channel == 1) { memcpy(chan_out, pv.ch.digest.b, 32); chan_out[8] = pv.ch.n_sent; }
    else BF_HIP(hipMemcpy(chan_out, fc.d_chan, 36, hipMemcpyDeviceToHost));
    return 0;
    API_CATCH
}
#endif
