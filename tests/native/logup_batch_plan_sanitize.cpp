// Stand-alone driver (its own main) for the host-only planner of bfhip_logup_program_generate_batch (csrc/logup_batch_plan.h), built by
// tests/test_logup_batch_cpu.py with g++ -fsanitize=address,undefined and run once. Over the component lists of the GPU tests (seams,
// 64 x log_size 1, LDS sizing, the launch threshold, more than one chunk of tile totals) in the four launch modes it checks by brute
// force that every wave of every row-stage launch, every scan tile and every 256-cell block maps to exactly one (component, local index) and
// that all of them are covered, that the tables do not decrease, that the scratch regions are 16-byte aligned, pairwise disjoint and within
// the stated bound; then the interval-overlap check on hand-made ranges.
#include "../../stwo-brainfuck_amd/csrc/logup_batch_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

using namespace bf;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// what the kernels do with a table: the entry k with table[k] <= b < table[k + 1], the last one if none follows
static uint32_t find(const uint32_t* table, uint32_t n, uint32_t b) {
    uint32_t k = 0;
    while (k + 1 < n && b >= table[k + 1]) k++;
    return k;
}

static void check_list(const std::vector<uint32_t>& logs, const std::vector<size_t>& lds, int mode) {
    const uint32_t n = (uint32_t)logs.size();
    const LogupBatchPlan p = logup_batch_plan(logs.data(), lds.data(), n, mode);
    CHECK(p.tile0.size() == n + 1 && p.block0.size() == n + 1 && p.scratch.size() == n && p.segs.size() == n);

    // row stage: every wave of every launch belongs to one component; every (component, wave) is owned exactly once over all launches
    std::map<std::pair<uint32_t, uint32_t>, int> owned;
    size_t segs_seen = 0;
    for (const LogupBatchGroup& g : p.groups) {
        CHECK(g.count >= 1 && g.first == segs_seen && g.first + g.count <= p.segs.size());
        segs_seen += g.count;
        const LogupBatchSeg* segs = p.segs.data() + g.first;
        CHECK(segs[0].block0 == 0);
        size_t max_lds = 0;
        for (size_t i = 0; i < g.count; i++) {
            if (i) CHECK(segs[i].block0 >= segs[i - 1].block0);
            CHECK(segs[i].comp < n);
            max_lds = std::max(max_lds, lds[segs[i].comp]);
            if (mode == 3 && g.count > 1) CHECK(logs[segs[i].comp] < LOGUP_BATCH_ALONE_LOG);
            // the rule: no wave of a large component gets LDS that lowers its occupancy; a small component never launches alone beside others
            if (mode == 0 && logs[segs[i].comp] >= LOGUP_BATCH_ALONE_LOG) CHECK(logup_batch_waves_per_cu(g.lds) == logup_batch_waves_per_cu(lds[segs[i].comp]) || g.lds == lds[segs[i].comp]);
            if ((mode == 0 || mode == 3) && logs[segs[i].comp] < LOGUP_BATCH_ALONE_LOG) CHECK(&g == &p.groups[0]);
        }
        CHECK(g.lds == max_lds);
        if (mode == 2) CHECK(g.count == 1);
        for (uint32_t b = 0; b < g.blocks; b++) {
            uint32_t k = 0;
            while (k + 1 < g.count && b >= segs[k + 1].block0) k++;
            const uint32_t comp = segs[k].comp, wave = b - segs[k].block0;
            CHECK((size_t)wave * LOGUP_BATCH_WAVE < (size_t(1) << logs[comp]));      // the wave has at least one cell of the component
            owned[{comp, wave}]++;
        }
    }
    CHECK(segs_seen == p.segs.size());
    if (mode == 1) CHECK(p.groups.size() == 1);
    size_t waves = 0;
    for (uint32_t k = 0; k < n; k++) waves += ((size_t(1) << logs[k]) + LOGUP_BATCH_WAVE - 1) / LOGUP_BATCH_WAVE;
    CHECK(owned.size() == waves);
    for (const auto& e : owned) CHECK(e.second == 1);

    // scan tiles and 256-cell blocks
    for (int which = 0; which < 2; which++) {
        const std::vector<uint32_t>& t = which ? p.block0 : p.tile0;
        CHECK(t[0] == 0);
        for (uint32_t k = 0; k < n; k++) {
            const size_t N = size_t(1) << logs[k];
            const size_t want = which ? (N + LOGUP_BATCH_BLOCK - 1) / LOGUP_BATCH_BLOCK : (N / 2 + LOGUP_BATCH_TILE - 1) / LOGUP_BATCH_TILE;
            CHECK(t[k + 1] >= t[k] && t[k + 1] - t[k] == want && want >= 1);
        }
        std::vector<uint32_t> count(n, 0);
        for (uint32_t b = 0; b < t[n]; b++) {
            const uint32_t k = find(t.data(), n, b);
            CHECK(k < n && b >= t[k] && b < t[k + 1]);
            CHECK(b - t[k] == count[k]);      // local indices come in order, each once
            count[k]++;
        }
        for (uint32_t k = 0; k < n; k++) CHECK(count[k] == t[k + 1] - t[k]);
    }

    // scratch: aligned, disjoint, within the bound
    std::vector<std::pair<size_t, size_t>> regions;
    size_t bound = 0;
    for (uint32_t k = 0; k < n; k++) {
        const size_t N = size_t(1) << logs[k];
        const LogupBatchScratch& s = p.scratch[k];
        CHECK(s.nb == p.tile0[k + 1] - p.tile0[k]);
        regions.push_back({s.v, s.v + 16 * N});
        regions.push_back({s.wloc, s.wloc + 16 * (N / 2)});
        regions.push_back({s.totals, s.totals + 16 * (size_t(s.nb) + 1)});
        bound += logup_scratch_bound(logs[k]);
    }
    regions.push_back({p.tails, p.tails + 32 * size_t(n)});
    for (size_t i = 0; i < regions.size(); i++) {
        CHECK(regions[i].first % 16 == 0 && regions[i].second % 16 == 0 && regions[i].first < regions[i].second && regions[i].second <= p.bytes);
        for (size_t j = 0; j < i; j++) CHECK(regions[i].second <= regions[j].first || regions[j].second <= regions[i].first);
    }
    CHECK(p.bytes <= bound);
}

static bool overlap(std::vector<LogupBatchRange> r, uint32_t* ca = nullptr, uint32_t* cb = nullptr) {
    LogupBatchRange a{}, b{};
    const bool hit = logup_batch_overlap(r, a, b);
    if (hit && ca) { *ca = a.comp; *cb = b.comp; }
    return hit;
}

int main() {
    const size_t small = 256 * (3 + 4 * 3), caps = 256 * (96 + 4 * 24);
    const std::vector<std::pair<std::vector<uint32_t>, std::vector<size_t>>> lists = {
        {{1, 12, 6, 11, 5, 12}, std::vector<size_t>(6, small)}, {{12, 5, 11, 6, 12, 1}, std::vector<size_t>(6, small)},      // GPU test 1
        {std::vector<uint32_t>(64, 1), std::vector<size_t>(64, small)}, {{6}, {small}},                                      // 2
        {{7, 7}, {caps, small}}, {{7, 7}, {small, caps}},                                                                    // 3
        {{15, 16, 17}, {small, small + 256, small + 512}}, {{17, 15, 16}, {small, caps, small}},                            // 4
        {{20, 4}, {small, small}}, {{4, 20}, {small, small}},                                                                // 5
    };
    int lists_checked = 0;
    for (const auto& l : lists)
        for (int mode = 0; mode < 4; mode++) { check_list(l.first, l.second, mode); lists_checked++; }
    {   // the threshold list under the size rule (mode 3): 15 shares, 16 and 17 launch alone, each with its own LDS
        const uint32_t logs[3] = {15, 16, 17};
        const size_t lds[3] = {1024, 2048, 512};
        const LogupBatchPlan p = logup_batch_plan(logs, lds, 3, 3);
        CHECK(p.groups.size() == 3 && p.groups[0].blocks == 512 && p.groups[0].lds == 1024 && p.groups[1].blocks == 1024 && p.groups[1].lds == 2048 &&
              p.groups[2].blocks == 2048 && p.groups[2].lds == 512);
        CHECK(p.segs[0].comp == 0 && p.segs[1].comp == 1 && p.segs[2].comp == 2);
        // the rule (mode 0) on the same list: 2048 bytes a wave do not bound the occupancy (32 waves a CU up to 5120 bytes), so one launch
        const LogupBatchPlan q = logup_batch_plan(logs, lds, 3, 0);
        CHECK(q.groups.size() == 1 && q.groups[0].blocks == 512 + 1024 + 2048 && q.groups[0].lds == 2048 && q.segs[2].block0 == 1536);
        // with a program at the caps (48 KiB: 3 waves a CU) in a small component: the two large ones launch alone, 15 shares with it
        const uint32_t logs4[4] = {15, 16, 3, 17};
        const size_t lds4[4] = {1024, 2048, caps, 512};
        const LogupBatchPlan r = logup_batch_plan(logs4, lds4, 4, 0);
        CHECK(r.groups.size() == 3 && r.groups[0].count == 2 && r.groups[0].lds == caps && r.groups[0].blocks == 513 && r.segs[0].comp == 0 && r.segs[1].comp == 2 &&
              r.segs[2].comp == 1 && r.groups[1].lds == 2048 && r.segs[3].comp == 3 && r.groups[2].lds == 512);
        // the large component that has the largest program stays in the shared launch: nothing is gained by its own
        const size_t lds5[4] = {1024, caps, 512, 2048};
        const LogupBatchPlan t = logup_batch_plan(logs4, lds5, 4, 0);
        CHECK(t.groups.size() == 2 && t.groups[0].count == 3 && t.groups[0].lds == caps && t.segs[3].comp == 3 && t.groups[1].lds == 2048);
        CHECK(logup_batch_waves_per_cu(0) == 32 && logup_batch_waves_per_cu(5120) == 32 && logup_batch_waves_per_cu(5121) == 31 && logup_batch_waves_per_cu(caps) == 3);
    }

    // ranges: {lo, hi, component, output}
    uint32_t a = 99, b = 99;
    CHECK(!overlap({}));
    CHECK(!overlap({{0, 16, 0, true}, {16, 32, 1, true}, {32, 48, 1, false}}));                           // touching
    CHECK(!overlap({{100, 200, 0, false}, {100, 200, 1, false}, {150, 160, 2, false}}));                  // inputs may share
    CHECK(!overlap({{0, 16, 0, true}, {1000, 1016, 1, true}, {500, 600, 2, false}}));                     // disjoint
    CHECK(overlap({{0, 16, 0, true}, {15, 31, 1, true}}, &a, &b) && a == 0 && b == 1);                    // one byte shared
    CHECK(overlap({{40, 50, 3, true}, {0, 100, 2, false}}, &a, &b) && a == 2 && b == 3);                  // an output nested in an input
    CHECK(overlap({{0, 100, 2, true}, {40, 50, 3, false}}, &a, &b) && a == 2 && b == 3);                  // an input nested in an output
    CHECK(overlap({{0, 100, 5, false}, {10, 20, 6, false}, {50, 60, 7, true}}, &a, &b) && a == 5 && b == 7);      // past a nested input, still inside the long one
    CHECK(overlap({{0, 100, 5, true}, {10, 20, 6, true}}, &a, &b) && a == 5 && b == 6);
    CHECK(overlap({{64, 128, 4, true}, {64, 128, 4, true}}, &a, &b) && a == 4 && b == 4);                 // one pointer given twice
    CHECK(!overlap({{64, 64, 0, true}, {0, 128, 1, false}}));                                             // an empty range
    CHECK(overlap({{~uint64_t(0) - 15, ~uint64_t(0), 0, true}, {~uint64_t(0) - 7, ~uint64_t(0), 1, false}}, &a, &b) && a == 0 && b == 1);      // at the top of the address space

    printf("lists checked: %d; failures: %d\n", lists_checked, failures);
    return failures ? 1 : 0;
}
