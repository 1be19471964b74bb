// Stand-alone driver (its own main) for the host-only FFT planner (csrc/fft_plan.h), built by tests/test_fft_plan_cpu.py with
// g++ -fsanitize=address,undefined and run once. It prints, for that test to read and to hash:
//   C  the named constants of the planner;
//   S  one line per single-job plan: inverse at log 0..28 and forward at every src_log <= log <= 28, times 24 column counts on both sides of every
//      cols_per_block rule, tw_root_log = 28 — under each of the four knob settings in circle mode, and under the default knobs in line mode;
//   M  multi-job plans under each knob setting: the size classes of the four commitment sessions of tests/fft_plan_model.py (per tree the forward plan,
//      for the tree of evaluations the inverse plan too), and a batch without a job of 2^12 cells or more, whose small transforms find no launch to ride in.
// A line is "<header> | <launch> ; <group> ; <group> | <launch> ; ..." with key=value fields. A group lists the fields of PassArgs that its kernel reads
// (tile_log only for a contiguous pass of k_fft_tile12 / k_fft_pass, cols_per_block not for k_fft_tiny), pointers as symbols: src / dst = which array of
// the group's job, tw / itw. Doubles are printed exactly (%a).
#include "../../stwo-brainfuck_amd/csrc/fft_plan.h"
#include <cstdio>
#include <string>

using namespace bf;

static u32* slots[64];          // job j: d_src = &slots[2 j], d_dst = &slots[2 j + 1]; never dereferenced
static u32 tw_word, itw_word;
static const u32 TW_ROOT_LOG = 28;

static FftJob job(size_t j, u32 ncols, u32 log, u32 src_log, bool circle) { return FftJob{&slots[2 * j], &slots[2 * j + 1], ncols, log, src_log, circle}; }

static void print_plan(const std::string& header, bool inverse, const std::vector<FftJob>& jobs, FftKnobs knobs) {
    FftPlan plan;
    fft_plan(plan, inverse, jobs.data(), jobs.size(), &tw_word, &itw_word, TW_ROOT_LOG, knobs);
    printf("%s knobs=%d%d inv=%d jobs=", header.c_str(), knobs.two_pass, knobs.fuse_small, plan.inverse);
    for (size_t j = 0; j < jobs.size(); j++) printf("%s%u:%u:%u:%d", j ? "," : "", jobs[j].log, jobs[j].src_log, jobs[j].ncols, jobs[j].circle);
    for (const FftLaunch& L : plan.launches) {
        printf(" | kind=%d ngroups=%u total_blocks=%u bytes=%a alg=%a bfly=%a", L.kind, L.ngroups, L.total_blocks, L.bytes, L.alg, L.bfly);
        for (u32 g = L.first_group; g < L.first_group + L.ngroups; g++) {
            const PassArgs& a = plan.groups[g];
            size_t j = 0;
            while (j < jobs.size() && a.dst != jobs[j].d_dst) j++;
            const char* src = j == jobs.size() ? "?" : a.src == jobs[j].d_src ? "src" : a.src == (const u32* const*)jobs[j].d_dst ? "dst" : "?";
            const int kernel = a.kind ? (int)a.kind : L.kind;      // whose body runs the group
            printf(" ; job=%zu gkind=%u src=%s ncols=%u log=%u lo=%u k=%u src_mask=%#x circle=%u scale=%u tw_total=%u tw=%s block0=%u grid_x=%u",
                   j, a.kind, src, a.ncols, a.log, a.lo, a.k, a.src_mask, a.circle, a.scale, a.tw_total, a.tw == &tw_word ? "tw" : a.tw == &itw_word ? "itw" : "?", a.block0, a.grid_x);
            if (kernel != K_TINY) printf(" cpb=%u", a.cols_per_block);
            if (a.lo == 0 && (kernel == K_TILE12 || kernel == K_PASS)) printf(" tile_log=%u", a.tile_log);
        }
    }
    printf("\n");
}

int main() {
    printf("C TILE_LOG=%d CHUNK_LOG=%d STRIDED_K=%d WIDE_MIN_LOG=%u MIN_BLOCKS=%u MAX_BLOCKS_GENERIC=%u TWO_PASS_MIN_LAYERS=%u TWO_PASS_MAX_LAYERS=%u STRIDED_K_CHUNK_LOG=%u "
           "STRIDED_K10_CHUNK_LOG=%u TINY_MAX_LOG=%u FAST_MIN_LAYERS=%u K_KINDS=%d kinds=%d%d%d%d%d%d%d%d sizeof_PassArgs=%zu\n",
           TILE_LOG, CHUNK_LOG, STRIDED_K, FFT_STRIDED_WIDE_MIN_LOG, FFT_MIN_BLOCKS, FFT_MAX_BLOCKS_GENERIC, FFT_TWO_PASS_MIN_LAYERS, FFT_TWO_PASS_MAX_LAYERS, FFT_STRIDED_K_CHUNK_LOG,
           FFT_STRIDED_K10_CHUNK_LOG, FFT_TINY_MAX_LOG, FFT_FAST_MIN_LAYERS, (int)K_KINDS, (int)K_TILE12, (int)K_STRIDED5, (int)K_STRIDED6, (int)K_PASS, (int)K_TINY, (int)K_STRIDED_K8,
           (int)K_STRIDED_K9, (int)K_STRIDED_K10, sizeof(PassArgs));

    const FftKnobs settings[4] = {{true, true}, {false, true}, {true, false}, {false, false}};
    const u32 counts[24] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 999, 1000};
    for (int mode = 0; mode < 5; mode++) {          // 0..3: the knob settings in circle mode; 4: the default knobs in line mode
        const FftKnobs knobs = settings[mode & 3];
        const bool circle = mode < 4;
        for (int inverse = 1; inverse >= 0; inverse--)
            for (u32 log = 0; log <= 28; log++)
                for (u32 src_log = inverse ? log : 0; src_log <= log; src_log++)
                    for (u32 ncols : counts) print_plan("S", inverse, {job(0, ncols, log, src_log, circle)}, knobs);
    }

    // the size classes of tests/test_gpu_pcs_commit_large.py: session_trees (tests/test_fft_plan_cpu.py holds this table to it)
    struct Session { const char* name; u32 blowup, top, nbig; };
    const Session sessions[4] = {{"b1", 1, 20, 17}, {"b2", 2, 21, 9}, {"b4", 4, 22, 5}, {"b1_top22", 1, 22, 9}};
    const std::vector<std::pair<u32, u32>> small[2] = {{{5, 1}, {9, 2}, {13, 2}, {16, 2}}, {{4, 1}, {7, 1}, {11, 1}, {12, 2}, {17, 2}}};      // (log, columns), ascending
    const std::vector<std::pair<u32, u32>> nohost = {{3, 2}, {5, 70}, {7, 1}, {9, 3}, {10, 40}};
    for (const FftKnobs knobs : settings) {
        for (const Session& s : sessions)
            for (int tree = 0; tree < 2; tree++) {
                std::vector<std::pair<u32, u32>> classes = small[tree];
                classes.push_back({s.top - s.blowup, s.nbig});
                for (int inverse = 0; inverse <= (tree == 0 ? 1 : 0); inverse++) {
                    std::vector<FftJob> jobs;
                    for (auto& c : classes) jobs.push_back(inverse ? job(jobs.size(), c.second, c.first, c.first, true) : job(jobs.size(), c.second, c.first + s.blowup, c.first, true));
                    print_plan(std::string("M name=") + s.name + " tree=" + std::to_string(tree), inverse, jobs, knobs);
                }
            }
        for (int inverse = 0; inverse <= 1; inverse++) {
            std::vector<FftJob> jobs;
            for (auto& c : nohost) jobs.push_back(inverse ? job(jobs.size(), c.second, c.first, c.first, true) : job(jobs.size(), c.second, c.first + 1, c.first, true));
            print_plan("M name=nohost tree=0", inverse, jobs, knobs);
        }
    }
    return 0;
}
