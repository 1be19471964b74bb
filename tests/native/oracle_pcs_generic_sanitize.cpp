// CPU sanitizer harness for the generic oracle shim (tests/native/oracle_pcs_generic.cpp, included below so that the shim and the oracle
// headers it instantiates are compiled under the sanitizers with it). tests/test_pcs_generic_oracle_cpu.py builds this file with
// g++ -fsanitize=address,undefined next to oracle/simd_port.cpp and runs the program directly:
//   oracle_pcs_generic_sanitize <case.txt> <proof.out>
// case.txt holds unsigned decimal numbers separated by white space: the four conventions; pow_bits, log_blowup, n_queries; the largest log
// size; the form; the number of trees; per tree its number of columns and their log sizes; the number of points and 8 words per point; the
// sample count of every column; the point indices; then every column's words in commit order. The program commits the trees, draws the
// point (printed: the caller compares it), opens the columns and writes the proof's bytes to proof.out. Any finding ends it with a report.
#include "oracle_pcs_generic.cpp"
#include <fstream>

static bool next_u32(FILE* f, u32& v) { unsigned long long x; if (fscanf(f, "%llu", &x) != 1 || x > 0xffffffffull) return false; v = (u32)x; return true; }
#define NEED(call) do { if (!(call)) { fprintf(stderr, "case file: %s\n", #call); return 2; } } while (0)
#define MUST(call) do { if ((call) != 0) { fprintf(stderr, "%s: %s\n", #call, opg_last_error()); return 3; } } while (0)

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: see the source header\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    u32 conv[4], pow_bits, blowup, n_queries, max_log, form, n_trees, n_points;
    for (u32& v : conv) NEED(next_u32(f, v));
    NEED(next_u32(f, pow_bits)); NEED(next_u32(f, blowup)); NEED(next_u32(f, n_queries)); NEED(next_u32(f, max_log)); NEED(next_u32(f, form));
    NEED(next_u32(f, n_trees));
    std::vector<std::vector<u32>> logs(n_trees);
    size_t total_cols = 0;
    for (auto& t : logs) { u32 n; NEED(next_u32(f, n)); t.resize(n); for (u32& l : t) NEED(next_u32(f, l) && l <= 20); total_cols += n; }
    NEED(next_u32(f, n_points));
    std::vector<u32> points(8 * size_t(n_points)), counts(total_cols), idx;
    for (u32& w : points) NEED(next_u32(f, w));
    size_t n_samples = 0;
    for (u32& n : counts) { NEED(next_u32(f, n)); n_samples += n; }
    idx.resize(n_samples);
    for (u32& i : idx) NEED(next_u32(f, i));
    std::vector<std::vector<std::vector<u32>>> cols(n_trees);
    for (u32 t = 0; t < n_trees; t++)
        for (u32 l : logs[t]) { cols[t].emplace_back(size_t(1) << l); for (u32& w : cols[t].back()) NEED(next_u32(f, w)); }
    fclose(f);

    MUST(opg_set_conventions(conv[0], conv[1], conv[2], conv[3]));
    void* ch = opg_channel_new();
    void* s = opg_session_new(pow_bits, blowup, n_queries, max_log);
    if (!s) { fprintf(stderr, "session: %s\n", opg_last_error()); return 3; }
    for (u32 t = 0; t < n_trees; t++) {
        std::vector<const u32*> ptrs;
        for (auto& c : cols[t]) ptrs.push_back(c.data());
        u8 root[32];
        MUST(opg_session_commit(s, ch, ptrs.data(), logs[t].data(), (u32)ptrs.size(), (int)form, root));
    }
    u32 oods[8];
    MUST(opg_channel_draw_point(ch, oods));
    printf("point");
    for (u32 w : oods) printf(" %u", w);
    printf("\n");
    std::vector<u32> sampled(4 * std::max<size_t>(1, n_samples));
    char* js = nullptr; size_t len = 0;
    MUST(opg_session_prove_values(s, ch, points.data(), n_points, counts.data(), idx.data(), sampled.data(), &js, &len));
    { std::ofstream out(argv[2], std::ios::binary); out.write(js, (std::streamsize)len); }
    opg_free(js);
    // what the shim refuses: a second opening, a commit after it, a point index out of range, a word that is no field element
    int refused = 0, tried = 0;
    auto expect = [&](int r) { tried++; if (r == -1) refused++; };
    expect(opg_session_prove_values(s, ch, points.data(), n_points, counts.data(), idx.data(), nullptr, &js, &len));
    { const u32* p = cols[0][0].data(); u8 root[32]; expect(opg_session_commit(s, ch, &p, logs[0].data(), 1, 0, root)); }
    { u32 bad[4] = {P, 0, 0, 0}; expect(opg_channel_mix_felts(ch, bad, 1)); }
    {
        void* s2 = opg_session_new(pow_bits, blowup, n_queries, max_log);
        const u32* p = cols[0][0].data(); u8 root[32]; u32 one = 1, far = n_points;
        expect(opg_session_prove_values(s2, ch, points.data(), n_points, &one, &far, nullptr, &js, &len));      // nothing committed
        MUST(opg_session_commit(s2, ch, &p, logs[0].data(), 1, 0, root));
        expect(opg_session_prove_values(s2, ch, points.data(), n_points, &one, &far, nullptr, &js, &len));      // index out of range
        opg_session_free(s2);
    }
    u8 digest[32]; u32 n_sent = 0;
    opg_channel_state(ch, digest, &n_sent);
    printf("refused %d of %d\n", refused, tried);
    opg_session_free(s);
    opg_channel_free(ch);
    return refused == tried ? 0 : 4;
}
