// The source that bfhip_air_source generates, compiled as host C++ (-DBFHIP_AIR_GEN_HOST: the row function is a plain function, the kernel
// wrapper is left out) and run over the rows of a domain: what tests/test_air_codegen_cpu.py compares word for word with tests/air_model.py,
// and the stand-alone program it builds once under -fsanitize=address,undefined. Nothing of the library is linked: the emitted file brings
// its own arithmetic (m31.h as text).
//   g++ -std=c++17 -DBFHIP_AIR_GEN_HOST -DBFHIP_AIR_GEN_FILE='"<emitted file>"' air_codegen_host.cpp
//   air_codegen_host <in> <out>
// in (u32 words): n_cases; per case log_size, log_expand, n_cols, n_params, n_coeffs, denom_inv[8], then n_cols columns of n = 2^(log_size +
// log_expand) cells, 4 n_params parameter words, 4 n_coeffs coefficient words, 4 accumulator columns of n words. out: per case the 4
// accumulator columns after the sweep.
#ifndef BFHIP_AIR_GEN_HOST
#error "compile with -DBFHIP_AIR_GEN_HOST"
#endif
#include BFHIP_AIR_GEN_FILE
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<uint32_t> read_all(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> w((size_t)bytes / 4);
    if (fread(w.data(), 4, w.size(), f) != w.size()) { fprintf(stderr, "short read\n"); exit(2); }
    fclose(f);
    return w;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    const std::vector<uint32_t> in = read_all(argv[1]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    size_t at = 0;
    auto take = [&](size_t n) { if (at + n > in.size()) { fprintf(stderr, "input ends early\n"); exit(2); } const uint32_t* p = in.data() + at; at += n; return p; };
    const uint32_t n_cases = *take(1);
    for (uint32_t c = 0; c < n_cases; c++) {
        const uint32_t* h = take(13);
        const uint32_t log_size = h[0], log_expand = h[1], n_cols = h[2], n_params = h[3], n_coeffs = h[4];
        const size_t n = (size_t)1 << (log_size + log_expand);
        // every buffer is exactly as large as the contract says: a read or write past one is the sanitizer's to find
        std::vector<std::vector<uint32_t>> cols(n_cols), acc(4);
        for (auto& col : cols) { const uint32_t* p = take(n); col.assign(p, p + n); }
        std::vector<bfair::U4> descs(n_cols ? n_cols : 1), params(n_params ? n_params : 1), coeffs(n_coeffs);
        for (uint32_t k = 0; k < n_cols; k++) {
            const unsigned long long p = (unsigned long long)cols[k].data();
            descs[k] = bfair::U4{(uint32_t)p, (uint32_t)(p >> 32), 0u, 0u};
        }
        for (uint32_t i = 0; i < n_params; i++) { const uint32_t* p = take(4); params[i] = bfair::U4{p[0], p[1], p[2], p[3]}; }
        for (uint32_t i = 0; i < n_coeffs; i++) { const uint32_t* p = take(4); coeffs[i] = bfair::U4{p[0], p[1], p[2], p[3]}; }
        for (auto& a : acc) { const uint32_t* p = take(n); a.assign(p, p + n); }
        bfair::Launch L{};
        L.cols = (unsigned long long)descs.data(); L.params = (unsigned long long)params.data(); L.coeffs = (unsigned long long)coeffs.data();
        for (int w = 0; w < 4; w++) L.acc[w] = (unsigned long long)acc[w].data();
        L.log_size = log_size; L.log_expand = log_expand;
        for (int i = 0; i < 8; i++) L.denom_inv[i] = h[5 + i];
        for (size_t row = 0; row < n; row++) bfair::air_row(&L, (uint32_t)row);
        for (auto& a : acc) if (fwrite(a.data(), 4, n, out) != n) { fprintf(stderr, "short write\n"); return 2; }
    }
    fclose(out);
    printf("cases: %u\n", n_cases);
    return 0;
}
