// CPU sanitizer harness for the host-only half of the row filling (stwo-brainfuck_amd/csrc/rows_fill_host.hip: bfhip_rows_fill_host, and the
// validator, the gap count and the value rule of csrc/rows_fill.h that bfhip_rows_fill shares with it). tests/test_rows_fill_cpu.py compiles
// this file TOGETHER with rows_fill_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program
// directly, without arguments. Every buffer fits exactly: the table ends with its last row's last word (a stride above n_cols included), the
// output holds 2^log_size x n_out words, the order n_entries. Seeded random fillings are checked against an independent walk that writes the
// sequence out element by element, then the edges (one entry, T = 2^log_size and one more, offset 16 at the end of the domain, a tail that
// wraps, a total above 2^32, the count-only form) and the refusals, and the header's inline rules. Prints a summary line per part.
#include "../../stwo-brainfuck_amd/csrc/rows_fill.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// what api_ctx.hip provides inside the library
static std::string g_error;
void bfhip_set_error(const std::string& s) { g_error = s; }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t below(uint32_t n) { return (uint32_t)(next64() % n); }
static const uint32_t P = 0x7fffffffu;
static const std::string WHO = "bfhip_rows_fill_host: ";

#define REQUIRE(cond) do { if (!(cond)) { printf("internal: line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); exit(2); } } while (0)

struct Case {
    uint64_t n_rows = 0, stride = 0, n_entries = 0, row_begin = 0; uint32_t n_cols = 0, log_size = 1, step = BFHIP_FILL_NO_STEP, flags = 0;
    std::vector<uint32_t> table;      // exactly (n_rows - 1) * stride + n_cols words
    std::vector<uint32_t> group, order; std::vector<bfhip_fill_out> outs;
    bool has_order = false;
    uint32_t word(uint64_t r, uint32_t c) const { return table[r * stride + c]; }
    uint64_t row_of(uint64_t i) const { return has_order ? order[i] : row_begin + i; }
    bfhip_rows_fill_desc desc() const {
        bfhip_rows_fill_desc d{};
        d.group_cols = group.empty() ? nullptr : group.data(); d.n_group = (uint32_t)group.size(); d.step_col = step;
        d.order_d = has_order ? order.data() : nullptr; d.n_entries = n_entries; d.row_begin = row_begin; d.flags = flags;
        return d;
    }
};

// the sequence written out: element -> (row whose words it shows, t), as far as `need` elements; returns T
static uint64_t walk(const Case& c, uint64_t need, std::vector<uint64_t>& rows, std::vector<uint32_t>& ts) {
    uint64_t T = 0;
    for (uint64_t i = 0; i < c.n_entries; i++) {
        if (i && (c.flags & BFHIP_FILL_GAPS)) {
            bool same = true;
            for (uint32_t g : c.group) same = same && c.word(c.row_of(i), g) == c.word(c.row_of(i - 1), g);
            const uint64_t a = c.word(c.row_of(i - 1), c.step), b = c.word(c.row_of(i), c.step);
            if (same && b > a + 1) {
                for (uint64_t t = 1; t < b - a && rows.size() < need; t++) { rows.push_back(c.row_of(i - 1)); ts.push_back((uint32_t)t); }
                T += b - a - 1;
            }
        }
        if (rows.size() < need) { rows.push_back(c.row_of(i)); ts.push_back(0); }
        T++;
    }
    for (uint32_t t = 1; rows.size() < need; t++) { rows.push_back(c.row_of(c.n_entries - 1)); ts.push_back(t); }
    return T;
}

// runs the case through the host function with exactly fitting buffers and checks the result against the walk; returns T, or -1 if the call
// failed (g_error says why)
static int64_t run(const Case& c, bool count_only) {
    const bfhip_rows_fill_desc d = c.desc();
    const uint64_t n = uint64_t(1) << c.log_size;
    std::vector<uint32_t> out(count_only ? 0 : n * c.outs.size(), 0xDEADBEEFu);
    uint64_t T = ~uint64_t(0);
    const int32_t rc = bfhip_rows_fill_host(c.table.data(), c.n_rows, c.n_cols, c.stride, &d, count_only ? 0 : c.log_size, count_only ? nullptr : c.outs.data(),
                                            count_only ? 0 : (uint32_t)c.outs.size(), count_only ? nullptr : out.data(), &T);
    if (rc != 0) {
        REQUIRE(rc == -1 && g_error.find(WHO) == 0);
        for (uint32_t v : out) REQUIRE(v == 0xDEADBEEFu || g_error.find("is not a canonical M31 value") != std::string::npos);
        return -1;
    }
    std::vector<uint64_t> rows; std::vector<uint32_t> ts;
    REQUIRE(T == walk(c, count_only ? 0 : n + BFHIP_FILL_MAX_OFFSET, rows, ts));
    if (!count_only)
        for (uint64_t i = 0; i < n; i++)
            for (size_t k = 0; k < c.outs.size(); k++) {
                const auto& o = c.outs[k];
                const uint64_t r = rows[i + o.offset]; const uint32_t t = ts[i + o.offset];
                uint32_t want;
                if (o.kind == BFHIP_FILL_MARK) want = t ? o.value : 0;
                else if (t == 0) want = c.word(r, o.col);
                else if (o.kind == BFHIP_FILL_SET) want = o.value;
                else want = o.col == c.step ? (uint32_t)((uint64_t(c.word(r, o.col)) + t) % P) : c.word(r, o.col);
                REQUIRE(out[i * c.outs.size() + k] == want);
            }
    return (int64_t)T;
}

static Case random_case(bool canonical) {
    Case c;
    c.n_cols = 2 + below(5); c.stride = c.n_cols + (below(3) == 0 ? below(4) : 0); c.n_rows = 1 + below(60);
    c.table.resize((c.n_rows - 1) * c.stride + c.n_cols);
    for (auto& v : c.table) { const uint32_t k = below(8); v = k < 4 ? below(3) : k == 4 ? P - 1 : k == 5 ? 0 : below(40); }
    // column 1 is what most cases step by: mostly ascending by 0 .. 3, now and then a drop
    uint32_t s = below(4) == 0 ? P - 1 - below(6) : below(50);
    for (uint64_t r = 0; r < c.n_rows; r++) { c.table[r * c.stride + 1] = s; const uint32_t up = below(4); s = below(9) == 0 ? below(30) : s + up < P ? s + up : s; }
    if (!canonical) for (int i = 0; i < 2; i++) c.table[below((uint32_t)c.table.size())] = P + below(5);
    c.has_order = below(3) == 0;
    if (c.has_order) {
        c.n_entries = 1 + below((uint32_t)c.n_rows);      // at most n_rows entries, though a row may appear more than once
        for (uint64_t i = 0; i < c.n_entries; i++) c.order.push_back(below((uint32_t)c.n_rows));
        if (below(2)) for (size_t i = 1; i < c.order.size(); i++) if (c.order[i] < c.order[i - 1]) c.order[i] = c.order[i - 1];      // ascending rows
    } else {
        c.row_begin = below((uint32_t)c.n_rows); c.n_entries = 1 + below((uint32_t)(c.n_rows - c.row_begin));
        if (below(3) == 0) { c.row_begin = 0; c.n_entries = c.n_rows; }
    }
    for (uint32_t i = below(5); i > 0; i--) c.group.push_back(below(2) ? 0 : below(c.n_cols));
    c.step = below(5) == 0 ? BFHIP_FILL_NO_STEP : below(4) == 0 ? below(c.n_cols) : 1;
    c.flags = c.step != BFHIP_FILL_NO_STEP && below(4) != 0 ? BFHIP_FILL_GAPS : 0;
    for (uint32_t i = 1 + below(6); i > 0; i--) {
        const uint32_t how = below(4);
        c.outs.push_back({below(c.n_cols), below(3), below(2) ? P - 1 : below(9), how == 0 ? 0u : how == 1 ? 1u : how == 2 ? 16u : below(17)});
    }
    return c;
}

int main() {
    // ---- random fillings: the count first (the count-only form), then the smallest domain, one below it where there is one ----
    int n_run = 0, n_gaps = 0, n_order = 0, n_count_refused = 0, n_bad = 0;
    for (int t = 0; t < 4000; t++) {
        Case c = random_case(t % 5 != 0);
        const int64_t T = run(c, true);
        if (T < 0) { REQUIRE(t % 5 == 0 && g_error.find("is not a canonical M31 value") != std::string::npos); n_bad++; continue; }
        if (T > (1 << 16)) { n_count_refused++; continue; }      // a non-canonical step word can open a gap of 2^31 rows: nothing to write out
        while ((uint64_t(1) << c.log_size) < (uint64_t)T) c.log_size++;
        if (below(3) == 0) c.log_size += below(3);
        const int64_t T2 = run(c, false);
        if (T2 < 0) { REQUIRE(t % 5 == 0 && g_error.find("is not a canonical M31 value") != std::string::npos); n_bad++; }
        else { REQUIRE(T2 == T); n_run++; n_gaps += T > (int64_t)c.n_entries; n_order += c.has_order; }
        if (T > 2) {      // a domain one size too small: refused by the count, the output untouched (run() checks that)
            c.log_size = 1;
            while ((uint64_t(2) << c.log_size) < (uint64_t)T) c.log_size++;
            if ((uint64_t(1) << c.log_size) < (uint64_t)T) {
                REQUIRE(run(c, false) == -1 && g_error == WHO + std::to_string(T) + " rows after filling, the domain has " + std::to_string(uint64_t(1) << c.log_size));
                n_count_refused++;
            }
        }
    }
    printf("random: %d fillings, %d with gaps, %d with an order, %d refused by the count, %d non-canonical\n", n_run, n_gaps, n_order, n_count_refused, n_bad);
    REQUIRE(n_run > 2000 && n_gaps > 500 && n_order > 500 && n_count_refused > 100 && n_bad > 100);

    // ---- edges ----
    {
        Case c; c.n_rows = 1; c.n_cols = 2; c.stride = 2; c.n_entries = 1; c.step = 1; c.flags = BFHIP_FILL_GAPS; c.table = {5, P - 2}; c.log_size = 5;
        c.outs = {{1, BFHIP_FILL_KEEP, 0, 0}, {1, BFHIP_FILL_KEEP, 0, 16}, {0, BFHIP_FILL_SET, 3, 16}, {0, BFHIP_FILL_MARK, 1, 1}};
        REQUIRE(run(c, false) == 1 && run(c, true) == 1);       // one entry: the tail wraps past p - 1 at once
        Case e; e.n_rows = 4; e.n_cols = 2; e.stride = 3; e.n_entries = 4; e.step = 0; e.flags = BFHIP_FILL_GAPS; e.log_size = 3;
        e.table = {0, 9, 7, 1, 9, 7, 6, 9, 7, 7, 9};            // steps 0, 1, 6, 7: T = 8 = 2^log_size, offset 16 behind the last row
        e.outs = {{0, BFHIP_FILL_KEEP, 0, 16}, {1, BFHIP_FILL_SET, 4, 1}};
        REQUIRE(run(e, false) == 8);
        e.table[9] = 8;                                         // steps 0, 1, 6, 8: one more
        REQUIRE(run(e, false) == -1 && g_error == WHO + "9 rows after filling, the domain has 8");
        Case w; w.n_rows = 6; w.n_cols = 1; w.stride = 1; w.n_entries = 6; w.step = 0; w.flags = BFHIP_FILL_GAPS; w.log_size = 4;
        w.table = {0, 1431655766u, 0, 1431655766u, 0, 1431655766u};      // three gaps of (2^32 - 1) / 3: T = 2^32 + 5
        w.outs = {{0, BFHIP_FILL_KEEP, 0, 0}};
        uint64_t T = 0; const bfhip_rows_fill_desc d = w.desc();
        REQUIRE(bfhip_rows_fill_host(w.table.data(), 6, 1, 1, &d, 0, nullptr, 0, nullptr, &T) == 0 && T == (uint64_t(1) << 32) + 5);
        std::vector<uint32_t> out(16, 0xDEADBEEFu);
        REQUIRE(bfhip_rows_fill_host(w.table.data(), 6, 1, 1, &d, 4, w.outs.data(), 1, out.data(), &T) == -1 && g_error == WHO + "4294967301 rows after filling, the domain has 16");
        for (uint32_t v : out) REQUIRE(v == 0xDEADBEEFu);
    }
    printf("edges ok\n");

    // ---- refusals: none may read through a null pointer or past a buffer ----
    {
        const uint32_t table[6] = {0, 1, 2, 3, 4, 5};
        const bfhip_fill_out outs[1] = {{0, 0, 0, 0}};
        const uint32_t group[5] = {0, 0, 0, 0, 0}, bad_order[2] = {1, 2};
        uint32_t out[2] = {9, 9};
        uint64_t T = 0;
        int tried = 0, refused = 0;
        auto expect = [&](int32_t rc) { tried++; if (rc == -1 && g_error.find(WHO) == 0) refused++; };
        bfhip_rows_fill_desc d{}; d.n_entries = 2; d.step_col = BFHIP_FILL_NO_STEP;
        expect(bfhip_rows_fill_host(nullptr, 2, 3, 3, &d, 1, outs, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, nullptr, 1, outs, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, nullptr));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, nullptr, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, nullptr, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 0, nullptr, 1, nullptr, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 2, &d, 1, outs, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 0, outs, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 31, outs, 1, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 0, out, &T));
        expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 257, out, &T));
        d.n_group = 1; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.n_group = 5; d.group_cols = group; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.n_group = 0; d.flags = BFHIP_FILL_GAPS; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.flags = 2; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.flags = 0; d.step_col = 3; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.step_col = 0; d.n_entries = 0; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.n_entries = 3; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.n_entries = 1; d.row_begin = 2; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.row_begin = 1; d.order_d = bad_order; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.row_begin = 0; d.n_entries = 2; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));      // order[1] = 2 is not a row
        d.order_d = nullptr; d.reserved = 1; expect(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T));
        d.reserved = 0;
        REQUIRE(out[0] == 9 && out[1] == 9 && tried == refused);
        REQUIRE(bfhip_rows_fill_host(table, 2, 3, 3, &d, 1, outs, 1, out, &T) == 0 && T == 2 && out[0] == 0 && out[1] == 3);
        printf("refused %d of %d\n", refused, tried);
    }

    // ---- the header's inline rules ----
    {
        REQUIRE(bf::fill_gap(5, 5) == 0 && bf::fill_gap(5, 6) == 0 && bf::fill_gap(5, 7) == 1 && bf::fill_gap(7, 5) == 0 && bf::fill_gap(0, P - 1) == P - 2);
        REQUIRE(bf::fill_gap(0xFFFFFFFFu, 0) == 0 && bf::fill_gap(0, 0xFFFFFFFFu) == 0xFFFFFFFEu);      // as integers, nothing wraps
        REQUIRE(bf::fill_value(BFHIP_FILL_KEEP, true, 9, P - 1, 3) == 2 && bf::fill_value(BFHIP_FILL_KEEP, false, 9, P - 1, 3) == P - 1 && bf::fill_value(BFHIP_FILL_KEEP, true, 9, 4, 0) == 4);
        REQUIRE(bf::fill_value(BFHIP_FILL_SET, true, 9, 4, 0) == 4 && bf::fill_value(BFHIP_FILL_SET, true, 9, 4, 2) == 9);
        REQUIRE(bf::fill_value(BFHIP_FILL_MARK, false, 9, 4, 0) == 0 && bf::fill_value(BFHIP_FILL_MARK, false, 9, 4, 1) == 9);
        REQUIRE(bf::fill_reads(BFHIP_FILL_KEEP, 0) && bf::fill_reads(BFHIP_FILL_KEEP, 5) && bf::fill_reads(BFHIP_FILL_SET, 0) && !bf::fill_reads(BFHIP_FILL_SET, 1) &&
                !bf::fill_reads(BFHIP_FILL_MARK, 0) && !bf::fill_reads(BFHIP_FILL_MARK, 1));
        bool threw = false;
        bf::FillPlan p;
        try { bf::fill_check_count("x: ", p, 3, 1); } catch (const bf::HipError& e) { threw = std::string(e.what()) == "x: 3 rows after filling, the domain has 2"; }
        REQUIRE(threw);
        REQUIRE(bf::fill_bad_order_message("x: ", 4, 9, 7) == "x: order[4] = 9 is not a row of the table (7 rows)");
    }
    printf("rows_fill_host_sanitize ok\n");
    return 0;
}
