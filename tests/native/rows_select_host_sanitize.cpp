// CPU sanitizer harness for the host-only half of the row selection (stwo-brainfuck_amd/csrc/rows_select_host.hip: bfhip_rows_select_host, and
// the validator and pass planner of csrc/rows_select.h that bfhip_rows_select shares with it). tests/test_rows_select_cpu.py compiles this
// file TOGETHER with rows_select_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program
// directly, without arguments. Every buffer fits exactly: the table ends with its last row's last word (a stride above n_cols included), the
// output holds 2^log_size x n_out words, the order row_end - row_begin. Seeded random selections are checked against the definition's
// properties (the selected set by a recount, the order sorted by the keys and by source row within ties, every output word, the padding), then
// the edges (S = 0, S = 2^log_size, one more, offsets at both ends, no candidates, an empty table, the count-only form) and the refusals, and
// the planner's passes for every key count. Prints a summary line per part.
#include "../../stwo-brainfuck_amd/csrc/rows_select.h"
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

#define REQUIRE(cond) do { if (!(cond)) { printf("internal: line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); exit(2); } } while (0)

struct Case {
    uint64_t n_rows, stride; uint32_t n_cols, log_size, repeat;
    std::vector<uint32_t> table;      // exactly (n_rows - 1) * stride + n_cols words
    std::vector<bfhip_select_term> terms; std::vector<bfhip_select_key> keys; std::vector<bfhip_select_out> outs;
    uint64_t begin, end;
    uint32_t word(uint64_t r, uint32_t c) const { return table[r * stride + c]; }
    bfhip_rows_select_desc desc() const {
        bfhip_rows_select_desc d{};
        d.terms = terms.empty() ? nullptr : terms.data(); d.keys = keys.empty() ? nullptr : keys.data();
        d.n_terms = (uint32_t)terms.size(); d.n_keys = (uint32_t)keys.size(); d.row_begin = begin; d.row_end = end;
        return d;
    }
};

static bool holds(uint32_t op, uint32_t w, uint32_t v) { return op == 0 ? w == v : op == 1 ? w != v : op == 2 ? w < v : op == 3 ? w <= v : op == 4 ? w > v : w >= v; }

// runs the case through the host function with exactly fitting buffers and checks the result against the definition; returns S, or -1 if the
// call failed (g_error says why)
static int64_t run(const Case& c, bool count_only, bool want_order) {
    const bfhip_rows_select_desc d = c.desc();
    const uint64_t n = uint64_t(1) << c.log_size;
    std::vector<uint32_t> out(count_only ? 0 : n * c.outs.size(), 0xDEADBEEFu), order(want_order ? c.end - c.begin : 0, 0xDEADBEEFu);
    uint64_t S = ~uint64_t(0);
    const int32_t rc = bfhip_rows_select_host(c.table.empty() ? nullptr : c.table.data(), c.n_rows, c.n_cols, c.stride, c.repeat, &d, count_only ? 0 : c.log_size,
                                              count_only ? nullptr : c.outs.data(), count_only ? 0 : (uint32_t)c.outs.size(), count_only ? nullptr : out.data(),
                                              want_order ? order.data() : nullptr, &S);
    if (rc != 0) { REQUIRE(rc == -1 && g_error.find("bfhip_rows_select_host: ") == 0); return -1; }
    // the selected set
    std::vector<uint64_t> sel;
    for (uint64_t r = c.begin; r < c.end; r++) {
        bool all = true;
        for (const auto& t : c.terms) all = all && holds(t.op, c.word(r, t.col), t.value);
        if (all) sel.push_back(r);
    }
    REQUIRE(S == sel.size());
    if (want_order) {
        // a permutation of the selected rows, sorted by the keys, ascending source row within equal keys
        std::vector<uint8_t> seen(c.end - c.begin + 1, 0);
        for (uint64_t i = 0; i < S; i++) {
            REQUIRE(order[i] >= c.begin && order[i] < c.end && !seen[order[i] - c.begin]);
            seen[order[i] - c.begin] = 1;
            bool all = true;
            for (const auto& t : c.terms) all = all && holds(t.op, c.word(order[i], t.col), t.value);
            REQUIRE(all);
            if (i) {
                int cmp = 0;
                for (const auto& k : c.keys) {
                    const uint32_t a = c.word(order[i - 1], k.col), b = c.word(order[i], k.col);
                    if (a != b) { cmp = ((a < b) != ((k.flags & 1) != 0)) ? -1 : 1; break; }
                }
                REQUIRE(cmp < 0 || (cmp == 0 && order[i - 1] < order[i]));
            }
        }
        for (uint64_t i = S; i < order.size(); i++) REQUIRE(order[i] == 0xDEADBEEFu);
    }
    if (!count_only && want_order) {
        for (uint64_t i = 0; i < n; i++)
            for (size_t k = 0; k < c.outs.size(); k++) {
                const auto& o = c.outs[k];
                const uint32_t got = out[i * c.outs.size() + k];
                if (i < S) REQUIRE(got == c.word((uint64_t)((int64_t)order[i] + o.offset), o.col));
                else if (c.repeat) REQUIRE(got == out[(S - 1) * c.outs.size() + k]);
                else REQUIRE(got == o.pad);
            }
    }
    return (int64_t)S;
}

static Case random_case(bool canonical) {
    Case c;
    c.n_cols = 1 + below(6); c.stride = c.n_cols + (below(3) == 0 ? below(4) : 0); c.n_rows = below(8) == 0 ? below(3) : 1 + below(90);
    c.table.resize(c.n_rows ? (c.n_rows - 1) * c.stride + c.n_cols : 0);
    for (auto& v : c.table) { const uint32_t k = below(8); v = k < 4 ? below(4) : k == 4 ? P - 1 : k == 5 ? 0 : below(P); }
    if (!canonical && !c.table.empty()) for (int i = 0; i < 3; i++) c.table[below((uint32_t)c.table.size())] = P + below(5);
    c.begin = c.n_rows ? below((uint32_t)c.n_rows + 1) : 0; c.end = c.begin + (c.n_rows > c.begin ? below((uint32_t)(c.n_rows - c.begin) + 1) : 0);
    if (below(3) == 0) { c.begin = 0; c.end = c.n_rows; }
    for (uint32_t i = below(4); i > 0; i--) c.terms.push_back({below(c.n_cols), below(6), below(3) == 0 ? P - 1 : below(4)});
    for (uint32_t i = below(5); i > 0; i--) c.keys.push_back({below(c.n_cols), below(2)});
    const int64_t lo = -(int64_t)c.begin, hi = (int64_t)(c.n_rows - c.end);
    for (uint32_t i = 1 + below(5); i > 0; i--) {
        const uint32_t how = below(4);
        const int64_t off = how == 0 ? lo : how == 1 ? hi : how == 2 ? 0 : lo + (int64_t)below((uint32_t)(hi - lo + 1));
        c.outs.push_back({below(c.n_cols), (int32_t)off, below(2) ? P - 1 : below(9)});
    }
    c.repeat = below(4) == 0;
    c.log_size = 1;
    return c;
}

int main() {
    // ---- random selections: the count first (the count-only form), then the smallest domain, one below it where there is one ----
    int n_run = 0, n_sorted = 0, n_count_refused = 0, n_bad = 0;
    for (int t = 0; t < 4000; t++) {
        Case c = random_case(t % 5 != 0);
        const int64_t S = run(c, true, t % 2 == 0);
        if (S < 0) { REQUIRE(t % 5 == 0 && g_error.find("is not a canonical M31 value") != std::string::npos); n_bad++; continue; }
        while ((uint64_t(1) << c.log_size) < (uint64_t)S) c.log_size++;
        if (below(3) == 0) c.log_size += below(3);
        const int64_t S2 = run(c, false, true);
        if (S2 < 0) {
            const bool by_repeat = c.repeat && S == 0 && g_error == "bfhip_rows_select_host: BFHIP_ROWS_REPEAT_LAST needs at least one selected row";
            REQUIRE(by_repeat || (t % 5 == 0 && g_error.find("is not a canonical M31 value") != std::string::npos));
            if (by_repeat) n_count_refused++; else n_bad++;
        } else {
            REQUIRE(S2 == S);
            n_run++; n_sorted += !c.keys.empty() && S > 1;
        }
        if (S > 2) {      // a domain one size too small: refused by the count, the output untouched (run() would have seen a written word)
            c.log_size = 1;
            while ((uint64_t(2) << c.log_size) < (uint64_t)S) c.log_size++;
            if ((uint64_t(1) << c.log_size) < (uint64_t)S) {
                REQUIRE(run(c, false, false) == -1 && g_error == "bfhip_rows_select_host: " + std::to_string(S) + " rows selected, the domain has " + std::to_string(uint64_t(1) << c.log_size));
                n_count_refused++;
            }
        }
    }
    printf("random: %d selections, %d with a sort, %d refused by the count, %d non-canonical\n", n_run, n_sorted, n_count_refused, n_bad);
    REQUIRE(n_run > 2000 && n_sorted > 500 && n_count_refused > 100 && n_bad > 100);

    // ---- edges ----
    {
        Case c; c.n_rows = 33; c.n_cols = 2; c.stride = 2; c.repeat = 0; c.begin = 0; c.end = 32; c.log_size = 5;
        c.table.resize(66);
        for (uint64_t r = 0; r < 33; r++) { c.table[2 * r] = 1; c.table[2 * r + 1] = (uint32_t)(P - 1 - r); }
        c.terms = {{0, BFHIP_SELECT_EQ, 1}}; c.keys = {{1, 0}, {0, BFHIP_SELECT_DESCENDING}, {1, BFHIP_SELECT_DESCENDING}}; c.outs = {{1, 1, 0}, {0, 0, 3}};
        REQUIRE(run(c, false, true) == 32);                     // S = 2^log_size, offset +1 up to the table's last row
        c.end = 33; c.outs = {{1, 0, 0}};
        REQUIRE(run(c, false, true) == -1 && g_error == "bfhip_rows_select_host: 33 rows selected, the domain has 32");
        c.begin = 1; c.outs = {{1, -1, 0}, {1, 0, P - 1}};
        REQUIRE(run(c, false, true) == 32);                     // offset -1 down to row 0
        c.terms = {{0, BFHIP_SELECT_GT, 1}};
        REQUIRE(run(c, false, true) == 0);                      // S = 0: all pad
        c.repeat = 1;
        REQUIRE(run(c, false, true) == -1);
        c.repeat = 0; c.begin = c.end = 17;
        REQUIRE(run(c, false, true) == 0 && run(c, true, true) == 0);      // no candidates: order_h is a buffer of no words
        Case e; e.n_rows = 0; e.n_cols = 3; e.stride = 5; e.repeat = 0; e.begin = e.end = 0; e.log_size = 1; e.outs = {{2, 0, 7}};
        REQUIRE(run(e, false, true) == 0 && run(e, true, false) == 0);     // an empty table: table_h null
    }
    printf("edges ok\n");

    // ---- refusals: none may read through a null pointer or past a buffer ----
    {
        const uint32_t table[6] = {0, 1, 2, 3, 4, 5};
        const bfhip_select_out outs[1] = {{0, 0, 0}};
        const bfhip_select_term terms[1] = {{0, 0, 0}};
        const bfhip_select_key keys[1] = {{0, 0}};
        uint32_t out[2] = {9, 9};
        uint64_t S = 0;
        int tried = 0, refused = 0;
        auto expect = [&](int32_t rc) { tried++; if (rc == -1 && g_error.find("bfhip_rows_select_host: ") == 0) refused++; };
        bfhip_rows_select_desc d{}; d.row_end = 2;
        expect(bfhip_rows_select_host(nullptr, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, nullptr, 1, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, nullptr));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, nullptr, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, nullptr, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 0, nullptr, 1, nullptr, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 2, 0, &d, 1, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 2, &d, 1, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 0, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 31, outs, 1, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 0, out, nullptr, &S));
        expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 257, out, nullptr, &S));
        d.n_terms = 1; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.n_terms = 9; d.terms = terms; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.n_terms = 0; d.n_keys = 1; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.n_keys = 5; d.keys = keys; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.n_keys = 0; d.row_end = 3; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.row_begin = 2; d.row_end = 1; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.row_begin = 0; d.row_end = 2; d.reserved[1] = 1; expect(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S));
        d.reserved[1] = 0;
        REQUIRE(out[0] == 9 && out[1] == 9 && tried == refused);
        REQUIRE(bfhip_rows_select_host(table, 2, 3, 3, 0, &d, 1, outs, 1, out, nullptr, &S) == 0 && S == 2 && out[0] == 0 && out[1] == 3);
        printf("refused %d of %d\n", refused, tried);
    }

    // ---- the planner: least significant pair first, an odd count ends with the most significant key alone ----
    {
        const bfhip_select_key keys[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
        const int want_hi[5][2] = {{0, 0}, {-1, 0}, {0, 0}, {1, -1}, {2, 0}}, want_lo[5][2] = {{0, 0}, {0, 0}, {1, 0}, {2, 0}, {3, 1}};
        for (uint32_t n = 0; n <= 4; n++) {
            bfhip_rows_select_desc d{}; d.keys = keys; d.n_keys = n; d.row_end = 5;
            const bf::SelectPlan p = bf::select_validate("x: ", bf::SelectShape{5, 1, false}, &d, 0, nullptr, 0, false, false);
            REQUIRE(p.count_only && p.n_candidates == 5 && p.n_passes == (n + 1) / 2);
            for (uint32_t i = 0; i < p.n_passes; i++) REQUIRE(p.hi[i] == want_hi[n][i] && p.lo[i] == want_lo[n][i]);
        }
        bool threw = false;
        try { bf::select_check_count("x: ", bf::SelectPlan{}, false, 3, 1); } catch (const bf::HipError& e) { threw = std::string(e.what()) == "x: 3 rows selected, the domain has 2"; }
        REQUIRE(threw);
        REQUIRE(bf::select_bad_word_message("x: ", bf::select_bad_key(5, 2), 9) == "x: row 5, column 2: 9 is not a canonical M31 value");
    }
    printf("rows_select_host_sanitize ok\n");
    return 0;
}
