// group_blocks_check.cpp -- csrc/group_blocks.h on the host, under AddressSanitizer and UBSan (tests/test_cluster_cases.py builds and runs
// it).  Two uses:
//     group_blocks_check plan WANTED FLOOR < sizes     prints the plan of the group sizes read from standard input (N, nb, parts, range_b0,
//                                                      the spanning groups), so that a test can assert which path a layout reaches;
//     group_blocks_check                               checks the invariants of the blocking and of the range cut over the named layouts of
//                                                      tests/cluster_cases.py and a few thousand random size lists, and that every bad table
//                                                      is refused with its message -- the tables are heap arrays of exactly T + 1 entries and
//                                                      the row arrays of exactly N, so a read or write past either is a sanitizer report.
#include "group_blocks.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<int32_t> starts_of(const std::vector<int>& sizes)
{
    std::vector<int32_t> s(sizes.size() + 1, 0);
    for (size_t t = 0; t < sizes.size(); ++t) s[t + 1] = s[t] + sizes[t];
    return s;
}

// what an entry does: the check, then the blocking
static Blocking blocked(const std::vector<int32_t>& start, int n_rows)
{
    check_groups("check", "row_start", start.data(), (int)start.size() - 1, n_rows);
    return Blocking(start.data(), (int)start.size() - 1, n_rows);
}

// K10's two numbers (cluster.hip) for a device of n_cu compute units
static int k10_wanted(int nb, int n_cu) { const int row_groups = (nb + 3) / 4; return (2 * 24 * 3 * n_cu + row_groups - 1) / row_groups; }
static int k10_floor(int nb) { return (nb >> 16) + 1; }

static void check_invariants(const std::vector<int>& sizes, int wanted, int floor)
{
    const std::vector<int32_t> start = starts_of(sizes);
    const int T = (int)sizes.size(), N = start[T];
    const Blocking g = blocked(start, N);
    std::vector<int> group(N);                     // the rows' groups, from the sizes alone
    for (int t = 0, r = 0; t < T; ++t) for (int k = 0; k < sizes[t]; ++k) group[r++] = t;
    CHECK(g.nb == (N + 15) / 16);
    CHECK((int)g.row_group.size() == N && (int)g.segidx.size() == N && (int)g.blk_cont.size() == g.nb && (int)g.blk_clean.size() == g.nb);
    CHECK(g.seg_group.size() == (size_t)g.nb * 16 && g.seg_part.size() == (size_t)g.nb * 16 && (int)g.is_big.size() == T);
    // every row has exactly one segment, numbered 0.. in row order inside its block, at most 16
    for (int b = 0; b < g.nb; ++b) {
        const int r0 = b * 16, nr = std::min(16, N - r0);
        int n_seg = 0;
        for (int r = r0; r < r0 + nr; ++r) {
            CHECK(g.row_group[r] == group[r]);
            if (r == r0) CHECK(g.segidx[r] == 0);
            else CHECK(g.segidx[r] == g.segidx[r - 1] + (group[r] != group[r - 1] ? 1 : 0));
            CHECK(g.segidx[r] >= 0 && g.segidx[r] < 16);
            CHECK(g.seg_group[(size_t)b * 16 + g.segidx[r]] == group[r]);
            n_seg = g.segidx[r] + 1;
        }
        for (int s = 0; s < 16; ++s) CHECK((g.seg_group[(size_t)b * 16 + s] >= 0) == (s < n_seg));
        // blk_cont: set exactly when the block's last row and the next block's first row share a group; then it names the last segment
        const bool goes_on = r0 + nr < N && group[r0 + nr] == group[r0 + nr - 1];
        CHECK((g.blk_cont[b] >= 0) == goes_on);
        if (goes_on) CHECK(g.blk_cont[b] == n_seg - 1);
        CHECK(g.blk_clean[b] == ((b > 0 && group[r0] == group[r0 - 1]) ? 0 : 1));
    }
    // the parts of a spanning group are consecutive and in block order; no other segment has one
    std::vector<int> part_seen((size_t)g.nb * 16, 0);
    int n_parts = 0;
    size_t k = 0;
    for (int t = 0; t < T; ++t) {
        const int b_first = start[t] / 16, b_last = (start[t + 1] - 1) / 16;
        CHECK(g.is_big[t] == (b_last > b_first ? 1 : 0));
        if (b_last == b_first) continue;
        CHECK(k < g.big_group.size());
        if (k >= g.big_group.size()) break;
        CHECK(g.big_group[k] == t && g.big_c0[k] == n_parts && g.big_nc[k] == b_last - b_first + 1);
        for (int b = b_first; b <= b_last; ++b) {
            const size_t at = (size_t)b * 16 + g.segidx[std::max(start[t], b * 16)];
            CHECK(g.seg_group[at] == t);
            CHECK(g.seg_part[at] == n_parts);
            part_seen[at] = 1;
            ++n_parts;
        }
        ++k;
    }
    CHECK(k == g.big_group.size() && g.big_c0.size() == k && g.big_nc.size() == k);
    CHECK(n_parts == g.n_parts);
    for (size_t at = 0; at < part_seen.size(); ++at) if (!part_seen[at]) CHECK(g.seg_part[at] == -1);
    // the ranges: strictly increasing from 0 to nb, every interior bound a clean block, never more than asked for
    const std::vector<int> rb = cut_ranges(g, wanted, floor);
    CHECK(rb.size() >= 2 && rb.front() == 0 && rb.back() == g.nb);
    for (size_t i = 1; i < rb.size(); ++i) CHECK(rb[i] > rb[i - 1]);
    for (size_t i = 1; i + 1 < rb.size(); ++i) CHECK(g.blk_clean[rb[i]] == 1);
    CHECK((int)rb.size() - 1 <= std::max(std::max(1, std::min(wanted, std::max(1, g.nb / 16))), floor));
}

static void expect_ranges(const char* name, const std::vector<int>& sizes, int n_rows, int nb, const std::vector<int>& want)
{
    const std::vector<int32_t> start = starts_of(sizes);
    const Blocking g = blocked(start, start.back());
    const std::vector<int> rb = cut_ranges(g, k10_wanted(g.nb, 256), k10_floor(g.nb));
    if (start.back() != n_rows || g.nb != nb || rb != want) {
        printf("FAILED layout %s: N %d nb %d ranges", name, (int)start.back(), g.nb);
        for (int b : rb) printf(" %d", b);
        printf("\n");
        ++failures;
    }
    check_invariants(sizes, k10_wanted(g.nb, 256), k10_floor(g.nb));
    for (int w = 1; w <= 6; ++w) check_invariants(sizes, w, 1);
}

static std::vector<int> rep(int n, int v) { return std::vector<int>(n, v); }
static std::vector<int> cat(std::vector<std::vector<int>> parts)
{
    std::vector<int> out;
    for (const auto& p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}

static void refused(const std::vector<int32_t>& start, int n_rows, const char* message)
{
    // (a heap copy of exactly the table: nothing behind it that a wrong read could land in)
    int32_t* tab = (int32_t*)malloc(start.size() * sizeof(int32_t));
    memcpy(tab, start.data(), start.size() * sizeof(int32_t));
    bool thrown = false;
    try {
        check_groups("check", "row_start", tab, (int)start.size() - 1, n_rows);
        const Blocking g(tab, (int)start.size() - 1, n_rows);     // never reached for a bad table
        (void)g;
    } catch (const PvfError& e) {
        thrown = true;
        if (std::string(e.what()) != std::string("check: row_start ") + message) { printf("FAILED message '%s', expected '... %s'\n", e.what(), message); ++failures; }
    }
    free(tab);
    if (!thrown) { printf("FAILED: a table that '%s' was accepted\n", message); ++failures; }
}

static int print_plan(int wanted, int floor)
{
    std::vector<int> sizes;
    int v;
    while (scanf("%d", &v) == 1) sizes.push_back(v);
    const std::vector<int32_t> start = starts_of(sizes);
    try {
        const Blocking g = blocked(start, start.back());
        const std::vector<int> rb = cut_ranges(g, wanted, floor);
        printf("N %d nb %d parts %d\nrange_b0", (int)start.back(), g.nb, g.n_parts);
        for (int b : rb) printf(" %d", b);
        printf("\nbig");
        for (int t : g.big_group) printf(" %d", t);
        printf("\n");
    } catch (const PvfError& e) {
        printf("refused: %s\n", e.what());
        return 2;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "plan")) return print_plan(atoi(argv[2]), atoi(argv[3]));
    // ---- the named layouts (tests/cluster_cases.py), with K10's numbers on 256 compute units
    expect_ranges("aligned16", rep(40, 16), 640, 40, {0, 20, 40});
    expect_ranges("singletons", rep(521, 1), 521, 33, {0, 16, 33});
    expect_ranges("cut_moved", cat({rep(36, 7), {70}, rep(45, 5), {3}}), 550, 35, {0, 22, 35});
    expect_ranges("one_cut_dropped", cat({rep(28, 9), {300}, rep(20, 11), rep(8, 2)}), 788, 50, {0, 40, 50});
    expect_ranges("tail1", cat({rep(51, 10), {3}}), 513, 33, {0, 20, 33});
    const std::vector<int> m20{1, 1, 2, 15, 16, 17, 3, 31, 32, 33, 1, 48, 5, 7, 16, 16, 1, 9, 64, 2};
    expect_ranges("mixed3", cat({m20, m20, {100, 1, 40, 16, 16, 9}}), 822, 52, {0, 20, 40, 52});
    // the size list of test_pair_mean_dist_matrix_core_kernel_all_block_shapes: two ranges wanted, one planned
    expect_ranges("all_block_shapes", {1, 1, 1, 15, 16, 17, 2, 3, 31, 32, 33, 1, 5, 5, 5, 1, 64, 7, 9, 250, 1, 1}, 501, 32, {0, 32});
    // ---- random size lists: sizes 1 to 300 (mostly short, so that blocks hold many segments), N up to 5000
    std::mt19937 rng(20240611);
    for (int it = 0; it < 3000; ++it) {
        const int n_max = 1 + (int)(rng() % 5000), kind = (int)(rng() % 4);
        std::vector<int> sizes;
        int n = 0;
        while (n < n_max) {
            int s;
            if (kind == 0) s = 1 + (int)(rng() % 4);
            else if (kind == 1) s = 1 + (int)(rng() % 40);
            else if (kind == 2) s = (rng() % 8 == 0) ? 1 + (int)(rng() % 300) : 1 + (int)(rng() % 12);
            else s = 1 + (int)(rng() % 300);
            s = std::min(s, n_max - n);
            sizes.push_back(s); n += s;
        }
        check_invariants(sizes, 1 + (int)(rng() % 40), 1 + (int)(rng() % 3));
        const int nb = (n + 15) / 16;
        check_invariants(sizes, k10_wanted(nb, 256), k10_floor(nb));
    }
    // ---- bad tables, each refused with its message before anything is indexed
    refused({0, 5, 3, 10}, 10, "must be non-decreasing");
    refused({0, 5, 5, 10}, 10, "holds an empty group");
    refused({0, 0, 10}, 10, "holds an empty group");
    refused({0, 5, 9}, 10, "must end at the number of rows");
    refused({0, 5, 12}, 10, "must end at the number of rows");
    refused({1, 5, 10}, 10, "must start at 0");
    refused({0, 5, 1000000, 10}, 10, "must be non-decreasing");          // an entry above N
    refused({0, 2000000000, 10}, 10, "must be non-decreasing");
    refused({0, -3, 10}, 10, "must be non-decreasing");
    bool null_refused = false;
    try { check_groups("check", "row_start", nullptr, 3, 10); } catch (const PvfError&) { null_refused = true; }
    CHECK(null_refused);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
