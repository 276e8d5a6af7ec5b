// group_blocks.h -- the group tables of K10 (tracks) and of identification (query groups, identities): their check, the 16-row blocking
// the matrix-core tile kernels work on, and the cut of the column blocks into ranges (no HIP here: a host-only program can include it;
// tests/csrc/group_blocks_check.cpp does, under AddressSanitizer and UBSan).
//
//     check_groups("pvf_identify", "row_start", row_start, T, N);    // refused before anything is indexed
//     const Blocking b(row_start, T, N);                              // O(N), depends on the group sizes only
//     const std::vector<int> range_b0 = cut_ranges(b, wanted, floor); // block bounds [n_ranges + 1]
//
// Rows are sorted by group.  A BLOCK is 16 consecutive rows, a SEGMENT a run of rows of one group inside a block (up to 16 per block); a
// group longer than what is left of its first block goes on in the next ones ("spans" blocks: one PART per block, summed in block order
// by the callers' chunk kernels).  A block is CLEAN when its first row starts a group: only there may a column range begin, because the
// sums of a spanning group are carried from tile to tile inside a range.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "scratch_layout.h"      // PvfError

// a group table start[n_groups + 1] over n_rows rows: starts at 0, never decreases, no empty group, ends at the number of rows.  Every
// entry is compared with its neighbour before it is used, so a table that passes indexes [0, n_rows) only.
inline void check_groups(const char* who, const char* what, const int32_t* start, int n_groups, int n_rows)
{
    const std::string p = std::string(who) + ": " + what;
    auto require = [](bool cond, const std::string& msg) { if (!cond) throw PvfError(msg); };
    require(start != nullptr, p + " is NULL");
    require(start[0] == 0, p + " must start at 0");
    for (int t = 0; t < n_groups; ++t) {
        require(start[t + 1] >= start[t], p + " must be non-decreasing");
        require(start[t + 1] > start[t], p + " holds an empty group");
    }
    require(start[n_groups] == n_rows, p + " must end at the number of rows");
}

// 16-row blocks of one table whose rows are sorted by group (the table has passed check_groups)
struct Blocking {
    int nb = 0, n_parts = 0;
    std::vector<int> row_group;                 // per row: its group
    std::vector<int> segidx;                    // per row: index of its segment inside its block
    std::vector<int> blk_cont;                  // per block: the segment that goes on in the next block, or -1
    std::vector<int> blk_clean;                 // per block: 1 when it does not take a segment over from its predecessor
    std::vector<int> seg_group, seg_part;       // [block][16]: group of each segment (-1: none); its part (-1: the segment is its whole group)
    std::vector<int> big_group, big_c0, big_nc; // the groups that span blocks, ascending: group, first part, number of parts
    std::vector<int> is_big;                    // per group
    Blocking(const int32_t* start, int n_groups, int n_rows)
    {
        nb = (n_rows + 15) / 16;
        row_group.assign(n_rows, 0);
        segidx.assign(n_rows, 0); blk_cont.assign(nb, -1); blk_clean.assign(nb, 1);
        seg_group.assign((size_t)nb * 16, -1); seg_part.assign((size_t)nb * 16, -1); is_big.assign(n_groups, 0);
        for (int t = 0; t < n_groups; ++t) for (int r = start[t]; r < start[t + 1]; ++r) row_group[r] = t;
        for (int b = 0; b < nb; ++b) {
            const int r0 = b * 16, nr = std::min(16, n_rows - r0);
            int seg = 0;
            for (int r = r0; r < r0 + nr; ++r) {
                if (r > r0 && row_group[r] != row_group[r - 1]) ++seg;
                segidx[r] = seg;
                seg_group[(size_t)b * 16 + seg] = row_group[r];
            }
            if (r0 + nr < n_rows && row_group[r0 + nr] == row_group[r0 + nr - 1]) blk_cont[b] = seg;     // the last segment's group goes on
            if (b > 0 && row_group[r0] == row_group[r0 - 1]) blk_clean[b] = 0;                            // ... and this block takes it over
        }
        // groups that span several blocks: one part per (group, block), summed in block order afterwards
        for (int t = 0; t < n_groups; ++t) {
            const int b_first = start[t] / 16, b_last = (start[t + 1] - 1) / 16;
            if (b_last == b_first) continue;
            big_group.push_back(t); big_c0.push_back(n_parts); big_nc.push_back(b_last - b_first + 1);
            is_big[t] = 1;
            for (int b = b_first; b <= b_last; ++b) seg_part[(size_t)b * 16 + (b == b_first ? segidx[start[t]] : 0)] = n_parts++;
        }
    }
};

// Column ranges over the blocks of `g`: block bounds, from 0 to g.nb.  `wanted` ranges at most, none shorter than 16 blocks when cut
// evenly, but at least `floor` of them (what the callers' 32-bit byte offsets inside a range need).  An even cut that falls inside a
// spanning group moves on to the next clean block; a cut that does not lie past the one before it, or that reaches the end, is dropped.
inline std::vector<int> cut_ranges(const Blocking& g, int wanted, int floor)
{
    int want_ranges = std::max(1, std::min(wanted, std::max(1, g.nb / 16)));
    want_ranges = std::max(want_ranges, floor);
    std::vector<int> range_b0{0};
    for (int k = 1; k < want_ranges; ++k) {
        int b = (int)((long long)g.nb * k / want_ranges);
        while (b < g.nb && !g.blk_clean[b]) ++b;
        if (b > range_b0.back() && b < g.nb) range_b0.push_back(b);
    }
    range_b0.push_back(g.nb);
    return range_b0;
}
