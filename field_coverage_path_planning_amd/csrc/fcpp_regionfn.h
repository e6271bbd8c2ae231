// fcpp_regionfn.h -- the connected regions of a coverage grid: which cells of the byte grids fcpp_polygon_cover writes form the missed (or
// overlapped, spilled, covered) patches of a field, where each patch lies and how large it is.  ONE set of expressions for the host
// (fcpp_debug_cover_regions, the tests' checker) and the device (fcpp_regions.hip).  All of it is integer arithmetic: the result is a
// function of the input alone, so host and device agree exactly whatever their order of work.  Plain C++: g++ compiles it as it is.
//
// THE RULE (include/fcpp.h states it for callers).
//   grids     as fcpp_polygon_cover writes them: dims (gx, gy float64, nx, ny int64), cell_offsets (n + 1), one byte per cell, row-major
//             [b][a].  A field with an empty grid has no regions.
//   members   cell c is a member iff (grid[c] & mask) == value (region_member); value & ~mask != 0 can never match: FCPP_EINVAL.
//   neighbours  connectivity 4: W, E, N, S; 8: plus the diagonals -- inside ONE field's nx x ny grid only (region_back_neighbour lists the
//             half of them that lies BEFORE a cell in row-major order: W, N, then NW, NE; the other half is their mirror image).
//   regions   the maximal connected sets of members.  A region's KEY is its smallest field-local cell index b nx + a; a field's regions are
//             numbered in ascending key.
//   record    RegionRecord, 48 bytes: first (the key), cells, the bounding box in cells, the sums of the members' column and row indices
//             (cells <= 2^28, indices < 2^28: every sum < 2^56).  No second moments: on a thin grid they overflow int64.
//   labels    int32 per cell: after the counts call a member holds its region's key, after the fill call its region's index within its
//             field; a non-member holds -1 after both.
#pragma once
#include <stdint.h>

#include <vector>

#include "fcpp_geom.h"

namespace fcpp {

constexpr int REGION_TILE = 64;                        // tile edge in cells: fcpp_polygon_cover's tiles (PCOVER_TILE)
constexpr int REGION_BLOCK_CELLS = 4096;               // cells per numbering block: consecutive in a field's row-major order, never across two fields
constexpr int64_t REGION_MAX_CELLS = (int64_t)1 << 28; // per field (PCOVER_MAX_CELLS): a field-local index fits an int32 label

struct RegionDims {         // fcpp_polygon_cover_sizes' record per field (PcoverDims): 32 bytes
    double gx, gy;
    int64_t nx, ny;
};

struct RegionRecord {       // 48 bytes
    int64_t first, cells;
    int32_t a_min, a_max, b_min, b_max;
    int64_t sum_a, sum_b;
};
static_assert(sizeof(RegionRecord) == 48, "the region record is 48 bytes");

FCPP_HD bool region_args_ok(int mask, int value, int connectivity)
{
    return mask >= 0 && mask <= 255 && value >= 0 && value <= 255 && (value & ~mask) == 0 && (connectivity == 4 || connectivity == 8);
}

FCPP_HD bool region_member(uint8_t byte, int mask, int value) { return ((int)byte & mask) == value; }

// how many of a cell's neighbours lie before it in row-major order: W, N (connectivity 4), NW, NE (8)
FCPP_HD int region_back_count(int connectivity) { return connectivity == 8 ? 4 : 2; }

// the k-th of them for cell (a, b) of an nx x ny grid -> (na, nb); false when it falls outside the grid (no wrap from column 0 to nx - 1)
FCPP_HD bool region_back_neighbour(int k, int64_t a, int64_t b, int64_t nx, int64_t ny, int64_t &na, int64_t &nb)
{
    const int da = k == 0 ? -1 : k == 1 ? 0 : k == 2 ? -1 : 1;
    const int db = k == 0 ? 0 : -1;
    na = a + da; nb = b + db;
    return na >= 0 && na < nx && nb >= 0 && nb < ny;
}

// the sum of c / nx over 0 <= c < m (c / nx takes every value below q = m / nx exactly nx times, and q itself m % nx times)
FCPP_HD int64_t region_row_prefix(int64_t m, int64_t nx)
{
    const int64_t q = m / nx, r = m % nx;
    return nx * (q * (q - 1) / 2) + q * r;
}

// a run of cells c0 .. c1 (field-local indices, c0 <= c1) of a grid nx wide: the sums of its column and row indices
FCPP_HD void region_run_sums(int64_t c0, int64_t c1, int64_t nx, int64_t &sum_a, int64_t &sum_b)
{
    const int64_t len = c1 - c0 + 1;
    const int64_t sum_c = (c0 + c1) * len / 2;          // (one of the two factors is even; below 2^57)
    sum_b = region_row_prefix(c1 + 1, nx) - region_row_prefix(c0, nx);
    sum_a = sum_c - nx * sum_b;
}

// the same run's columns: all of a row when it runs over a row's end, else from c0's to c1's
FCPP_HD void region_run_columns(int64_t c0, int64_t c1, int64_t nx, int32_t &a_min, int32_t &a_max)
{
    if (c0 / nx == c1 / nx) { a_min = (int32_t)(c0 % nx); a_max = (int32_t)(c1 % nx); }
    else { a_min = 0; a_max = (int32_t)(nx - 1); }
}

// a member cell (a, b) joins a record (the host's order; the device adds whole runs with integer atomics: the same sums)
inline void region_record_add(RegionRecord &r, int64_t a, int64_t b)
{
    if (r.cells == 0) { r.a_min = r.a_max = (int32_t)a; r.b_min = r.b_max = (int32_t)b; }
    r.cells += 1;
    if ((int32_t)a < r.a_min) r.a_min = (int32_t)a;
    if ((int32_t)a > r.a_max) r.a_max = (int32_t)a;
    if ((int32_t)b < r.b_min) r.b_min = (int32_t)b;
    if ((int32_t)b > r.b_max) r.b_max = (int32_t)b;
    r.sum_a += a; r.sum_b += b;
}

// ONE field on the host: a sequential two-pass union-find over region_member and region_back_neighbour.  keys, index: nx ny labels each
// (after counts / after fill; either may be NULL), records: appended in ascending key.  parent: nx ny words of scratch.  Returns the
// field's number of regions.  Every find ends within its cell's index steps: a parent is never above its cell, a root is its own parent.
inline int64_t region_field_host(const uint8_t *grid, int64_t nx, int64_t ny, int mask, int value, int connectivity, int32_t *parent,
                                 int32_t *keys, int32_t *index, std::vector<RegionRecord> &records)
{
    const int64_t nc = nx * ny;
    const int nb = region_back_count(connectivity);
    auto find = [&](int32_t c) {
        int32_t r = c;
        while (parent[r] != r) r = parent[r];          // at most c steps
        while (parent[c] != r) { const int32_t up = parent[c]; parent[c] = r; c = up; }
        return r;
    };
    for (int64_t b = 0; b < ny; ++b)
        for (int64_t a = 0; a < nx; ++a) {
            const int64_t c = b * nx + a;
            if (!region_member(grid[c], mask, value)) { parent[c] = -1; continue; }
            parent[c] = (int32_t)c;
            for (int k = 0; k < nb; ++k) {
                int64_t na, nbb;
                if (!region_back_neighbour(k, a, b, nx, ny, na, nbb)) continue;
                const int64_t m = nbb * nx + na;
                if (parent[m] < 0) continue;
                const int32_t x = find((int32_t)c), y = find((int32_t)m);
                if (x < y) parent[y] = x; else if (y < x) parent[x] = y;       // the smaller index stays the root: the root is the key
            }
        }
    const size_t base = records.size();
    int64_t count = 0;
    for (int64_t c = 0; c < nc; ++c) {                  // roots in ascending index: the numbering
        if (parent[c] != (int32_t)c) continue;
        RegionRecord r = { c, 0, 0, 0, 0, 0, 0, 0 };
        records.push_back(r);
        ++count;
    }
    // second pass: every member looks its root up among the field's keys and joins that record
    std::vector<int32_t> number((size_t)count);
    {
        int64_t k = 0;
        for (int64_t c = 0; c < nc; ++c)
            if (parent[c] == (int32_t)c) number[(size_t)k++] = (int32_t)c;
    }
    for (int64_t b = 0; b < ny; ++b)
        for (int64_t a = 0; a < nx; ++a) {
            const int64_t c = b * nx + a;
            if (parent[c] < 0) {
                if (keys) keys[c] = -1;
                if (index) index[c] = -1;
                continue;
            }
            const int32_t root = find((int32_t)c);
            int64_t lo = 0, hi = count;                 // the last region whose key is <= root: the device's binary search
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (number[(size_t)mid] <= root) lo = mid; else hi = mid;
            }
            if (keys) keys[c] = root;
            if (index) index[c] = (int32_t)lo;
            region_record_add(records[base + (size_t)lo], a, b);
        }
    return count;
}

}  // namespace fcpp
