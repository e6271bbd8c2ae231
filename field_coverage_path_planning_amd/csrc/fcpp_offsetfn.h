// fcpp_offsetfn.h -- the exclusive prefix of a count column over the fields of a small batch FROM TWO LEVELS, without a scan:
//     fields are grouped in blocks of OFF_B; agg[col][b] = the sum of the column over block b, accumulated with integer atomics by the
//     kernel that produced the counts (read only after that kernel has ended)
//     prefix(col, i) = sum of agg[col][b] over b < i / OFF_B  +  sum of counts[col][j] over the block's j < i
//     total(col)     = sum of agg[col][b] over all blocks
// Integer sums: exact in any order.  The host version (plain loops) is the checker of the wave version (tests/test_offset_rule_host.py,
// tests/test_gpu_setup_offsets.py); both read the same layout.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "fcpp_geom.h"

namespace fcpp {

// 64 fields per block: at the 8192 fields of the largest small batch a wavefront reads the 128 aggregates of a column with two 8-byte loads
// per lane and the counts of its own block with one
constexpr int OFF_B = 64;
constexpr int OFF_FIELDS_MAX = 8192;
constexpr int OFF_NB = OFF_FIELDS_MAX / OFF_B;             // aggregates per column
static_assert(OFF_NB == 2 * 64, "two loads per lane");
// The aggregates lie BLOCK-major, a row of OFF_ROW words (256 bytes) per block, the columns side by side: agg[b * OFF_ROW + col].  A field's
// wavefront adds its whole row of counts with ONE atomic instruction into one contiguous stretch, and the blocks' rows are spread over the
// memory channels -- column-major (all fields of the batch adding into a few adjacent lines per column) the atomics queued up behind each
// other: the counting pass of 4096 fields took 15 us longer.
constexpr int OFF_ROW = 32;
constexpr int OFF_WORDS = OFF_NB * OFF_ROW;                // words of one buffer of aggregates
FCPP_HD int64_t offset_at(int col, int64_t b) { return b * OFF_ROW + col; }

FCPP_HD int64_t offset_blocks(int64_t n) { return (n + OFF_B - 1) / OFF_B; }

// the checker: prefix of field i (0 <= i <= n; i == n: the total), column `col` of counts[col * n + field]
FCPP_HD int64_t offset_prefix(const int64_t *agg, const int64_t *counts, int64_t n, int col, int64_t i)
{
    int64_t s = 0;
    const int64_t b = i / OFF_B;
    for (int64_t k = 0; k < b; ++k) s += agg[offset_at(col, k)];
    for (int64_t j = b * OFF_B; j < i; ++j) s += counts[(int64_t)col * n + j];
    return s;
}
FCPP_HD int64_t offset_total(const int64_t *agg, int64_t n, int col)
{
    int64_t s = 0;
    for (int64_t k = 0; k < offset_blocks(n); ++k) s += agg[offset_at(col, k)];
    return s;
}
// what the counting kernels do with atomics: the aggregates of one column of n fields (host; agg: OFF_WORDS words)
inline void offset_aggregate(const int64_t *counts, int64_t n, int col, int64_t *agg)
{
    for (int64_t k = 0; k < OFF_NB; ++k) agg[offset_at(col, k)] = 0;
    for (int64_t j = 0; j < n; ++j) agg[offset_at(col, j / OFF_B)] += counts[(int64_t)col * n + j];
}

#if defined(__HIPCC__)
// ---- the wave version: the loads are issued where a kernel begins, the sums taken where a position is first needed --------------------
template <int CTRL>
__device__ __forceinline__ int64_t off_dpp_mov(int64_t v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, 0xf, 0xf, true);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// the wavefront's sum, in every lane (the butterflies of wave_sum_to63, fcpp_pointfn.h: quad, half row, row, two row broadcasts -> lane 63)
__device__ __forceinline__ int64_t off_wave_sum(int64_t v)
{
    v += off_dpp_mov<0xB1>(v);
    v += off_dpp_mov<0x4E>(v);
    v += off_dpp_mov<0x141>(v);
    v += off_dpp_mov<0x140>(v);
    v += off_dpp_mov<0x142>(v);
    v += off_dpp_mov<0x143>(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), 63);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// this lane's share of prefix(col, field): the aggregates `lane` and 64 + `lane` in front of the field's block and the count of the block's
// field `lane` in front of the field -- three independent loads, nothing waited for
__device__ __forceinline__ int64_t offset_prefix_part(const int64_t *__restrict__ agg, const int64_t *__restrict__ counts, int64_t n, int col, int64_t field, int lane)
{
    const int b = (int)(field / OFF_B), r = (int)(field % OFF_B);
    int64_t v = 0;
    if (lane < b) v += agg[offset_at(col, lane)];
    if (b > 64 && 64 + lane < b) v += agg[offset_at(col, 64 + lane)];
    if (lane < r) v += counts[(int64_t)col * n + (field - r) + lane];
    return v;
}
// A field per HALF of a wavefront (k_tile_rows_direct: rows of 32 lanes): the half's sum, in every lane of the half -- the four butterflies
// of off_wave_sum that stay inside a DPP row of sixteen lanes, then the other row's sum by a shuffle
__device__ __forceinline__ int64_t off_half_sum(int64_t v)
{
    v += off_dpp_mov<0xB1>(v);
    v += off_dpp_mov<0x4E>(v);
    v += off_dpp_mov<0x141>(v);
    v += off_dpp_mov<0x140>(v);
    v += __shfl_xor(v, 16);
    return v;
}
// ... and lane `lr` of the half's share of prefix(col, field): 32 lanes by two rounds over the aggregates in front of the field's block (four
// rounds beyond 64 blocks) and over the counts of the block's fields in front of the field -- independent loads, nothing waited for
__device__ __forceinline__ int64_t offset_prefix_part_half(const int64_t *__restrict__ agg, const int64_t *__restrict__ counts, int64_t n, int col, int64_t field, int lr)
{
    static_assert(OFF_B == 2 * 32 && OFF_NB == 4 * 32, "two rounds of 32 lanes per 64 words");
    const int b = (int)(field / OFF_B), r = (int)(field % OFF_B);
    int64_t v = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = lr + 32 * j;
        if (k < b) v += agg[offset_at(col, k)];
        if (k < r) v += counts[(int64_t)col * n + (field - r) + k];
    }
    if (b > 64) {
#pragma unroll
        for (int j = 2; j < 4; ++j) { const int k = lr + 32 * j; if (k < b) v += agg[offset_at(col, k)]; }
    }
    return v;
}
// this lane's share of total(col)
__device__ __forceinline__ int64_t offset_total_part(const int64_t *__restrict__ agg, int nblk, int col, int lane)
{
    int64_t v = 0;
    if (lane < nblk) v += agg[offset_at(col, lane)];
    if (nblk > 64 && 64 + lane < nblk) v += agg[offset_at(col, 64 + lane)];
    return v;
}
// Every column at once, the rows read as the contiguous words they are (a lane per block, one column at a time, costs a cache line per lane
// and load: the fill pass of 4096 fields took 7 us longer).  Lane l takes the 16 bytes -- columns 2 (l & 15) and 2 (l & 15) + 1 -- of row
// 4k + (l >> 4), k = 0, 1, ...: four rows per load, all of it coalesced.  Returns, in every lane, the sums of those two columns over the rows
// below b (p0, p1: the first level of prefix(col, field of block b)) and over all nb rows (t0, t1: total(col)); offset_col picks a column.
__device__ __forceinline__ void offset_row_sums(const int64_t *__restrict__ agg, int b, int nb, int lane, int64_t &p0, int64_t &p1, int64_t &t0, int64_t &t1)
{
    static_assert(OFF_ROW == 32, "sixteen lanes of two words per row");
    p0 = p1 = t0 = t1 = 0;
    const longlong2 *rows = reinterpret_cast<const longlong2 *>(agg) + (lane & 15);
    const int nk = (nb + 3) / 4;
#pragma unroll 8
    for (int k = 0; k < nk; ++k) {
        const int row = 4 * k + (lane >> 4);
        longlong2 w = make_longlong2(0, 0);
        if (row < nb) w = rows[row * (OFF_ROW / 2)];
        t0 += w.x; t1 += w.y;
        if (row < b) { p0 += w.x; p1 += w.y; }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) { p0 += __shfl_xor(p0, o); p1 += __shfl_xor(p1, o); t0 += __shfl_xor(t0, o); t1 += __shfl_xor(t1, o); }
}
__device__ __forceinline__ int64_t offset_col(int64_t s0, int64_t s1, int col)
{
    const int64_t v = (col & 1) ? s1 : s0;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, col >> 1), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), col >> 1);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
#endif

}  // namespace fcpp
