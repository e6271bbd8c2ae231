// fcpp_samplefn.h -- device code the fixed-step samplers share (fcpp_traj.hip: a trajectory every dt seconds; fcpp_conn.hip: a solved
// connector every `spacing` metres): the offsets of all paths' samples and the path of a sample.  How many samples a path of total T
// gets is the host+device count rule of fcpp_connfn.h (sample_count, sample_count_runs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcpp_connfn.h"
#include "fcpp_launch.h"

namespace fcpp {

// out_offsets (n + 1) = the exclusive scan of the paths' sample counts, err[0] = the number of bad paths.  count_of(p, bad): the samples
// of path p (0 and ++bad for a bad one).  One workgroup of BLOCK lanes walks the paths BLOCK at a time (an integer scan: exact in any order).
template <int BLOCK, class CountOf>
__device__ __forceinline__ void sample_scan(int64_t n, CountOf count_of, int64_t *__restrict__ out_offsets, int64_t *__restrict__ err)
{
    constexpr int NWAVE = BLOCK / 64;
    __shared__ int64_t sh[NWAVE];
    __shared__ int64_t carry_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t bad = 0;
    if (tid == 0) carry_sh = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += BLOCK) {
        const int64_t p = base + tid;
        const int64_t K = p < n ? count_of(p, bad) : 0;
        int64_t inc = K;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t pv = __shfl_up(inc, o);
            if (lane >= o) inc += pv;
        }
        if (lane == 63) sh[wave] = inc;
        __syncthreads();
        int64_t pre = carry_sh, tot = 0;
        for (int w = 0; w < NWAVE; ++w) { if (w < wave) pre += sh[w]; tot += sh[w]; }
        if (p < n) out_offsets[p] = pre + inc - K;
        __syncthreads();
        if (tid == 0) carry_sh += tot;
        __syncthreads();
    }
    if (tid == 0) out_offsets[n] = carry_sh;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    __syncthreads();
    if (lane == 0) sh[wave] = bad;
    __syncthreads();
    if (tid == 0) { int64_t b = 0; for (int w = 0; w < NWAVE; ++w) b += sh[w]; err[0] = b; }
}

// the counts of paths sampled from end to end: total_of(p) is the total of path p
template <int BLOCK, class TotalOf>
__global__ __launch_bounds__(BLOCK) void k_sample_counts(int64_t n, TotalOf total_of, double step, int with_end, int nan_one,
                                                         int64_t *__restrict__ out_offsets, int64_t *__restrict__ err)
{
    sample_scan<BLOCK>(n, [=](int64_t p, int64_t &bad) { return sample_count(total_of(p), step, with_end != 0, nan_one != 0, bad); }, out_offsets, err);
}

// the counts of paths with a count rule of their own: count_of(p, bad) as for sample_scan
template <int BLOCK, class CountOf>
__global__ __launch_bounds__(BLOCK) void k_path_counts(int64_t n, CountOf count_of, int64_t *__restrict__ out_offsets, int64_t *__restrict__ err)
{
    sample_scan<BLOCK>(n, count_of, out_offsets, err);
}

// the launches of the two: one workgroup of BLOCK lanes, whatever n
template <int BLOCK, class TotalOf>
inline int launch_sample_counts(hipStream_t st, int64_t n, TotalOf total_of, double step, int with_end, int nan_one, int64_t *out_offsets, int64_t *err)
{
    return launch(st, k_sample_counts<BLOCK, TotalOf>, 1, BLOCK, n, total_of, step, with_end, nan_one, out_offsets, err);
}

template <int BLOCK, class CountOf>
inline int launch_path_counts(hipStream_t st, int64_t n, CountOf count_of, int64_t *out_offsets, int64_t *err)
{
    return launch(st, k_path_counts<BLOCK, CountOf>, 1, BLOCK, n, count_of, out_offsets, err);
}

// the last index i of 0 .. n - 1 with key(i) <= q, for a non-decreasing key with key(0) <= q: the path of a sample, the group of a slot
template <class Key>
__device__ __forceinline__ int64_t last_at_or_before(int64_t n, int64_t q, Key key)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (key(mid) <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// sample q of all: p = the last path with out_offsets[p] <= q, k = its index in that path, K = the path's samples
__device__ __forceinline__ void sample_path(const int64_t *__restrict__ out_offsets, int64_t n, int64_t q, int64_t &p, int64_t &k, int64_t &K)
{
    p = last_at_or_before(n, q, [&](int64_t i) { return out_offsets[i]; });
    k = q - out_offsets[p]; K = out_offsets[p + 1] - out_offsets[p];
}

}  // namespace fcpp
