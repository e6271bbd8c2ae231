// fcpp_samplefn.h -- device code the fixed-step samplers share (fcpp_traj.hip: a trajectory every dt seconds; fcpp_dubins.hip: a solved
// path every `spacing` metres; fcpp_rs.hip: the same per gear run): how many samples a path of total T gets, the offsets of all paths' samples, and the path of a sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fcpp {

// The count rule: K = floor(T / step) + 1 samples at k * step, and one more AT T when with_end is set and the last of them lies before
// it.  A total that is negative or not finite, or 2^31 samples or more, counts as bad (K = 0); nan_one: a NaN total is one sample instead.
__device__ __forceinline__ int64_t sample_count(double T, double step, bool with_end, bool nan_one, int64_t &bad)
{
    const double q = floor(T / step);
    if (nan_one && T != T) return 1;
    if (!(T >= 0.0) || !(q < 2147483646.0)) { ++bad; return 0; }
    const int64_t K = (int64_t)q + 1;
    return K + (with_end && (double)(K - 1) * step < T ? 1 : 0);
}

// A path sampled PER RUN (fcpp_rs.hip: a Reeds-Shepp path, run by run of one gear): every run of length len[r] by the count rule with its
// end, so that a junction of two runs is a sample of both.  2^31 samples or more in all count as bad, like one run of that many.
__device__ __forceinline__ int64_t sample_count_runs(const double *len, int n_runs, double step, int64_t &bad)
{
    int64_t K = 0, b = 0;
    for (int r = 0; r < n_runs; ++r) K += sample_count(len[r], step, true, false, b);
    if (b || K > 2147483646) { ++bad; return 0; }
    return K;
}

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

// sample q of all: p = the last path with out_offsets[p] <= q, k = its index in that path, K = the path's samples
__device__ __forceinline__ void sample_path(const int64_t *__restrict__ out_offsets, int64_t n, int64_t q, int64_t &p, int64_t &k, int64_t &K)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (out_offsets[mid] <= q) lo = mid; else hi = mid;
    }
    p = lo; k = q - out_offsets[p]; K = out_offsets[p + 1] - out_offsets[p];
}

}  // namespace fcpp
