// fcpp_solveclear.hip -- gfx950 (MI355X) kernels of the clear connectors: per pair of poses the shortest feasible Dubins or Reeds-Shepp word
// that stays inside the pair's field.  The rule is ONE set of host+device expressions, fcpp_solveclearfn.h over fcpp_clearfn.h and the two
// solvers; float64, -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_conn_solve_clear gives.
//
// Two passes, because most pairs need one word only and the few that need all of them need 6 or 48 times the work.
//
// k_solve_clear_pairs, a lane per pair: solve_clear_first -- the solve, the shortest word's pieces, the field's edges read from GLOBAL
// memory through the CSR (clear_walk, as in k_clear_conn: pairs grouped by field make a wavefront read one cache line, pairs that are
// not are still right).  EVERY lane writes a complete result; for a pair whose shortest word starts inside and crosses the boundary that
// is the rank -1 answer, and the lane appends the pair's index to a list: per wavefront one ballot, ONE vector atomicAdd of the ballot's
// count by its first listed lane, the base handed round by a shuffle, each listed lane at base + its position in the ballot.  The call
// reads the count back (it synchronises anyway) and skips the second launch when it is 0.
//
// k_solve_clear_words, a group of G lanes per listed pair (G = 8 for Dubins' 6 words, 64 for Reeds-Shepp's 48), lane w of the group for
// word w.  A lane runs the solver's own word enumeration into an accumulator that keeps word w only (SolveClearOne): the enumeration
// shares nearly everything between words -- the polar forms, the roots -- so a lane that skipped the other words would save little and
// the code would have to name every word's formula a second time; as it is there is one enumeration, and the kept word has the
// solver's bits by construction.  Then the lane builds its pieces and walks the field's edges; the whole group reads the same vertex.
// xor-shuffles within the group find the least (not clear, total, word); rank is the number of candidates of the group ordered before
// the winner, counted from a ballot.  The winner's lane overwrites the pair's result -- when no word is clear the winner is the shortest
// word and what it writes is what the first pass wrote.  No result depends on the list's order and no entry has two writers in a launch.
// No lane leaves before the shuffles: lanes without a pair or a word carry the key of an infeasible word and write nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_solveclear.h"
#include "fcpp_solveclearfn.h"

namespace fcpp {

static constexpr int SBLOCK = SOLVECLEAR_BLOCK;

#define SOLVECLEAR_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

template <int NSEG>
__device__ __forceinline__ void solve_clear_store(const SolveClearIo &io, int64_t i, int word, const double *seg, double len, int rank, int crossings)
{
    if (io.word) io.word[i] = word;
    if (io.seg) {
#pragma unroll
        for (int k = 0; k < NSEG; ++k) io.seg[i * NSEG + k] = seg[k];
    }
    if (io.len) io.len[i] = len;
    if (io.rank) io.rank[i] = rank;
    if (io.crossings) io.crossings[i] = crossings;
}

template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_solve_clear_pairs(int64_t n, SolveClearIo io, double R, ClearFields F, int64_t *__restrict__ list,
                                                              unsigned long long *__restrict__ count)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    const int64_t i = (int64_t)blockIdx.x * SBLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool more = false;
    if (i < n) {
        SolveClearResult r;
        more = solve_clear_first<MODE>(F, io.pair_field[i], io.fx[i], io.fy[i], io.fh[i], io.tx[i], io.ty[i], io.th[i], R, r);
        solve_clear_store<NSEG>(io, i, r.word, r.seg, r.len, r.rank, r.crossings);
    }
    const unsigned long long m = __ballot(more);
    if (m == 0) return;                                   // (uniform over the wavefront)
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    // (at most one entry per pair: base + position < n, the room the caller gave)
    if (more) list[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_solve_clear_words(int64_t count, const int64_t *__restrict__ list, SolveClearIo io, double R, ClearFields F)
{
    constexpr int NSEG = Conn<MODE>::NSEG, NW = SolveClearWords<MODE>::NW, G = MODE == 0 ? 8 : 64;
    static_assert(NW <= G && 64 % G == 0 && SBLOCK % G == 0, "a lane per word, groups within a wavefront");
    const int64_t t = (int64_t)blockIdx.x * SBLOCK + threadIdx.x, j = t / G;
    const int lane = threadIdx.x & 63, w = lane & (G - 1);
    const bool have = j < count;
    const int64_t i = have ? list[j] : 0;
    const double x0 = have ? io.fx[i] : 0.0, y0 = have ? io.fy[i] : 0.0, h0 = have ? io.fh[i] : 0.0;

    SolveClearOne<MODE> one(w);
    int key = 2, crossings = 0;                           // 0 clear, 1 not clear, 2 no candidate
    if (have && w < NW) {
        const int64_t f = io.pair_field[i];
        const bool fin = solve_clear_words<MODE>(x0, y0, h0, io.tx[i], io.ty[i], io.th[i], R, one);
        // (a listed pair is solved and names a valid field; checked again so that a lane never walks a field that is not there)
        if (fin && one.ok && f >= 0 && f < F.n) {
            bool valid;
            const ClearResult c = solve_clear_test<MODE>(F, f, x0, y0, h0, R, w, one.seg, valid);
            key = c.clear ? 0 : 1;
            crossings = c.crossings;
        }
    }
    const bool cand = key < 2;
    const double total = cand ? one.total : INFINITY;

    int bk = key, bw = w;
    double bt = total;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const int ok_ = __shfl_xor(bk, o), ow = __shfl_xor(bw, o);
        const double ot = __shfl_xor(bt, o);
        if (ok_ < bk || (ok_ == bk && solve_clear_before(ot, ow, bt, bw))) { bk = ok_; bt = ot; bw = ow; }
    }
    const bool before = cand && solve_clear_before(total, w, bt, bw);
    const unsigned long long mask = __ballot(before);
    const unsigned long long group = G == 64 ? mask : (mask >> (lane & ~(G - 1))) & ((1ull << G) - 1ull);
    if (!have || bk == 2 || w != bw) return;
    solve_clear_store<NSEG>(io, i, w, one.seg, one.total, bk == 0 ? (int)__popcll(group) : -1, bk == 0 ? 0 : crossings);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_solve_clear_pairs(hipStream_t st, int mode, int64_t n, const SolveClearIo &io, double R, const ClearFields &F, int64_t *list,
                             unsigned long long *count)
{
    if (n <= 0) return 0;
    const dim3 grid((unsigned)((n + SBLOCK - 1) / SBLOCK));
    if (mode == 0) hipLaunchKernelGGL(k_solve_clear_pairs<0>, grid, dim3(SBLOCK), 0, st, n, io, R, F, list, count);
    else hipLaunchKernelGGL(k_solve_clear_pairs<1>, grid, dim3(SBLOCK), 0, st, n, io, R, F, list, count);
    SOLVECLEAR_LAUNCH_CHECK();
    return 0;
}

int launch_solve_clear_words(hipStream_t st, int mode, int64_t count, const int64_t *list, const SolveClearIo &io, double R, const ClearFields &F)
{
    if (count <= 0) return 0;
    const int64_t per = SBLOCK / (mode == 0 ? 8 : 64);
    const dim3 grid((unsigned)((count + per - 1) / per));
    if (mode == 0) hipLaunchKernelGGL(k_solve_clear_words<0>, grid, dim3(SBLOCK), 0, st, count, list, io, R, F);
    else hipLaunchKernelGGL(k_solve_clear_words<1>, grid, dim3(SBLOCK), 0, st, count, list, io, R, F);
    SOLVECLEAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace fcpp
