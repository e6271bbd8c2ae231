// fcpp_solvegroupfn.h -- device code the second passes of the clear-connector rule share (fcpp_solveclear.hip: the clear connectors, the clear
// field paths, the priced transit block; fcpp_transit.hip: the loop transits' stations pass): a group of lanes per item, a lane per word.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_solveclear.h"
#include "fcpp_solveclearfn.h"

namespace fcpp {

// the lanes of a second-pass group: a lane per word, a power of two, within a wavefront
template <int MODE> struct SolveClearGroup { static constexpr int G = MODE == 0 ? 8 : 64; };

// The body of both second passes: lane w of a group of G looks at word w of the group's pair (have: the group has one; f its field, a
// valid one) and the group's winner hands (word, seg, total, rank, crossings) to store.  Called by every lane of the wavefront.
template <int MODE, class Store>
__device__ __forceinline__ void solve_clear_group(bool have, int64_t f, double x0, double y0, double h0, double x1, double y1, double h1, double R,
                                                  const ClearFields &F, const Store &store)
{
    constexpr int NW = SolveClearWords<MODE>::NW, G = SolveClearGroup<MODE>::G;
    static_assert(NW <= G && 64 % G == 0 && SOLVECLEAR_BLOCK % G == 0, "a lane per word, groups within a wavefront");
    const int lane = threadIdx.x & 63, w = lane & (G - 1);

    SolveClearOne<MODE> one(w);
    int key = 2, crossings = 0;                           // 0 clear, 1 not clear, 2 no candidate
    if (have && w < NW) {
        const bool fin = solve_clear_words<MODE>(x0, y0, h0, x1, y1, h1, R, one);
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
    store(w, one.seg, one.total, bk == 0 ? (int)__popcll(group) : -1, bk == 0 ? 0 : crossings);
}

}  // namespace fcpp
