// fcpp_listfn.h -- device code the two-pass operators share (fcpp_solveclear.hip: the clear connectors and the clear field paths;
// fcpp_clear.hip: the priced transit block): the append of a first pass, which lists the items its second pass has to look at.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fcpp {

// The append of every first pass.  Called by every lane of the wavefront; `more` lanes get a place each: per wavefront one ballot, ONE
// vector atomicAdd of the ballot's count by its first listed lane, the base handed round by a shuffle, each listed lane at base + its
// position in the ballot.
__device__ __forceinline__ void solve_clear_append(bool more, int64_t item, int64_t *__restrict__ list, unsigned long long *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(more);
    if (m == 0) return;                                   // (uniform over the wavefront)
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    // (at most one entry per item: base + position stays below the room the caller gave)
    if (more) list[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = item;
}

}  // namespace fcpp
