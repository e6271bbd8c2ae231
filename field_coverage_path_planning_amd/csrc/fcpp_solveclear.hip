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
//
// The CLEAR FIELD PATHS (fcpp_field_path_counts_clear / _fill_clear) run the same two passes over the connector slots of the leg records
// k_fpath_legs wrote: k_fpath_clear_slots and k_fpath_clear_words below share the append (solve_clear_append) and the whole second-pass
// body (solve_clear_group) with the two kernels above; only where the poses come from and where the winner writes differ.
//
// The PRICED TRANSIT BLOCK (fcpp_route_transit_priced) has its first pass in fcpp_clear.hip -- k_clear_transit's tiled walk, which lists
// entries of T through the same append (fcpp_listfn.h) -- and its second pass here: k_route_priced_words, solve_clear_group on the poses
// of a listed entry's pair.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_listfn.h"
#include "fcpp_samplefn.h"
#include "fcpp_solveclear.h"
#include "fcpp_solveclearfn.h"
#include "fcpp_solvegroupfn.h"

namespace fcpp {

static constexpr int SBLOCK = SOLVECLEAR_BLOCK;

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
    bool more = false;
    if (i < n) {
        SolveClearResult r;
        more = solve_clear_first<MODE>(F, io.pair_field[i], io.fx[i], io.fy[i], io.fh[i], io.tx[i], io.ty[i], io.th[i], R, r);
        solve_clear_store<NSEG>(io, i, r.word, r.seg, r.len, r.rank, r.crossings);
    }
    solve_clear_append(more, i, list, count);
}

template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_solve_clear_words(int64_t count, const int64_t *__restrict__ list, SolveClearIo io, double R, ClearFields F)
{
    constexpr int NSEG = Conn<MODE>::NSEG, G = SolveClearGroup<MODE>::G;
    const int64_t t = (int64_t)blockIdx.x * SBLOCK + threadIdx.x, j = t / G;
    const bool have = j < count;
    const int64_t i = have ? list[j] : 0;
    const double x0 = have ? io.fx[i] : 0.0, y0 = have ? io.fy[i] : 0.0, h0 = have ? io.fh[i] : 0.0;
    const double x1 = have ? io.tx[i] : 0.0, y1 = have ? io.ty[i] : 0.0, h1 = have ? io.th[i] : 0.0;
    solve_clear_group<MODE>(have, have ? io.pair_field[i] : -1, x0, y0, h0, x1, y1, h1, R, F,
                            [&](int word, const double *seg, double total, int rank, int crossings) {
                                solve_clear_store<NSEG>(io, i, word, seg, total, rank, crossings);
                            });
}

// ---- the priced transit block (fcpp_route_transit_priced) -- behind k_clear_transit<MODE, true> of fcpp_clear.hip -------------------------
// k_route_priced_words, a group of lanes per listed ENTRY of T: the entry's field by bisection of the block offsets (a field without a
// block owns no entry: the last field that starts at or before the entry is the one that holds it), (p, q) from its place in the block,
// the poses by route_pose as the first pass formed them, then solve_clear_group as it is.  A winner of rank >= 0 writes its total and rank
// to both mirrored entries; with no clear word nothing is written and the first pass's answer stands.  Listed entries are canonical
// pairs, each listed once: no entry has two writers, no atomics.  The edges come from global memory through the CSR.
template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_route_priced_words(int64_t count, const int64_t *__restrict__ list, int64_t n,
                                                               const int64_t *__restrict__ soff, const double *__restrict__ ax,
                                                               const double *__restrict__ ay, const double *__restrict__ bx,
                                                               const double *__restrict__ by, const double *__restrict__ angle, double R,
                                                               const int64_t *__restrict__ toff, int64_t t_total, ClearFields F,
                                                               double *__restrict__ T, int8_t *__restrict__ K)
{
    constexpr int G = SolveClearGroup<MODE>::G;
    const int64_t t = (int64_t)blockIdx.x * SBLOCK + threadIdx.x, j = t / G;
    bool have = j < count;
    const int64_t g = have ? list[j] : 0;
    int64_t f = -1, e2 = 0;
    double x0 = 0.0, y0 = 0.0, h0 = 0.0, x1 = 0.0, y1 = 0.0, h1 = 0.0;
    have = have && g >= 0 && g < t_total;                  // (a listed entry lies in T: checked again so that nothing is written beside it)
    if (have) {
        f = last_at_or_before(n, g, [&](int64_t i) { return toff[i]; });
        const int64_t s0 = soff[f], N = 2 * (soff[f + 1] - s0), e = g - toff[f];
        have = N > 0 && e < N * N && toff[f + 1] - toff[f] == N * N;
        if (have) {
            const int p = (int)(e / N), q = (int)(e - (int64_t)p * N);
            e2 = toff[f] + (int64_t)(q ^ 1) * N + (p ^ 1);
            route_pose(ax + s0, ay + s0, bx + s0, by + s0, angle[f], p, true, x0, y0, h0);
            route_pose(ax + s0, ay + s0, bx + s0, by + s0, angle[f], q, false, x1, y1, h1);
        }
    }
    solve_clear_group<MODE>(have, f, x0, y0, h0, x1, y1, h1, R, F, [&](int, const double *, double total, int rank, int) {
        if (rank < 0) return;
        T[g] = total;
        T[e2] = total;
        if (K) { K[g] = (int8_t)rank; K[e2] = (int8_t)rank; }
    });
}

// ---- the clear field paths (the rule: fcpp_fpathfn.h) -- between k_fpath_legs and the scan ------------------------------------------------
// k_fpath_clear_slots, a lane per CONNECTOR slot: field i owns m_i + 1 of them, the field by bisection of soff[i] + i.  The lane does not
// solve: word, seg and start pose are the record's, as k_fpath_legs wrote it; it tests that word against field i of the region
// (solve_clear_test), writes the slot's rank and crossings by solve_clear_first's decision rules and appends a slot whose word starts
// inside a valid region field but crosses (solve_clear_append).  Slots without a solved connector and fields that failed are skipped: their
// rank and crossings stay the 0 the call set.  Against fcpp_conn_solve_clear on the legs' poses this saves the second solve of every
// connector -- the record already holds the shortest word -- and the gather of six pose arrays and a field index per leg on the host side;
// static reasoning, nothing measured.
template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_fpath_clear_slots(int64_t n, int64_t n_conn, const int64_t *__restrict__ soff, double R,
                                                              const FpathLeg *__restrict__ legs, const int32_t *__restrict__ status, ClearFields F,
                                                              int32_t *__restrict__ rank, int32_t *__restrict__ crossings,
                                                              int64_t *__restrict__ list, unsigned long long *__restrict__ count)
{
    const int64_t c = (int64_t)blockIdx.x * SBLOCK + threadIdx.x;
    bool more = false;
    int64_t p = 0;
    if (c < n_conn) {
        const int64_t i = last_at_or_before(n, c, [&](int64_t f) { return soff[f] + f; });      // the field that holds connector slot c
        p = fpath_first_slot(soff, i) + 2 * (c - (soff[i] + i));
        const FpathLeg &lg = legs[p];      // (read where it lies: a copy with its indexed segments would live in scratch)
        if (fpath_is_conn(lg) && (!status || status[i] == FPATH_OK) && i < F.n) {
            bool valid;
            const ClearResult r = solve_clear_test<MODE>(F, i, lg.x0, lg.y0, lg.h0, R, lg.word, lg.seg, valid);
            int rk = -1, cr = 0;
            if (valid) {
                if (r.clear) rk = 0;
                else { cr = r.crossings; more = r.inside != 0; }
            }
            if (rank) rank[p] = rk;
            if (crossings) crossings[p] = cr;
        }
    }
    solve_clear_append(more, p, list, count);
}

// k_fpath_clear_words, a group of lanes per listed slot: solve_clear_group on the slot's poses (fpath_conn_poses: the very poses the
// record was solved from).  The winner's lane overwrites the record's word, seg and total, the slot's count, rank and crossings; the
// other lanes of the group read the record's field and slot only, which nobody writes.
template <int MODE>
__global__ __launch_bounds__(SBLOCK) void k_fpath_clear_words(int64_t count, const int64_t *__restrict__ list, FpathIn in, ClearFields F,
                                                              FpathLeg *__restrict__ legs, int64_t *__restrict__ cnt, int32_t *__restrict__ rank,
                                                              int32_t *__restrict__ crossings)
{
    constexpr int G = SolveClearGroup<MODE>::G;
    const int64_t t = (int64_t)blockIdx.x * SBLOCK + threadIdx.x, j = t / G;
    bool have = j < count;
    const int64_t p = have ? list[j] : 0;
    int64_t f = -1;
    double x0 = 0.0, y0 = 0.0, h0 = 0.0, x1 = 0.0, y1 = 0.0, h1 = 0.0;
    if (have) {
        bool invalid = false;
        f = legs[p].field;
        have = fpath_conn_poses(in, f, legs[p].slot, x0, y0, h0, x1, y1, h1, invalid);      // (a listed slot has a record: so poses)
    }
    solve_clear_group<MODE>(have, f, x0, y0, h0, x1, y1, h1, in.R, F, [&](int word, const double *seg, double total, int rk, int cr) {
        const int64_t K = fpath_set_word<MODE>(legs[p], word, seg, total, in.spacing);
        if (cnt) cnt[p] = K;
        if (rank) rank[p] = rk;
        if (crossings) crossings[p] = cr;
    });
}

// k_fpath_clear_report, a lane per slot: the record's word, seg and total in fcpp_debug_field_paths' layout; then a lane per field: its
// legs of rank -1 and of rank > 0 (m_i + 1 loads).
__global__ __launch_bounds__(SBLOCK) void k_fpath_clear_report(int64_t n, int64_t n_slots, const int64_t *__restrict__ soff,
                                                               const FpathLeg *__restrict__ legs, const int32_t *__restrict__ rank,
                                                               int32_t *__restrict__ leg_word, double *__restrict__ leg_seg,
                                                               double *__restrict__ leg_total, int32_t *__restrict__ blocked,
                                                               int32_t *__restrict__ reshaped)
{
    const int64_t g = (int64_t)blockIdx.x * SBLOCK + threadIdx.x;
    if (g < n_slots) {
        const FpathLeg &lg = legs[g];
        if (leg_word) leg_word[g] = lg.kind == FPATH_DUBINS || lg.kind == FPATH_RS ? lg.word : -1;
        if (leg_seg) {
#pragma unroll
            for (int k = 0; k < 5; ++k) leg_seg[5 * g + k] = lg.seg[k];
        }
        if (leg_total) leg_total[g] = lg.total;
        return;
    }
    const int64_t i = g - n_slots;
    if (i >= n || !rank) return;
    int32_t b = 0, r = 0;
    for (int64_t p = fpath_first_slot(soff, i); p < fpath_first_slot(soff, i + 1); p += 2) {
        b += rank[p] < 0;
        r += rank[p] > 0;
    }
    if (blocked) blocked[i] = b;
    if (reshaped) reshaped[i] = r;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_solve_clear_pairs(hipStream_t st, int mode, int64_t n, const SolveClearIo &io, double R, const ClearFields &F, int64_t *list,
                             unsigned long long *count)
{
    if (n <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_solve_clear_pairs<M()>, blocks_for(n, SBLOCK), SBLOCK, n, io, R, F, list, count);
    });
}

int launch_solve_clear_words(hipStream_t st, int mode, int64_t count, const int64_t *list, const SolveClearIo &io, double R, const ClearFields &F)
{
    if (count <= 0) return 0;
    const int64_t per = SBLOCK / (mode == 0 ? SolveClearGroup<0>::G : SolveClearGroup<1>::G);
    return by_mode(mode, [&](auto M) {
        return launch(st, k_solve_clear_words<M()>, blocks_for(count, per), SBLOCK, count, list, io, R, F);
    });
}

int launch_route_priced_words(hipStream_t st, int mode, int64_t count, const int64_t *list, int64_t n, const int64_t *soff, const double *ax,
                              const double *ay, const double *bx, const double *by, const double *angle, double R, const int64_t *toff,
                              int64_t t_total, const ClearFields &F, double *T, int8_t *K)
{
    if (count <= 0 || n <= 0) return 0;
    const int64_t per = SBLOCK / (mode == 0 ? SolveClearGroup<0>::G : SolveClearGroup<1>::G);
    return by_mode(mode, [&](auto M) {
        return launch(st, k_route_priced_words<M()>, blocks_for(count, per), SBLOCK, count, list, n, soff, ax, ay, bx, by, angle, R, toff, t_total, F,
                      T, K);
    });
}

int launch_fpath_clear_slots(hipStream_t st, int mode, int64_t n, int64_t n_conn, const int64_t *soff, double R, const FpathLeg *legs,
                             const int32_t *status, const ClearFields &F, int32_t *rank, int32_t *crossings, int64_t *list,
                             unsigned long long *count)
{
    if (n <= 0 || n_conn <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_fpath_clear_slots<M()>, blocks_for(n_conn, SBLOCK), SBLOCK, n, n_conn, soff, R, legs, status, F, rank, crossings, list,
                      count);
    });
}

int launch_fpath_clear_words(hipStream_t st, int mode, int64_t count, const int64_t *list, const FpathIn &in, const ClearFields &F, FpathLeg *legs,
                             int64_t *cnt, int32_t *rank, int32_t *crossings)
{
    if (count <= 0) return 0;
    const int64_t per = SBLOCK / (mode == 0 ? SolveClearGroup<0>::G : SolveClearGroup<1>::G);
    return by_mode(mode, [&](auto M) {
        return launch(st, k_fpath_clear_words<M()>, blocks_for(count, per), SBLOCK, count, list, in, F, legs, cnt, rank, crossings);
    });
}

int launch_fpath_clear_report(hipStream_t st, int64_t n, int64_t n_slots, const int64_t *soff, const FpathLeg *legs, const int32_t *rank,
                              int32_t *leg_word, double *leg_seg, double *leg_total, int32_t *blocked, int32_t *reshaped)
{
    if (n <= 0 || !(leg_word || leg_seg || leg_total || blocked || reshaped)) return 0;
    return launch(st, k_fpath_clear_report, blocks_for(n_slots + n, SBLOCK), SBLOCK, n, n_slots, soff, legs, rank, leg_word, leg_seg, leg_total,
                  blocked, reshaped);
}

}  // namespace fcpp
