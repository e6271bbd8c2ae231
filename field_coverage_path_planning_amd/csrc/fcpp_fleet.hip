// fcpp_fleet.hip -- gfx950 (MI355X) kernel of the vehicle shares: k_fleet_solve splits every field's candidate tours, in both driving
// directions, among at most K vehicles of one depot so that the largest share cost is least, and among those splits takes the least sum.
// The rule is ONE set of host+device expressions, fcpp_fleetfn.h; float64, -ffp-contract=off like every other translation unit, so the
// kernel gives the bits fcpp_debug_fleet_solve gives.
//
// One workgroup of 256 threads per field.  Wavefront w takes the variants v = w, w + 4, .. (with both_ways = 0, where only the even
// variants exist, 2 w, 2 w + 8, ..): each wavefront keeps the tables of its variant (t, P, S, the way in per position) and two layer rows
// in LDS of its own, 21 KiB, so the four share nothing until the end.  The kernel has two instances, for batches whose largest field has
// at most FLSMALL = 192 swaths and for all others: the tables are sized by the instance's cap, and the small one lets three workgroups
// share a CU's LDS where the large one leaves room for one.  A variant:
//   tables     a lane per position: the oriented swath, its length, its way in, the transit behind it (all loads in flight together).
//   chains     P and S are left-to-right rounded sums, sequential by rule: lane 0 walks both from LDS.
//   layers     stage 1 (min-max), then stage 2 (min-sum under M): per layer k a lane per END position j, in rounds of 64; the lane walks
//              the starts i ascending with a strict "less than", so ties go to the lowest i by construction and no reduction tree is
//              needed; at step i every lane reads the same LDS words (a broadcast).  No start is skipped: the windows are not monotone
//              in floating point.  K m^2 / 2 share costs per stage and variant.
// The variants are solved for their VALUES only; pred for 16 layers x 513 positions is 16 KiB, which does not fit beside the rows four
// times.  Behind one barrier the block picks the least (M, sum, v) of the four wavefronts, and the first wavefront solves the winner's
// stage 2 once more with pred kept (M is known: stage 1 is not repeated), backtracks (lane 0, at most K steps) and the block writes the
// shares.  The candidates are validated before anything is indexed by them (a bit per swath in LDS, set by LDS atomics): a bad tour never
// reaches T.  No float atomics, no per-thread arrays (no scratch), every loop bounded by m, K or C.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_fleet.h"
#include "fcpp_fleetfn.h"
#include "fcpp_launch.h"

namespace fcpp {

static constexpr int FLBLOCK = 256;
static constexpr int FLWAVES = FLBLOCK / 64;
static constexpr int FLSMALL = 192;             // the small instance's cap on a field's swaths

template <int MCAP>
struct FleetWave {           // a wavefront's LDS, for fields of at most MCAP swaths
    static constexpr int POS = MCAP + 1;
    double P[POS], S[MCAP], A[MCAP], row[2][POS];
    int16_t t[MCAP];
};

// what one lane of a wavefront wrote to LDS, for the others to read
__device__ __forceinline__ void fleet_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// fleet_tables_host by ONE wavefront (m > 0): t, P, S and A[k] = In[t[k]] of variant v in W
template <class WV>
__device__ __forceinline__ void fleet_tables_wave(const FleetField &F, int v, WV &W)
{
    const int lane = threadIdx.x & 63, m = F.m, N = 2 * m, r = v & 1;
    const int32_t *cand = F.tours + (v >> 1) * F.stride;
    fleet_wave_sync();
    // W.P[k + 1] holds the swath's length and W.S[k] the transit into position k until the chains have walked them
    for (int k = lane; k < m; k += 64) {
        const int b = trip_at(cand, m, r, k);
        W.t[k] = (int16_t)b;
        W.P[k + 1] = F.length[b >> 1];
        W.A[k] = F.In[b];
        W.S[k] = k > 0 ? F.T[trip_at(cand, m, r, k - 1) * N + b] : 0.0;
    }
    fleet_wave_sync();
    if (lane == 0) {
        double s = 0.0;
        W.P[0] = 0.0;
        for (int k = 0; k < m; ++k) { s = s + W.P[k + 1]; W.P[k + 1] = s; }
        s = 0.0;
        W.S[0] = 0.0;
        for (int k = 1; k < m; ++k) { s = s + W.S[k]; W.S[k] = s; }
    }
    fleet_wave_sync();
}

// layer k (1 <= k <= min(K, m)) of stage 1 or 2 by one wavefront: W.row[cur][j] for j = k .. m from W.row[cur ^ 1]; KEEP: pred_row[j] too
template <int STAGE, bool KEEP, class WV>
__device__ __forceinline__ void fleet_layer_wave(const FleetField &F, WV &W, int k, int cur, double M, int16_t *pred_row)
{
    const int lane = threadIdx.x & 63, m = F.m;
    const double nan = __builtin_nan("");
    const double *prev = W.row[cur ^ 1];
    double *next = W.row[cur];
    for (int j0 = k; j0 <= m; j0 += 64) {
        const int j = j0 + lane, jj = j <= m ? j : m;                    // (a lane beyond m reads m's words and stores nothing)
        const int last = j0 + 63 < m ? j0 + 63 : m;                      // the round's last end position (uniform)
        const int end = k == 1 ? 1 : last;                               // layer 1 starts at 0 alone
        const double Sj1 = W.S[jj - 1], Pj = W.P[jj], out_j = F.Out[W.t[jj - 1]];
        double best = STAGE == 1 ? INFINITY : 0.0;
        int bi = -1;
        for (int i = k - 1; i < end; ++i) {                              // (uniform: W.A[i], W.S[i], W.P[i], prev[i] are broadcasts)
            const double c = fleet_cost(W.A[i], W.S[i], W.P[i], Sj1, out_j, Pj, F.omega);
            const double h = prev[i];
            if (STAGE == 1) {
                const double g = fleet_max(h, c);
                if (i < j && g < best) best = g;
            } else if (i < j && fleet_is(h) && c <= M) {
                const double s = tour_plus(c, h);
                if (bi < 0 || s < best) { best = s; bi = i; }
            }
        }
        if (j <= m) {
            next[j] = STAGE == 1 || bi >= 0 ? best : nan;
            if (KEEP) pred_row[j] = (int16_t)bi;
        }
    }
    fleet_wave_sync();
}

// fleet_variant_host by ONE wavefront on the tables in W, every lane of which calls it with the same arguments; the result is the same
// in every lane.  KEEP: M is the variant's, known; stage 2 alone, pred (FLEET_MAX_VEHICLES rows of WV::POS) kept
template <bool KEEP, class WV>
__device__ __forceinline__ FleetVariant fleet_variant_wave(const FleetField &F, WV &W, double M, int16_t *pred)
{
    const int lane = threadIdx.x & 63, m = F.m, Kc = fleet_layers(F.K, m);
    if (m == 0) return { 0.0, 0.0, 0 };
    if (!KEEP) {
        if (lane == 0) W.row[0][0] = -INFINITY;                  // layer 0: the empty split, below every cost
        fleet_wave_sync();
        M = INFINITY;
        for (int k = 1, cur = 1; k <= Kc; ++k, cur ^= 1) {
            fleet_layer_wave<1, false>(F, W, k, cur, M, nullptr);
            const double g = W.row[cur][m];
            if (g < M) M = g;
        }
    }
    FleetVariant out = { M, __builtin_nan(""), 0 };
    if (lane == 0) W.row[0][0] = 0.0;
    fleet_wave_sync();
    for (int k = 1, cur = 1; k <= Kc; ++k, cur ^= 1) {
        fleet_layer_wave<2, KEEP>(F, W, k, cur, M, KEEP ? pred + (k - 1) * WV::POS : nullptr);
        const double h = W.row[cur][m];
        if (fleet_is(h) && (out.k == 0 || h < out.sum)) { out.sum = h; out.k = k; }
    }
    return out;
}

// MCAP: no field of the batch that has a block holds more swaths (the launcher's choice; a field beyond it is answered as one without)
template <int MCAP>
__global__ __launch_bounds__(FLBLOCK) void k_fleet_solve(FleetArgs a)
{
    using WV = FleetWave<MCAP>;
    __shared__ WV sh[FLWAVES];
    __shared__ int16_t sh_pred[FLEET_MAX_VEHICLES * WV::POS];
    __shared__ double sh_Ms[2 * TRIP_MAX_CANDIDATES], sh_sums[2 * TRIP_MAX_CANDIDATES];
    __shared__ uint32_t sh_seen[FLWAVES][ROUTE_MAX_SWATHS / 32];
    __shared__ double sh_M[FLWAVES], sh_sum[FLWAVES];
    __shared__ int sh_v[FLWAVES], sh_first[FLEET_MAX_VEHICLES + 1];
    __shared__ int sh_used, sh_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.x, s0 = a.soff[f], m64 = a.soff[f + 1] - s0;
    const int n_var = trip_n_variants(a.C), ks = a.k_stride;
    const double nan = __builtin_nan("");
    const int32_t *cand0 = a.tours + s0;
    const int Kf = a.K[f];
    int status = m64 > MCAP ? FLEET_EUNSUPPORTED : fleet_size_status(m64, Kf, ks);
    const int m = status == FLEET_OK ? (int)m64 : 0, N = 2 * m;
    const FleetField F = { a.T + a.toff[f], a.In + 2 * s0, a.Out + 2 * s0, a.length + s0, cand0, a.n_total, m, a.C, a.both_ways, Kf, ks, a.omega };
    if (status == FLEET_OK) {                  // (uniform: the whole workgroup is one field's)
        if (tid == 0) sh_bad = 0;
        __syncthreads();
        // the field's status before anything is indexed by a candidate: lengths, every candidate a permutation
        bool bad = false;
        for (int k = tid; k < m; k += FLBLOCK) bad |= !trip_length_ok(F.length[k]);
        for (int c0 = 0; c0 < a.C; c0 += FLWAVES) {
            const int c = c0 + wave;
            if (lane < ROUTE_MAX_SWATHS / 32) sh_seen[wave][lane] = 0;
            fleet_wave_sync();
            if (c < a.C) {
                const int32_t *cand = F.tours + c * F.stride;
                for (int k = lane; k < m; k += 64) {
                    const int32_t p = cand[k];
                    if (p < 0 || p >= N) { bad = true; continue; }
                    const uint32_t bit = 1u << ((p >> 1) & 31);
                    if (atomicOr(&sh_seen[wave][p >> 6], bit) & bit) bad = true;
                }
            }
            fleet_wave_sync();
        }
        if (bad) atomicOr(&sh_bad, 1);
        __syncthreads();
        if (!sh_bad) {
            WV &W = sh[wave];
            double best_M = INFINITY, best_sum = INFINITY;
            int best_v = INT32_MAX;
            // (one direction: the even variants alone, dealt to all four wavefronts; the odd slots of the value rows are NaN)
            const int step = a.both_ways ? 1 : 2;
            if (!a.both_ways && tid < a.C) { sh_Ms[2 * tid + 1] = nan; sh_sums[2 * tid + 1] = nan; }
            for (int v = wave * step; v < n_var; v += FLWAVES * step) {           // (uniform within a wavefront)
                if (m > 0) fleet_tables_wave(F, v, W);
                if (v == 0 && m > 0 && lane == 0 && !tour_finite(W.S[m - 1])) atomicOr(&sh_bad, 1);
                const FleetVariant r = fleet_variant_wave<false>(F, W, 0.0, nullptr);
                if (lane == 0) { sh_Ms[v] = r.M; sh_sums[v] = r.sum; }
                if (fleet_better(r.M, r.sum, v, best_M, best_sum, best_v) || best_v == INT32_MAX) { best_M = r.M; best_sum = r.sum; best_v = v; }
            }
            if (lane == 0) { sh_M[wave] = best_M; sh_sum[wave] = best_sum; sh_v[wave] = best_v; }
        }
        __syncthreads();
        if (sh_bad) status = FLEET_EINVAL;
    }
    double *Ms = a.makespans ? a.makespans + f * n_var : nullptr, *sums = a.totals ? a.totals + f * n_var : nullptr;
    int32_t *first = a.share_first ? a.share_first + f * ks : nullptr;
    double *scost = a.share_cost ? a.share_cost + f * ks : nullptr;
    if (status != FLEET_OK) {                  // candidate 0 as given, one share
        for (int64_t k = tid; k < m64; k += FLBLOCK) {
            if (a.tour) a.tour[s0 + k] = cand0[k];
            if (a.share) a.share[s0 + k] = 0;
        }
        if (tid < n_var) {
            if (Ms) Ms[tid] = nan;
            if (sums) sums[tid] = nan;
        }
        if (tid < ks) {
            if (first) first[tid] = tid == 0 && m64 > 0 ? 0 : -1;
            if (scost) scost[tid] = nan;
        }
        if (tid != 0) return;
        if (a.makespan) a.makespan[f] = nan;
        if (a.total) a.total[f] = nan;
        if (a.n_used) a.n_used[f] = m64 > 0 ? 1 : 0;
        if (a.winner) a.winner[f] = 0;
        if (a.status) a.status[f] = status;
        return;
    }
    int ww = 0;                                // the wavefront that holds the winner: the least (M, sum, v) of the four
#pragma unroll
    for (int x = 1; x < FLWAVES; ++x)
        if (sh_v[x] != INT32_MAX && fleet_better(sh_M[x], sh_sum[x], sh_v[x], sh_M[ww], sh_sum[ww], sh_v[ww])) ww = x;
    const int win = sh_v[ww];
    // the winner once more, by the first wavefront, stage 2 with pred kept; its tables stay in sh[0] for the share costs
    if (wave == 0) {
        if (m > 0) fleet_tables_wave(F, win, sh[0]);
        const FleetVariant r = fleet_variant_wave<true>(F, sh[0], sh_M[ww], sh_pred);
        if (lane == 0) {
            for (int k = r.k, j = m; k > 0; --k) {
                j = sh_pred[(k - 1) * WV::POS + j];
                if (j < 0) j = 0;                      // (never: the winner's split exists; an index stays an index)
                sh_first[k - 1] = j;
            }
            sh_first[r.k] = m;
            sh_used = r.k;
        }
    }
    __syncthreads();
    const int used = sh_used;
    const int32_t *cand = F.tours + (win >> 1) * F.stride;
    for (int k = tid; k < m; k += FLBLOCK) {
        if (a.tour) a.tour[s0 + k] = trip_at(cand, m, win & 1, k);
        if (a.share) {
            int s = 0;
            for (int x = 1; x < used; ++x) s += sh_first[x] <= k;
            a.share[s0 + k] = s;
        }
    }
    if (tid < n_var) {
        if (Ms) Ms[tid] = sh_Ms[tid];
        if (sums) sums[tid] = sh_sums[tid];
    }
    if (tid < ks) {
        const WV &W = sh[0];
        if (first) first[tid] = tid < used ? sh_first[tid] : -1;
        if (scost) {
            double c = nan;
            if (tid < used) {
                const int i = sh_first[tid], j = sh_first[tid + 1];
                c = fleet_cost(W.A[i], W.S[i], W.P[i], W.S[j - 1], F.Out[W.t[j - 1]], W.P[j], F.omega);
            }
            scost[tid] = c;
        }
    }
    if (tid != 0) return;
    if (a.makespan) a.makespan[f] = sh_M[ww];
    if (a.total) a.total[f] = sh_sum[ww];
    if (a.n_used) a.n_used[f] = used;
    if (a.winner) a.winner[f] = win;
    if (a.status) a.status[f] = FLEET_OK;
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------------------
// max_m: the most swaths of a field that has a block.  Up to FLSMALL the small instance runs: 41 KiB of LDS instead of 103, so that three
// workgroups share a CU and not one
int launch_fleet_solve(hipStream_t st, int64_t n, int64_t max_m, const FleetArgs &a)
{
    if (n <= 0) return 0;
    if (max_m <= FLSMALL) return launch(st, k_fleet_solve<FLSMALL>, (unsigned)n, FLBLOCK, a);
    return launch(st, k_fleet_solve<ROUTE_MAX_SWATHS>, (unsigned)n, FLBLOCK, a);
}

}  // namespace fcpp
