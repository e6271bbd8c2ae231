// fcpp_mission.hip -- gfx950 (MI355X) kernels of the mission paths: the path sets of a field joined into one drivable path, every closed
// loop entered at the station that makes the joints shortest in all (the rule: fcpp_missionfn.h over fcpp_connfn.h).  float64,
// -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_mission_paths gives on the host.
// Plain C++: no inline assembly, no atomics, every loop bounded.
//
// k_mission_stations, a wavefront per item: the candidates (local index c stride, c below mission_node_room) 64 at a time; a ballot of the
// lanes whose sample is a station gives every one its place (the count so far + the set bits below the lane), so the list is in sample
// order whatever the hardware does.  An open item has one node or none.  Lane 0 writes the count.
//
// THE SOLVE PASS, k_mission_layers, a workgroup of four wavefronts per field, walks the field's kept items in driving order.  The costs
// of the layer before and of the layer being made live in LDS (2 x 1024 doubles, 16 KiB).  A wavefront per target node b (b = wave,
// wave + 4, ...): the target's pose is prepared once, the lanes stride over the source nodes a (a = lane, lane + 64, ...), each one solve
// and the rule's one addition; the wavefront reduces (cost, a) lexicographically by xor-shuffles -- the order is total, so any tree
// gives the minimiser the host's loop gives -- and lane 0 writes the cost to LDS and the predecessor (4 B) to global memory.  The S x S
// lengths of a transition are never stored.  One barrier per layer.  The end (the exit's edge, or the last layer as it is) is one more
// target node, made by wavefront 0.  A field that is MISSION_EUNSUPPORTED leaves at once (uniform: nobody is left at a barrier).
// One wavefront per SIMD is all the Reeds-Shepp solve's registers allow (the compiler's figures: DESIGN.md, section 5), hence 256 threads.
//
// k_mission_finish, a lane per field: mission_finish -- the backtrack, then the chosen joints by the sequential form of the solve (once to
// learn whether all have a word, once to write), the records, the totals.
//
// COUNTS AND FILL: the samplers' scan (k_path_counts of fcpp_samplefn.h) over the SLOTS on mission_slot_count, a lane per field copies its
// first slot's offset; then a lane per output sample: its slot by bisection of the slot offsets, its field by bisection of the fields'
// first slots, mission_eval -- a joint's sample by Conn<MODE>::eval, an item's a copy of six columns.  Every element written once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_mission.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int MBLOCK = MISSION_BLOCK;
static constexpr int MWAVES = MBLOCK / 64;

__global__ __launch_bounds__(MBLOCK) void k_mission_stations(MissionIn in, MissionTemp T)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = ((int64_t)blockIdx.x * MBLOCK + threadIdx.x) >> 6;
    if (item >= in.n_items) return;                       // (uniform over the wavefront)
    const int64_t p = in.item_path[item], p0 = in.path_off[p], n_p = in.path_off[p + 1] - p0;
    const bool closed = in.item_closed[item] != 0;
    int64_t count = !closed && n_p > 0 ? 1 : 0;
    if (closed) {
        const int64_t room = mission_node_room(n_p, true, in.stride), base = T.st_base[item];
        for (int64_t c0 = 0; c0 < room; c0 += 64) {
            const int64_t c = c0 + lane;
            const bool is = c < room && mission_is_station(in, p0, n_p, c * in.stride);
            const unsigned long long m = __ballot(is);
            if (is) T.st_idx[base + count + (int64_t)__popcll(m & ((1ull << lane) - 1ull))] = p0 + c * in.stride;
            count += (int64_t)__popcll(m);
        }
    }
    if (lane == 0) T.n_nodes[item] = count;
}

// the least (cost, a) of a wavefront, in every lane
__device__ __forceinline__ void mission_wave_min(MissionPick &best)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(best.c, o);
        const int64_t oa = __shfl_xor(best.a, o);
        mission_pick_take(best, oc, oa);
    }
}

template <int MODE>
__global__ __launch_bounds__(MBLOCK) void k_mission_layers(MissionIn in, MissionTemp T)
{
    __shared__ double cost[2][MISSION_MAX_STATIONS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.x;
    if (f >= in.n_fields) return;                         // (uniform over the workgroup)
    int32_t skipped;
    if (mission_field_status(in, T.n_nodes, f, skipped) != MISSION_OK) return;      // (uniform: every layer below has at most 1024 nodes)
    int cur = 0;
    int64_t prev = -1, m = 0;
    if (in.ex) {
        if (tid == 0) cost[0][0] = 0.0;
        m = 1;
    }
    __syncthreads();
    for (int64_t i = in.item_off[f]; i < in.item_off[f + 1]; ++i) {
        const int64_t n = T.n_nodes[i], base = T.st_base[i];
        if (n <= 0) continue;                             // (uniform)
        if (m == 0) {
            for (int64_t b = tid; b < n; b += MBLOCK) { cost[cur ^ 1][b] = 0.0; T.pred[base + b] = 0; }
        } else {
            for (int64_t b = wave; b < n; b += MWAVES) {
                const int64_t gb = mission_node_sample(in, T, i, b, false);
                const typename Conn<MODE>::Pose to = Conn<MODE>::prep(in.x[gb], in.y[gb], in.h[gb], in.R);
                MissionPick best = mission_pick_none();
                for (int64_t a = lane; a < m; a += 64) {
                    double x0, y0, h0;
                    if (prev >= 0) {
                        const int64_t ga = mission_node_sample(in, T, prev, a, true);
                        x0 = in.x[ga]; y0 = in.y[ga]; h0 = in.h[ga];
                    } else { x0 = in.ex[f]; y0 = in.ey[f]; h0 = in.eh[f]; }
                    int word;
                    double seg[5], total;
                    Conn<MODE>::solve_prepped(Conn<MODE>::prep(x0, y0, h0, in.R), to, in.R, word, seg, total);
                    mission_pick_take(best, cost[cur][a] + total, a);
                }
                mission_wave_min(best);
                if (lane == 0) { cost[cur ^ 1][b] = best.c; T.pred[base + b] = (int32_t)best.a; }
            }
        }
        __syncthreads();                                  // (the layer is made; the one before is no longer read)
        cur ^= 1; prev = i; m = n;
    }
    if (wave != 0) return;
    if (prev < 0) {
        if (lane == 0) T.end_node[f] = -1;
        return;
    }
    MissionPick end = mission_pick_none();
    for (int64_t a = lane; a < m; a += 64) {
        double d = 0.0;
        if (in.xx) {
            const int64_t ga = mission_node_sample(in, T, prev, a, true);
            int word;
            double seg[5];
            Conn<MODE>::solve(in.x[ga], in.y[ga], in.h[ga], in.xx[f], in.xy[f], in.xh[f], in.R, word, seg, d);
        }
        mission_pick_take(end, cost[cur][a] + d, a);
    }
    mission_wave_min(end);
    if (lane == 0) T.end_node[f] = (int32_t)end.a;
}

template <int MODE>
__global__ __launch_bounds__(MBLOCK) void k_mission_finish(MissionIn in, MissionTemp T, MissionOut out)
{
    const int64_t f = (int64_t)blockIdx.x * MBLOCK + threadIdx.x;
    if (f >= in.n_fields) return;
    mission_finish<MODE>(in, T, f, out);
}

// the field of slot s
__device__ __forceinline__ int64_t mission_slot_field(const MissionIn &in, int64_t s)
{
    return last_at_or_before(in.n_fields, s, [&](int64_t f) { return mission_first_slot(in.item_off, f); });
}

// the samples of slot s as the scan takes them
template <int MODE> struct MissionCount {
    MissionIn in;
    MissionRec rec;
    double spacing;
    __device__ int64_t operator()(int64_t s, int64_t &bad) const { return mission_slot_count<MODE>(in, rec, spacing, mission_slot_field(in, s), s, bad); }
};

__global__ __launch_bounds__(MBLOCK) void k_mission_path_offsets(MissionIn in, const int64_t *__restrict__ slot_offsets, int64_t *__restrict__ path_offsets)
{
    const int64_t f = (int64_t)blockIdx.x * MBLOCK + threadIdx.x;
    if (f > in.n_fields) return;
    path_offsets[f] = slot_offsets[f < in.n_fields ? mission_first_slot(in.item_off, f) : 2 * in.n_items + in.n_fields];
}

template <int MODE>
__global__ __launch_bounds__(MBLOCK) void k_mission_fill(MissionIn in, MissionRec rec, double spacing, const int64_t *__restrict__ slot_offsets,
                                                         int64_t total_samples, double *__restrict__ xs, double *__restrict__ ys,
                                                         double *__restrict__ hs, double *__restrict__ kappas, int8_t *__restrict__ parts,
                                                         int8_t *__restrict__ gears, int32_t *__restrict__ slots, int64_t *__restrict__ srcs)
{
    const int64_t q = (int64_t)blockIdx.x * MBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t s, k, K, src;
    sample_path(slot_offsets, 2 * in.n_items + in.n_fields, q, s, k, K);
    const int64_t f = mission_slot_field(in, s);
    double x, y, h, kap;
    int part, gear;
    mission_eval<MODE>(in, rec, spacing, f, s, k, K, x, y, h, kap, part, gear, src);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (parts) parts[q] = (int8_t)part;
    if (gears) gears[q] = (int8_t)gear;
    if (slots) slots[q] = (int32_t)(s - mission_first_slot(in.item_off, f));
    if (srcs) srcs[q] = src;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_mission_stations(hipStream_t st, const MissionIn &in, const MissionTemp &T)
{
    if (in.n_items <= 0) return 0;
    return launch(st, k_mission_stations, blocks_for(in.n_items * 64, MBLOCK), MBLOCK, in, T);
}

int launch_mission_layers(hipStream_t st, int mode, const MissionIn &in, const MissionTemp &T)
{
    if (in.n_fields <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_mission_layers<M()>, (unsigned)in.n_fields, MBLOCK, in, T);
    });
}

int launch_mission_finish(hipStream_t st, int mode, const MissionIn &in, const MissionTemp &T, const MissionOut &out)
{
    if (in.n_fields <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_mission_finish<M()>, blocks_for(in.n_fields, MBLOCK), MBLOCK, in, T, out);
    });
}

int launch_mission_counts(hipStream_t st, int mode, const MissionIn &in, const MissionRec &rec, double spacing, int64_t *slot_offsets,
                          int64_t *path_offsets, int64_t *err)
{
    const int64_t n_slots = 2 * in.n_items + in.n_fields;
    const int e = by_mode(mode, [&](auto M) {
        return launch_path_counts<MBLOCK>(st, n_slots, MissionCount<M()>{ in, rec, spacing }, slot_offsets, err);
    });
    return e ? e : launch(st, k_mission_path_offsets, blocks_for(in.n_fields + 1, MBLOCK), MBLOCK, in, slot_offsets, path_offsets);
}

int launch_mission_fill(hipStream_t st, int mode, const MissionIn &in, const MissionRec &rec, double spacing, const int64_t *slot_offsets,
                        int64_t total_samples, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *slot,
                        int64_t *src)
{
    if (in.n_fields <= 0 || total_samples <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_mission_fill<M()>, blocks_for(total_samples, MBLOCK), MBLOCK, in, rec, spacing, slot_offsets, total_samples, x, y,
                      heading, kappa, part, gear, slot, src);
    });
}

}  // namespace fcpp
