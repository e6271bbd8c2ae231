// fcpp_ga.h -- device state and launchers of the GA evolution kernels (fcpp_ga.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/fcpp.h"

namespace fcpp {

struct GaState {
    double best_fit, best_dist;
    int32_t gwi;            // generations without improvement
    int32_t generations;    // generation + 1 of the last completed generation
    int32_t converged;
    int32_t _pad;
    // fitness of the last (elite_size-th) elite of the previous generation: elitism carries the elites over, so the elites of the
    // next population are among its last elite_size rows and the members strictly above this value (0 before the first selection: everybody)
    double elite_thr;
    // round 5b: a word of the host's pinned memory (or null) the bookkeeping role writes after every generation it completes --
    // (converged << 32) | generations, one 8-byte store -- so that fcpp_ga_evolve follows the run without a copy command or a drained
    // stream between the generations' launches (it used to drain the stream every 32 generations: a bubble of ~20 us each time)
    unsigned long long *mirror;
};

constexpr int GA_MAX_NODES = 2048;

int launch_ga_check_perm(hipStream_t st, int n, int pop, const int32_t *routes, int32_t *bad);   // *bad |= 1 unless every row is a permutation
int launch_ga_pairs(hipStream_t st, int n, int pop, const double *D, const int32_t *cur, const double *cur_fit, int32_t *nxt,
                    double *nxt_fit, double *nxt_dist, const fcpp_ga_config &cfg, int gen, const GaState *state);
// stats of the population `cur` (generation gen, -1 = the initial one), then the elites of `cur` into the tail of `nxt`
int launch_ga_stats_elite(hipStream_t st, int n, int pop, const int32_t *cur, const double *cur_fit, const double *cur_dist, int32_t *nxt,
                          double *nxt_fit, double *nxt_dist, const fcpp_ga_config &cfg, int gen, GaState *state, int32_t *best_route,
                          double *hist);
// what fcpp_ga_evolve launches per generation for (n, pop) on a device of n_cu compute units (fcpp_ctx::n_cu; 0 = not known: eight pairs
// per workgroup) -- a pure function, the one description the launchers and fcpp_debug_ga_launch_plan read.  one_launch (tours and
// populations whose LDS needs fit): k_ga_generation (groups pair workgroups beside its two roles; workgroup b takes
// base + (b < extra) pairs, per_wg the most of one; lds = its dynamic LDS bytes), else k_ga_pairs beside k_ga_stats_elite on two
// streams (groups = pop / 2 workgroups of one pair; lds = k_ga_pairs' dynamic LDS bytes)
struct GaLaunchPlan {
    bool one_launch;
    unsigned groups;
    int base, extra, per_wg;
    size_t lds;
};
GaLaunchPlan ga_launch_plan(int n, int pop, int n_cu);
// one generation in one launch (ga_launch_plan(n, pop, n_cu).one_launch): statistics / elites of `cur` (generation index gen - 1) beside
// its children (generation index gen)
int launch_ga_generation(hipStream_t st, int n_cu, int n, int pop, const double *D, const int32_t *cur, const double *cur_fit, const double *cur_dist,
                         int32_t *nxt, double *nxt_fit, double *nxt_dist, const fcpp_ga_config &cfg, int gen, GaState *state,
                         int32_t *best_route, double *hist);

}  // namespace fcpp
