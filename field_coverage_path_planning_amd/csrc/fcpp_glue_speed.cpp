// fcpp_glue_speed.cpp -- C-ABI glue of the path speeds: the speed profile of sampled paths from their kappa, part and gear (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_parallel.h"
#include "fcpp_speed.h"

using namespace fcpp;

namespace {
// what the entry and the host twin check alike before any offsets are read
int speed_args(const fcpp_speed_params *params, int64_t n_paths, const void *offsets, int64_t total, bool sample_arrays, const int32_t *status,
               SpeedRule &rule)
{
    if (!params || !offsets || (total > 0 && !sample_arrays) || (n_paths > 0 && !status)) return fail(FCPP_EINVAL, "bad arguments");
    if (!speed_rule(*params, rule))
        return fail(FCPP_EINVAL, "speeds, accelerations, safety_factor and kappa_eps must be positive and finite (turn_kmh and the nominals may be "
                                 "+inf, a nominal may be 0); flags: FCPP_SPEED_*");
    return FCPP_OK;
}
}  // namespace

extern "C" {

int fcpp_path_speeds(fcpp_ctx *c, const fcpp_speed_params *params, int64_t n_paths, const int64_t *offsets, int64_t total, const double *x,
                     const double *y, const double *kappa, const int8_t *part, const int8_t *gear, double *v_out, double *cap_out,
                     int32_t *status_out, const int64_t *offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    SpeedRule rule;
    int rc = speed_args(params, n_paths, offsets ? (const void *)offsets : (const void *)offsets_host, total, x && y && kappa && part && gear,
                        status_out, rule);
    if (rc) return rc;
    DevTiling *dt = nullptr;
    rc = path_tiling(c, n_paths, offsets, offsets_host, total, &dt);
    if (rc) return rc;
    if (n_paths <= 0) return FCPP_OK;
    hipStream_t st = c->stream;
    const SpeedIn in = { x, y, kappa, part, gear };
    HIPCHK(hipMemsetAsync(status_out, 0, (size_t)n_paths * sizeof(int32_t), st));
    LAUNCHCHK(launch_speed_tiles(st, dt->n_tiles, dt->tiles.p, dt->paths.p, rule, in, dt->agg_f.p, dt->agg_b.p, status_out));
    LAUNCHCHK(launch_scan_spine(st, dt->n_tiles, dt->agg_f.p, dt->agg_b.p, dt->carry_f.p, dt->carry_b.p, dt->spine.p));
    if (v_out || cap_out)
        LAUNCHCHK(launch_speed_apply(st, dt->n_tiles, dt->tiles.p, dt->paths.p, rule, in, dt->carry_f.p, dt->carry_b.p, status_out, v_out, cap_out));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp_debug_path_speeds(const fcpp_speed_params *params, int64_t n_paths, const int64_t *offsets, int64_t total, const double *x,
                           const double *y, const double *kappa, const int8_t *part, const int8_t *gear, double *v_out, double *cap_out,
                           int32_t *status_out)
{
    SpeedRule rule;
    int rc = speed_args(params, n_paths, offsets, total, x && y && kappa && part && gear, status_out, rule);
    if (rc) return rc;
    if (n_paths < 0 || total < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    std::vector<int64_t> off;
    rc = host_offsets(nullptr, n_paths, offsets, nullptr, total, "offsets", off);
    if (rc) return rc;
    std::vector<double> u;
    try { u.assign((size_t)total, 0.0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    WorkerPool::parallel_for(n_paths, [&](int64_t p) {
        const int64_t a = off[(size_t)p], n = off[(size_t)p + 1] - a;
        status_out[p] = speed_path_host(rule, n, x + a, y + a, kappa + a, part + a, gear + a, u.data() + a, v_out ? v_out + a : nullptr,
                                        cap_out ? cap_out + a : nullptr);
    });
    return FCPP_OK;
}

}  // extern "C"
