// fcpp_launch.h -- the launch layer between the launchers at the bottom of every .hip file and their kernels: enqueue and read the
// error once (launch), the same with the dispatch's profiling events (launch_stage), the grid of n items (blocks_for) and the choice
// of a kernel's <0> / <1> instance (by_mode).  No .hip file writes a launch macro or reads hipGetLastError() itself.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

#include "fcpp_device.h"

namespace fcpp {

// a workgroup: its lanes and, where a kernel sizes its LDS at launch, the dynamic LDS bytes
struct Block {
    unsigned lanes;
    size_t lds;
    constexpr Block(int lanes_, size_t lds_ = 0) : lanes((unsigned)lanes_), lds(lds_) {}
};

// kernel<<<grid, block, block.lds, st>>>(args...), each argument converted to the kernel's own parameter type; 0 or the hipError_t value
template <class... P, class... A>
inline int launch(hipStream_t st, void (*kernel)(P...), dim3 grid, Block block, A &&...args)
{
    hipLaunchKernelGGL(kernel, grid, dim3(block.lanes), block.lds, st, static_cast<P>(args)...);
    return (int)hipGetLastError();
}

// launch() for a stage of the planner pipelines: when profiling is armed (fcpp_device.h: g_launch_prof) the dispatch carries the start
// and stop events, and the launcher disarms it
template <class... P, class... A>
inline int launch_stage(hipStream_t st, void (*kernel)(P...), dim3 grid, Block block, A &&...args)
{
    if (!g_launch_prof.start) return launch(st, kernel, grid, block, args...);
    hipExtLaunchKernelGGL(kernel, grid, dim3(block.lanes), block.lds, st, g_launch_prof.start, g_launch_prof.stop, 0, static_cast<P>(args)...);
    g_launch_prof = LaunchProf();
    return (int)hipGetLastError();
}

// workgroups of `per` items that hold n items
constexpr unsigned blocks_for(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }
static_assert(blocks_for(0, 256) == 0 && blocks_for(1, 256) == 1 && blocks_for(256, 256) == 1 && blocks_for(257, 256) == 2, "ceiling");

// f(<0>) for mode 0, f(<1>) otherwise: a launcher of a two-instance kernel names the kernel<M()> and its arguments once
template <class F>
inline int by_mode(int mode, F f)
{
    return mode == 0 ? f(std::integral_constant<int, 0>{}) : f(std::integral_constant<int, 1>{});
}

}  // namespace fcpp
