// Host side of a kernel launch, shared by the environment kernels' launchers (fjsp_kernels.hip, fjsp_group.hip,
// fjsp_lp_device.hip).  Host only: nothing here reaches device code.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fjsp_device.h"

namespace fjsp {
template <int I>
using int_c = std::integral_constant<int, I>;

// grids: four environments (waves of 64 lanes, or 16-lane rows of one wave) per 256 threads; 16 environments per
// 1024-thread workgroup of the policy kernels, or W of them to one of 64 W threads (policy_geometry); the row family's
// waves, wpb of them to a workgroup
inline unsigned waves_for(int N) { return (unsigned)((N + 3) / 4); }
inline dim3 grid_for(int N) { return dim3(waves_for(N)); }
inline dim3 grid_for16(int n) { return dim3((unsigned)((n + 15) / 16)); }
inline dim3 grid_for_envs(int n, int W) { return dim3((unsigned)((n + W - 1) / W)); }
inline dim3 grid_for_rows(int N, unsigned wpb) { return dim3((waves_for(N) + wpb - 1) / wpb); }

// Launch `kernel`; 0 = launched.  Dynamic LDS beyond the 64 KB default must be allowed per kernel (up to the 160 KB of a
// gfx950 CU; create refuses batches beyond that, step_lds_bytes()): on every launch, per device, result ignored -- a
// refusal shows as the launch's error.
template <class K, class... Args>
inline int launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// A kernel and its recording build (fjsp_env_record_schedule): the same launch, `rec` appended while recording is on.
template <class K, class KRec, class... Args>
inline int launch_rec(K plain, KRec recording, const SchedRec &rec, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    return rec.rec ? launch(recording, grid, block, lds, st, args..., rec) : launch(plain, grid, block, lds, st, args...);
}
}  // namespace fjsp
