// Wave-level helpers of the device simplex kernels (fjsp_lp_device.hip: tableau in LDS; fjsp_lp_global.hip: tableau in
// global memory): one f64 of a given lane, DPP moves of an f64, the wave's minimum in every lane.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fjsp {
namespace {
__device__ inline double lane_f64(double v, int lane) {     // v of a wave-uniform lane
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <int CTRL>
__device__ inline double dpp_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)u, (int)(unsigned)u, CTRL, 0xF, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(u >> 32), (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ inline double wave_fmin_f64(double x) {                 // the smallest x of the wave (no NaNs among them), in every lane
    x = __builtin_fmin(x, dpp_f64<0xB1>(x));
    x = __builtin_fmin(x, dpp_f64<0x4E>(x));
    x = __builtin_fmin(x, dpp_f64<0x141>(x));
    x = __builtin_fmin(x, dpp_f64<0x140>(x));
    return __builtin_fmin(__builtin_fmin(lane_f64(x, 0), lane_f64(x, 16)), __builtin_fmin(lane_f64(x, 32), lane_f64(x, 48)));
}

__device__ inline uint32_t wave_min_u32(uint32_t x) {              // the smallest x of the wave, in every lane
#define LP_UMIN(CTRL) { const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xF, 0xF, false); x = o < x ? o : x; }
    LP_UMIN(0xB1) LP_UMIN(0x4E) LP_UMIN(0x141) LP_UMIN(0x140)
#undef LP_UMIN
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}
}  // namespace
}  // namespace fjsp
