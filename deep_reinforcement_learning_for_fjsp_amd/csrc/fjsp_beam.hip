// The selection step of a beam search over the batched environments (policy_search.beam_search): from the width_in x
// n_actions scored candidates of every source environment keep the width_out best, in a total order that no launch
// geometry can change.
//
// One wavefront per source environment.  Candidate c = parent * n_actions + action belongs to lane c % 64; its key is
// (an order-preserving integer image of the cost, c), compared lexicographically, so equal costs fall in the order of c =
// lower parent first, then lower action.  Every lane holds the smallest key among its own candidates; a rank is one
// wave-wide minimum of those 64 keys (four DPP steps inside a row, then lane ^ 16 and lane ^ 32 through ds_bpermute:
// a butterfly, every lane ends with the winner), after which the one lane that owned the winner looks through its
// candidates again for its next key above it.  At most 128 candidates per lane (64 x 128 / 64), read from global memory
// each time, eight loads in flight: the costs of an environment are a few KB to 64 KB and stay in the caches.
//
// The costs are only ever compared (as integers, after the usual sign fold; -0.0 is folded onto +0.0 first); the cost
// written for a rank is read back from the input, so the three outputs are a function of the input bits alone.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fjsp_amd.h"
#include "fjsp_common.h"
#include "fjsp_host.h"

namespace {

constexpr int kMaxWidth = 64, kMaxActions = 128;   // the limits of fjsp_beam_select (include/fjsp_amd.h)
constexpr int kWaves = 4;                          // source environments per workgroup
constexpr int kBatch = 8;                          // candidates a lane loads together
constexpr uint32_t kNone = 0xFFFFFFFFu;            // the index of "no candidate"; its key is above every candidate's

struct Key {
    uint64_t cost;      // cost_image of the candidate's cost
    uint32_t c;         // parent * n_actions + action
};

__device__ __forceinline__ bool key_less(const Key &a, const Key &b) { return a.cost < b.cost || (a.cost == b.cost && a.c < b.c); }

// u < v as doubles  <=>  cost_image(u) < cost_image(v), for everything but NaN; +-0.0 share one image.  Never 0 and never
// 2^64 - 1 for a candidate (those would be a negative and a positive NaN).
__device__ __forceinline__ uint64_t cost_image(double x) {
    uint64_t u = (uint64_t)__double_as_longlong(x);
    if ((u << 1) == 0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ Key key_min(const Key &a, const Key &b) { return key_less(b, a) ? b : a; }

#define FJSP_KEY_DPP(k, ctrl) \
    Key{((uint64_t)(uint32_t)DPP((int)(uint32_t)((k).cost >> 32), (ctrl), 0) << 32) | (uint32_t)DPP((int)(uint32_t)(k).cost, (ctrl), 0), \
        (uint32_t)DPP((int)(k).c, (ctrl), 0)}
__device__ __forceinline__ Key key_lane(const Key &k, int lane) {
    const int a = lane << 2;
    return Key{((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)(k.cost >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)k.cost),
               (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)k.c)};
}
// The smallest key of the wave, in every lane.  All 64 lanes must be active.
__device__ __forceinline__ Key wave_min(Key k, int lane) {
    k = key_min(k, FJSP_KEY_DPP(k, 0xB1));        // quad_perm [1,0,3,2]
    k = key_min(k, FJSP_KEY_DPP(k, 0x4E));        // quad_perm [2,3,0,1]
    k = key_min(k, FJSP_KEY_DPP(k, 0x141));       // row_half_mirror
    k = key_min(k, FJSP_KEY_DPP(k, 0x140));       // row_mirror
    k = key_min(k, key_lane(k, lane ^ 16));
    k = key_min(k, key_lane(k, lane ^ 32));
    return k;
}
#undef FJSP_KEY_DPP

struct BeamArgs {
    const double *cost;          // f64[width_in][n_src][n_actions]
    const unsigned char *done;   // u8[width_in][n_src], nullable
    int n_src, width_in, n_actions, width_out;
    int *parent, *action;        // i32[width_out][n_src]
    double *cost_out;            // f64[width_out][n_src]
    uint32_t div_m;              // ceil(2^20 / n_actions): see parent_of
};

// c / n_actions for a candidate index c < 64 * 128 = 2^13 without the ~30 instructions of an integer division (the
// look through a lane's candidates is bound by instruction issue): with m = ceil(2^20 / d) and d <= 2^7, (c * m) >> 20 is
// the exact quotient for every c < 2^13 (m d - 2^20 < d, so the error term c (m d - 2^20) / (2^20 d) stays below 1 / d);
// tests/test_beam_reference_host.py checks every (c, d) of the limits.  c << 12 fits 32 bits, so the product's high word is the quotient.
__device__ __forceinline__ int parent_of(const BeamArgs &g, int c) { return (int)__umulhi((uint32_t)c << 12, g.div_m); }

// The smallest key above `last` among this lane's candidates of source env i (c = lane, lane + 64, ...); kNone if none is.
__device__ Key next_key(const BeamArgs &g, int i, int lane, const Key &last) {
    Key best{~0ull, kNone};
    const int C = g.width_in * g.n_actions;
    // kBatch candidates at a time, their loads issued together before any of them is looked at (one memory round trip per
    // batch, not per candidate): nothing is conditional on a loaded value until the loads are out, so the entries a done
    // beam ignores are loaded and dropped, and a candidate index past the end loads the last entry and is dropped too.
    for (int c0 = lane; c0 < C; c0 += 64 * kBatch) {
        double x[kBatch];
        unsigned char d[kBatch];
        int a[kBatch];
        size_t env[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int c = min(c0 + 64 * u, C - 1), b = parent_of(g, c);
            a[u] = c - b * g.n_actions;
            env[u] = (size_t)b * (size_t)g.n_src + (size_t)i;
            x[u] = g.cost[env[u] * (size_t)g.n_actions + (size_t)a[u]];
            d[u] = 0;
        }
        if (g.done) {
#pragma unroll
            for (int u = 0; u < kBatch; ++u) d[u] = g.done[env[u]];
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int c = c0 + 64 * u;
            const Key k{cost_image(x[u]), (uint32_t)c};
            // a done beam's one candidate sits at action 0; NaN and +inf are not candidates
            const bool candidate = c < C && !(d[u] != 0 && a[u] != 0) && x[u] < __builtin_inf();
            if (candidate && key_less(last, k) && key_less(k, best)) best = k;
        }
    }
    return best;
}

__global__ __launch_bounds__(64 * kWaves) void beam_select_kernel(BeamArgs g) {
    const int lane = (int)threadIdx.x & 63;
    const int i = (int)blockIdx.x * kWaves + ((int)threadIdx.x >> 6);
    if (i >= g.n_src) return;                      // (a whole wave: the ones that stay are fully active)
    Key cur = next_key(g, i, lane, Key{0, 0});     // (no candidate has the image 0)
    uint32_t mine = kNone;                         // lane k: the candidate of rank k
    for (int k = 0; k < g.width_out; ++k) {
        const Key w = wave_min(cur, lane);
        if (w.c == kNone) break;                   // (the same in every lane)
        if (lane == k) mine = w.c;
        if ((int)(w.c & 63u) == lane) cur = next_key(g, i, lane, w);
    }
    if (lane < g.width_out) {
        int parent = -1, action = -1;
        double x = __builtin_inf();
        if (mine != kNone) {
            parent = parent_of(g, (int)mine);
            action = (int)mine - parent * g.n_actions;
            const size_t env = (size_t)parent * (size_t)g.n_src + (size_t)i;
            x = g.cost[env * (size_t)g.n_actions + (size_t)action];
            if (g.done && g.done[env]) action = -1;
        }
        const size_t o = (size_t)lane * (size_t)g.n_src + (size_t)i;
        g.parent[o] = parent;
        g.action[o] = action;
        g.cost_out[o] = x;
    }
}

}  // namespace

extern "C" int fjsp_beam_select(const double *d_cost, const uint8_t *d_done, int32_t n_src, int32_t width_in, int32_t n_actions,
                                int32_t width_out, int32_t *d_parent, int32_t *d_action, double *d_cost_out, void *stream) {
    if (!d_cost || !d_parent || !d_action || !d_cost_out) { fjsp::set_error("fjsp_beam_select: null cost or output pointer"); return FJSP_E_ARG; }
    if (n_src < 1 || width_in < 1 || width_in > kMaxWidth || width_out < 1 || width_out > kMaxWidth || n_actions < 1 || n_actions > kMaxActions) {
        fjsp::set_error("fjsp_beam_select: needs n_src >= 1, widths in 1..64 and n_actions in 1..128"); return FJSP_E_ARG;
    }
    BeamArgs g{d_cost, d_done, (int)n_src, (int)width_in, (int)n_actions, (int)width_out, d_parent, d_action, d_cost_out,
               (uint32_t)(((1 << 20) + n_actions - 1) / n_actions)};
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)(((int64_t)n_src + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, (hipStream_t)stream, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fjsp::set_error(std::string("fjsp_beam_select: ") + hipGetErrorString(e)); return FJSP_E_HIP; }
    return FJSP_OK;
}
