// The non-dominated set of the candidates of every source environment (pareto.select; the reference's
// filter_pareto_front, utilities/Utility_Class.py:132-146), in an order that no launch geometry can change.
//
// A group of threads owns one source env: a 256-thread workgroup when there are more than 64 candidates (thread t owns
// candidates t, t + 256, ... : at most four), one wavefront otherwise (lane c owns candidate c; four envs per
// workgroup).  The group stages the env's objective vectors in LDS as f64[n_cand][n_obj rounded up to 1, 2 or 4]
// (32 KB at the limits), every entry of a candidate that is not one (valid == 0, or a NaN objective) set to NaN, so that
// it compares false against everything and needs no flag in the loops.  Then
//   pass 1  every thread walks all j with its own candidates in registers; the threads of a wave read the same LDS
//           address, a broadcast.  Candidate c leaves the front if some j is <= in every objective and either < in one
//           (dominated) or j < c (an equal vector with a lower index);
//   between the vectors of the candidates that left are overwritten with NaN, and the front is counted by ballot +
//           popcount (summed over the four waves through LDS);
//   pass 2  rank[c] = the number of front members lexicographically below c (objective 0 most significant).  Front
//           members are distinct vectors, so the ranks are the positions 0 .. count - 1 and no sort is needed;
//           index[rank] = c is written by exactly one thread, and the slots from count to cap by the group, -1.
//
// The input is candidate-major, so a group's loads of its env are strided by n_src * n_obj * 8 bytes and not coalesced.
// That is accepted, not staged through a transposed copy: the neighbouring envs that share the cache lines are loaded
// by neighbouring workgroups at about the same time, every element is read once (n_obj * 8 bytes against the 2 * n_cand
// * n_obj compares made with it), and a transposed copy would be a second launch that moves the same bytes twice.
//
// The values are only ever compared (IEEE: -0.0 == 0.0, the infinities are ordinary values); there are no atomics; the
// three outputs are a function of the input bits.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fjsp_amd.h"
#include "fjsp_common.h"
#include "fjsp_host.h"

namespace {

constexpr int kMaxCand = 1024, kMaxObj = 4;        // the limits of fjsp_pareto_select (include/fjsp_amd.h)
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kWaveCand = 64;                      // up to this many candidates a wavefront owns the env

struct ParetoArgs {
    const double *obj;           // f64[n_cand][n_src][n_obj]
    const unsigned char *valid;  // u8[n_cand][n_src], nullable
    int n_src, n_cand, cap;
    int *index;                  // i32[n_src][cap]
    int *count;                  // i32[n_src]
    unsigned char *mask;         // u8[n_cand][n_src], nullable
};

constexpr int padded(int D) { return D == 3 ? 4 : D; }

// The front of source env i by a group of T threads (tid = 0 .. T - 1; T = 64: one wavefront; T = 256: the workgroup).
// v: the group's LDS, f64[n_cand][padded(D)]; red: LDS int[kWaves] of the workgroup (T = 256 only).  Every thread of
// the WORKGROUP calls this the same number of times (the barriers are the workgroup's); a group with active == false
// loads and stores nothing.
template <int D, int T>
__device__ __forceinline__ void select_env(const ParetoArgs &g, int i, bool active, int tid, double *v, int *red) {
    constexpr int DP = padded(D), kOwn = T == 64 ? 1 : kMaxCand / T;
    const int C = g.n_cand;
    const double nan = __builtin_nan("");
    double x[kOwn][D];
    bool front[kOwn];
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
        const int c = tid + T * u;
        bool cand = active && c < C;
        if (cand) {
            const size_t env = (size_t)c * (size_t)g.n_src + (size_t)i;
#pragma unroll
            for (int d = 0; d < D; ++d) x[u][d] = g.obj[env * D + d];
            if (g.valid) cand = g.valid[env] != 0;
#pragma unroll
            for (int d = 0; d < D; ++d) cand = cand && x[u][d] == x[u][d];
        }
        if (!cand) {
#pragma unroll
            for (int d = 0; d < D; ++d) x[u][d] = nan;
        }
        if (c < C) {
#pragma unroll
            for (int d = 0; d < D; ++d) v[c * DP + d] = x[u][d];
        }
        front[u] = cand;
    }
    __syncthreads();

    // pass 1: dominated, or equal to a candidate of lower index (le without lt is equality: no NaN gets this far)
    for (int j = 0; j < C; ++j) {
        double y[D];
#pragma unroll
        for (int d = 0; d < D; ++d) y[d] = v[j * DP + d];
#pragma unroll
        for (int u = 0; u < kOwn; ++u) {
            if (T * u < C) {
                bool le = true, lt = false;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    le = le && y[d] <= x[u][d];
                    lt = lt || y[d] < x[u][d];
                }
                if (le && (lt || j < tid + T * u)) front[u] = false;
            }
        }
    }
    __syncthreads();

    int n = 0;                   // the wave's front members
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
        const int c = tid + T * u;
        if (c < C && !front[u]) {
#pragma unroll
            for (int d = 0; d < D; ++d) v[c * DP + d] = nan;
        }
        n += __popcll(__ballot(front[u]));
    }
    if (T != 64 && (tid & 63) == 0) red[tid >> 6] = n;
    __syncthreads();
    if (T != 64) {
        n = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) n += red[w];
    }

    // pass 2: the position of a front member = the front members lexicographically below it
    int rank[kOwn];
#pragma unroll
    for (int u = 0; u < kOwn; ++u) rank[u] = 0;
    for (int j = 0; j < C; ++j) {
        double y[D];
#pragma unroll
        for (int d = 0; d < D; ++d) y[d] = v[j * DP + d];
#pragma unroll
        for (int u = 0; u < kOwn; ++u) {
            if (T * u < C) {
                bool below = false;
#pragma unroll
                for (int d = D - 1; d >= 0; --d) below = y[d] < x[u][d] || (y[d] == x[u][d] && below);
                rank[u] += below ? 1 : 0;
            }
        }
    }

    if (!active) return;
    int *index = g.index + (size_t)i * (size_t)g.cap;
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
        const int c = tid + T * u;
        if (c < C) {
            if (front[u] && rank[u] < g.cap) index[rank[u]] = c;
            if (g.mask) g.mask[(size_t)c * (size_t)g.n_src + (size_t)i] = front[u] ? 1 : 0;
        }
    }
    for (int k = n + tid; k < g.cap; k += T) index[k] = -1;
    if (tid == 0) g.count[i] = n;
}

extern __shared__ __attribute__((aligned(16))) double pareto_lds[];

// more than kWaveCand candidates: one workgroup per source env.  LDS: f64[n_cand][padded(D)], then int[kWaves]
template <int D>
__global__ __launch_bounds__(kThreads) void pareto_select_block_kernel(ParetoArgs g) {
    int *red = reinterpret_cast<int *>(pareto_lds + (size_t)g.n_cand * padded(D));
    select_env<D, kThreads>(g, (int)blockIdx.x, true, (int)threadIdx.x, pareto_lds, red);
}

// at most kWaveCand candidates: one wavefront per source env.  LDS: kWaves x f64[n_cand][padded(D)]
template <int D>
__global__ __launch_bounds__(kThreads) void pareto_select_wave_kernel(ParetoArgs g) {
    const int wave = (int)threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kWaves + wave;
    select_env<D, 64>(g, (int)(i < g.n_src ? i : 0), i < g.n_src, (int)threadIdx.x & 63, pareto_lds + (size_t)wave * g.n_cand * padded(D),
                      nullptr);
}

template <int D>
void launch(const ParetoArgs &g, hipStream_t stream) {
    if (g.n_cand <= kWaveCand) {
        const size_t lds = (size_t)kWaves * g.n_cand * padded(D) * sizeof(double);
        hipLaunchKernelGGL(pareto_select_wave_kernel<D>, dim3((unsigned)(((int64_t)g.n_src + kWaves - 1) / kWaves)), dim3(kThreads), lds, stream, g);
    } else {
        const size_t lds = (size_t)g.n_cand * padded(D) * sizeof(double) + 16;
        hipLaunchKernelGGL(pareto_select_block_kernel<D>, dim3((unsigned)g.n_src), dim3(kThreads), lds, stream, g);
    }
}

}  // namespace

extern "C" int fjsp_pareto_select(const double *d_obj, const uint8_t *d_valid, int32_t n_src, int32_t n_cand, int32_t n_obj,
                                  int32_t cap, int32_t *d_index, int32_t *d_count, uint8_t *d_mask, void *stream) {
    if (!d_obj || !d_index || !d_count) { fjsp::set_error("fjsp_pareto_select: null objective or output pointer"); return FJSP_E_ARG; }
    if (n_src < 1 || n_cand < 1 || n_cand > kMaxCand || n_obj < 1 || n_obj > kMaxObj || cap < 1 || cap > n_cand) {
        fjsp::set_error("fjsp_pareto_select: needs n_src >= 1, n_cand in 1..1024, n_obj in 1..4 and cap in 1..n_cand"); return FJSP_E_ARG;
    }
    const ParetoArgs g{d_obj, d_valid, (int)n_src, (int)n_cand, (int)cap, d_index, d_count, d_mask};
    switch (n_obj) {
        case 1: launch<1>(g, (hipStream_t)stream); break;
        case 2: launch<2>(g, (hipStream_t)stream); break;
        case 3: launch<3>(g, (hipStream_t)stream); break;
        default: launch<4>(g, (hipStream_t)stream); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fjsp::set_error(std::string("fjsp_pareto_select: ") + hipGetErrorString(e)); return FJSP_E_HIP; }
    return FJSP_OK;
}
