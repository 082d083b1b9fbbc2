// The fluid-model LP of an order arrival (environments/class_FJSSP.py:246-280, class_MODFJSP.py:240-280) ON THE DEVICE:
// one workgroup per parked environment, the simplex tableau in LDS.
//
// At an order arrival the blocking service of fjsp_env.hip used to bring the LP inputs to the host, solve there
// (csrc/fjsp_lp.cpp) and upload x -- one stream synchronisation and 0.05-0.8 ms of host time per vector step.  The solver
// here is fjsp_lp_simplex.h, the host's pivot for pivot, so the environment's trajectory does not depend on where its LPs
// were solved.  What is particular to this kernel:
//   * the tableau of the reference's industrial instances (K = 31, M = 20: 79 rows x 137 columns) is 87 KB: it lives in
//     LDS (160 KB per CU); a batch whose largest possible tableau does not fit keeps the host service (fjsp_env.hip
//     decides at create time: lp_device_lds_bytes, fjsp_lp_limits.h);
//   * the objective row and the scaled pivot row live in registers, lane l holding the columns l, l + 64, ...: the pivot
//     loop is compiled for 2, 3, 4, 6 and 8 chunks of 64 columns (nc <= 512);
//   * a lane holds two row groups, rows l and 64 + l.  No batch the create rule admits has more than 128 rows -- nr >= 129
//     needs K >= 49 operation types at M <= 32, hence nc >= K + nr + 2 >= 180 columns and 129 * 180 * 8 B of tableau, beyond
//     the 156 KB of choose_lp_service; tests/test_lp_reference.py sweeps every admissible shape -- and an LP beyond the
//     limits ends with an error code, not a write;
//   * the launch needs no host round trip: the workgroups read the number of parked environments from the pending list
//     the step kernel filled (DevBatch::pending_count) and stride over the slots.
#include <hip/hip_runtime.h>

#include "../../include/fjsp_amd.h"
#include "fjsp_common.h"
#include "fjsp_device.h"
#include "fjsp_launch.h"
#include "fjsp_lp_limits.h"
#include "fjsp_lp_simplex.h"

#pragma clang fp contract(off)

namespace fjsp {

namespace {
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = 2;          // row groups of 64 a lane holds: nr <= 128
constexpr int kZT = 8;              // registers of a lane for the objective row / the pivot row: columns l, l + 64, ...
static_assert(kLpLdsColumns == 64 * kZT, "the widest tableau the create rule admits fills the row registers");

extern __shared__ __attribute__((aligned(16))) unsigned char lp_lds[];

// The pivots of one LP (every thread of the workgroup; returns the failure code, 0 = optimal).
//
// Every wave holds the objective row in registers; rows of the elimination are dealt to the waves, and the scaled pivot
// row travels in registers.  The waves of a workgroup share four SIMDs: a single wave issues a dependent instruction
// every ~10 cycles, the others fill the gaps.
template <int NT>
__device__ __forceinline__ int lp_pivots(double *const T, int *const basis, const int nr, const int nc, const int nv, const int tcol,
                                         const int w, const int l, const int tid, long &n_piv) {
    const int rhs = nc - 1;
    constexpr int RB = NT <= 4 ? 4 : 2;                                // rows of the elimination a wave has in flight
    double zr[NT];                                                     // the objective row, in every wave: maximise t
#pragma unroll
    for (int t = 0; t < NT; ++t) zr[t] = (l + 64 * t == tcol) ? -1.0 : 0.0;
    const long max_iter = 200L * (nr + nc) + 1000;
    for (long it = 0;; ++it) {
        if (it > max_iter) return 2;                                   // "iteration limit"
        const int s = lp_entering_column([&](int t) { return zr[t]; }, NT, nc, l);
        if (s < 0) return 0;                                           // optimal
        double a[kGroups];                                             // column s of rows l and 64 + l: the elimination's factors
        const LpLeaving lv = lp_leaving_row<kGroups>(T, nr, nc, nv, s, l, a);
        const int r = lv.r;
        if (r < 0) return 3;                                           // "unbounded"
        // ---- pivot: the scaled row r into registers (column s becomes exactly 1), the objective's factor from its lane
        const double *rowr = &T[(size_t)r * nc];
        double rr[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = l + 64 * t;
            rr[t] = j < nc ? (j == s ? 1.0 : rowr[j] / lv.ar) : 0.0;
        }
        double fz = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if ((s >> 6) == t) fz = lane_f64(zr[t], s & 63);
        __syncthreads();                      // every wave has read column s, the right-hand sides and row r
        // ---- elimination: a wave takes RB of its rows at a time -- all their loads in flight together; lane l has the
        // columns l, l + 64, ...  (x - f * 1 of column s is exactly 0, as the host writes it; the clean-up of a tiny
        // negative right-hand side touches one lane of one chunk.)
        const int rhs_t = rhs >> 6, rhs_l = rhs & 63;
        unsigned long long my[kGroups];
        lp_deal_rows<kGroups, kWaves>(a, nr, r, w, l, my);
        for (;;) {
            int row[RB];
            double f[RB], x[RB][NT];
#pragma unroll
            for (int u = 0; u < RB; ++u) lp_next_row(my, a, row[u], f[u]);
            if (row[0] < 0) break;
#pragma unroll
            for (int u = 0; u < RB; ++u)
                if (row[u] >= 0) {
                    const double *rowi = &T[(size_t)row[u] * nc];
#pragma unroll
                    for (int t = 0; t < NT; ++t) { const int j = l + 64 * t; x[u][t] = j < nc ? rowi[j] : 0.0; }
                }
#pragma unroll
            for (int u = 0; u < RB; ++u)
                if (row[u] >= 0) {
                    double *rowi = &T[(size_t)row[u] * nc];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int j = l + 64 * t;
                        double v = x[u][t] - f[u] * rr[t];
                        if (t == rhs_t && l == rhs_l && v < 0.0 && v > -1e-12) v = 0.0;
                        if (j < nc) rowi[j] = v;
                    }
                }
        }
        if (w == kWaves - 1) {                // the scaled pivot row (nobody reads row r between the two barriers)
            double *rowi = &T[(size_t)r * nc];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int j = l + 64 * t;
                if (j < nc) rowi[j] = rr[t];
            }
        }
        if (fz != 0.0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) zr[t] = zr[t] - fz * rr[t];
        }
        if (tid == 0) basis[r] = s;
        ++n_piv;
        __syncthreads();
    }
}
}  // namespace

// One workgroup per parked environment (slot): solves its LP, writes x to lp_x[slot] (f64[KP][MP], zeros elsewhere).
// err[0] becomes nonzero when an LP fails (infeasible input, unbounded, iteration limit, beyond the kernel's limits): the
// host reports it at the next synchronising call.
__global__ __launch_bounds__(kThreads) void lp_device_kernel(DevBatch b, const uint32_t *count_dev, int count_host, const uint32_t *ids,
                                                             const uint16_t *lp_in, double *lp_x, uint32_t *err, unsigned long long *solved,
                                                             uint32_t lds_bytes) {
    const int tid = (int)threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
    const uint32_t count = count_dev ? min(*count_dev, (uint32_t)b.N) : (uint32_t)count_host;
    if (blockIdx.x == 0 && tid == 0 && solved) atomicAdd(solved, (unsigned long long)count);
    for (uint32_t slot = blockIdx.x; slot < count; slot += gridDim.x) {
        const int env = (int)ids[slot];
        const int inst = b.n_inst == b.N ? env : env % b.n_inst;
        const unsigned char *ir = b.inst + (size_t)inst * b.L.i_stride;
        const InstHeader h = *reinterpret_cast<const InstHeader *>(ir);
        const int K = h.K, M = h.M, MP = b.MP, KP = b.KP;
        // the small data at the tail of the allocation: its place does not depend on the tableau's size
        unsigned char *tail = lp_lds + lds_bytes;
        LpView v;
        v.p = reinterpret_cast<uint16_t *>(tail - (size_t)K * MP * 2 - (size_t)K * 8 - 16);
        v.Q = v.p + (size_t)K * MP; v.now = v.Q + K;
        v.kB = reinterpret_cast<uint32_t *>(tail - (size_t)K * 4 - 8);
        v.col_of = v.p - ((size_t)K * M + K + 8);
        v.prec = v.col_of + (size_t)K * M;
        __shared__ LpDims dims;
        __shared__ int s_fail;
        __syncthreads();                                                                   // (the previous slot's readers are done)
        lp_stage_inputs<kThreads>(v, K, MP, KP, reinterpret_cast<const uint16_t *>(ir + b.L.i_p), lp_in + (size_t)slot * 2 * KP,
                                  reinterpret_cast<const uint32_t *>(ir + b.L.i_kB), tid);
        if (tid == 0) s_fail = 0;
        __syncthreads();
        if (w == 0) {
            const LpDims d = lp_dimensions(v, K, M, MP, l);
            if (l == 0) {
                dims = d;
                if (d.nr > 64 * kGroups || d.nc > kLpLdsColumns) s_fail = 5;               // the limits of this kernel: nothing below writes beyond them
            }
        }
        __syncthreads();
        const int nr = dims.nr, nc = dims.nc;
        double *T = reinterpret_cast<double *>(lp_lds);
        v.val = T + (size_t)nr * nc;
        v.basis = reinterpret_cast<int *>(v.val + nc + 2 * (size_t)nr);
        long n_piv = 0;
        int fail = s_fail;
        if (!fail) {
            lp_fill<kThreads>(v, dims, T, MP, tid, &s_fail);
            fail = s_fail;
        }
        if (!fail) {                          // (the rows a lane handles stay in registers: one loop per chunk count)
            const int nt = (nc + 63) >> 6, nv = dims.nv, tcol = dims.nx;
            fail = nt <= 2 ? lp_pivots<2>(T, v.basis, nr, nc, nv, tcol, w, l, tid, n_piv) : nt <= 3 ? lp_pivots<3>(T, v.basis, nr, nc, nv, tcol, w, l, tid, n_piv)
                 : nt <= 4 ? lp_pivots<4>(T, v.basis, nr, nc, nv, tcol, w, l, tid, n_piv) : nt <= 6 ? lp_pivots<6>(T, v.basis, nr, nc, nv, tcol, w, l, tid, n_piv)
                                                                                                  : lp_pivots<8>(T, v.basis, nr, nc, nv, tcol, w, l, tid, n_piv);
        }
        __syncthreads();
        lp_extract_x<kThreads>(v, dims, T, lp_x + (size_t)slot * KP * MP, KP, MP, fail, tid, &s_fail);
        if (tid == 0 && (fail || s_fail)) atomicOr(err, (uint32_t)(fail ? fail : s_fail));
        if (tid == 0 && solved) atomicAdd(solved + 1, (unsigned long long)n_piv);
    }
}

int launch_lp_device(const DevBatch &b, const uint32_t *count_dev, int count_host, const uint32_t *ids, const uint16_t *lp_in, double *lp_x,
                     uint32_t *err, unsigned long long *solved, size_t lds, hipStream_t st) {
    const int grid = count_dev ? (b.N < 256 ? b.N : 256) : count_host;
    if (grid <= 0) return 0;
    return launch(lp_device_kernel, dim3((unsigned)grid), dim3(kThreads), lds, st, b, count_dev, count_host, ids, lp_in, lp_x, err, solved, (uint32_t)lds);
}

}  // namespace fjsp
