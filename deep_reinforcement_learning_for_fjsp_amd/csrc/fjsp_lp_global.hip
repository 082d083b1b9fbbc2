// The fluid-model LP on the device with its simplex tableau in GLOBAL memory: the LPs whose tableau does not fit the LDS
// of a CU (fjsp_lp_device.hip keeps tableaus of up to 156 KB and 512 columns there).  The reference's own training
// instances are of that kind: data/HMPSAC 71-113 rows x 328-538 columns (213-474 KB), data/MPPPO up to 133 x 673 (699 KB),
// the MPPPO generator's worst case 128 x 1330 (1.36 MB).
//
// The solver is fjsp_lp_simplex.h, as in lp_device_kernel: x is BIT-IDENTICAL to fjsp_lp.cpp's (tests/test_gpu_lp_global.py).
// What is particular to this kernel is where things live:
//   * the tableau f64[nr][nc] in a slot of a scratch pool in HBM, one slot per workgroup (the pool is allocated at create,
//     only by handles that chose this service); a workgroup strides over the LPs of a launch and re-uses its slot;
//   * LDS holds the small data only: the staged inputs p, Q, n_now, kB, the column map, the precedence list, basis, val, and
//     the objective row and the scaled pivot row (nc <= 1536: 12 KB each).  The two rows are in LDS, not in registers: at
//     24 chunks of 64 columns a lane would hold 2 x 24 f64 = 96 VGPRs for them alone, and every wave a copy; in LDS one
//     copy serves the workgroup, the pivot loop needs no chunk-count template, and a workgroup of 256 threads takes
//     22-73 KB of LDS, so two to seven of them share a CU (profiles/lp_global_resources.txt: no scratch memory);
//   * rows: up to 256, four row groups per lane (rows l, 64 + l, 128 + l, 192 + l).
// Synchronisation is __syncthreads() alone -- it orders the workgroup's global-memory writes and reads --: no cooperative
// launch, nothing between workgroups, no flags in memory.  A row chunk is read coalesced: lane l has columns l + 64 t.
// An LP outside the limits or the slot (never one an admitted handle can meet) ends with an error code, not a write.
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
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = 4;          // row groups of 64 a lane holds: nr <= 256
constexpr int kRB = 2;              // rows of the elimination a wave has in flight
constexpr int kCB = 4;              // ... and chunks of each
static_assert(kLpGlobalRows == 64 * kGroups, "the tallest tableau the create rule admits fills the row groups");

extern __shared__ __attribute__((aligned(16))) unsigned char lpg_lds[];
}  // namespace

// The LDS of a workgroup, from the largest sizes the handle can meet
LpGlobalLds lp_global_lds(int K, int M, int MP, int nr, int nc) {
    LpGlobalLds L{};
    uint32_t o = 0;
    auto take = [&](size_t bytes) { const uint32_t at = o; o += (uint32_t)((bytes + 15) & ~(size_t)15); return at; };
    L.zr = take((size_t)nc * 8); L.rr = take((size_t)nc * 8); L.val = take((size_t)nc * 8); L.basis = take((size_t)nr * 4);
    L.col_of = take((size_t)K * M * 2); L.prec = take((size_t)K * 2); L.p = take((size_t)K * MP * 2); L.Q = take((size_t)K * 4);
    L.kB = take((size_t)K * 4);
    L.total = o;
    L.cap_K = K; L.cap_M = M; L.cap_nr = nr; L.cap_nc = nc;
    return L;
}

namespace {
// The pivots of one LP (every thread of the workgroup; returns the failure code, 0 = optimal): the tableau T in global
// memory, the objective row zr and the scaled pivot row rr in LDS.
__device__ __forceinline__ int lpg_pivots(double *const T, double *const zr, double *const rr, int *const basis, const int nr, const int nc,
                                          const int nv, const int w, const int l, const int tid, long &n_piv) {
    const int rhs = nc - 1, nt = (nc + 63) >> 6;
    const long max_iter = 200L * (nr + nc) + 1000;
    for (long it = 0;; ++it) {
        if (it > max_iter) return 2;                                   // "iteration limit"
        const int s = lp_entering_column([&](int t) { return zr[l + 64 * t]; }, nt, nc, l);
        if (s < 0) return 0;                                           // optimal
        double a[kGroups];                                             // column s of rows l, 64 + l, 128 + l, 192 + l
        const LpLeaving lv = lp_leaving_row<kGroups>(T, nr, nc, nv, s, l, a);
        const int r = lv.r;
        if (r < 0) return 3;                                           // "unbounded"
        // ---- pivot: the scaled row r into LDS (column s becomes exactly 1), the objective's factor
        {
            const double *rowr = &T[(size_t)r * nc];
            for (int j = tid; j < nc; j += kThreads) rr[j] = j == s ? 1.0 : rowr[j] / lv.ar;
        }
        const double fz = zr[s];
        __syncthreads();                      // every wave has read column s, the right-hand sides, row r and zr[s]; rr is complete
        // ---- elimination: a wave takes kRB of its rows and kCB chunks of them at a time; lane l has the columns l,
        // l + 64, ...  (x - f * 1 of column s is exactly 0, as the host writes it.)
        unsigned long long my[kGroups];
        lp_deal_rows<kGroups, kWaves>(a, nr, r, w, l, my);
        for (;;) {
            int row[kRB];
            double f[kRB];
#pragma unroll
            for (int u = 0; u < kRB; ++u) lp_next_row(my, a, row[u], f[u]);
            if (row[0] < 0) break;
            for (int t0 = 0; t0 < nt; t0 += kCB) {
                double x[kRB][kCB];
#pragma unroll
                for (int u = 0; u < kRB; ++u)
                    if (row[u] >= 0) {
                        const double *rowi = &T[(size_t)row[u] * nc];
#pragma unroll
                        for (int t = 0; t < kCB; ++t) { const int j = l + 64 * (t0 + t); x[u][t] = j < nc ? rowi[j] : 0.0; }
                    }
#pragma unroll
                for (int u = 0; u < kRB; ++u)
                    if (row[u] >= 0) {
                        double *rowi = &T[(size_t)row[u] * nc];
#pragma unroll
                        for (int t = 0; t < kCB; ++t) {
                            const int j = l + 64 * (t0 + t);
                            if (j < nc) {
                                double val = x[u][t] - f[u] * rr[j];
                                if (j == rhs && val < 0.0 && val > -1e-12) val = 0.0;
                                rowi[j] = val;
                            }
                        }
                    }
            }
        }
        if (w == kWaves - 1) {                // the scaled pivot row (nobody reads row r between the two barriers)
            double *rowi = &T[(size_t)r * nc];
            for (int j = l; j < nc; j += 64) rowi[j] = rr[j];
        }
        if (fz != 0.0)
            for (int j = tid; j < nc; j += kThreads) zr[j] = zr[j] - fz * rr[j];
        if (tid == 0) basis[r] = s;
        ++n_piv;
        __syncthreads();
    }
}
}  // namespace

// One workgroup per scratch slot: solves the LPs blockIdx.x, blockIdx.x + gridDim.x, ... of the launch in its slot and
// writes x to lp_x[LP] (f64[KP][MP], zeros elsewhere); lp_device_kernel's arguments, counters and error word.
__global__ __launch_bounds__(kThreads) void lp_global_kernel(DevBatch b, const uint32_t *count_dev, int count_host, const uint32_t *ids,
                                                             const uint16_t *lp_in, double *lp_x, uint32_t *err, unsigned long long *solved,
                                                             double *pool, unsigned long long slot_f64, LpGlobalLds L) {
    const int tid = (int)threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
    const uint32_t count = count_dev ? min(*count_dev, (uint32_t)b.N) : (uint32_t)count_host;
    if (blockIdx.x == 0 && tid == 0 && solved) atomicAdd(solved, (unsigned long long)count);
    double *const T = pool + (size_t)blockIdx.x * slot_f64;
    double *const zr = reinterpret_cast<double *>(lpg_lds + L.zr), *const rr = reinterpret_cast<double *>(lpg_lds + L.rr);
    LpView v;
    v.val = reinterpret_cast<double *>(lpg_lds + L.val);
    v.basis = reinterpret_cast<int *>(lpg_lds + L.basis);
    v.col_of = reinterpret_cast<uint16_t *>(lpg_lds + L.col_of);
    v.prec = reinterpret_cast<uint16_t *>(lpg_lds + L.prec);
    v.p = reinterpret_cast<uint16_t *>(lpg_lds + L.p);
    v.Q = reinterpret_cast<uint16_t *>(lpg_lds + L.Q);
    v.kB = reinterpret_cast<uint32_t *>(lpg_lds + L.kB);
    __shared__ LpDims dims;
    __shared__ int s_fail;
    for (uint32_t slot = blockIdx.x; slot < count; slot += gridDim.x) {
        const int env = (int)ids[slot];
        const int inst = b.n_inst == b.N ? env : env % b.n_inst;
        const unsigned char *ir = b.inst + (size_t)inst * b.L.i_stride;
        const InstHeader h = *reinterpret_cast<const InstHeader *>(ir);
        const int K = h.K, M = h.M, MP = b.MP, KP = b.KP;
        v.now = v.Q + K;
        __syncthreads();                                                                   // (the previous LP's readers are done)
        const bool sized = K >= 1 && M >= 1 && K <= L.cap_K && M <= L.cap_M && M <= MP;   // (the staging arrays hold this instance)
        if (sized)
            lp_stage_inputs<kThreads>(v, K, MP, KP, reinterpret_cast<const uint16_t *>(ir + b.L.i_p), lp_in + (size_t)slot * 2 * KP,
                                      reinterpret_cast<const uint32_t *>(ir + b.L.i_kB), tid);
        if (tid == 0) s_fail = sized ? 0 : 5;
        __syncthreads();
        if (w == 0 && sized) {
            const LpDims d = lp_dimensions(v, K, M, MP, l);
            if (l == 0) {
                dims = d;
                // the limits of this kernel, of the LDS rows and of the slot: nothing below writes beyond them
                if (d.nr > kLpGlobalRows || d.nc > kLpGlobalColumns || d.nr > L.cap_nr || d.nc > L.cap_nc ||
                    (unsigned long long)d.nr * (unsigned long long)d.nc > slot_f64)
                    s_fail = 5;
            }
        }
        __syncthreads();
        int fail = s_fail;
        long n_piv = 0;
        if (!fail) {
            for (int j = tid; j < dims.nc; j += kThreads) zr[j] = j == dims.nx ? -1.0 : 0.0;      // the objective row: maximise t
            lp_fill<kThreads>(v, dims, T, MP, tid, &s_fail);
            fail = s_fail;
        }
        if (!fail) fail = lpg_pivots(T, zr, rr, v.basis, dims.nr, dims.nc, dims.nv, w, l, tid, n_piv);
        __syncthreads();
        lp_extract_x<kThreads>(v, dims, T, lp_x + (size_t)slot * KP * MP, KP, MP, fail, tid, &s_fail);
        if (tid == 0 && (fail || s_fail)) atomicOr(err, (uint32_t)(fail ? fail : s_fail));
        if (tid == 0 && solved) atomicAdd(solved + 1, (unsigned long long)n_piv);
    }
}

int launch_lp_global(const DevBatch &b, const uint32_t *count_dev, int count_host, const uint32_t *ids, const uint16_t *lp_in, double *lp_x,
                     uint32_t *err, unsigned long long *solved, const LpGlobalPool &pool, hipStream_t st) {
    const int grid = count_dev ? pool.slots : (count_host < pool.slots ? count_host : pool.slots);
    if (grid <= 0 || !pool.mem) return count_dev || count_host > 0 ? -1 : 0;
    return launch(lp_global_kernel, dim3((unsigned)grid), dim3(kThreads), (size_t)pool.lds.total, st, b, count_dev, count_host, ids, lp_in, lp_x,
                  err, solved, pool.mem, (unsigned long long)(pool.slot_bytes / 8), pool.lds);
}

}  // namespace fjsp

extern "C" int64_t fjsp_lp_global_bytes(int32_t K, int32_t M, int32_t nx, int32_t R) {
    using namespace fjsp;
    if (K <= 0 || M <= 0 || nx < 0 || R <= 0 || R > K) return 0;
    if (K > kLpGlobalRows || M > kLpGlobalRows || nx > kLpGlobalColumns) return 0;        // (beyond the limits on their own: no overflow below)
    if (lp_max_rows(K, M, R) > kLpGlobalRows || lp_max_columns(K, M, nx, R) > kLpGlobalColumns) return 0;
    return (int64_t)lp_global_slot_bytes(lp_max_rows(K, M, R), lp_max_columns(K, M, nx, R));
}
