// The fluid-model LP on the device with its simplex tableau in GLOBAL memory: the LPs whose tableau does not fit the LDS
// of a CU (fjsp_lp_device.hip keeps tableaus of up to 156 KB and 512 columns there).  The reference's own training
// instances are of that kind: data/HMPSAC 71-113 rows x 328-538 columns (213-474 KB), data/MPPPO up to 133 x 673 (699 KB),
// the MPPPO generator's worst case 128 x 1330 (1.36 MB).
//
// The same solver as fjsp_lp.cpp and lp_device_kernel, pivot for pivot -- Dantzig pricing with the first smallest reduced
// cost, the lexicographic ratio test with its tolerances, f64 divide / multiply / subtract without FMA, the clean-up of a
// tiny negative right-hand side, the same extraction of x -- so x is BIT-IDENTICAL to theirs (tests/test_gpu_lp_global.py).
// What differs is where things live:
//   * the tableau f64[nr][nc] in a slot of a scratch pool in HBM, one slot per workgroup (the pool is allocated at create,
//     only by handles that chose this service); a workgroup strides over the LPs of a launch and re-uses its slot;
//   * LDS holds the small data only: the staged inputs p, Q, n_now, kB, the column map, the precedence list, basis, val, and
//     the objective row and the scaled pivot row (nc <= 1536: 12 KB each).  The two rows are in LDS, not in registers: at
//     24 chunks of 64 columns a lane would hold 2 x 24 f64 = 96 VGPRs for them alone, and every wave a copy; in LDS one
//     copy serves the workgroup, the pivot loop needs no chunk-count template, and a workgroup of 256 threads takes
//     22-73 KB of LDS, so two to seven of them share a CU (profiles/lp_global_resources.txt: no scratch memory);
//   * rows: up to 256, held as four row groups per lane (rows l, 64 + l, 128 + l, 192 + l) in the order-independent ratio
//     test, in the elimination's factor ballots and in its dealing of rows to the waves.  The claim that makes the
//     order-independent choice legal does not depend on the row count: on a clean split the sequential scan's answer is
//     the first lexicographic minimum among the exactly tied rows, in row order (tests/test_lp_global_reference.py checks
//     it on every clean-split pivot of the cases beyond 128 rows).  `bad` splits take the sequential scan, as there.
// Synchronisation is __syncthreads() alone -- it orders the workgroup's global-memory writes and reads --: no cooperative
// launch, nothing between workgroups, no flags in memory.  A row chunk is read coalesced: lane l has columns l + 64 t.
// An LP outside the limits or the slot (never one an admitted handle can meet) ends with an error code, not a write.
#include <hip/hip_runtime.h>

#include "../../include/fjsp_amd.h"
#include "fjsp_common.h"
#include "fjsp_device.h"
#include "fjsp_launch.h"
#include "fjsp_lp_wave.h"

#pragma clang fp contract(off)

namespace fjsp {

namespace {
constexpr double kEpsCost = 1e-9;   // entering threshold on reduced cost            (fjsp_lp.cpp)
constexpr double kEpsPiv = 1e-9;    // minimum pivot element
constexpr double kEpsZero = 1e-11;  // |x| below this is reported as exactly 0
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = 4;          // row groups of 64 a lane holds: nr <= 256
constexpr int kMaxRows = 64 * kGroups;
constexpr int kMaxCols = 1536;      // 24 chunks of 64
constexpr int kLexCols = 16;        // slack columns of a tie-break step: their signs fit one 32-bit signature
constexpr int kRB = 2;              // rows of the elimination a wave has in flight
constexpr int kCB = 4;              // ... and chunks of each

extern __shared__ __attribute__((aligned(16))) unsigned char lpg_lds[];

struct LpDims { int K, M, nx, nv, nr, nc, nprec; };
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
// The pivots of one LP (every thread of the workgroup; returns the failure code, 0 = optimal).  lp_pivots of
// fjsp_lp_device.hip with the tableau in global memory, the objective row zr and the scaled pivot row rr in LDS, and four
// row groups.  Every wave chooses the entering column and the leaving row by itself from the same values; two workgroup
// barriers per pivot.
__device__ __forceinline__ int lpg_pivots(double *const T, double *const zr, double *const rr, int *const basis, const int nr, const int nc,
                                          const int nv, const int w, const int l, const int tid, long &n_piv) {
    const int rhs = nc - 1, nt = (nc + 63) >> 6;
    auto at = [&](int i, int j) -> double & { return T[(size_t)i * nc + j]; };
    const double inf = __builtin_huge_val();
    const long max_iter = 200L * (nr + nc) + 1000;
    for (long it = 0;; ++it) {
        if (it > max_iter) return 2;                                   // "iteration limit"
        // ---- entering column: the first smallest reduced cost below -eps (the smallest value, then its first column)
        int s = -1;
        {
            double m = inf;
            for (int t = 0; t < nt; ++t) {
                const int j = l + 64 * t;
                if (j < nc - 1) m = __builtin_fmin(m, zr[j]);
            }
            m = wave_fmin_f64(m);
            if (!(m < -kEpsCost)) return 0;                            // optimal
            for (int t = 0; t < nt && s < 0; ++t) {
                const int j = l + 64 * t;
                const unsigned long long hit = __ballot(j < nc - 1 && zr[j] == m);
                if (hit) s = 64 * t + __builtin_ctzll(hit);
            }
        }
        // ---- lexicographic ratio test (fjsp_lp.cpp, fjsp_lp_device.hip): when the rows split cleanly into those with
        // exactly the smallest ratio and those the scan's own two tests put strictly beyond the tolerance from them, the
        // scan's result is the FIRST LEXICOGRAPHIC MINIMUM among the former, narrowed column by column with the rows in
        // lanes -- here four row groups of them; anything else takes the sequential scan below.
        int r = -1;
        double ar = 0.0, vr = 0.0;
        double a[kGroups], v[kGroups];        // column s and the ratios of rows l, 64 + l, 128 + l, 192 + l
        bool el[kGroups];
        unsigned long long any_el = 0ull;
#pragma unroll
        for (int g = 0; g < kGroups; ++g) {
            const int i = 64 * g + l;
            a[g] = i < nr ? at(i, s) : 0.0;
            el[g] = a[g] > kEpsPiv;
            v[g] = el[g] ? at(i, rhs) / a[g] : 0.0;
            any_el |= __ballot(el[g]);
        }
        if (!any_el) return 3;                                         // "unbounded"
        bool chosen = false;
        {
            double x = inf;
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
                if (el[g] && v[g] < x) x = v[g];
            const double vmin = wave_fmin_f64(x);
            const double tolmin = 1e-12 * (fabs(vmin) > 1.0 ? fabs(vmin) : 1.0), hi = vmin + tolmin;
            bool k[kGroups];                                           // the rows still in the race
            unsigned long long bad = 0ull;
            int cnt = 0;
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
                k[g] = el[g] && v[g] == vmin;
                const double tol = 1e-12 * (fabs(v[g]) > 1.0 ? fabs(v[g]) : 1.0);
                const bool far = v[g] > hi && vmin < v[g] - tol;
                bad |= __ballot(el[g] && !k[g] && !far);
                cnt += __builtin_popcountll(__ballot(k[g]));
            }
            if (!bad) {
                const int cend = nv + nr;
                for (int c = nv; c < cend && cnt > 1; c += kLexCols) {
                    // sign signatures of the next 16 columns, first column in the top bits: negative 0 < zero 1 < positive 2
                    // (x / a keeps x's sign and is nonzero: a > 1e-9 and |x| >= 1e-280)
                    bool small = false;                                // a nonzero entry whose quotient could underflow
                    uint32_t sig[kGroups];
#pragma unroll
                    for (int g = 0; g < kGroups; ++g) {
                        sig[g] = 0x55555555u;
                        if (__ballot(k[g]) == 0ull) continue;          // (no row of this group in the race)
                        const double *row = &T[(size_t)(64 * g + l) * nc];
                        double t[kLexCols];
#pragma unroll
                        for (int u = 0; u < kLexCols; ++u) t[u] = (k[g] && c + u < cend) ? row[c + u] : 0.0;
                        uint32_t sg = 0u;
#pragma unroll
                        for (int u = 0; u < kLexCols; ++u) {
                            small = small || (t[u] != 0.0 && !(fabs(t[u]) >= 1e-280));
                            sg = (sg << 2) | (uint32_t)((t[u] == 0.0 ? 1 : 0) + (t[u] > 0.0 ? 2 : 0));
                        }
                        sig[g] = sg;
                    }
                    const bool exact_signs = __ballot(small) == 0ull;
                    if (exact_signs) {
                        uint32_t smine = 0xFFFFFFFFu;
#pragma unroll
                        for (int g = 0; g < kGroups; ++g) {
                            if (!k[g]) sig[g] = 0xFFFFFFFFu;
                            smine = sig[g] < smine ? sig[g] : smine;
                        }
                        const uint32_t smin = wave_min_u32(smine);
                        const uint32_t d = smin ^ 0x55555555u;                         // 0: the best rows are zero in all 16 columns
                        // the rows that agree with the best signature up to and including its first nonzero sign
                        const uint32_t keep = d ? ~((1u << (2 * ((31 - __builtin_clz(d)) >> 1))) - 1u) : 0xFFFFFFFFu;
                        bool p[kGroups];
                        int np = 0;
#pragma unroll
                        for (int g = 0; g < kGroups; ++g) {
                            p[g] = k[g] && ((sig[g] ^ smin) & keep) == 0u;
                            np += __builtin_popcountll(__ballot(p[g]));
                        }
                        if (d == 0u || np == 1) {
#pragma unroll
                            for (int g = 0; g < kGroups; ++g) k[g] = p[g];
                            cnt = np;
                            continue;
                        }
                        // (several rows share a nonzero sign in the deciding column: magnitudes decide, column by column below)
                    }
                    for (int u = 0; u < kLexCols; ++u) {
                        if (c + u >= cend || cnt <= 1) break;
                        double x4[kGroups];
                        bool sl[kGroups];                              // the rows whose quotients are compared
#pragma unroll
                        for (int g = 0; g < kGroups; ++g) {
                            x4[g] = k[g] ? at(64 * g + l, c + u) : 0.0;
                            sl[g] = k[g];
                        }
                        // signs decide most columns without a division: one negative entry wins, positives lose against zeros
                        if (exact_signs) {
                            bool gn[kGroups];
                            int nn = 0;
#pragma unroll
                            for (int g = 0; g < kGroups; ++g) { gn[g] = k[g] && x4[g] < 0.0; nn += __builtin_popcountll(__ballot(gn[g])); }
                            if (nn == 1) {
#pragma unroll
                                for (int g = 0; g < kGroups; ++g) k[g] = gn[g];
                                cnt = 1;
                                continue;
                            }
                            if (nn == 0) {
                                bool z[kGroups];
                                int nz = 0;
#pragma unroll
                                for (int g = 0; g < kGroups; ++g) { z[g] = k[g] && x4[g] == 0.0; nz += __builtin_popcountll(__ballot(z[g])); }
                                if (nz > 0) {
#pragma unroll
                                    for (int g = 0; g < kGroups; ++g) k[g] = z[g];
                                    cnt = nz;
                                    continue;
                                }
                            } else {
#pragma unroll
                                for (int g = 0; g < kGroups; ++g) sl[g] = gn[g];
                            }
                        }
                        double wq[kGroups], wl = inf;
#pragma unroll
                        for (int g = 0; g < kGroups; ++g) { wq[g] = sl[g] ? x4[g] / a[g] : inf; wl = __builtin_fmin(wl, wq[g]); }
                        const double wm = wave_fmin_f64(wl);
                        cnt = 0;
#pragma unroll
                        for (int g = 0; g < kGroups; ++g) { k[g] = sl[g] && wq[g] == wm; cnt += __builtin_popcountll(__ballot(k[g])); }
                    }
                }
#pragma unroll
                for (int g = 0; g < kGroups; ++g) {
                    const unsigned long long E = __ballot(k[g]);
                    if (!chosen && E) {                                // the first row of the race, in row order
                        const int q = __builtin_ctzll(E);
                        chosen = true; vr = vmin; r = 64 * g + q; ar = lane_f64(a[g], q);
                    }
                }
            }
        }
        if (!chosen) {
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
                const int base = 64 * g;
                if (base >= nr) continue;
                unsigned long long mask = __ballot(el[g]);
                while (mask) {
                    // rows the scan would pass with "vi > vr + tol: continue" are passed in one step: the next row it
                    // looks at closer is the first remaining one for which that test fails
                    if (r >= 0) {
                        const double tol = 1e-12 * (fabs(vr) > 1.0 ? fabs(vr) : 1.0);
                        mask &= __ballot(el[g] && !(v[g] > vr + tol));
                        if (!mask) break;
                    }
                    const int q = __builtin_ctzll(mask);
                    mask &= mask - 1ull;
                    const int irow = base + q;
                    const double ai = lane_f64(a[g], q), vi = lane_f64(v[g], q);
                    if (r < 0) { r = irow; ar = ai; vr = vi; continue; }
                    const double tol = 1e-12 * (fabs(vr) > 1.0 ? fabs(vr) : 1.0);
                    if (vi < vr - tol) { r = irow; ar = ai; vr = vi; continue; }
                    for (int c0 = nv; c0 < nv + nr; c0 += 64) {         // a tie: 64 slack columns at a time
                        const int c = c0 + l;
                        const bool in = c < nv + nr;
                        const double wi = in ? at(irow, c) / ai : 0.0, wr = in ? at(r, c) / ar : 0.0;
                        const unsigned long long lt = __ballot(in && wi < wr), gt = __ballot(in && wi > wr);
                        if (lt | gt) {
                            const int f = __builtin_ctzll(lt | gt);
                            if ((lt >> f) & 1ull) { r = irow; ar = ai; vr = vi; }
                            break;
                        }
                    }
                }
            }
        }
        if (r < 0) return 3;                                           // "unbounded"
        // ---- pivot: the scaled row r into LDS (column s becomes exactly 1), the objective's factor
        {
            const double piv = ar;
            const double *rowr = &T[(size_t)r * nc];
            for (int j = tid; j < nc; j += kThreads) rr[j] = j == s ? 1.0 : rowr[j] / piv;
        }
        const double fz = zr[s];
        __syncthreads();                      // every wave has read column s, the right-hand sides, row r and zr[s]; rr is complete
        // ---- elimination.  Column s is sparse: only rows with a nonzero factor change.  Those rows (a ballot of the
        // factors every wave holds, over the four row groups) are dealt round-robin to the waves, and a wave takes kRB of
        // its rows and kCB chunks of them at a time; lane l has the columns l, l + 64, ...  (x - f * 1 of column s is
        // exactly 0, as the host writes it.)
        {
            unsigned long long my[kGroups];
            int before = 0;
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
                const int i = 64 * g + l;
                const bool nz = i < nr && i != r && a[g] != 0.0;
                const unsigned long long Z = __ballot(nz);
                const int rank = before + __builtin_popcountll(Z & ((1ull << l) - 1ull));
                my[g] = __ballot(nz && (rank & (kWaves - 1)) == w);
                before += __builtin_popcountll(Z);
            }
            for (;;) {
                int row[kRB];
                double f[kRB];
#pragma unroll
                for (int u = 0; u < kRB; ++u) {
                    row[u] = -1; f[u] = 0.0;
#pragma unroll
                    for (int g = 0; g < kGroups; ++g)
                        if (row[u] < 0 && my[g]) {
                            const int q = __builtin_ctzll(my[g]);
                            my[g] &= my[g] - 1ull;
                            row[u] = 64 * g + q; f[u] = lane_f64(a[g], q);
                        }
                }
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
    double *const val = reinterpret_cast<double *>(lpg_lds + L.val);                      // [nc]: value of a column's basic variable
    int *const basis = reinterpret_cast<int *>(lpg_lds + L.basis);
    uint16_t *const col_of = reinterpret_cast<uint16_t *>(lpg_lds + L.col_of);            // [K][M] -> column, 0xFFFF = ineligible
    uint16_t *const prec = reinterpret_cast<uint16_t *>(lpg_lds + L.prec);
    uint16_t *const p = reinterpret_cast<uint16_t *>(lpg_lds + L.p);                      // [K][MP]
    uint16_t *const Q = reinterpret_cast<uint16_t *>(lpg_lds + L.Q);
    uint32_t *const kB = reinterpret_cast<uint32_t *>(lpg_lds + L.kB);
    __shared__ LpDims dims;
    __shared__ int s_fail;
    for (uint32_t slot = blockIdx.x; slot < count; slot += gridDim.x) {
        const int env = (int)ids[slot];
        const int inst = b.n_inst == b.N ? env : env % b.n_inst;
        const unsigned char *ir = b.inst + (size_t)inst * b.L.i_stride;
        const InstHeader h = *reinterpret_cast<const InstHeader *>(ir);
        const int K = h.K, M = h.M, MP = b.MP, KP = b.KP;
        const uint16_t *p_g = reinterpret_cast<const uint16_t *>(ir + b.L.i_p);         // [KP][MP], 0 = ineligible
        const uint32_t *kB_g = reinterpret_cast<const uint32_t *>(ir + b.L.i_kB);
        const uint16_t *Q_g = lp_in + (size_t)slot * 2 * KP;
        double *xout = lp_x + (size_t)slot * KP * MP;
        uint16_t *now = Q + K;
        __syncthreads();                                                                   // (the previous LP's readers are done)
        const bool sized = K >= 1 && M >= 1 && K <= L.cap_K && M <= L.cap_M && M <= MP;   // (the staging arrays hold this instance)
        if (sized) {
            for (int q = tid; q < K * MP; q += kThreads) p[q] = p_g[q];
            for (int q = tid; q < K; q += kThreads) { Q[q] = Q_g[q]; now[q] = Q_g[KP + q]; kB[q] = kB_g[q]; }
        }
        if (tid == 0) s_fail = sized ? 0 : 5;
        __syncthreads();
        // ---- dimensions: columns = eligible pairs in (m, k) order, then t; precedence rows in k order (fjsp_lp.cpp).
        // The column numbers and the precedence list are prefix counts: wave 0 takes them 64 at a time from ballots.
        if (w == 0 && sized) {
            int nx = 0, nprec = 0;
            for (int base = 0; base < K * M; base += 64) {
                const int q = base + l, m = q / K, k = q - m * K;                          // (m, k) order
                const bool el = q < K * M && p[k * MP + m] > 0;
                const unsigned long long mask = __ballot(el);
                if (q < K * M) col_of[k * M + m] = el ? (uint16_t)(nx + __builtin_popcountll(mask & ((1ull << l) - 1ull))) : (uint16_t)0xFFFFu;
                nx += __builtin_popcountll(mask);
            }
            for (int base = 0; base + 1 < K; base += 64) {
                const int k = base + l;
                bool pr = false;
                if (k + 1 < K) {
                    const uint32_t kb = kB[k];
                    pr = (kb & 0xFFu) + 1u < ((kb >> 8) & 0xFFu) && now[k + 1] == 0;        // j + 1 < J_r: k + 1 is the same kind's next stage
                }
                const unsigned long long mask = __ballot(pr);
                if (pr) prec[nprec + __builtin_popcountll(mask & ((1ull << l) - 1ull))] = (uint16_t)k;
                nprec += __builtin_popcountll(mask);
            }
            if (l == 0) {
                dims.K = K; dims.M = M; dims.nx = nx; dims.nv = nx + 1; dims.nprec = nprec;
                dims.nr = K + M + nprec; dims.nc = nx + 1 + dims.nr + 1;
                // the limits of this kernel, of the LDS rows and of the slot: nothing below writes beyond them
                if (dims.nr > kMaxRows || dims.nc > kMaxCols || dims.nr > L.cap_nr || dims.nc > L.cap_nc ||
                    (unsigned long long)dims.nr * (unsigned long long)dims.nc > slot_f64)
                    s_fail = 5;
            }
        }
        __syncthreads();
        int fail = s_fail;
        long n_piv = 0;
        const int nv = dims.nv, nr = dims.nr, nc = dims.nc, tcol = dims.nx, rhs = nc - 1, nprec = dims.nprec;
        auto at = [&](int i, int j) -> double & { return T[(size_t)i * nc + j]; };
        if (!fail) {
            for (int q = tid; q < nr * nc; q += kThreads) T[q] = 0.0;
            for (int j = tid; j < nc; j += kThreads) zr[j] = j == tcol ? -1.0 : 0.0;      // the objective row: maximise t
            __syncthreads();
            // ---- fill
            for (int k = tid; k < K; k += kThreads) {
                if (Q[k] == 0) s_fail = 1;                                                 // "fluid LP: Q[k] <= 0"
                bool any = false;
                for (int m = 0; m < M; ++m) {
                    const uint16_t c = col_of[k * M + m];
                    if (c == 0xFFFFu) continue;
                    any = true;
                    const double rate = 1.0 / (double)p[k * MP + m];
                    at(k, c) = -(rate / (double)Q[k]);
                }
                if (!any) s_fail = 1;                                                      // "operation type without eligible machine"
                at(k, tcol) = 1.0;
            }
            for (int m = tid; m < M; m += kThreads) {
                for (int k = 0; k < K; ++k) {
                    const uint16_t c = col_of[k * M + m];
                    if (c != 0xFFFFu) at(K + m, c) = 1.0;
                }
                at(K + m, rhs) = 1.0;
            }
            for (int q = tid; q < nprec; q += kThreads) {
                const int k = prec[q], row = K + M + q;
                for (int m = 0; m < M; ++m) {
                    const uint16_t c1 = col_of[(k + 1) * M + m], c0 = col_of[k * M + m];
                    if (c1 != 0xFFFFu) at(row, c1) += 1.0 / (double)p[(k + 1) * MP + m];
                    if (c0 != 0xFFFFu) at(row, c0) -= 1.0 / (double)p[k * MP + m];
                }
            }
            for (int i = tid; i < nr; i += kThreads) { at(i, nv + i) = 1.0; basis[i] = nv + i; }
            __syncthreads();
            fail = s_fail;
            // ---- pivots
            if (!fail) fail = lpg_pivots(T, zr, rr, basis, nr, nc, nv, w, l, tid, n_piv);
        }
        __syncthreads();
        // ---- x out of the basis (values below 1e-11 are exact zeros, above 1 clamp to 1)
        for (int q = tid; q < KP * MP; q += kThreads) xout[q] = 0.0;
        if (!fail) {
            for (int q = tid; q < nv; q += kThreads) val[q] = 0.0;
            __syncthreads();
            for (int i = tid; i < nr; i += kThreads)
                if (basis[i] < nv) val[basis[i]] = at(i, rhs);
            __syncthreads();
            for (int q = tid; q < K * M; q += kThreads) {
                const int k = q / M, m = q % M;
                const uint16_t c = col_of[q];
                if (c == 0xFFFFu) continue;
                double v = val[c];
                if (v < kEpsZero) v = 0.0;
                if (v > 1.0) v = 1.0;
                xout[k * MP + m] = v;
            }
            __syncthreads();
            // every operation type must keep a positive fluid rate (fluid_time_sum = 1 / rate_sum)
            for (int k = tid; k < K; k += kThreads) {
                double sacc = 0.0;
                for (int m = 0; m < M; ++m)
                    if (p[k * MP + m] > 0) sacc += xout[k * MP + m] / (double)p[k * MP + m];
                if (!(sacc > 0.0)) s_fail = 4;
            }
        }
        __syncthreads();
        if (tid == 0 && (fail || s_fail)) atomicOr(err, (uint32_t)(fail ? fail : s_fail));
        if (tid == 0 && solved) atomicAdd(solved + 1, (unsigned long long)n_piv);
    }
}

int lp_global_max_rows() { return kMaxRows; }
int lp_global_max_columns() { return kMaxCols; }

int launch_lp_global(const DevBatch &b, const uint32_t *count_dev, int count_host, const uint32_t *ids, const uint16_t *lp_in, double *lp_x,
                     uint32_t *err, unsigned long long *solved, const LpGlobalPool &pool, hipStream_t st) {
    const int grid = count_dev ? pool.slots : (count_host < pool.slots ? count_host : pool.slots);
    if (grid <= 0 || !pool.mem) return count_dev || count_host > 0 ? -1 : 0;
    return launch(lp_global_kernel, dim3((unsigned)grid), dim3(kThreads), (size_t)pool.lds.total, st, b, count_dev, count_host, ids, lp_in, lp_x,
                  err, solved, pool.mem, (unsigned long long)(pool.slot_bytes / 8), pool.lds);
}

}  // namespace fjsp

extern "C" int64_t fjsp_lp_global_bytes(int32_t K, int32_t M, int32_t nx, int32_t R) {
    if (K <= 0 || M <= 0 || nx < 0 || R <= 0 || R > K) return 0;
    const int64_t nr = (int64_t)K + M + (K - R), nc = (int64_t)nx + 1 + nr + 1;
    if (nr > fjsp::kMaxRows || nc > fjsp::kMaxCols) return 0;
    return (nr * nc * 8 + 255) & ~(int64_t)255;
}
