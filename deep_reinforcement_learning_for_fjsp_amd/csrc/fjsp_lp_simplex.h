// The device simplex of the fluid-model LP: the solver text lp_device_kernel (fjsp_lp_device.hip, tableau in LDS) and
// lp_global_kernel (fjsp_lp_global.hip, tableau in global memory) share.  Device code only.
//
// csrc/fjsp_lp.cpp restated pivot for pivot: the same tableau (rows: one per operation type, one per machine, one per
// precedence constraint; columns: eligible (m, k) pairs in (m, k) order, t, the slacks, the right-hand side), the same
// entering rule (Dantzig, first smallest reduced cost), the same lexicographic ratio test with its tolerances, the same
// extraction of x; f64 divide, multiply, subtract without FMA (-ffp-contract=off; the host's AVX clones are built without
// FMA for the same reason).  So x is BIT-IDENTICAL to the host's wherever an LP is solved (tests/test_gpu_lp_device.py,
// tests/test_gpu_lp_global.py; tests/lp_reference.py restates this file in numpy and counts which branches the tested
// LPs take).  What the two kernels keep for themselves: where the tableau, the objective row and the scaled pivot row
// live, the elimination's inner loop, their LDS layouts and launchers.
//
// Every wave of a workgroup chooses the entering column and the leaving row BY ITSELF from the same values with the same
// operations -- the same answer in every wave, nothing to exchange -- so a pivot costs two workgroup barriers.  A lane
// holds G row groups of 64 (rows l, 64 + l, ...): G = 2 in lp_device_kernel, G = 4 in lp_global_kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace fjsp {
namespace {
constexpr double kEpsCost = 1e-9;   // entering threshold on reduced cost            (fjsp_lp.cpp)
constexpr double kEpsPiv = 1e-9;    // minimum pivot element
constexpr double kEpsZero = 1e-11;  // |x| below this is reported as exactly 0 (x != 0 test, class_FJSSP.py:290)
constexpr int kLexCols = 16;        // slack columns of a tie-break step: their signs fit one 32-bit signature

// ---- wave-level helpers: one f64 of a given lane, DPP moves of an f64, the wave's minimum in every lane
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

__device__ inline int wave_count(bool x) { return __builtin_popcountll(__ballot(x)); }

// ---- the set-up of one LP and the extraction of x, by every thread of a workgroup of NTH threads
struct LpDims { int K, M, nx, nv, nr, nc, nprec; };

// The small data of one LP, in LDS: each kernel points it into its own layout (basis and val once the dimensions are known)
struct LpView {
    uint16_t *p;         // [K][MP] processing times, 0 = ineligible
    uint16_t *Q, *now;   // [K] jobs of the order, jobs at the operation type now
    uint32_t *kB;        // [K] stage and stage count of the operation type's kind
    uint16_t *col_of;    // [K][M] -> column, 0xFFFF = ineligible
    uint16_t *prec;      // [nprec] operation types with a precedence row
    int *basis;          // [nr]
    double *val;         // [nc] value of a column's basic variable (x extraction)
};

// The inputs once into LDS (coalesced): everything below reads them there
template <int NTH>
__device__ __forceinline__ void lp_stage_inputs(const LpView &v, int K, int MP, int KP, const uint16_t *p_g, const uint16_t *Q_g,
                                                const uint32_t *kB_g, int tid) {
    for (int q = tid; q < K * MP; q += NTH) v.p[q] = p_g[q];
    for (int q = tid; q < K; q += NTH) { v.Q[q] = Q_g[q]; v.now[q] = Q_g[KP + q]; v.kB[q] = kB_g[q]; }
}

// Dimensions: columns = eligible pairs in (m, k) order, then t; precedence rows in k order (fjsp_lp.cpp).  The column
// numbers and the precedence list are prefix counts: ONE WAVE takes them 64 at a time from ballots (every lane returns
// the dimensions)
__device__ __forceinline__ LpDims lp_dimensions(const LpView &v, int K, int M, int MP, int l) {
    int nx = 0, nprec = 0;
    for (int base = 0; base < K * M; base += 64) {
        const int q = base + l, m = q / K, k = q - m * K;                          // (m, k) order
        const bool el = q < K * M && v.p[k * MP + m] > 0;
        const unsigned long long mask = __ballot(el);
        if (q < K * M) v.col_of[k * M + m] = el ? (uint16_t)(nx + __builtin_popcountll(mask & ((1ull << l) - 1ull))) : (uint16_t)0xFFFFu;
        nx += __builtin_popcountll(mask);
    }
    for (int base = 0; base + 1 < K; base += 64) {
        const int k = base + l;
        bool pr = false;
        if (k + 1 < K) {
            const uint32_t kb = v.kB[k];
            pr = (kb & 0xFFu) + 1u < ((kb >> 8) & 0xFFu) && v.now[k + 1] == 0;      // j + 1 < J_r: k + 1 is the same kind's next stage
        }
        const unsigned long long mask = __ballot(pr);
        if (pr) v.prec[nprec + __builtin_popcountll(mask & ((1ull << l) - 1ull))] = (uint16_t)k;
        nprec += __builtin_popcountll(mask);
    }
    LpDims d;
    d.K = K; d.M = M; d.nx = nx; d.nv = nx + 1; d.nprec = nprec;
    d.nr = K + M + nprec; d.nc = nx + 1 + d.nr + 1;
    return d;
}

// The tableau T[nr][nc] and the slack basis; *s_fail = 1 on an input the host refuses.  Ends with a barrier.
template <int NTH>
__device__ __forceinline__ void lp_fill(const LpView &v, const LpDims &d, double *const T, int MP, int tid, int *s_fail) {
    const int K = d.K, M = d.M, nv = d.nv, nr = d.nr, nc = d.nc, tcol = d.nx, rhs = nc - 1;
    auto at = [&](int i, int j) -> double & { return T[(size_t)i * nc + j]; };
    for (int q = tid; q < nr * nc; q += NTH) T[q] = 0.0;
    __syncthreads();
    for (int k = tid; k < K; k += NTH) {
        if (v.Q[k] == 0) *s_fail = 1;                                                  // "fluid LP: Q[k] <= 0"
        bool any = false;
        for (int m = 0; m < M; ++m) {
            const uint16_t c = v.col_of[k * M + m];
            if (c == 0xFFFFu) continue;
            any = true;
            const double rate = 1.0 / (double)v.p[k * MP + m];
            at(k, c) = -(rate / (double)v.Q[k]);
        }
        if (!any) *s_fail = 1;                                                         // "operation type without eligible machine"
        at(k, tcol) = 1.0;
    }
    for (int m = tid; m < M; m += NTH) {
        for (int k = 0; k < K; ++k) {
            const uint16_t c = v.col_of[k * M + m];
            if (c != 0xFFFFu) at(K + m, c) = 1.0;
        }
        at(K + m, rhs) = 1.0;
    }
    for (int q = tid; q < d.nprec; q += NTH) {
        const int k = v.prec[q], row = K + M + q;
        for (int m = 0; m < M; ++m) {
            const uint16_t c1 = v.col_of[(k + 1) * M + m], c0 = v.col_of[k * M + m];
            if (c1 != 0xFFFFu) at(row, c1) += 1.0 / (double)v.p[(k + 1) * MP + m];
            if (c0 != 0xFFFFu) at(row, c0) -= 1.0 / (double)v.p[k * MP + m];
        }
    }
    for (int i = tid; i < nr; i += NTH) { at(i, nv + i) = 1.0; v.basis[i] = nv + i; }
    __syncthreads();
}

// x out of the final basis into xout (f64[KP][MP], zeros elsewhere and when the LP failed: `fail`, the same in every
// thread): values below 1e-11 are exact zeros, above 1 clamp to 1.  *s_fail = 4 when an operation type is left without a
// positive fluid rate (fluid_time_sum = 1 / rate_sum, class_FJSSP.py:295).  Ends with a barrier.
template <int NTH>
__device__ __forceinline__ void lp_extract_x(const LpView &v, const LpDims &d, const double *const T, double *xout, int KP, int MP,
                                             int fail, int tid, int *s_fail) {
    const int K = d.K, M = d.M, nv = d.nv, nr = d.nr, nc = d.nc, rhs = nc - 1;
    for (int q = tid; q < KP * MP; q += NTH) xout[q] = 0.0;
    if (!fail) {
        for (int q = tid; q < nv; q += NTH) v.val[q] = 0.0;
        __syncthreads();
        for (int i = tid; i < nr; i += NTH)
            if (v.basis[i] < nv) v.val[v.basis[i]] = T[(size_t)i * nc + rhs];
        __syncthreads();
        for (int q = tid; q < K * M; q += NTH) {
            const int k = q / M, m = q % M;
            const uint16_t c = v.col_of[q];
            if (c == 0xFFFFu) continue;
            double x = v.val[c];
            if (x < kEpsZero) x = 0.0;
            if (x > 1.0) x = 1.0;
            xout[k * MP + m] = x;
        }
        __syncthreads();
        for (int k = tid; k < K; k += NTH) {
            double sacc = 0.0;
            for (int m = 0; m < M; ++m)
                if (v.p[k * MP + m] > 0) sacc += xout[k * MP + m] / (double)v.p[k * MP + m];
            if (!(sacc > 0.0)) *s_fail = 4;
        }
    }
    __syncthreads();
}

// ---- one pivot's decisions, by every wave for itself

// Entering column: the first smallest reduced cost below -eps (the smallest value, then its first column); -1 = optimal.
// z(t) is the objective row's entry of column l + 64 t, wherever the kernel keeps it; nt chunks of 64 cover the nc columns.
template <class Row>
__device__ __forceinline__ int lp_entering_column(const Row &z, const int nt, const int nc, const int l) {
    double m = __builtin_huge_val();
    for (int t = 0; t < nt; ++t)
        if (l + 64 * t < nc - 1) m = __builtin_fmin(m, z(t));
    m = wave_fmin_f64(m);
    if (!(m < -kEpsCost)) return -1;
    int s = -1;
    for (int t = 0; t < nt && s < 0; ++t) {
        const unsigned long long hit = __ballot(l + 64 * t < nc - 1 && z(t) == m);
        if (hit) s = 64 * t + __builtin_ctzll(hit);
    }
    return s;
}

__device__ inline double lp_ratio_tol(double v) { return 1e-12 * (fabs(v) > 1.0 ? fabs(v) : 1.0); }   // the ratio test's tolerance around v

struct LpLeaving { int r; double ar, vr; };      // the leaving row (-1: none, the LP is unbounded), its pivot element, its ratio

// Lexicographic ratio test (fjsp_lp.cpp): a strictly sequential scan over the rows with a > eps, which compares the row
// it meets with the best so far -- by the ratio v, and inside a tolerance by the slack columns over the pivot element,
// lexicographically.  These LPs are degenerate (every operation row and precedence row has a zero right-hand side): most
// rows tie, and pairwise tie-breaks would be where a pivot's time goes.  When the rows split cleanly into those with
// exactly the smallest ratio and those the scan's own two tests (evaluated here with its expressions) put strictly beyond
// the tolerance from them, the scan's result is the FIRST LEXICOGRAPHIC MINIMUM among the former -- an order-independent
// quantity, whatever the row count (tests/test_lp_reference.py and tests/test_lp_global_reference.py check it on every
// clean-split pivot of their cases) -- and the whole set is narrowed column by column with the rows in lanes; anything
// else (near-ties with different ratios) takes the sequential scan, run by one lane's worth of control flow over values
// the lanes have laid out.
// T[nr][nc], nr <= 64 G; s the entering column.  Leaves column s of the lane's rows in a[]: the elimination's factors.
template <int G>
__device__ __forceinline__ LpLeaving lp_leaving_row(const double *const T, const int nr, const int nc, const int nv, const int s, const int l,
                                                    double (&a)[G]) {
    const int rhs = nc - 1, cend = nv + nr;
    auto at = [&](int i, int j) -> const double & { return T[(size_t)i * nc + j]; };
    const double inf = __builtin_huge_val();
    LpLeaving out{-1, 0.0, 0.0};
    double v[G];                              // the ratios of rows l, 64 + l, ...
    bool el[G];
    unsigned long long any_el = 0ull;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = 64 * g + l;
        a[g] = i < nr ? at(i, s) : 0.0;
        el[g] = a[g] > kEpsPiv;
        v[g] = el[g] ? at(i, rhs) / a[g] : 0.0;
        any_el |= __ballot(el[g]);
    }
    if (!any_el) return out;
    double x = inf;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (el[g] && v[g] < x) x = v[g];
    const double vmin = wave_fmin_f64(x), hi = vmin + lp_ratio_tol(vmin);
    bool k[G];                                // the rows still in the race
    unsigned long long bad = 0ull;
    int cnt = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        k[g] = el[g] && v[g] == vmin;
        const bool far = v[g] > hi && vmin < v[g] - lp_ratio_tol(v[g]);
        bad |= __ballot(el[g] && !k[g] && !far);
        cnt += wave_count(k[g]);
    }
    if (!bad) {
        for (int c = nv; c < cend && cnt > 1; c += kLexCols) {
            // sign signatures of the next 16 columns, first column in the top bits: negative 0 < zero 1 < positive 2
            // (x / a keeps x's sign and is nonzero: a > 1e-9 and |x| >= 1e-280) -- rows order by them as by their
            // quotients wherever the signs differ
            bool small = false;               // a nonzero entry whose quotient could underflow
            uint32_t sig[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sig[g] = 0xFFFFFFFFu;         // (a row out of the race: behind every signature)
                if (__ballot(k[g]) == 0ull) continue;
                const double *row = &at(64 * g + l, c);
                double t[kLexCols];
#pragma unroll
                for (int u = 0; u < kLexCols; ++u) t[u] = (k[g] && c + u < cend) ? row[u] : 0.0;
                uint32_t sg = 0u;
#pragma unroll
                for (int u = 0; u < kLexCols; ++u) {
                    small = small || (t[u] != 0.0 && !(fabs(t[u]) >= 1e-280));
                    sg = (sg << 2) | (uint32_t)((t[u] == 0.0 ? 1 : 0) + (t[u] > 0.0 ? 2 : 0));
                }
                if (k[g]) sig[g] = sg;
            }
            const bool exact_signs = __ballot(small) == 0ull;
            if (exact_signs) {
                uint32_t smine = sig[0];
#pragma unroll
                for (int g = 1; g < G; ++g) smine = sig[g] < smine ? sig[g] : smine;
                const uint32_t smin = wave_min_u32(smine);
                const uint32_t d = smin ^ 0x55555555u;                         // 0: the best rows are zero in all 16 columns
                // the rows that agree with the best signature up to and including its first nonzero sign
                const uint32_t keep = d ? ~((1u << (2 * ((31 - __builtin_clz(d)) >> 1))) - 1u) : 0xFFFFFFFFu;
                bool p[G];
                int np = 0;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    p[g] = k[g] && ((sig[g] ^ smin) & keep) == 0u;
                    np += wave_count(p[g]);
                }
                if (d == 0u || np == 1) {
#pragma unroll
                    for (int g = 0; g < G; ++g) k[g] = p[g];
                    cnt = np;
                    continue;
                }
                // (several rows share a nonzero sign in the deciding column: magnitudes decide, column by column below)
            }
            for (int u = 0; u < kLexCols; ++u) {                               // (rare: the entries are read again)
                if (c + u >= cend || cnt <= 1) break;
                double xg[G];
                bool sl[G];                   // the rows whose quotients are compared
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    xg[g] = k[g] ? at(64 * g + l, c + u) : 0.0;
                    sl[g] = k[g];
                }
                // signs decide most columns without a division: one negative entry wins, positives lose against zeros
                if (exact_signs) {
                    bool gn[G];
                    int nn = 0;
#pragma unroll
                    for (int g = 0; g < G; ++g) { gn[g] = k[g] && xg[g] < 0.0; nn += wave_count(gn[g]); }
                    if (nn == 1) {
#pragma unroll
                        for (int g = 0; g < G; ++g) k[g] = gn[g];
                        cnt = 1;
                        continue;
                    }
                    if (nn == 0) {
                        bool z[G];
                        int nz = 0;
#pragma unroll
                        for (int g = 0; g < G; ++g) { z[g] = k[g] && xg[g] == 0.0; nz += wave_count(z[g]); }
                        if (nz > 0) {
#pragma unroll
                            for (int g = 0; g < G; ++g) k[g] = z[g];
                            cnt = nz;
                            continue;
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < G; ++g) sl[g] = gn[g];
                    }
                }
                double wq[G], wl = inf;
#pragma unroll
                for (int g = 0; g < G; ++g) { wq[g] = sl[g] ? xg[g] / a[g] : inf; wl = __builtin_fmin(wl, wq[g]); }
                const double wm = wave_fmin_f64(wl);
                cnt = 0;
#pragma unroll
                for (int g = 0; g < G; ++g) { k[g] = sl[g] && wq[g] == wm; cnt += wave_count(k[g]); }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const unsigned long long E = __ballot(k[g]);
            if (out.r < 0 && E) {             // the first row of the race, in row order
                const int q = __builtin_ctzll(E);
                out.r = 64 * g + q; out.ar = lane_f64(a[g], q); out.vr = vmin;
            }
        }
        if (out.r >= 0) return out;
    }
    // ---- the scan itself
    int r = -1;
    double ar = 0.0, vr = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int base = 64 * g;
        if (base >= nr) continue;
        unsigned long long mask = __ballot(el[g]);
        while (mask) {
            // rows the scan would pass with "vi > vr + tol: continue" are passed in one step: the next row it
            // looks at closer is the first remaining one for which that test fails
            if (r >= 0) {
                mask &= __ballot(el[g] && !(v[g] > vr + lp_ratio_tol(vr)));
                if (!mask) break;
            }
            const int q = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int irow = base + q;
            const double ai = lane_f64(a[g], q), vi = lane_f64(v[g], q);
            if (r < 0 || vi < vr - lp_ratio_tol(vr)) { r = irow; ar = ai; vr = vi; continue; }
            for (int c0 = nv; c0 < cend; c0 += 64) {                           // a tie: 64 slack columns at a time
                const int c = c0 + l;
                const bool in = c < cend;
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
    out.r = r; out.ar = ar; out.vr = vr;
    return out;
}

// ---- elimination: column s is sparse, only rows with a nonzero factor change.  Those rows (a ballot of the factors a[]
// every wave holds) are dealt round-robin to the W waves: my[g] = the rows 64 g + lane of wave w
template <int G, int W>
__device__ __forceinline__ void lp_deal_rows(const double (&a)[G], const int nr, const int r, const int w, const int l,
                                             unsigned long long (&my)[G]) {
    static_assert((W & (W - 1)) == 0, "the waves of a workgroup: a power of two");
    int before = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = 64 * g + l;
        const bool nz = i < nr && i != r && a[g] != 0.0;
        const unsigned long long Z = __ballot(nz);
        const int rank = before + __builtin_popcountll(Z & ((1ull << l) - 1ull));
        my[g] = __ballot(nz && (rank & (W - 1)) == w);
        before += __builtin_popcountll(Z);
    }
}

// Pop this wave's next row and its factor (row = -1, f = 0: none left)
template <int G>
__device__ __forceinline__ void lp_next_row(unsigned long long (&my)[G], const double (&a)[G], int &row, double &f) {
    row = -1; f = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (row < 0 && my[g]) {
            const int q = __builtin_ctzll(my[g]);
            my[g] &= my[g] - 1ull;
            row = 64 * g + q; f = lane_f64(a[g], q);
        }
}
}  // namespace
}  // namespace fjsp
