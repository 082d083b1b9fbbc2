// The instance generator's draw stream and its shop, stated once for the host generator (fjsp_instance.cpp, plain C++) and
// the device generator (fjsp_generate.hip): which draw of which stream is what, and the arithmetic that makes an instance of
// the draws (environments/Instance_generate.py:19-94; the :NN marks are its lines).  The host calls the element functions in
// loops, the device from the lanes of a wave; they are templates over the element type of the rows they write (int vectors
// there, u8 / u16 rows in LDS here), allocate nothing, and must inline on the device so that the rows keep their address
// space.  tests/test_generate*_host.py restate the stream once more, in Python, on purpose: a mistake here breaks host and
// device together and only they would see it.  No a * b + c may contract into an FMA: under clang the pragma below says so,
// any other compiler relies on the build's -ffp-contract=off, which every build line of the project carries.
#pragma once
#include <cstdint>
#include "../../include/fjsp_amd.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define FJSP_GEN_FN __host__ __device__ __forceinline__
#else
#define FJSP_GEN_FN inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fjsp::gen {

// ---- the stream: splitmix64, whose state advances by a constant per draw, so draw i (0-based) is a function of (seed, i)
FJSP_GEN_FN uint64_t draw(uint64_t seed, uint32_t i) {
    uint64_t z = seed + (uint64_t)(i + 1u) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
FJSP_GEN_FN int randint(uint64_t seed, uint32_t i, int a, int b) { return a + (int)(((draw(seed, i) >> 32) * (uint64_t)(b - a + 1)) >> 32); }   // a..b
FJSP_GEN_FN double uniform(uint64_t seed, uint32_t i, double lo, double hi) { return lo + (hi - lo) * ((double)(draw(seed, i) >> 11) * (1.0 / 9007199254740992.0)); }

// ---- positions in the shop stream (seed): R (:42), J_r (:46,71), then the chain -- per operation type its number of
// eligible machines n and n shuffle draws (:73) --, behind all shuffles the processing times in list order (:74), at the
// chain's end the S x R job counts order-major (:80, q = s * R + r), behind them the intervals of the orders s >= 1 (:83-84)
FJSP_GEN_FN uint32_t pos_kinds() { return 0u; }
FJSP_GEN_FN uint32_t pos_operations(int r) { return 1u + (uint32_t)r; }
FJSP_GEN_FN uint32_t pos_chain(int R) { return 1u + (uint32_t)R; }
FJSP_GEN_FN uint32_t pos_count(uint32_t chain_end, int q) { return chain_end + (uint32_t)q; }
FJSP_GEN_FN uint32_t pos_interval(uint32_t chain_end, int S, int R, int s) { return chain_end + (uint32_t)(S * R) + (uint32_t)(s - 1); }
// ---- the auxiliary stream (seed ^ FJSP_GEN_AUX_STREAM): M, DDT and S of an instance whose parameters are ranges
FJSP_GEN_FN int aux_machines(uint64_t seed, int M_min, int M_max) { return randint(seed ^ FJSP_GEN_AUX_STREAM, 0u, M_min, M_max); }
FJSP_GEN_FN double aux_ddt(uint64_t seed, double lo, double hi) { return uniform(seed ^ FJSP_GEN_AUX_STREAM, 1u, lo, hi); }
FJSP_GEN_FN int aux_orders(uint64_t seed, int S_min, int S_max) { return randint(seed ^ FJSP_GEN_AUX_STREAM, 2u, S_min, S_max); }
// ---- the seed of attempt j of instance `seed` (fjsp_gen_dynamic): its own, then the draws of its redraw stream
FJSP_GEN_FN uint64_t attempt_seed(uint64_t seed, int j) { return j == 0 ? seed : draw(seed ^ FJSP_GEN_REDRAW_STREAM, (uint32_t)(j - 1)); }
// ---- positions in the machine stream (fjsp_gen_machine): idle power and window count per machine, power per
// (operation type, machine) pair q = k * M + m, then W_max (gap, length) pairs per machine
FJSP_GEN_FN uint64_t machine_stream(uint64_t seed) { return seed ^ FJSP_GEN_MACHINE_STREAM; }
FJSP_GEN_FN uint32_t pos_idle_power(int m) { return (uint32_t)m; }
FJSP_GEN_FN uint32_t pos_window_count(int M, int m) { return (uint32_t)(M + m); }
FJSP_GEN_FN uint32_t pos_power(int M, int q) { return (uint32_t)(2 * M + q); }
FJSP_GEN_FN uint32_t pos_window(int M, int K, int W, int m, int w) { return (uint32_t)(2 * M + K * M + 2 * (m * W + w)); }

// ---- the shop
// The one serial chain there is: n of operation type k decides where type k + 1's draws start.  n[k]; off[k], poff[k]: the
// first shuffle draw and the first processing-time draw of type k; nx: eligible pairs; end: the first draw behind the
// processing times.  0, or FJSP_E_FORMAT for an n outside 1..M (the rows are then written up to that type).
template <class TN, class TO> FJSP_GEN_FN int chain(uint64_t seed, int R, int K, int M, TN *n, TO *off, TO *poff, uint32_t &nx, uint32_t &end) {
    uint32_t pos = pos_chain(R);
    nx = 0u; end = pos;
    for (int k = 0; k < K; ++k) {
        const int v = randint(seed, pos, 1, M);
        if (v < 1 || v > M) return FJSP_E_FORMAT;
        n[k] = (TN)v; off[k] = (TO)(pos + 1u);
        pos += 1u + (uint32_t)v; nx += (uint32_t)v;
    }
    for (int k = 0; k < K; ++k) { poff[k] = (TO)pos; pos += (uint32_t)n[k]; }
    end = pos;
    return 0;
}
// One operation type: choice(M, n, replace=False) as a Fisher-Yates prefix into list[0..n) with zeros behind it (list holds
// M elements), the processing times in list order into p[0..M) (0 = ineligible).  Returns time_rj, their mean (:78).
template <class TL, class TP> FJSP_GEN_FN double operation_type(uint64_t seed, int M, int n, uint32_t off, uint32_t poff, int p_min, int p_max, TL *list, TP *p) {
    for (int m = 0; m < M; ++m) { list[m] = (TL)m; p[m] = (TP)0; }
    for (int i = 0; i < n; ++i) {
        int j = randint(seed, off + (uint32_t)i, i, M - 1);
        j = j < i ? i : (j > M - 1 ? M - 1 : j);
        const TL t = list[i]; list[i] = list[j]; list[j] = t;
    }
    long sum = 0;
    for (int i = 0; i < n; ++i) {
        const int pv = randint(seed, poff + (uint32_t)i, p_min, p_max);
        p[list[i]] = (TP)pv; sum += pv;
    }
    for (int m = n; m < M; ++m) list[m] = (TL)0;
    return (double)sum / (double)n;
}
// One order s: its gap summed strictly left to right over the operation types (:81-82; kind_of[k] is type k's kind, count
// the order's own row), its arrival time the truncated running sum of the intervals, accumulated from order 0 again
// (:85-86; interval[0] = 0.0 and 0.0 + 0.0 is 0.0).  Returns arrive + gap, the delivery time before the sort.
template <class TC, class TK> FJSP_GEN_FN double order(uint64_t seed, int s, int S, int R, int K, int M, double DDT, uint32_t chain_end, double t_si_min, double t_si_max,
                         const double *time_rj, const TC *count, const TK *kind_of, int &arrive) {
    double acc = 0.0, t = 0.0;
    for (int k = 0; k < K; ++k) acc = acc + time_rj[k] * (double)count[kind_of[k]];
    for (int q = 1; q <= s; ++q) t = t + uniform(seed, pos_interval(chain_end, S, R, q), t_si_min, t_si_max);
    arrive = (int)t;
    return (double)arrive + acc * DDT / (double)(M * 2);
}
// :87-88 the delivery times sorted ascending, then truncated.  An insertion sort: S is small, equal keys are equal values.
template <class TD> FJSP_GEN_FN void sort_deliveries(double *dl, int S, TD *delivery) {
    for (int i = 1; i < S; ++i) {
        const double v = dl[i];
        int j = i - 1;
        for (; j >= 0 && dl[j] > v; --j) dl[j + 1] = dl[j];
        dl[j + 1] = v;
    }
    for (int s = 0; s < S; ++s) delivery[s] = (TD)(int)dl[s];
}
// The operation types eligible on machine m (rows of `stride` elements); 0: SO_DFJSP and MO_DFJSP cannot play the shop
template <class TP> FJSP_GEN_FN int operations_on_machine(const TP *p, int stride, int K, int m) {
    int n = 0;
    for (int k = 0; k < K; ++k) n += p[k * stride + m] > 0 ? 1 : 0;
    return n;
}

// ---- the machine data of an MO_DFJSP shop, ms = machine_stream(the seed the shop was made of)
FJSP_GEN_FN int idle_power(uint64_t ms, int m, const fjsp_gen_machine &g) { return randint(ms, pos_idle_power(m), g.idle_min, g.idle_max); }
FJSP_GEN_FN int power(uint64_t ms, int M, int q, const fjsp_gen_machine &g) { return randint(ms, pos_power(M, q), g.pw_min, g.pw_max); }
FJSP_GEN_FN int window_count(uint64_t ms, int M, int m, const fjsp_gen_machine &g) {
    const int n = randint(ms, pos_window_count(M, m), 0, g.W_max);
    return n < 0 ? 0 : (n > g.W_max ? g.W_max : n);
}
// window w of machine m from the end of the one before it (0 in front of the first): its start; `end` moves to its end
FJSP_GEN_FN int window(uint64_t ms, int M, int K, int m, int w, const fjsp_gen_machine &g, int &end) {
    const uint32_t pos = pos_window(M, K, g.W_max, m, w);
    const int st = end + randint(ms, pos, g.gap_min, g.gap_max);
    end = st + randint(ms, pos + 1u, g.len_min, g.len_max);
    return st;
}

}  // namespace fjsp::gen
