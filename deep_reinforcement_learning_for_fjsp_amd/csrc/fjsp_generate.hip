// Training instances generated ON THE DEVICE: fjsp_env_create_generated / fjsp_env_regenerate (include/fjsp_amd.h).
//
// The host path of a fresh batch is fjsp_instances_generate (fjsp_instance.cpp), fjsp_instances_solve_fluid (the order-0
// fluid LP, fjsp_lp.cpp), pack_instance (fjsp_env.hip), two uploads and a new allocation.  A generated handle owns its
// instance records and refills them in place from a seed:
//   generate_pack_kernel    record i from (seed_base + i, parameters): byte for byte what pack_instance(generate(...)) writes,
//                           except x and the static state row, which need the LP; the LP inputs (Q, n_now); and on which
//                           of two lists the instance goes -- its order-0 tableau fits the LDS of a CU, or it does not;
//                           under FJSP_LP_IMPL=global of three: fits the LDS, within the limits of the global-memory simplex
//                           (256 rows x 1536 columns), neither
//   lp_device_kernel        (fjsp_lp_device.hip, unchanged) over the fitting list, in bounded chunks of staging slots
//   lp_global_kernel        (fjsp_lp_global.hip) over the second of the three lists, on the second stream, in bounded chunks
//   solve_fluid_lp          (fjsp_lp.cpp) on the handle's host threads for the last list: the solvers are pivot for pivot the same
//   generate_finish_kernel  x from the staging slot into the record, the static state row
//   fluid_tables_kernel, reset_kernel (fjsp_kernels.hip, unchanged), every env marked done: the state a create leaves
//
// The generator itself -- the stream, the position of every draw, the arithmetic that makes a shop of the draws -- is
// fjsp_gen_stream.h, which fjsp_instance.cpp compiles too; the kernels here spread its element functions over a wave, one
// wave per instance.  Draw i is a pure function of (seed, i): lane 0 walks the one serial chain there is (K dependent
// hashes), the lanes then take their own operation types from the chain's offsets and write the record's rows side by side.
// (One lane per instance would leave the per-type machine lists in scratch memory and the record writes uncoalesced.)
//
// Several orders (fjsp_env_create_generated_orders): lane s computes order s, lane 0 sorts the at most FJSP_GEN_MAX_ORDERS
// delivery times.  The handle is then a multi-order one: its arrival service (fjsp_arrivals.hip) is chosen at create from
// the parameters' worst tableau and, where it runs on the host, reads fjsp_env::lp_mirror, the records' heads that
// refresh_lp_mirror gathers after every refill.
//
// MO_DFJSP (fjsp_env_create_generated_dynamic): the same kernel built with its redraw loop -- an attempt whose shop leaves a
// machine without an eligible operation is drawn again from the next seed of the instance's redraw stream, at most
// GenDynArgs::redraws times -- and generate_machine_kernel behind it: the machine data of the seed the instance was made of,
// every draw at a position of its own, so the lanes need no chain but the running end of a machine's own windows.  The other
// handles launch neither.
//
// Part of a batch (fjsp_env_regenerate_masked): generate_list_kernel compacts a mask over the instances -- or the envs' done
// flags -- into an ascending list, generate_clear_kernel zeroes the listed records and their envs' in place of the whole
// refill's memsets, and the kernels above run over the list: every other record keeps its bytes and its envs play on.  Every
// instance is made of its own seed (GenArgs::seeds), which the snapshot fingerprint follows (gen_hash).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>

#include "fjsp_env_impl.h"
#include "fjsp_gen_stream.h"
#include "fjsp_launch.h"
#include "fjsp_lp_pool.h"
#include "fjsp_lp_limits.h"

#pragma clang fp contract(off)

namespace fjsp {

// per instance, written by generate_pack_kernel and read back by the host in the call's one synchronisation
struct GenInfo {
    int32_t status;      // 0 or a negative FJSP_E_* code
    int32_t K, R, nj;    // operation types, kinds, jobs
    int32_t nx;          // eligible (operation type, machine) pairs
    int32_t lds;         // LDS bytes of the order-0 tableau (lp_device_lds_bytes, fjsp_lp_limits.h)
    int32_t ops;         // operations (schedule slots), of all orders as nj
    int32_t delivery;    // delivery time of the first order due (every order's: GenArgs::deliv)
    int32_t M, S;        // machines and orders of the instance (its own draws on a ranges / orders handle)
    double ddt;          // its due-date tightness
};
static_assert(sizeof(GenInfo) == 48, "GenInfo is twelve words");

// The words of GenArgs::counts, shared by the kernels and the host: the lengths of fit_ids and of host_ids, the largest fitting
// tableau (bytes of LDS), the first instance whose LP left no rate (0xFFFFFFFF: none), the length of glob_ids, the length of
// GenArgs::list (a masked refill: generate_list_kernel)
enum GenCount : int { kCountFit, kCountHost, kCountLdsMax, kCountFailed, kCountGlob, kCountListed, kGenCounts };

struct GenArgs {
    fjsp_gen_params g;       // ranged: g.M and g.DDT are not read
    int32_t ranged;          // 1: M and DDT of instance `seed` are draws 0 and 1 of the stream seed ^ FJSP_GEN_AUX_STREAM (fjsp_gen_ranges)
    int32_t M_min, M_max;
    double DDT_min, DDT_max;
    int32_t orders;          // 1: S of instance `seed` is draw 2 of that stream (fjsp_gen_orders); 0: one order
    int32_t S_min, S_max;
    uint64_t seed_base;
    int32_t class_fjsp;      // SO_DFJSP: the order's delivery time is every job's due date, every machine needs an operation
    int32_t allow_device;    // 0: every LP goes to the host list (FJSP_LP_IMPL=host)
    int32_t kmax;            // operation types of the largest possible instance: stride of the eligible-list rows
    int32_t RP;
    uint8_t *elig;           // [n_inst][kmax][MP] machine_rj_dict in FILE order (zeros behind each list)
    int32_t *deliv;          // [n_inst][SP] delivery_s, ascending: the record keeps the jobs' due dates only
    GenInfo *info;           // [n_inst]
    uint32_t *counts;        // [kGenCounts], by GenCount
    uint32_t *fit_ids;       // [n_inst] instances whose LP runs on the device, in arrival order
    uint32_t *host_ids;      // [n_inst] the others
    uint16_t *lp_in;         // [slot of fit_ids][2][KP] (Q, n_now), lp_device_kernel's format
    // FJSP_LP_IMPL=global: the third list -- tableaus beyond the LDS rule and within kLpGlobalRows x kLpGlobalColumns;
    // its length is counts[kCountGlob]
    int32_t allow_global;
    uint32_t *glob_ids;      // [n_inst]
    uint16_t *lp_in_glob;    // [slot of glob_ids][2][KP]
    // every instance is made of its own seed: seed_base + i of the call that made it last
    uint64_t *seeds;         // [n_inst]
    // a masked refill (fjsp_env_regenerate_masked): the instances it makes, ascending, counts[kCountListed] of them; the
    // generator kernels then run one wave per listed instance.  nullptr: every instance
    const uint32_t *list;
};

// What a dynamic handle's kernels take beside GenArgs (whose class_fjsp is 1 there: MO_DFJSP shares SO_DFJSP's due dates and
// its need of an operation on every machine)
struct GenDynArgs {
    fjsp_gen_machine mc;
    int32_t redraws;         // further attempts for an instance with an idle machine, at most FJSP_GEN_MAX_REDRAWS
    int32_t windows;         // window pairs a record's i_bk holds (Shape::B = M_max x W_max)
    uint64_t *seed_used;     // [n_inst] the seed the instance was made of
};

constexpr int kGenMaxK = kWave * kMaxKC;

namespace {
// M, DDT and S of instance `seed`: the handle's own, or the instance's draws of the auxiliary stream
__device__ inline int gen_machines(const GenArgs &a, uint64_t seed) { return a.ranged ? gen::aux_machines(seed, a.M_min, a.M_max) : a.g.M; }
__device__ inline double gen_ddt(const GenArgs &a, uint64_t seed) { return a.ranged ? gen::aux_ddt(seed, a.DDT_min, a.DDT_max) : a.g.DDT; }
__device__ inline int gen_orders(const GenArgs &a, uint64_t seed) { return a.orders ? gen::aux_orders(seed, a.S_min, a.S_max) : 1; }
constexpr int kGenMaxS = FJSP_GEN_MAX_ORDERS;
// The words of generate_pack's s_hdr: what lane 0 leaves for the wave (the first draw behind the chain, where the job counts
// start; jobs and operations of all orders; the delivery time of the first order due), and the slot the instance got on its LP list
enum GenHdr : int { kHdrSlot, kHdrK, kHdrStatus, kHdrNx, kHdrChainEnd, kHdrJobs, kHdrDelivery, kHdrOps, kGenHdrWords };
// The instance of workgroup blockIdx.x of a generator kernel: its own number, or on a masked refill the entry of the list;
// -1: none (the grid covers every instance, the list's length stays on the device until the call's one read-back)
__device__ inline int gen_listed(const DevBatch &b, const GenArgs &a) {
    const uint32_t slot = blockIdx.x;
    if (slot >= (uint32_t)b.n_inst || (a.list && slot >= a.counts[kCountListed])) return -1;
    const uint32_t inst = a.list ? a.list[slot] : slot;
    return inst < (uint32_t)b.n_inst ? (int)inst : -1;
}
}  // namespace

// One wave per instance.  DYN (a dynamic handle, d given): the shop is drawn again, from the next seed of the instance's
// redraw stream, while it leaves a machine idle and attempts remain; without DYN there is one attempt and no loop is compiled.
template <bool DYN>
__device__ __forceinline__ void generate_pack(const DevBatch &b, const GenArgs &a, const GenDynArgs *d) {
    __shared__ uint8_t s_el[kGenMaxK * kMaxM];       // the shuffle of operation type k, then its eligible list
    __shared__ uint16_t s_p[kGenMaxK * kMaxM];       // p[k][m], 0 = ineligible
    __shared__ double s_tr[kGenMaxK];                // time_rj: mean processing time over the eligible list
    __shared__ uint32_t s_off[kGenMaxK], s_poff[kGenMaxK];   // first shuffle draw / first processing-time draw of type k
    __shared__ uint16_t s_rk[kGenMaxK], s_koff[kGenMaxK + 1], s_jbeg[kGenMaxK + 1];
    __shared__ uint16_t s_cnt[kGenMaxS * kGenMaxK];  // count[s][r] at s * kGenMaxK + r: order 0 in front
    __shared__ uint16_t s_tot[kGenMaxK];             // jobs of kind r over all orders
    __shared__ uint8_t s_n[kGenMaxK], s_jk[kGenMaxK], s_Jr[kGenMaxK];
    __shared__ int32_t s_hdr[kGenHdrWords];          // by GenHdr
    __shared__ double s_dl[kGenMaxS];                // arrive + gap of order s, then sorted
    __shared__ int32_t s_arr[kGenMaxS], s_del[kGenMaxS];     // time_arrive_s, delivery_s (ascending)
    const int l = (int)threadIdx.x, inst = gen_listed(b, a);
    if (inst < 0) return;
    const fjsp_gen_params &g = a.g;
    const uint64_t seed0 = a.seeds[inst];
    const int MP = b.MP, KP = b.KP;
    unsigned char *rec = b.inst + (size_t)inst * b.L.i_stride;
    const Layout &L = b.L;
    const int redraws = DYN ? (d->redraws < FJSP_GEN_MAX_REDRAWS ? d->redraws : FJSP_GEN_MAX_REDRAWS) : 0;     // the loop's hard bound
    uint64_t seed = seed0;
    int M, S, R, K, nx, status, nj, delivery, ops_m;
    double DDT;
    for (int attempt = 0;; ++attempt) {
        if (DYN && attempt > 0) {
            seed = gen::attempt_seed(seed0, attempt);
            __syncthreads();                         // the lanes have read the last attempt's shop
        }
        M = gen_machines(a, seed); S = gen_orders(a, seed); DDT = gen_ddt(a, seed);
        // ---- R, J_r, the kinds' first operation types
        R = gen::randint(seed, gen::pos_kinds(), g.R_min, g.R_max);
        const bool r_ok = R >= 1 && R <= a.RP && R <= kGenMaxK && M >= 1 && M <= MP && M <= kMaxM && S >= 1 && S <= b.SP && S <= kGenMaxS;
        for (int r = l; r_ok && r < R; r += kWave) s_Jr[r] = (uint8_t)gen::randint(seed, gen::pos_operations(r), g.J_min, g.J_max);
        __syncthreads();
        if (l == 0) {
            int K = 0, st = r_ok ? 0 : FJSP_E_FORMAT;
            for (int r = 0; st == 0 && r < R; ++r) {
                const int J = s_Jr[r];
                if (J < 1 || K + J > KP || K + J > a.kmax) { st = FJSP_E_FORMAT; break; }
                s_koff[r] = (uint16_t)K;
                for (int j = 0; j < J; ++j) { s_rk[K + j] = (uint16_t)r; s_jk[K + j] = (uint8_t)j; }
                K += J;
            }
            uint32_t nx = 0, end = 0;
            if (st == 0) s_koff[R] = (uint16_t)K;
            if (st == 0) st = gen::chain(seed, R, K, M, s_n, s_off, s_poff, nx, end);      // the one serial chain
            s_hdr[kHdrK] = K; s_hdr[kHdrStatus] = st; s_hdr[kHdrNx] = (int)nx; s_hdr[kHdrChainEnd] = (int)end;
        }
        __syncthreads();
        K = s_hdr[kHdrK]; nx = s_hdr[kHdrNx]; status = s_hdr[kHdrStatus];
        const uint32_t chain_end = (uint32_t)s_hdr[kHdrChainEnd];
        if (status != 0) {
            if (l == 0) a.info[inst] = GenInfo{status, 0, 0, 0, 0, 0, 0, 0, M, S, DDT};
            return;
        }
        for (int k = l; k < K; k += kWave)          // per operation type: its eligible list, its processing times
            s_tr[k] = gen::operation_type(seed, M, s_n[k], s_off[k], s_poff[k], g.p_min, g.p_max, s_el + k * kMaxM, s_p + k * kMaxM);
        for (int q = l; q < S * R; q += kWave)      // the S x R job counts, order-major
            s_cnt[(q / R) * kGenMaxK + q % R] = (uint16_t)gen::randint(seed, gen::pos_count(chain_end, q), g.N_min, g.N_max);
        __syncthreads();
        if (l < S) s_dl[l] = gen::order(seed, l, S, R, K, M, DDT, chain_end, g.t_si_min, g.t_si_max, s_tr, s_cnt + l * kGenMaxK, s_rk, s_arr[l]);
        __syncthreads();
        if (l == 0) {
            int nj = 0, ops = 0;
            for (int r = 0; r < R; ++r) {
                int tot = 0;
                for (int so = 0; so < S; ++so) tot += s_cnt[so * kGenMaxK + r];
                s_jbeg[r] = (uint16_t)nj; s_tot[r] = (uint16_t)tot; nj += tot; ops += tot * (int)s_Jr[r];
            }
            s_jbeg[R] = (uint16_t)nj;
            gen::sort_deliveries(s_dl, S, s_del);
            s_hdr[kHdrJobs] = nj; s_hdr[kHdrDelivery] = s_del[0]; s_hdr[kHdrOps] = ops;
            if (nj > b.JP || nj > 65535) s_hdr[kHdrStatus] = FJSP_E_FORMAT;
        }
        __syncthreads();
        nj = s_hdr[kHdrJobs]; delivery = s_hdr[kHdrDelivery]; status = s_hdr[kHdrStatus];
        // SO_DFJSP and MO_DFJSP divide by the number of operation types of every machine (check_instance, fjsp_env.hip)
        ops_m = l < M ? gen::operations_on_machine(s_p, kMaxM, K, l) : 0;
        if (a.class_fjsp && __any(l < M && ops_m == 0) && status == 0) status = FJSP_E_UNSUPPORTED;
        if (!DYN || status != FJSP_E_UNSUPPORTED || attempt >= redraws) break;
    }
    if (DYN && l == 0) d->seed_used[inst] = seed;
    const uint32_t lds = lp_device_lds_bytes(K, M, nx, R, MP);
    if (l == 0) a.info[inst] = GenInfo{status, K, R, nj, nx, (int32_t)lds, s_hdr[kHdrOps], delivery, M, S, DDT};
    if (status != 0) return;

    // ---- the record (pack_instance, fjsp_env.hip); the slab was zeroed before the launch
    if (l == 0) *reinterpret_cast<InstHeader *>(rec) = InstHeader{K, M, R | (b.mord ? S << 16 : 0), nj};
    if (l < S) {
        reinterpret_cast<int32_t *>(rec + L.i_oarr)[l] = s_arr[l];
        a.deliv[(size_t)inst * (size_t)b.SP + l] = s_del[l];
    }
    uint16_t *ocnt = reinterpret_cast<uint16_t *>(rec + L.i_ocnt);
    uint32_t *kA = reinterpret_cast<uint32_t *>(rec + L.i_kA), *kB = reinterpret_cast<uint32_t *>(rec + L.i_kB);
    uint32_t *elig = reinterpret_cast<uint32_t *>(rec + L.i_elig), *first4 = reinterpret_cast<uint32_t *>(rec + L.i_f4);
    uint32_t *jinfo = reinterpret_cast<uint32_t *>(rec + L.i_jinfo);
    int32_t *due = reinterpret_cast<int32_t *>(rec + L.i_due);
    uint16_t *p = reinterpret_cast<uint16_t *>(rec + L.i_p);
    uint8_t *el_out = a.elig + (size_t)inst * (size_t)a.kmax * (size_t)MP;
    for (int r = l; r < R; r += kWave) {
        const int J = s_Jr[r], jb = s_jbeg[r];
        // the jobs of kind r over all orders in arrival order; class_FJSSP.py:214-218 with Python's round (half to even: rint in
        // the default rounding mode), the ABSOLUTE job number n and the order's own count
        int cnt = 0;
        for (int so = 0; so < S; ++so) {
            const int c = s_cnt[so * kGenMaxK + r], dl = s_del[so];
            ocnt[(size_t)so * b.RP + r] = (uint16_t)c;
            const long r_due = (long)rint((double)((long)dl * J) / (double)c);
            for (int n = cnt; n < cnt + c; ++n) {
                due[jb + n] = a.class_fjsp ? dl : (int32_t)(long)rint((double)(r_due * n) / (double)c);
                jinfo[jb + n] = (uint32_t)s_koff[r] | ((uint32_t)J << 16);
            }
            cnt += c;
        }
    }
    for (int k = l; k < K; k += kWave) {
        const int r = s_rk[k], j = s_jk[k], J = s_Jr[r], n = s_n[k];
        kA[k] = (uint32_t)s_jbeg[r] | ((uint32_t)s_tot[r] << 16);
        kB[k] = (uint32_t)j | ((uint32_t)J << 8) | ((uint32_t)(r & 0xFF) << 16) | ((uint32_t)((j == J - 1 ? 1u : 0u) | 2u) << 24);
        uint32_t em = 0, f4 = 0;
        for (int m = 0; m < M; ++m) {
            const uint16_t pv = s_p[k * kMaxM + m];
            if (pv > 0) em |= 1u << m;
            p[(size_t)k * MP + m] = pv;
            el_out[(size_t)k * MP + m] = s_el[k * kMaxM + m];
        }
        for (int q = 0; q < n && q < 4; ++q) f4 |= (uint32_t)s_el[k * kMaxM + q] << (8 * q);
        elig[k] = em;
        first4[k] = f4;
    }
    if (b.grp && l < 16) {
        // the row kernels' head line (pack_instance): one job per kind there, job index == kind index, the job's number is 0
        uint32_t w = l < M ? (uint32_t)ops_m : 0u;
        if (l < R) {
            w |= (uint32_t)s_koff[l] << 8; w |= (uint32_t)s_Jr[l] << 16;
            const int c = s_cnt[l];
            const long r_due = (long)rint((double)((long)delivery * s_Jr[l]) / (double)c);
            reinterpret_cast<int32_t *>(rec + L.i_op + 2048 + 64)[l] = a.class_fjsp ? delivery : (int32_t)(long)rint((double)(r_due * 0) / (double)c);
        }
        w |= (uint32_t)(l == 0 ? K : (l == 1 ? M : (l == 2 ? nj : 0))) << 24;
        reinterpret_cast<uint32_t *>(rec + L.i_op + 2048)[l] = w;
    }
    // ---- the order-0 LP: Q[k] = count[r], n_now[k] = (j == 0 ? count[r] : 0) (solve_order0), and where it is solved
    // (nc is lp_max_columns and nc - nx - 2 is lp_max_rows of fjsp_lp_limits.h, in the wave's own integer arithmetic)
    const int nc = nx + 1 + (K + M + K - R) + 1;
    const bool fit = a.allow_device && lds <= kLpLdsLimit && nc <= kLpLdsColumns;
    const bool glob = !fit && a.allow_global && nc - nx - 2 <= kLpGlobalRows && nc <= kLpGlobalColumns;
    if (l == 0) {
        if (fit) {
            s_hdr[kHdrSlot] = (int)atomicAdd(a.counts + kCountFit, 1u);
            atomicMax(a.counts + kCountLdsMax, lds);
        } else if (glob) {
            s_hdr[kHdrSlot] = (int)atomicAdd(a.counts + kCountGlob, 1u);
        } else {
            a.host_ids[atomicAdd(a.counts + kCountHost, 1u)] = (uint32_t)inst;
        }
    }
    __syncthreads();
    if (fit || glob) {
        const uint32_t slot = (uint32_t)s_hdr[kHdrSlot];
        if (l == 0) (fit ? a.fit_ids : a.glob_ids)[slot] = (uint32_t)inst;
        uint16_t *Q = (fit ? a.lp_in : a.lp_in_glob) + (size_t)slot * 2 * KP;
        for (int k = l; k < K; k += kWave) {
            const uint16_t c = s_cnt[s_rk[k]];      // order 0's count, not the kind's total
            Q[k] = c;
            Q[KP + k] = s_jk[k] == 0 ? c : (uint16_t)0;
        }
    }
}

__global__ __launch_bounds__(kWave) void generate_pack_kernel(DevBatch b, GenArgs a) { generate_pack<false>(b, a, nullptr); }
__global__ __launch_bounds__(kWave) void generate_pack_dynamic_kernel(DevBatch b, GenArgs a, GenDynArgs d) { generate_pack<true>(b, a, &d); }

// One wave per instance of a dynamic handle, behind generate_pack_dynamic_kernel: the machine data of the seed the instance was
// made of into the record, as pack_instance writes them (i_pw, i_ipw, i_bkoff, i_bk; the due-date tightness in front of
// the static state row).  K, M and the eligible pairs are the record's.
__global__ __launch_bounds__(kWave) void generate_machine_kernel(DevBatch b, GenArgs a, GenDynArgs d) {
    __shared__ uint16_t s_w[kMaxM];                  // windows of machine m
    const int l = (int)threadIdx.x, inst = gen_listed(b, a);
    if (inst < 0 || a.info[inst].status != 0) return;
    unsigned char *rec = b.inst + (size_t)inst * b.L.i_stride;
    const InstHeader h = *reinterpret_cast<const InstHeader *>(rec);
    const int K = h.K, M = h.M, MP = b.MP, W = d.mc.W_max;
    if (K < 1 || K > b.KP || M < 1 || M > MP || MP > kMaxM || W < 0 || M * W > d.windows) return;     // (generate_pack's own checks; the size of i_bk)
    const uint64_t ms = gen::machine_stream(d.seed_used[inst]);
    const uint16_t *p = reinterpret_cast<const uint16_t *>(rec + b.L.i_p);
    uint16_t *pw = reinterpret_cast<uint16_t *>(rec + b.L.i_pw);
    for (int q = l; q < K * M; q += kWave) {
        const size_t at = (size_t)(q / M) * MP + q % M;
        pw[at] = p[at] > 0 ? (uint16_t)gen::power(ms, M, q, d.mc) : (uint16_t)0;
    }
    if (l < M) {
        reinterpret_cast<int32_t *>(rec + b.L.i_ipw)[l] = gen::idle_power(ms, l, d.mc);
        s_w[l] = (uint16_t)gen::window_count(ms, M, l, d.mc);
    }
    __syncthreads();
    if (l <= MP) {
        // the first window of machine l: the windows of the machines in front of it (i_bkoff[MP] = all of them)
        int off = 0;
        for (int m = 0; m < l && m < M; ++m) off += s_w[m];
        reinterpret_cast<uint16_t *>(rec + b.L.i_bkoff)[l] = (uint16_t)off;
        if (l < M) {
            int32_t *bk = reinterpret_cast<int32_t *>(rec + b.L.i_bk) + 2 * off;
            for (int w = 0, end = 0; w < (int)s_w[l]; ++w) {
                bk[2 * w] = gen::window(ms, M, K, l, w, d.mc, end);
                bk[2 * w + 1] = end;
            }
        }
    }
    if (l == 0) reinterpret_cast<double *>(rec + b.L.i_ss)[0] = a.info[inst].ddt;      // observation[0] = self.DDT
}

// One wave per listed instance: x from its staging slot into the record, then the static state row (pack_static_state).
__global__ __launch_bounds__(kWave) void generate_finish_kernel(DevBatch b, GenArgs a, const uint32_t *ids, int count, const double *stage) {
    __shared__ double s_v[kGenMaxK];
    const int slot = (int)blockIdx.x, l = (int)threadIdx.x;
    if (slot >= count) return;
    const int inst = (int)ids[slot];
    unsigned char *rec = b.inst + (size_t)inst * b.L.i_stride;
    const InstHeader h = *reinterpret_cast<const InstHeader *>(rec);
    const int K = h.K, M = h.M, MP = b.MP, KP = b.KP;
    const double *xs = stage + (size_t)slot * KP * MP;
    double *x = reinterpret_cast<double *>(rec + b.L.i_x);
    for (int q = l; q < K * MP; q += kWave) x[q] = xs[q];
    const uint16_t *p = reinterpret_cast<const uint16_t *>(rec + b.L.i_p);
    const uint32_t *kA = reinterpret_cast<const uint32_t *>(rec + b.L.i_kA), *kB = reinterpret_cast<const uint32_t *>(rec + b.L.i_kB);
    const uint32_t *elig = reinterpret_cast<const uint32_t *>(rec + b.L.i_elig);
    const uint8_t *el = a.elig + (size_t)inst * (size_t)a.kmax * (size_t)MP;
    // fluid_completed_time = max_k Q_k / rate_k, rate_k summed over machine_rj_dict in FILE order (class_FJSSP.py:276-278)
    for (int k = l; k < K; k += kWave) {
        const int n = __builtin_popcount(elig[k]);
        double acc = 0.0;
        for (int q = 0; q < n; ++q) {
            const int m = el[(size_t)k * MP + q];
            acc = acc + xs[(size_t)k * MP + m] * (1.0 / (double)p[(size_t)k * MP + m]);
        }
        s_v[k] = acc;
    }
    __syncthreads();
    if (l != 0) return;
    double *ss = reinterpret_cast<double *>(rec + b.L.i_ss);
    // (Q_k is the count of the kind in order 0 -- i_ocnt's first row; kA >> 16 is the kind's total over all orders)
    const uint16_t *ocnt = reinterpret_cast<const uint16_t *>(rec + b.L.i_ocnt);
    double best = 0.0;
    bool lp_ok = true;
    for (int k = 0, r = -1; k < K; ++k) {
        if ((kB[k] & 0xFFu) == 0u) ++r;                      // a kind's first operation type
        if (!(s_v[k] > 0.0)) lp_ok = false;                  // a failed LP leaves x = 0: no fluid rate
        const double v = (double)ocnt[r] / s_v[k];
        if (k == 0 || v > best) best = v;
    }
    ss[7] = best;
    if (!lp_ok) atomicMin(a.counts + kCountFailed, (uint32_t)inst);
    if (b.variant == FJSP_VARIANT_MO_FJSSP_DISCRETES) {
        // MO_FJSSP_discretes.py:55-64 static_state_extract; the host's pow(d, 2.0) is d * d here
        long ns = 0, js = 0;
        int R = 0;
        for (int k = 0; k < K; ++k)
            if ((kB[k] & 0xFFu) == 0u) { ns += (long)(kA[k] >> 16); js += (long)((kB[k] >> 8) & 0xFFu); ++R; }
        const double N_ave = (double)ns / (double)R, J_ave = (double)js / (double)R;
        double va = 0.0, vc = 0.0;
        for (int k = 0; k < K; ++k)
            if ((kB[k] & 0xFFu) == 0u) { const double d = (double)(kA[k] >> 16) - N_ave; va = va + d * d; }
        for (int k = 0; k < K; ++k)
            if ((kB[k] & 0xFFu) == 0u) { const double d = (double)((kB[k] >> 8) & 0xFFu) - J_ave; vc = vc + d * d; }
        ss[0] = gen_ddt(a, a.seeds[inst]); ss[1] = (double)M; ss[2] = (double)R; ss[3] = N_ave;
        ss[4] = sqrt(va / (double)R); ss[5] = J_ave; ss[6] = sqrt(vc / (double)R);
    }
}

// The head of the listed instances' records (everything in front of x), side by side: the host route's one read-back.
// A multi-order handle's rows carry `tail` more words from word tail0 on: the orders' counts (i_oarr, i_ocnt), which lie
// behind x.  ids == nullptr: instances 0 .. count - 1.
__global__ __launch_bounds__(256) void generate_gather_kernel(DevBatch b, const uint32_t *ids, int count, uint4 *out, int head, int tail0, int tail) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, words16 = (size_t)(head + tail);
    if (idx >= (size_t)count * words16) return;
    const int slot = (int)(idx / words16), w = (int)(idx % words16);
    const size_t inst = ids ? (size_t)ids[slot] : (size_t)slot;
    out[idx] = reinterpret_cast<const uint4 *>(b.inst + inst * b.L.i_stride)[w < head ? w : tail0 + (w - head)];
}

// Every env as a create leaves it: done, so that a step before the reset is flagged; the row kernels' per-env operation count.
// env_mask != nullptr (a masked refill): the envs it marks alone.
__global__ __launch_bounds__(256) void generate_mark_done_kernel(DevBatch b, uint8_t *kenv, const uint8_t *env_mask) {
    const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (env >= b.N || (env_mask && env_mask[env] == 0)) return;
    env_ptr<EnvScalars>(b, env, 0)->done = 1;
    if (kenv) kenv[env] = (uint8_t)inst_ptr<const InstHeader>(b, env % b.n_inst, 0)->K;
}

// Every instance's seed of a whole refill.
__global__ __launch_bounds__(256) void generate_seeds_kernel(DevBatch b, GenArgs a) {
    const int inst = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (inst < b.n_inst) a.seeds[inst] = a.seed_base + (uint64_t)inst;
}

// A masked refill's list, by one workgroup of sixteen waves over tiles of 1024 instances: instance i is on iff mask[i] != 0 --
// mask == nullptr: iff every env that plays it is done -- or pending[i] != 0 (the instances a failed call left half made).
// A wave's ballot gives a lane its place among the wave's, the waves' counts in LDS its wave's place in the tile, the
// running sum the tile's: the list is ascending and takes no atomics.  Also the seeds of the listed instances, the mask that
// was applied (refreshed, u8[n_inst], nullable), the same per env (env_mask, u8[N]: launch_reset's mask) and the list's
// length.
__global__ __launch_bounds__(1024) void generate_list_kernel(DevBatch b, GenArgs a, const uint8_t *mask, const uint8_t *pending, uint32_t *list,
                                                            uint8_t *refreshed, uint8_t *env_mask) {
    __shared__ uint32_t s_wave[16];
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
    uint32_t base = 0;
    for (int i0 = 0; i0 < b.n_inst; i0 += 1024) {
        const int i = i0 + t;
        bool on = false;
        if (i < b.n_inst) {
            if (mask) on = mask[i] != 0;
            else {
                on = true;
                for (int q = i; q < b.N; q += b.n_inst) on = on && env_ptr<const EnvScalars>(b, q, 0)->done != 0;
            }
            if (pending && pending[i] != 0) on = true;
        }
        const unsigned long long bal = __ballot(on);
        if (lane == 0) s_wave[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < 16; ++w) { const uint32_t c = s_wave[w]; before += w < wv ? c : 0u; total += c; }
        if (i < b.n_inst) {
            if (on) {
                list[base + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)i;
                a.seeds[i] = a.seed_base + (uint64_t)i;
            }
            if (refreshed) refreshed[i] = on ? 1 : 0;
            for (int q = i; q < b.N; q += b.n_inst) env_mask[q] = on ? 1 : 0;
        }
        base += total;
        __syncthreads();          // s_wave is written again
    }
    if (t == 0) a.counts[kCountListed] = base;
}

// One workgroup per listed instance of a masked refill: its record, the records of the envs that play it and their dispatch
// records to zero -- what the whole refill's memsets do to the slabs.
__global__ __launch_bounds__(256) void generate_clear_kernel(DevBatch b, GenArgs a, SchedRec rec) {
    const int t = (int)threadIdx.x, inst = gen_listed(b, a);
    if (inst < 0) return;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    uint4 *ir = reinterpret_cast<uint4 *>(b.inst + (size_t)inst * b.L.i_stride);
    for (uint32_t w = (uint32_t)t; w < b.L.i_stride / 16u; w += 256u) ir[w] = zero;
    for (int q = inst; q < b.N; q += b.n_inst) {
        uint4 *er = reinterpret_cast<uint4 *>(b.envs + (size_t)q * b.L.e_stride);
        for (uint32_t w = (uint32_t)t; w < b.L.e_stride / 16u; w += 256u) er[w] = zero;
        if (rec.rec)
            for (int s = t; s < rec.cap; s += 256) rec.rec[(size_t)s * (size_t)b.N + (size_t)q] = zero;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
struct LpCounters { unsigned long long solved, pivots; };      // what a device simplex counts (launch_lp_device's `solved`)

// One way the order-0 LPs get solved.  generate_pack_kernel puts every instance on one route's list; the host runs each
// list in chunks of GenState::chunk staging slots: its producer leaves x in d_stage, generate_finish_kernel takes it from there.
struct LpRoute {
    enum Producer { kLds, kGlobal, kHost } producer = kLds;     // lp_device_kernel; lp_global_kernel; gather, solve on host threads, upload
    GenCount length = kCountFit;      // the counts word that holds the list's length
    const char *launch_error = "";    // when a launch of the route fails
    uint32_t *ids = nullptr;          // the list, on the device
    uint16_t *lp_in = nullptr;        // [slot of ids][2][KP] (Q, n_now): device routes
    double *d_stage = nullptr;        // [chunk][KP][MP] x; nullptr: the handle has no such route
    LpCounters *d_solved = nullptr, *h_solved = nullptr;    // device routes: the kernel's counters and where the host reads them
    hipStream_t st = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;        // device routes: the time of their launches (the first route's begins at ev_packed)
    bool present() const { return d_stage != nullptr; }
};
enum GenRoute : int { kRouteLds, kRouteGlobal, kRouteHost, kGenRoutes };      // in the order they are started

// The slots of GenState::stats and ::ms (milliseconds), of the last call.  Their values ARE the positions in the arrays that
// fjsp_env_generated_stats (the first four), _times (the first five) and _stats2 (all six) fill: the ABI's order is stated here alone.
enum GenStat : int { kStatInstances, kStatLpLds, kStatLpHost, kStatDevicePivots, kStatLpGlobal, kStatGlobalPivots, kGenStats };
enum GenTime : int { kMsGenerate, kMsLpLds, kMsLpHost, kMsTablesReset, kMsTotal, kMsLpGlobal, kGenTimes };
struct LpErrWord { uint32_t code, unused; };                    // launch_lp_device's `err`: nonzero when an LP failed on the device
struct GenReadback { LpCounters lds, glob; LpErrWord lp_err; };  // pinned: what the host reads of the device simplexes

struct GenState {
    GenArgs a{};
    bool dynamic = false;                // made by fjsp_env_create_generated_dynamic: d is in use
    GenDynArgs d{};
    uint64_t *h_seed_used = nullptr;     // pinned [n_inst], dynamic handles
    LpRoute route[kGenRoutes];
    int chunk = 0;                       // staging slots of one LP launch / one host-route round
    int head16 = 0;                      // 16-byte words of a record in front of x
    int tail0 = 0, tail16 = 0;           // multi-order handles: the words that hold i_oarr and i_ocnt, gathered behind the head
    uint8_t *d_kenv = nullptr;
    uint32_t *d_lp_err = nullptr;
    uint4 *d_head = nullptr, *h_head = nullptr;      // [chunk][head16] record heads of the host route, and pinned
    double *h_stage = nullptr;           // pinned, as all that follow: [chunk][KP][MP] x of the host route
    GenInfo *h_info = nullptr;
    uint32_t *h_counts = nullptr, *h_host_ids = nullptr;
    GenReadback *h_back = nullptr;
    hipEvent_t ev_start = nullptr, ev_packed = nullptr, ev_end = nullptr;
    hipEvent_t ev_joined = nullptr;      // a side route's x has reached the first stream
    hipEvent_t ev_lps = nullptr;         // (not owned) the event on the first stream behind which every device route's x is there
    hipStream_t st_dev = nullptr, st_host = nullptr;       // the first route's stream and the side routes': they run side by side
    int64_t stats[kGenStats] = {};
    double ms[kGenTimes] = {};
    LpGlobalPool pool;                   // FJSP_LP_IMPL=global only (nothing of that route is allocated otherwise)
    // per instance: the seed it was made of last (GenArgs::seeds on the host), and whether a failed call left it half made --
    // the next masked refill takes those too, a whole one takes every instance anyway
    std::vector<uint64_t> seeds;
    std::vector<uint8_t> unfinished;
    // a masked refill (generate_list_kernel): the list and pinned, the applied mask per env, the upload of `unfinished`
    uint32_t *d_list = nullptr, *h_list = nullptr;
    uint8_t *d_env_mask = nullptr, *d_pending = nullptr, *h_pending = nullptr;
};
// What fjsp_env_regenerate_masked passes to the refill; nullptr there: the whole batch
struct MaskedCall { const uint8_t *d_mask; uint8_t *d_refreshed; };

void generated_release(fjsp_env *e) {
    if (!e || !e->gen) return;
    GenState &G = *e->gen;
    for (hipEvent_t ev : {G.ev_start, G.ev_packed, G.ev_end, G.ev_joined, G.route[kRouteLds].ev_end, G.route[kRouteGlobal].ev_begin, G.route[kRouteGlobal].ev_end})
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : {G.st_dev, G.st_host})
        if (st) (void)hipStreamDestroy(st);
    delete e->gen;
    e->gen = nullptr;
}

namespace {
// check_instance (fjsp_env.hip) on the worst case of the parameters, sizes into sh.  Over M in M_min..M_max and |DDT| up to
// ddt_max: sizes from M_max, the largest delivery time from ddt_max / (2 M_min)
// With S_max > 1 orders: jobs, operations and the clock count all of them, the clock starts from the last arrival
// mc != nullptr (MO_DFJSP): every breakdown window stretches the clock (the bk_total term of check_instance)
int check_worst_case(const fjsp_gen_params &g, int M_min, int M_max, double ddt_max, int S_max, const fjsp_gen_machine *mc, Shape &sh) {
    const long long K = (long long)g.R_max * g.J_max, nj = (long long)g.R_max * g.N_max * S_max, ops = K * g.N_max * S_max;
    if (S_max > 1) {
        if (nj > 65535) { set_error("generated instances can have more than 65535 jobs (R_max x N_max x S_max)"); return FJSP_E_UNSUPPORTED; }
        if (ops > 65535) { set_error("generated instances can have more than 65535 operations (R_max x J_max x N_max x S_max)"); return FJSP_E_UNSUPPORTED; }
    }
    if (K > kWave * kMaxKC) { set_error("generated instances can have more than 256 operation types (R_max x J_max)"); return FJSP_E_UNSUPPORTED; }
    if (M_max > kMaxM) { set_error(M_min == M_max ? "more than 32 machines" : "more than 32 machines (M_max)"); return FJSP_E_UNSUPPORTED; }
    if (nj > 65535) { set_error("generated instances can have more than 65535 jobs (R_max x N_max)"); return FJSP_E_UNSUPPORTED; }
    if (ops > 65535) { set_error("generated instances can have more than 65535 operations (R_max x J_max x N_max)"); return FJSP_E_UNSUPPORTED; }
    if (g.J_max > 255) { set_error("more than 255 operations in a kind"); return FJSP_E_UNSUPPORTED; }
    // (a handle with order arrivals keeps 255 in a job's next-stage byte for orders still to come: fjsp_env_create_family)
    if (g.J_max > 254 && (S_max > 1 || mc)) {
        set_error("more than 254 operations in a kind (J_max) of a handle with order arrivals (S_max > 1, MO_DFJSP)");
        return FJSP_E_UNSUPPORTED;
    }
    if (g.p_max > 65535) { set_error("processing time above 65535"); return FJSP_E_UNSUPPORTED; }
    // the 32-bit clocks: every operation in sequence at the largest processing time; the largest delivery time is every
    // operation type at p_max with N_max jobs, times DDT / (2 M)
    // (several orders: the last one arrives at (S_max - 1) t_si_max at the latest, its delivery time lies one order's gap behind
    // that, the work of all orders follows the last arrival, and a kind has N_max jobs in every order)
    const double arrive = S_max > 1 ? (double)(S_max - 1) * g.t_si_max : 0.0;
    const double due = arrive + std::fabs((double)K * (double)g.p_max * (double)g.N_max * ddt_max / (double)(M_min * 2));
    const double windows = mc ? (double)M_max * (double)mc->W_max * (double)mc->len_max : 0.0;
    const double clock = arrive + (double)ops * (double)g.p_max + windows;
    if (!(clock + due <= 2147483647.0) || !((double)g.N_max * (double)S_max * (clock + due) <= 2147483647.0)) {
        set_error(mc ? "generated instances can be too long for the kernels' 32-bit clocks: (last arrival (S_max - 1) x t_si_max + operations "
                       "of all orders x max processing time + every breakdown window M_max x W_max x len_max + largest delivery time) x jobs "
                       "per kind (N_max x S_max) must stay below 2^31"
                  : S_max > 1 ? "generated instances can be too long for the kernels' 32-bit clocks: (last arrival (S_max - 1) x t_si_max + operations "
                              "of all orders x max processing time + largest delivery time) x jobs per kind (N_max x S_max) must stay below 2^31"
                            : "generated instances can be too long for the kernels' 32-bit clocks: (operations x max processing time + "
                              "largest delivery time) x jobs per kind must stay below 2^31; the largest delivery time grows with DDT (DDT_max) "
                              "and shrinks with the machine count (M_min)");
        return FJSP_E_UNSUPPORTED;
    }
    sh.K = (int)K; sh.M = M_max; sh.J = (int)nj; sh.R = g.R_max; sh.S = S_max;
    if (mc) {
        if ((long long)M_max * mc->W_max > 65535) { set_error("generated instances can have more than 65535 breakdown windows (M_max x W_max)"); return FJSP_E_UNSUPPORTED; }
        sh.B = std::max(1, M_max * mc->W_max);
    }
    sh.single_job = g.N_min == 1 && g.N_max == 1 && g.R_max <= 255;
    return FJSP_OK;
}

// The fingerprint of a generated handle's instances: its parameters and its seeds.  Seeds s + i for one s (a create, a whole
// refill, a masked one of every instance) mix s alone; any other seeds a tag and all of them.
uint64_t gen_hash(const GenArgs &a, const GenDynArgs *d, int n_inst, const std::vector<uint64_t> &seeds) {
    const fjsp_gen_params &g = a.g;
    const int class_fjsp = a.class_fjsp;
    uint64_t h = 1469598103934665603ULL;
    auto mix = [&](const void *p, size_t n) {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ULL;
    };
    // (class_fjsp: SO_DFJSP runs as variant SO_FJSSP with other due dates, so the variant alone does not tell the two apart)
    const int32_t iv[12] = {g.R_min, g.R_max, g.J_min, g.J_max, g.M, g.p_min, g.p_max, g.N_min, g.N_max, g.S, n_inst, class_fjsp};
    const double dv[3] = {g.DDT, g.t_si_min, g.t_si_max};
    mix(iv, sizeof(iv)); mix(dv, sizeof(dv));
    bool affine = true;
    for (size_t i = 0; i < seeds.size(); ++i) affine = affine && seeds[i] == seeds[0] + (uint64_t)i;
    if (affine) mix(&seeds[0], sizeof(uint64_t));
    else {
        const int32_t tag = 0x53454544;
        mix(&tag, sizeof(tag)); mix(seeds.data(), seeds.size() * sizeof(uint64_t));
    }
    if (a.ranged) {     // a tag and the ranges: never the fingerprint of a fixed-parameter handle (g.M, g.DDT are zeroed there)
        const int32_t rv[3] = {0x52414E47, a.M_min, a.M_max};
        const double rd[2] = {a.DDT_min, a.DDT_max};
        mix(rv, sizeof(rv)); mix(rd, sizeof(rd));
    }
    if (a.orders) {     // likewise: a tag, the order range and the interval bounds
        const int32_t ov[3] = {0x4F524453, a.S_min, a.S_max};
        const double od[2] = {g.t_si_min, g.t_si_max};
        mix(ov, sizeof(ov)); mix(od, sizeof(od));
    }
    if (d) {            // likewise: a tag, the machine ranges and the redraw bound
        const int32_t tag = 0x44594E4D;
        mix(&tag, sizeof(tag)); mix(&d->mc, sizeof(d->mc)); mix(&d->redraws, sizeof(d->redraws));
    }
    return h;
}

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
double ms_between(hipEvent_t a, hipEvent_t b) { float f = 0.f; (void)hipEventElapsedTime(&f, a, b); return f; }

// The head of a packed record (pack_instance, generate_pack_kernel: everything in front of x) back on the host (RecordHead,
// fjsp_env_impl.h).  ocnt: the record's i_ocnt, whose first row is order 0; nullptr on a one-order handle, where kA >> 16 is it
void decode_head(const DevBatch &b, const unsigned char *rec, const uint16_t *ocnt, RecordHead &o) {
    o.h = *reinterpret_cast<const InstHeader *>(rec);
    o.h.R &= 0xFFFF;                                     // (the order count rides in the high half on a multi-order handle)
    const uint32_t *kA = reinterpret_cast<const uint32_t *>(rec + b.L.i_kA), *kB = reinterpret_cast<const uint32_t *>(rec + b.L.i_kB);
    const uint16_t *p16 = reinterpret_cast<const uint16_t *>(rec + b.L.i_p);
    const size_t K = (size_t)o.h.K, M = (size_t)o.h.M;
    o.Jr.clear(); o.count.clear(); o.p.assign(K * M, 0);
    for (size_t k = 0; k < K; ++k) {
        if ((kB[k] & 0xFFu) == 0u) { o.count.push_back(ocnt ? (int)ocnt[o.Jr.size()] : (int)(kA[k] >> 16)); o.Jr.push_back((int)((kB[k] >> 8) & 0xFFu)); }     // a kind's first operation type
        for (size_t m = 0; m < M; ++m) o.p[k * M + m] = p16[k * (size_t)b.MP + m];
    }
}

// a gathered row (generate_gather_kernel): its bytes, and decode_head of it
size_t row_bytes(const GenState &G) { return (size_t)(G.head16 + G.tail16) * 16; }
void decode_row(const DevBatch &b, const GenState &G, const unsigned char *row, RecordHead &o) {
    const unsigned char *tail = row + (size_t)G.head16 * 16 - (size_t)G.tail0 * 16;       // where the record's byte 0 would lie for the tail's offsets
    decode_head(b, row, G.tail16 ? reinterpret_cast<const uint16_t *>(tail + b.L.i_ocnt) : nullptr, o);
}

int fail_generate(fjsp_env *e, int rc, const std::string &msg) {
    e->gen_failed = true;
    set_error(msg);
    return rc;
}
std::string who(const GenState &G, size_t i) { return "instance " + std::to_string(i) + " (seed " + std::to_string(G.seeds[i]) + ")"; }
int launch_failed(const char *text) { set_error(text); return FJSP_E_HIP; }

// The host route's producer: the record heads of ids[c0, c0 + n) read back, their order-0 LPs (solve_order0) on the
// handle's host threads, x uploaded into the staging slots
int solve_on_host(fjsp_env *e, const LpRoute &r, int c0, int n, const std::string &call) {
    GenState &G = *e->gen;
    const DevBatch &b = e->b;
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP, head = row_bytes(G), words = (size_t)n * (head / 16);
    if (launch(generate_gather_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, r.st, b, (const uint32_t *)(r.ids + c0), n, G.d_head, G.head16, G.tail0, G.tail16) != 0)
        return launch_failed("generate_gather_kernel launch failed");
    HIP_TRY(hipMemcpyAsync(G.h_head, G.d_head, words * 16, hipMemcpyDeviceToHost, r.st));
    HIP_TRY(hipStreamSynchronize(r.st));
    const LpFailure bad = lp_pool_of(e->arr.pool, e->arr.lp_threads).run((uint32_t)n, [&](uint32_t s) {
        static thread_local RecordHead in;        // a thread's buffers, kept across its LPs
        static thread_local std::vector<int> Q, now;
        static thread_local std::vector<double> x;
        decode_row(b, G, reinterpret_cast<const unsigned char *>(G.h_head) + (size_t)s * head, in);
        const int K = in.h.K, M = in.h.M;
        Q.clear(); now.clear(); x.assign((size_t)K * M, 0.0);
        for (int kind = 0; kind < in.h.R; ++kind)
            for (int j = 0; j < in.Jr[(size_t)kind]; ++j) { Q.push_back(in.count[(size_t)kind]); now.push_back(j == 0 ? in.count[(size_t)kind] : 0); }
        double obj = 0.0, *out = G.h_stage + (size_t)s * KP * MP;
        std::memset(out, 0, KP * MP * 8);
        if (solve_fluid_lp(in.h.R, M, in.Jr.data(), in.p.data(), Q.data(), now.data(), x.data(), &obj) != 0) return false;
        for (int k = 0; k < K; ++k)
            for (int m = 0; m < M; ++m) out[(size_t)k * MP + m] = x[(size_t)k * M + m];
        return true;
    });
    if (bad) return fail_generate(e, FJSP_E_LP, call + ": the fluid LP of " + who(G, G.h_host_ids[c0 + bad.index]) + " failed");
    HIP_TRY(hipMemcpyAsync(r.d_stage, G.h_stage, (size_t)n * KP * MP * 8, hipMemcpyHostToDevice, r.st));
    return FJSP_OK;
}

// The n LPs of route r, in bounded chunks of staging slots: each its producer and the finish of its instances
int run_route(fjsp_env *e, const LpRoute &r, int n_total, const std::string &call) {
    GenState &G = *e->gen;
    const DevBatch &b = e->b;
    const bool side = r.st != G.st_dev;               // on the second stream, beside the first route
    if (side && n_total == 0) return FJSP_OK;         // (the first route always marks its end: the tables' time counts from there)
    if (r.ev_begin) HIP_TRY(hipEventRecord(r.ev_begin, r.st));
    for (int c0 = 0; c0 < n_total; c0 += G.chunk) {
        const int n = std::min(G.chunk, n_total - c0);
        const uint32_t *ids = r.ids + c0;
        const uint16_t *lp_in = r.lp_in ? r.lp_in + (size_t)c0 * 2 * (size_t)b.KP : nullptr;
        int rc = FJSP_OK, launched = 0;
        if (r.producer == LpRoute::kLds) launched = launch_lp_device(b, nullptr, n, ids, lp_in, r.d_stage, G.d_lp_err, &r.d_solved->solved, G.h_counts[kCountLdsMax], r.st);
        else if (r.producer == LpRoute::kGlobal) launched = launch_lp_global(b, nullptr, n, ids, lp_in, r.d_stage, G.d_lp_err, &r.d_solved->solved, G.pool, r.st);
        else rc = solve_on_host(e, r, c0, n, call);
        if (rc != FJSP_OK) return rc;
        if (launched != 0 || launch(generate_finish_kernel, dim3((unsigned)n), dim3(kWave), 0, r.st, b, G.a, ids, n, (const double *)r.d_stage) != 0) return launch_failed(r.launch_error);
        if (r.producer == LpRoute::kHost) HIP_TRY(hipStreamSynchronize(r.st));       // h_stage and h_head are reused by the next round
    }
    if (!r.ev_end) return FJSP_OK;
    HIP_TRY(hipEventRecord(r.ev_end, r.st));
    G.ev_lps = r.ev_end;
    if (side) {       // the tables read every x
        HIP_TRY(hipStreamWaitEvent(G.st_dev, r.ev_end, 0));
        HIP_TRY(hipEventRecord(G.ev_joined, G.st_dev));
        G.ev_lps = G.ev_joined;
    }
    return FJSP_OK;
}

}  // namespace

// The heads of records into mirror, in rounds of GenState::chunk through the host route's gather buffers: of all records, or
// of the `listed` first entries of a masked refill's list (mirror then holds every instance already).
static int gather_heads(fjsp_env *e, std::vector<RecordHead> &mirror, int count, bool listed) {
    GenState &G = *e->gen;
    const DevBatch &b = e->b;
    const size_t row = row_bytes(G);
    for (int c0 = 0; c0 < count; c0 += G.chunk) {
        const int n = std::min(G.chunk, count - c0);
        const size_t words = (size_t)n * (row / 16);
        DevBatch part = b;                               // not listed: instances c0 .. c0 + n - 1, by position
        if (!listed) part.inst = b.inst + (size_t)c0 * b.L.i_stride;
        if (launch(generate_gather_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, G.st_host, part, listed ? (const uint32_t *)(G.d_list + c0) : (const uint32_t *)nullptr, n,
                   G.d_head, G.head16, G.tail0, G.tail16) != 0)
            return launch_failed("generate_gather_kernel launch failed");
        HIP_TRY(hipMemcpyAsync(G.h_head, G.d_head, words * 16, hipMemcpyDeviceToHost, G.st_host));
        HIP_TRY(hipStreamSynchronize(G.st_host));
        for (int q = 0; q < n; ++q)
            decode_row(b, G, reinterpret_cast<const unsigned char *>(G.h_head) + (size_t)q * row, mirror[listed ? (size_t)G.h_list[c0 + q] : (size_t)(c0 + q)]);
    }
    return FJSP_OK;
}

// The heads of all records into e->lp_mirror.  Called with no regenerate under way.
int refresh_lp_mirror(fjsp_env *e) {
    std::vector<RecordHead> mirror((size_t)e->b.n_inst);
    if (const int rc = gather_heads(e, mirror, e->b.n_inst, false)) return rc;
    e->lp_mirror.swap(mirror);
    return FJSP_OK;
}

namespace {
// The refill: records, LPs, tables, reset -- of every instance and env (mc == nullptr: fjsp_env_regenerate, the creates), or
// of the instances a masked call lists and the envs that play them (fjsp_env_regenerate_masked; rng_seed is not read: those
// envs' streams start over from the handle's).  Synchronous; on the handle's device.
int regenerate(fjsp_env *e, uint64_t seed_base, uint64_t rng_seed, const std::string &call, const MaskedCall *mc) {
    GenState &G = *e->gen;
    DevBatch &b = e->b;
    const size_t N = (size_t)b.N, n_inst = (size_t)b.n_inst;
    const auto t_call = Clock::now();
    HIP_TRY(hipDeviceSynchronize());         // steps still queued on any stream read the records this call rewrites
    const bool was_failed = e->gen_failed;
    e->gen_failed = true;                    // until the call has gone through
    G.a.seed_base = seed_base;
    G.a.list = mc ? G.d_list : nullptr;
    if (!mc) b.rng_seed = rng_seed;
    std::fill(G.stats, G.stats + kGenStats, 0);
    std::fill(G.ms, G.ms + kGenTimes, 0.0);
    hipStream_t st = G.st_dev;
    // ---- clear
    HIP_TRY(hipMemsetAsync(G.a.counts, 0, kGenCounts * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(G.a.counts + kCountFailed, 0xFF, sizeof(uint32_t), st));
    for (const LpRoute &r : G.route) if (r.d_solved) HIP_TRY(hipMemsetAsync(r.d_solved, 0, sizeof(LpCounters), st));
    HIP_TRY(hipMemsetAsync(G.d_lp_err, 0, sizeof(LpErrWord), st));
    if (!mc) {
        std::fill(G.unfinished.begin(), G.unfinished.end(), (uint8_t)1);
        HIP_TRY(hipMemsetAsync(b.inst, 0, n_inst * b.L.i_stride, st));
        HIP_TRY(hipMemsetAsync(b.envs, 0, N * b.L.e_stride, st));       // the draw counters too: the env streams start over
        if (b.mord) HIP_TRY(hipMemsetAsync(b.pending_count, 0, 4, st)); // no env is parked at an arrival
        if (e->sched.rec) HIP_TRY(hipMemsetAsync(e->sched.rec, 0, (size_t)e->sched.cap * N * sizeof(uint4), st));
        if (launch(generate_seeds_kernel, dim3((unsigned)((n_inst + 255) / 256)), dim3(256), 0, st, b, G.a) != 0) return launch_failed("generate_seeds_kernel launch failed");
    } else {
        // the list (with what a failed call left half made), then the listed records and their envs' to zero
        const bool pending = std::find(G.unfinished.begin(), G.unfinished.end(), (uint8_t)1) != G.unfinished.end();
        if (pending) {
            std::copy(G.unfinished.begin(), G.unfinished.end(), G.h_pending);
            HIP_TRY(hipMemcpyAsync(G.d_pending, G.h_pending, n_inst, hipMemcpyHostToDevice, st));
        }
        if (launch(generate_list_kernel, dim3(1), dim3(1024), 0, st, b, G.a, mc->d_mask, pending ? (const uint8_t *)G.d_pending : (const uint8_t *)nullptr, G.d_list,
                   mc->d_refreshed, G.d_env_mask) != 0 ||
            launch(generate_clear_kernel, dim3((unsigned)n_inst), dim3(256), 0, st, b, G.a, e->sched) != 0)
            return launch_failed("generate_list_kernel / generate_clear_kernel launch failed");
    }
    // ---- pack
    HIP_TRY(hipEventRecord(G.ev_start, st));
    if (G.dynamic) {
        if (launch(generate_pack_dynamic_kernel, dim3((unsigned)n_inst), dim3(kWave), 0, st, b, G.a, G.d) != 0 ||
            launch(generate_machine_kernel, dim3((unsigned)n_inst), dim3(kWave), 0, st, b, G.a, G.d) != 0)
            return launch_failed("generate_pack_dynamic_kernel / generate_machine_kernel launch failed");
    } else if (launch(generate_pack_kernel, dim3((unsigned)n_inst), dim3(kWave), 0, st, b, G.a) != 0) return launch_failed("generate_pack_kernel launch failed");
    HIP_TRY(hipEventRecord(G.ev_packed, st));
    // ---- the call's one read-back before the LPs: status words, sizes, the lists' lengths, the host list, a masked call's list; validate
    HIP_TRY(hipMemcpyAsync(G.h_info, G.a.info, n_inst * sizeof(GenInfo), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(G.h_counts, G.a.counts, kGenCounts * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(G.h_host_ids, G.a.host_ids, n_inst * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (G.dynamic) HIP_TRY(hipMemcpyAsync(G.h_seed_used, G.d.seed_used, n_inst * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (mc) HIP_TRY(hipMemcpyAsync(G.h_list, G.d_list, n_inst * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t n_made = mc ? std::min<size_t>(G.h_counts[kCountListed], n_inst) : n_inst;
    const auto made = [&](size_t s) { return mc ? (size_t)G.h_list[s] : s; };      // the s-th instance of this call, ascending
    if (n_made == 0) {                       // an empty mask: nothing was written but the (all zero) applied masks
        e->gen_failed = was_failed;
        G.ms[kMsTotal] = ms_since(t_call);
        return FJSP_OK;
    }
    for (size_t s = 0; s < n_made; ++s) { G.seeds[made(s)] = seed_base + made(s); G.unfinished[made(s)] = 1; }
    for (size_t s = 0; s < n_made; ++s) {
        const size_t i = made(s);
        const GenInfo &f = G.h_info[i];
        if (f.status == FJSP_E_UNSUPPORTED && G.dynamic)
            return fail_generate(e, FJSP_E_UNSUPPORTED, call + ": " + who(G, i) + ": MO_DFJSP: a machine with no eligible operation (ZeroDivisionError in the reference) in each of " +
                                 std::to_string(G.d.redraws + 1) + " attempts (redraws = " + std::to_string(G.d.redraws) + ")");
        if (f.status == FJSP_E_UNSUPPORTED)
            return fail_generate(e, FJSP_E_UNSUPPORTED, call + ": " + who(G, i) + ": SO_DFJSP: a machine with no eligible operation (ZeroDivisionError in the reference)");
        if (f.status != 0)
            return fail_generate(e, f.status, call + ": " + who(G, i) + ": a draw left the record's fields (internal error)");
        if (f.ops > e->ops_max || f.M < 1 || f.M > b.MP || f.S < 1 || f.S > b.SP)
            return fail_generate(e, FJSP_E_UNSUPPORTED, call + ": " + who(G, i) + ": sizes disagree with the host's (internal error)");
    }
    double bytes = 0.0;                      // the mean over all instances, those this call left alone too
    for (size_t i = 0; i < n_inst; ++i) {
        const GenInfo &f = G.h_info[i];
        bytes += step_bytes(b, f.K, f.nj, f.M);
        if (G.dynamic) bytes += f.M * 14.0 + 2.0 * sizeof(DynScalars);      // step_bytes_of (fjsp_env.hip)
    }
    size_t listed = 0;
    bool routed = true;      // no instance is on a list this handle has no route for
    for (const LpRoute &r : G.route) { listed += G.h_counts[r.length]; routed = routed && (r.present() || G.h_counts[r.length] == 0); }
    if (listed != n_made || !routed) return fail_generate(e, FJSP_E_HIP, call + ": the LP lists do not cover the instances (internal error)");
    const int n_host = (int)G.h_counts[kCountHost];
    if (e->plan.lp_device_forced == 1 && n_host > 0) {
        const uint32_t i = *std::min_element(G.h_host_ids, G.h_host_ids + n_host);
        const GenInfo &f = G.h_info[i];
        return fail_generate(e, FJSP_E_UNSUPPORTED, call + ": FJSP_LP_IMPL=device, but the order-0 tableau of " + who(G, i) +
                             " does not fit: " + std::to_string(f.lds) + " bytes of LDS (limit " +
                             std::to_string(kLpLdsLimit) + "), " + std::to_string(lp_max_columns(f.K, f.M, f.nx, f.R)) + " columns (limit " +
                             std::to_string(kLpLdsColumns) + ")");
    }
    for (size_t s = 0; s < n_made; ++s) { const size_t i = made(s); e->inst_K[i] = G.h_info[i].K; e->inst_M[i] = G.h_info[i].M; }
    e->step_bytes = (int64_t)(bytes / (double)n_inst + 0.5);
    // ---- the routes: the device's on their streams, then the host's while the device works on its lists
    for (const LpRoute &r : G.route) {
        if (!r.present()) continue;
        const auto t_route = Clock::now();
        if (const int rc = run_route(e, r, (int)G.h_counts[r.length], call)) return rc;
        if (r.producer == LpRoute::kHost && n_host) G.ms[kMsLpHost] = ms_since(t_route);
    }
    // ---- the fluid tables, one reset of every env made (publishes i_obs0), those envs done again: as upload_batch leaves them
    const dim3 gN((unsigned)((N + 255) / 256));
    const uint8_t *envs = mc ? G.d_env_mask : nullptr;
    if (launch(generate_mark_done_kernel, gN, dim3(256), 0, st, b, G.d_kenv, envs) != 0 ||
        launch_fluid_tables(b, st, mc ? G.d_list : nullptr, (int)n_made) != 0 ||
        launch_reset(b, envs, nullptr, st) != 0 || launch(generate_mark_done_kernel, gN, dim3(256), 0, st, b, (uint8_t *)nullptr, envs) != 0)
        return launch_failed("fluid_tables_kernel / reset_kernel launch failed");
    // ---- the counters
    HIP_TRY(hipMemcpyAsync(G.h_counts, G.a.counts, kGenCounts * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    for (const LpRoute &r : G.route) if (r.d_solved) HIP_TRY(hipMemcpyAsync(r.h_solved, r.d_solved, sizeof(LpCounters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&G.h_back->lp_err, G.d_lp_err, sizeof(LpErrWord), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(G.ev_end, st));
    HIP_TRY(hipDeviceSynchronize());
    // ---- report
    const LpRoute &lds = G.route[kRouteLds], &glob = G.route[kRouteGlobal];
    const int n_glob = (int)G.h_counts[kCountGlob];
    G.ms[kMsGenerate] = ms_between(G.ev_start, G.ev_packed);
    G.ms[kMsLpLds] = ms_between(G.ev_packed, lds.ev_end);
    G.ms[kMsTablesReset] = ms_between(G.ev_lps, G.ev_end);
    if (n_glob > 0) G.ms[kMsLpGlobal] = ms_between(glob.ev_begin, glob.ev_end);
    const uint32_t failed = G.h_counts[kCountFailed], lp_err = G.h_back->lp_err.code;
    if (failed != 0xFFFFFFFFu || lp_err != 0u)
        return fail_generate(e, FJSP_E_LP, failed != 0xFFFFFFFFu ? call + ": the fluid LP of " + who(G, failed) + " failed"
                                                                 : call + ": a fluid LP failed on the device (code " + std::to_string(lp_err) + ")");
    G.stats[kStatInstances] = (int64_t)n_made; G.stats[kStatLpLds] = G.h_counts[kCountFit]; G.stats[kStatLpHost] = n_host;
    G.stats[kStatDevicePivots] = (int64_t)lds.h_solved->pivots;
    if (glob.present()) {
        G.stats[kStatLpGlobal] = n_glob; G.stats[kStatGlobalPivots] = (int64_t)glob.h_solved->pivots;
        G.stats[kStatDevicePivots] += G.stats[kStatGlobalPivots];
    }
    e->inst_hash = gen_hash(G.a, G.dynamic ? &G.d : nullptr, b.n_inst, G.seeds);
    if (b.mord) {
        // the memo of solved arrival LPs is keyed by the instance index, which names another instance now (the counters of
        // solved LPs and pivots keep running); the host services read the new records' heads
        arrivals_forget(e->arr);
        const bool mirrored = !e->arr.lp_device || e->arr.ring;
        if (mc && mirrored && e->lp_mirror.size() == n_inst) {
            if (const int rc = gather_heads(e, e->lp_mirror, (int)n_made, true)) return rc;
        } else {
            e->lp_mirror.clear();
            if (mirrored)
                if (const int rc = refresh_lp_mirror(e)) return rc;
        }
    }
    std::fill(G.unfinished.begin(), G.unfinished.end(), (uint8_t)0);
    e->gen_failed = false;
    G.ms[kMsTotal] = ms_since(t_call);
    return FJSP_OK;
}

// The three creates: q == nullptr is the fixed parameter set *prm; else *prm is q->base and M, DDT are drawn per instance;
// o != nullptr: q is &o->r and the number of orders is drawn as well; dq != nullptr (fjsp_env_create_generated_dynamic): o is
// &dq->o, the variant is MO_DFJSP and the machine data are drawn too
int create_generated(const std::string &call, const fjsp_gen_params *prm, const fjsp_gen_ranges *q, const fjsp_gen_orders *o, const fjsp_gen_dynamic *dq,
                     int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device, uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out) {
    if (!prm || !out || n_inst <= 0 || n_envs <= 0) { set_error(call + ": bad arguments"); return FJSP_E_ARG; }
    if (family < -1 || family > 1) { set_error(call + ": family must be -1, 0 or 1"); return FJSP_E_ARG; }
    // (MO_DFJSP shares SO_DFJSP's due dates -- the order's delivery time -- and its need of an operation on every machine)
    const bool class_fjsp = variant == FJSP_VARIANT_SO_DFJSP || dq;
    if (variant == FJSP_VARIANT_MO_DFJSP && !dq) {
        set_error(call + ": MO_DFJSP needs machine data: use fjsp_env_create_generated_dynamic (or fjsp_env_create)");
        return FJSP_E_UNSUPPORTED;
    }
    if (variant == FJSP_VARIANT_SO_DFJSP) variant = FJSP_VARIANT_SO_FJSSP;
    if (variant != FJSP_VARIANT_SO_FJSSP && variant != FJSP_VARIANT_SO_SFJSP && variant != FJSP_VARIANT_MO_FJSSP_DISCRETES && !dq) {
        set_error(call + ": unknown variant"); return FJSP_E_ARG;
    }
    int rc = dq ? check_gen_dynamic(*dq) : (o ? check_gen_orders(*o) : (q ? check_gen_ranges(*q) : FJSP_OK));
    if (rc != FJSP_OK) return rc;
    fjsp_gen_params g = *prm;
    if (q) { g.M = q->M_min; g.DDT = 0.0; }       // base.M and base.DDT are not read
    if (o) g.S = o->S_max;                        // nor is base.S
    if ((rc = check_gen_params(g)) != FJSP_OK) return rc;
    const int S_max = o ? o->S_max : 1;
    if (S_max > FJSP_GEN_MAX_ORDERS) {
        set_error(call + ": more than " + std::to_string(FJSP_GEN_MAX_ORDERS) + " orders (S_max): the generator kernel keeps the orders' counts and times in LDS");
        return FJSP_E_UNSUPPORTED;
    }
    if (S_max > 1 && variant != FJSP_VARIANT_SO_FJSSP && !dq) {
        set_error(call + ": only SO_FJSSP handles order arrivals (the subclasses are single-order, SO_SFJSP.py:20 / MO_FJSSP_discretes.py:21): S_max must be 1");
        return FJSP_E_UNSUPPORTED;
    }
    const int M_min = q ? q->M_min : g.M, M_max = q ? q->M_max : g.M;
    const double ddt_max = q ? std::max(std::fabs(q->DDT_min), std::fabs(q->DDT_max)) : g.DDT;
    if (!o && prm->S != 1) {
        set_error(call + ": one order only (S == 1): order arrivals need the per-env fluid tables (use fjsp_env_create)");
        return FJSP_E_UNSUPPORTED;
    }
    Shape sh;
    if ((rc = check_worst_case(g, M_min, M_max, ddt_max, S_max, dq ? &dq->m : nullptr, sh)) != FJSP_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device visible: the environment kernels need an MI355X (there is no CPU path)");
        return FJSP_E_HIP;
    }
    if (device < 0 || device >= ndev) { set_error(call + ": device index out of range"); return FJSP_E_ARG; }
    DeviceGuard guard(device);

    std::unique_ptr<fjsp_env, void (*)(fjsp_env *)> e(new fjsp_env(), fjsp_env_destroy);
    e->device = device; e->src = nullptr; e->first = 0;
    DevBatch &b = e->b;
    if ((rc = plan_batch(b, e->plan, sh, n_inst, n_envs, variant, rng_seed, family)) != FJSP_OK) return rc;
    // src stays null: the order-arrival services (fjsp_arrivals.hip) of a multi-order handle read lp_mirror in its place
    if ((b.mord != 0) != (S_max > 1 || dq)) { set_error(call + ": internal error (multi-order layout)"); return FJSP_E_UNSUPPORTED; }
    e->inst_K.assign((size_t)n_inst, 0); e->inst_M.assign((size_t)n_inst, sh.M);
    e->ops_max = sh.K * prm->N_max * S_max;
    if (b.mord) {
        // the arrival service, once: from the worst tableau of the parameters, with its staging and pools
        const LpTableau worst = lp_worst_case(prm->R_max, prm->J_max, sh.M);
        choose_lp_service(e.get(), &worst, 1);
        if ((rc = alloc_arrival_staging(e.get())) != FJSP_OK) return rc;
    }

    e->gen = new GenState();
    GenState &G = *e->gen;
    const size_t N = (size_t)n_envs, NI = (size_t)n_inst, KP = (size_t)b.KP, MP = (size_t)b.MP;
    if (q) { g.M = 0; G.a.ranged = 1; G.a.M_min = q->M_min; G.a.M_max = q->M_max; G.a.DDT_min = q->DDT_min; G.a.DDT_max = q->DDT_max; }
    G.a.g = g; G.a.class_fjsp = class_fjsp ? 1 : 0; G.a.allow_device = e->plan.lp_device_forced == 0 ? 0 : 1;
    G.a.allow_global = e->plan.lp_device_forced == 2 ? 1 : 0;
    if (o) { G.a.orders = 1; G.a.S_min = o->S_min; G.a.S_max = o->S_max; }
    if (dq) { G.dynamic = true; G.d.mc = dq->m; G.d.redraws = dq->redraws; G.d.windows = sh.B; }
    G.a.kmax = sh.K; G.a.RP = sh.R;
    G.chunk = (int)std::min<size_t>(NI, 1024);
    G.head16 = (int)((b.L.i_x + 15) / 16);
    if (b.mord) {
        G.tail0 = (int)(b.L.i_oarr / 16);
        G.tail16 = (int)((b.L.i_ocnt + (size_t)b.SP * b.RP * 2 + 15) / 16) - G.tail0;
    }
    const size_t heads = (size_t)G.chunk * row_bytes(G);
    const size_t stage = (size_t)G.chunk * KP * MP * 8, ids = NI * sizeof(uint32_t), lp_in = NI * 2 * KP * sizeof(uint16_t);
    LpRoute &lds = G.route[kRouteLds], &glob = G.route[kRouteGlobal], &host = G.route[kRouteHost];
    lds.producer = LpRoute::kLds; lds.length = kCountFit; lds.launch_error = "lp_device_kernel / generate_finish_kernel launch failed";
    glob.producer = LpRoute::kGlobal; glob.length = kCountGlob; glob.launch_error = "lp_global_kernel / generate_finish_kernel launch failed";
    host.producer = LpRoute::kHost; host.length = kCountHost; host.launch_error = "generate_finish_kernel launch failed";
    if (!dev_alloc(e.get(), NI * b.L.i_stride, &b.inst, "hipMalloc instance slab") ||
        !dev_alloc(e.get(), N * b.L.e_stride, &b.envs, "hipMalloc env slab") ||
        !dev_alloc(e.get(), N + 16, &e->d_done_scratch, "hipMalloc scratch") ||
        !dev_alloc(e.get(), NI * (size_t)sh.K * MP, &G.a.elig, "hipMalloc eligible lists") ||
        !dev_alloc(e.get(), NI * (size_t)b.SP * sizeof(int32_t), &G.a.deliv, "hipMalloc delivery times") ||
        !dev_alloc(e.get(), NI * sizeof(GenInfo), &G.a.info, "hipMalloc generator status") ||
        !dev_alloc(e.get(), kGenCounts * sizeof(uint32_t), &G.a.counts, "hipMalloc list lengths") ||
        !dev_alloc(e.get(), ids, &G.a.fit_ids, "hipMalloc LP list") || !dev_alloc(e.get(), ids, &G.a.host_ids, "hipMalloc LP list") ||
        !dev_alloc(e.get(), lp_in, &G.a.lp_in, "hipMalloc LP inputs") ||
        !dev_alloc(e.get(), stage, &lds.d_stage, "hipMalloc LP solutions") || !dev_alloc(e.get(), stage, &host.d_stage, "hipMalloc LP solutions") ||
        !dev_alloc(e.get(), heads, &G.d_head, "hipMalloc record heads") ||
        !dev_alloc(e.get(), sizeof(LpErrWord), &G.d_lp_err, "hipMalloc LP error word") ||
        !dev_alloc(e.get(), sizeof(LpCounters), &lds.d_solved, "hipMalloc LP counters") ||
        !dev_alloc(e.get(), NI * sizeof(uint64_t), &G.a.seeds, "hipMalloc instance seeds") || !dev_alloc(e.get(), ids, &G.d_list, "hipMalloc refill list") ||
        !dev_alloc(e.get(), N, &G.d_env_mask, "hipMalloc refill mask") ||
        !dev_alloc(e.get(), NI, &G.d_pending, "hipMalloc refill mask") || !host_alloc(e.get(), ids, &G.h_list) || !host_alloc(e.get(), NI, &G.h_pending) ||
        (b.grp && !dev_alloc(e.get(), N, &G.d_kenv, "hipMalloc K table")) ||
        (dq && (!dev_alloc(e.get(), NI * sizeof(uint64_t), &G.d.seed_used, "hipMalloc instance seeds") || !host_alloc(e.get(), NI * sizeof(uint64_t), &G.h_seed_used))) ||
        !host_alloc(e.get(), NI * sizeof(GenInfo), &G.h_info) || !host_alloc(e.get(), kGenCounts * sizeof(uint32_t), &G.h_counts) ||
        !host_alloc(e.get(), ids, &G.h_host_ids) || !host_alloc(e.get(), stage, &G.h_stage) ||
        !host_alloc(e.get(), heads, &G.h_head) || !host_alloc(e.get(), sizeof(GenReadback), &G.h_back))
        return FJSP_E_HIP;
    if (G.a.allow_global) {
        // the scratch pool of the global-memory simplex, sized for the largest tableau the parameters admit within its limits:
        // K - R <= R_max (J_max - 1) precedence rows
        const int nr_cap = std::min(kLpGlobalRows, sh.K + sh.M + prm->R_max * (prm->J_max - 1));
        const int nc_cap = std::min(kLpGlobalColumns, sh.K * sh.M + 1 + nr_cap + 1);
        G.pool.slot_bytes = lp_global_slot_bytes(nr_cap, nc_cap);
        G.pool.slots = lp_global_slots((size_t)G.chunk, G.pool.slot_bytes);
        G.pool.lds = lp_global_lds(sh.K, sh.M, (int)MP, nr_cap, nc_cap);
        if (!dev_alloc(e.get(), (size_t)G.pool.slots * G.pool.slot_bytes, &G.pool.mem, "hipMalloc LP tableau pool") ||
            !dev_alloc(e.get(), ids, &G.a.glob_ids, "hipMalloc LP list") || !dev_alloc(e.get(), lp_in, &G.a.lp_in_glob, "hipMalloc LP inputs") ||
            !dev_alloc(e.get(), stage, &glob.d_stage, "hipMalloc LP solutions") ||
            !dev_alloc(e.get(), sizeof(LpCounters), &glob.d_solved, "hipMalloc LP counters"))
            return FJSP_E_HIP;
        for (hipEvent_t *ev : {&glob.ev_begin, &glob.ev_end}) HIP_TRY(hipEventCreate(ev));
    }
    G.seeds.assign(NI, 0); G.unfinished.assign(NI, 0);
    b.kenv = G.d_kenv;
    for (hipEvent_t *ev : {&G.ev_start, &G.ev_packed, &G.ev_end, &G.ev_joined, &lds.ev_end}) HIP_TRY(hipEventCreate(ev));
    HIP_TRY(hipStreamCreateWithFlags(&G.st_dev, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&G.st_host, hipStreamNonBlocking));
    lds.ids = G.a.fit_ids; lds.lp_in = G.a.lp_in; lds.h_solved = &G.h_back->lds; lds.st = G.st_dev;
    glob.ids = G.a.glob_ids; glob.lp_in = G.a.lp_in_glob; glob.h_solved = &G.h_back->glob; glob.st = G.st_host;
    host.ids = G.a.host_ids; host.st = G.st_host;
    if ((rc = regenerate(e.get(), seed_base, rng_seed, call, nullptr)) != FJSP_OK) return rc;
    *out = e.release();
    return FJSP_OK;
}
}  // namespace
}  // namespace fjsp

using namespace fjsp;

extern "C" {
int fjsp_env_create_generated(const fjsp_gen_params *prm, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                              uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out) {
    return create_generated("fjsp_env_create_generated", prm, nullptr, nullptr, nullptr, n_inst, n_envs, variant, device, rng_seed, family, seed_base, out);
}

int fjsp_env_create_generated_ranges(const fjsp_gen_ranges *q, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                                     uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out) {
    return create_generated("fjsp_env_create_generated_ranges", q ? &q->base : nullptr, q, nullptr, nullptr, n_inst, n_envs, variant, device, rng_seed,
                            family, seed_base, out);
}

int fjsp_env_create_generated_orders(const fjsp_gen_orders *q, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                                     uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out) {
    return create_generated("fjsp_env_create_generated_orders", q ? &q->r.base : nullptr, q ? &q->r : nullptr, q, nullptr, n_inst, n_envs, variant,
                            device, rng_seed, family, seed_base, out);
}

int fjsp_env_create_generated_dynamic(const fjsp_gen_dynamic *q, int32_t n_inst, int32_t n_envs, int32_t device, uint64_t rng_seed, uint64_t seed_base,
                                      fjsp_env **out) {
    return create_generated("fjsp_env_create_generated_dynamic", q ? &q->o.r.base : nullptr, q ? &q->o.r : nullptr, q ? &q->o : nullptr, q, n_inst, n_envs,
                            FJSP_VARIANT_MO_DFJSP, device, rng_seed, 0, seed_base, out);
}

int fjsp_env_regenerate(fjsp_env *e, uint64_t seed_base, uint64_t rng_seed) {
    if (!e) { set_error("fjsp_env_regenerate: null env"); return FJSP_E_ARG; }
    if (!e->gen) { set_error("fjsp_env_regenerate: the batch was not made by fjsp_env_create_generated"); return FJSP_E_STATE; }
    if (!async_idle(e)) {
        set_error("fjsp_env_regenerate: environments are parked in the asynchronous arrival service; call fjsp_env_arrivals_flush first");
        return FJSP_E_STATE;
    }
    DeviceGuard guard(e->device);
    return regenerate(e, seed_base, rng_seed, "fjsp_env_regenerate", nullptr);
}

int fjsp_env_regenerate_masked(fjsp_env *e, const uint8_t *d_mask, uint64_t seed_base, uint8_t *d_refreshed) {
    if (!e) { set_error("fjsp_env_regenerate_masked: null env"); return FJSP_E_ARG; }
    if (!e->gen) { set_error("fjsp_env_regenerate_masked: the batch was not made by fjsp_env_create_generated"); return FJSP_E_STATE; }
    if (!async_idle(e)) {
        set_error("fjsp_env_regenerate_masked: environments are parked in the asynchronous arrival service; call fjsp_env_arrivals_flush first");
        return FJSP_E_STATE;
    }
    DeviceGuard guard(e->device);
    const MaskedCall mc{d_mask, d_refreshed};
    return regenerate(e, seed_base, 0, "fjsp_env_regenerate_masked", &mc);
}

int fjsp_env_instance_seed(const fjsp_env *e, int32_t i, uint64_t *seed) {
    if (!e || !seed) { set_error("fjsp_env_instance_seed: null argument"); return FJSP_E_ARG; }
    if (!e->gen) { set_error("fjsp_env_instance_seed: the batch was not made by fjsp_env_create_generated"); return FJSP_E_STATE; }
    if (i < 0 || i >= e->b.n_inst) { set_error("fjsp_env_instance_seed: instance index out of range"); return FJSP_E_ARG; }
    *seed = e->gen->seeds[(size_t)i];
    return FJSP_OK;
}

// The three accessors hand out prefixes of GenState::stats and ::ms; `given`: the caller passed the array the call is about
static int copy_stats(const fjsp_env *e, const std::string &fn, bool given, int64_t *out, int n_out, double *out_ms, int n_ms) {
    if (!e || !given) { set_error(fn + ": null argument"); return FJSP_E_ARG; }
    if (!e->gen) { set_error(fn + ": the batch was not made by fjsp_env_create_generated"); return FJSP_E_STATE; }
    if (out) std::copy(e->gen->stats, e->gen->stats + n_out, out);
    if (out_ms) std::copy(e->gen->ms, e->gen->ms + n_ms, out_ms);
    return FJSP_OK;
}
int fjsp_env_generated_stats(const fjsp_env *e, int64_t out[4]) { return copy_stats(e, "fjsp_env_generated_stats", out, out, kStatDevicePivots + 1, nullptr, 0); }
int fjsp_env_generated_stats2(const fjsp_env *e, int64_t out[6], double out_ms[6]) { return copy_stats(e, "fjsp_env_generated_stats2", out, out, kGenStats, out_ms, kGenTimes); }
int fjsp_env_generated_times(const fjsp_env *e, double out_ms[5]) { return copy_stats(e, "fjsp_env_generated_times", out_ms, nullptr, 0, out_ms, kMsTotal + 1); }

int fjsp_env_instance_read(fjsp_env *e, int32_t i, int32_t dims[6], int32_t *Jr, int32_t *p, int32_t *elig_n, int32_t *elig_list,
                           int32_t *count, int32_t *arrive, int32_t *delivery, double *ddt, double *x) {
    if (!e || i < 0 || i >= e->b.n_inst) { set_error("fjsp_env_instance_read: bad arguments"); return FJSP_E_ARG; }
    if (!e->gen) { set_error("fjsp_env_instance_read: the batch was not made by fjsp_env_create_generated"); return FJSP_E_STATE; }
    if (e->gen_failed) { set_error("fjsp_env_instance_read: the last fjsp_env_regenerate of this batch failed"); return FJSP_E_STATE; }
    DeviceGuard guard(e->device);
    const DevBatch &b = e->b;
    const GenState &G = *e->gen;
    const size_t MP = (size_t)b.MP;
    std::vector<unsigned char> rec(b.L.i_stride), el((size_t)G.a.kmax * MP);
    GenInfo f;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rec.data(), b.inst + (size_t)i * b.L.i_stride, rec.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(el.data(), G.a.elig + (size_t)i * el.size(), el.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&f, G.a.info + i, sizeof(f), hipMemcpyDeviceToHost));
    std::vector<int32_t> dl((size_t)b.SP);
    HIP_TRY(hipMemcpy(dl.data(), G.a.deliv + (size_t)i * (size_t)b.SP, dl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    RecordHead in;
    const uint16_t *ocnt = reinterpret_cast<const uint16_t *>(rec.data() + b.L.i_ocnt);
    const int32_t *oarr = reinterpret_cast<const int32_t *>(rec.data() + b.L.i_oarr);
    decode_head(b, rec.data(), ocnt, in);
    const InstHeader &h = in.h;
    const int S = f.S;
    if (S < 1 || S > b.SP) { set_error("fjsp_env_instance_read: the record's order count is out of range (internal error)"); return FJSP_E_STATE; }
    int jobs0 = 0;
    for (int r = 0; r < h.R; ++r) jobs0 += ocnt[r];
    const uint32_t *em = reinterpret_cast<const uint32_t *>(rec.data() + b.L.i_elig);
    const double *xr = reinterpret_cast<const double *>(rec.data() + b.L.i_x);
    if (dims) { dims[0] = h.R; dims[1] = h.M; dims[2] = h.K; dims[3] = S; dims[4] = jobs0; dims[5] = h.njobs; }
    if (Jr) std::copy(in.Jr.begin(), in.Jr.end(), Jr);
    for (int so = 0; count && so < S; ++so)
        for (int r = 0; r < h.R; ++r) count[(size_t)so * h.R + r] = ocnt[(size_t)so * b.RP + r];
    if (p) std::copy(in.p.begin(), in.p.end(), p);
    for (int k = 0; k < h.K; ++k) {
        if (elig_n) elig_n[k] = __builtin_popcount(em[k]);
        for (int m = 0; m < h.M; ++m) {
            if (elig_list) elig_list[(size_t)k * h.M + m] = el[(size_t)k * MP + m];
            if (x) x[(size_t)k * h.M + m] = xr[(size_t)k * MP + m];
        }
    }
    for (int so = 0; so < S; ++so) {
        if (arrive) arrive[so] = oarr[so];
        if (delivery) delivery[so] = dl[(size_t)so];
    }
    if (ddt) *ddt = f.ddt;
    return FJSP_OK;
}

int fjsp_env_instance_read_dynamic(fjsp_env *e, int32_t i, int32_t *power, int32_t *idle_power, int32_t *bk_n, int32_t *bk, uint64_t *seed_used,
                                   int32_t dims[2]) {
    if (!e || i < 0 || i >= e->b.n_inst) { set_error("fjsp_env_instance_read_dynamic: bad arguments"); return FJSP_E_ARG; }
    if (!e->gen || !e->gen->dynamic) { set_error("fjsp_env_instance_read_dynamic: the batch was not made by fjsp_env_create_generated_dynamic"); return FJSP_E_STATE; }
    if (e->gen_failed) { set_error("fjsp_env_instance_read_dynamic: the last fjsp_env_regenerate of this batch failed"); return FJSP_E_STATE; }
    DeviceGuard guard(e->device);
    const DevBatch &b = e->b;
    const size_t MP = (size_t)b.MP;
    std::vector<unsigned char> rec(b.L.i_stride);
    uint64_t used = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rec.data(), b.inst + (size_t)i * b.L.i_stride, rec.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&used, e->gen->d.seed_used + i, sizeof(used), hipMemcpyDeviceToHost));
    const InstHeader h = *reinterpret_cast<const InstHeader *>(rec.data());
    const uint16_t *pw = reinterpret_cast<const uint16_t *>(rec.data() + b.L.i_pw), *bko = reinterpret_cast<const uint16_t *>(rec.data() + b.L.i_bkoff);
    const int32_t *ipw = reinterpret_cast<const int32_t *>(rec.data() + b.L.i_ipw), *win = reinterpret_cast<const int32_t *>(rec.data() + b.L.i_bk);
    const int total = bko[MP];
    if (h.K < 1 || h.K > b.KP || h.M < 1 || h.M > b.MP || total > e->gen->d.windows) {
        set_error("fjsp_env_instance_read_dynamic: the record's sizes are out of range (internal error)"); return FJSP_E_STATE;
    }
    for (int k = 0; power && k < h.K; ++k)
        for (int m = 0; m < h.M; ++m) power[(size_t)k * h.M + m] = pw[(size_t)k * MP + m];
    for (int m = 0; m < h.M; ++m) {
        if (idle_power) idle_power[m] = ipw[m];
        if (bk_n) bk_n[m] = (int)bko[m + 1] - (int)bko[m];
    }
    if (bk) std::copy(win, win + 2 * (size_t)total, bk);
    if (seed_used) *seed_used = used;
    if (dims) { dims[0] = 1; dims[1] = total; }
    return FJSP_OK;
}
}  // extern "C"
