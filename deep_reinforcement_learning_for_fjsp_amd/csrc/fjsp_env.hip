// Device side of the C ABI (include/fjsp_amd.h): packs an instance set into the
// padded struct-of-arrays of fjsp_device.h, owns the HBM allocations of a batch
// of environments and launches the kernels of fjsp_kernels.hip.  The order-arrival
// services live in fjsp_arrivals.hip, saved env states in fjsp_snapshot.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "fjsp_env_impl.h"
#include "fjsp_lp_limits.h"
#include "fjsp_pyset.h"
#include "fjsp_policy.h"

using namespace fjsp;

namespace {
// Python round(): half to even on the correctly rounded quotient (class_FJSSP.py:214-218)
long py_round(double v) { return (long)std::nearbyint(v); }

// ---- fjsp_env_create_family, stage by stage

// Stage 1 (before any HIP call): the kernels can play `in` as `variant`; its sizes go into *sh.
int check_instance(const Instance &in, int variant, bool class_fjsp, Shape &sh) {
    const bool dyn = variant == FJSP_VARIANT_MO_DFJSP;
    if (!in.valid) { set_error("fjsp_env_create: instance not populated"); return FJSP_E_STATE; }
    if (!in.has_x) { set_error("fjsp_env_create: fluid solution missing (call fjsp_instances_solve_fluid)"); return FJSP_E_STATE; }
    if (dyn && !in.has_dynamic) { set_error("MO_DFJSP needs machine data (machine_data.csv / fjsp_instances_set_dynamic)"); return FJSP_E_STATE; }
    // class_FJSP.py:159 divides by len(kind_task_tuple) (with at least one operation type n + 1e-18 == n in f64), and so does
    // Machine.gap_ave with no epsilon (class_MODFJSP.py:158-159)
    for (int m = 0; (class_fjsp || dyn) && m < in.M; ++m) {
        int ops_m = 0;
        for (int k = 0; k < in.K; ++k) ops_m += in.p[(size_t)k * in.M + m] > 0 ? 1 : 0;
        if (ops_m == 0) {
            set_error(std::string(class_fjsp ? "SO_DFJSP" : "MO_DFJSP") + ": a machine with no eligible operation (ZeroDivisionError in the reference)");
            return FJSP_E_UNSUPPORTED;
        }
    }
    long long bk_total = 0;
    if (dyn) {
        int nb = 0;
        for (int m = 0; m < in.M; ++m) nb += in.bk_n[m];
        if (nb > 65535) { set_error("more than 65535 breakdown windows"); return FJSP_E_UNSUPPORTED; }
        sh.B = std::max(sh.B, nb);
        for (size_t q = 0; q < in.p.size(); ++q) {
            if (in.power[q] < 0 || in.power[q] > 65535) { set_error("power above 65535"); return FJSP_E_UNSUPPORTED; }
            if ((long long)in.power[q] * in.p[q] > 0x7fffffffLL) { set_error("energy of one operation above 2^31"); return FJSP_E_UNSUPPORTED; }
        }
        for (size_t q = 0; q + 1 < in.bk.size(); q += 2) bk_total += std::max(0, in.bk[q + 1] - in.bk[q]);
    }
    if (in.S != 1 && variant != FJSP_VARIANT_SO_FJSSP && !dyn) { set_error("only SO_FJSSP handles order arrivals (the subclasses are single-order, SO_SFJSP.py:20 / MO_FJSSP_discretes.py:21)"); return FJSP_E_UNSUPPORTED; }
    if (in.S > 64) { set_error("more than 64 orders"); return FJSP_E_UNSUPPORTED; }
    if (in.K > kWave * kMaxKC) { set_error("more than 256 operation types"); return FJSP_E_UNSUPPORTED; }
    if (in.M > kMaxM) { set_error("more than 32 machines"); return FJSP_E_UNSUPPORTED; }
    const int nj = in.jobs_total(), ops = in.ops_total();
    if (nj > 65535) { set_error("more than 65535 jobs"); return FJSP_E_UNSUPPORTED; }
    if (ops > 65535) { set_error("more than 65535 operations"); return FJSP_E_UNSUPPORTED; }
    for (int r = 0; r < in.R; ++r)
        if (in.Jr[r] > 255) { set_error("more than 255 operations in a kind"); return FJSP_E_UNSUPPORTED; }
    long long pmax = 0;
    for (int v : in.p) {
        if (v > 65535) { set_error("processing time above 65535"); return FJSP_E_UNSUPPORTED; }
        pmax = std::max<long long>(pmax, v);
    }
    // The kernels keep the clock, the machines' time_end and the per-kind tardiness sums in 32-bit integers (Python integers
    // do not wrap).  Worst case of the clock: every operation in sequence at the largest processing time, after the last
    // order arrival, stretched by every breakdown window; worst case of a per-kind sum: every job of the kind late by that much.
    long long jobs_kind_max = 0, t_arr_max = 0, due_max = 0;
    for (int r = 0; r < in.R; ++r) {
        long long jk = 0;
        for (int so = 0; so < in.S; ++so) jk += in.count[(size_t)so * in.R + r];
        jobs_kind_max = std::max(jobs_kind_max, jk);
    }
    for (int so = 0; so < in.S; ++so) {
        t_arr_max = std::max<long long>(t_arr_max, in.arrive[so]);
        due_max = std::max<long long>(due_max, std::llabs((long long)in.delivery[so]));
    }
    const long long clock_max = t_arr_max + (long long)ops * pmax + bk_total;
    if (clock_max + due_max > 0x7fffffffLL || jobs_kind_max * (clock_max + due_max) > 0x7fffffffLL) {
        set_error("instance too long for the kernels' 32-bit clocks: (last arrival + operations x max processing time + "
                  "breakdown windows) x jobs per kind must stay below 2^31");
        return FJSP_E_UNSUPPORTED;
    }
    for (int r = 0; r < in.R; ++r) sh.single_job = sh.single_job && in.S == 1 && in.R <= 255 && in.count[(size_t)r] == 1;
    sh.S = std::max(sh.S, in.S); sh.R = std::max(sh.R, in.R);
    sh.K = std::max(sh.K, in.K); sh.M = std::max(sh.M, in.M); sh.J = std::max(sh.J, nj);
    return FJSP_OK;
}

}  // namespace

namespace fjsp {
// Stages 2 and 3 of a create: the batch's sizes from its largest instance, then plan_launch and plan_layout
int plan_batch(DevBatch &b, LaunchPlan &p, const Shape &sh, int n_inst, int n_envs, int variant, uint64_t rng_seed, int family) {
    const bool dyn = variant == FJSP_VARIANT_MO_DFJSP;
    b.N = n_envs; b.n_inst = n_inst;
    b.KC = sh.K <= 64 ? 1 : (sh.K <= 128 ? 2 : 4);
    b.KP = b.KC * kWave;
    b.MP = sh.M;
    b.variant = variant;
    b.n_obs = variant == FJSP_VARIANT_SO_FJSSP ? 10 : (dyn ? 15 : 9);
    b.n_static = variant == FJSP_VARIANT_MO_FJSSP_DISCRETES ? 7 : 0;
    b.state_size = b.n_static + 2 * b.n_obs;
    b.rng_seed = rng_seed;
    b.mord = (sh.S > 1 || dyn) ? 1 : 0; b.SP = sh.S; b.RP = sh.R;     // MO_DFJSP always runs on the per-env fluid tables
    b.single_job = (sh.single_job && !b.mord) ? 1 : 0;
    b.kmax = sh.K;
    const int rc = plan_launch(b, p, sh, family);
    return rc == FJSP_OK ? plan_layout(b, sh) : rc;
}

// Stage 2: the kernel family and the build of it the handle launches, kept in its LaunchPlan.  The one place where the
// library reads its environment variables: at every create.  One 16-lane row per environment (fjsp_group.hip):
// FJSP_STEP_IMPL=wave (family -1) or family 0 keeps such batches on the one-wave-per-environment kernels; family 1 asks for
// the row kernels, FJSP_E_UNSUPPORTED if the batch does not fit them.  The row kernels' builds: group_build (fjsp_group.hip).
int plan_launch(DevBatch &b, LaunchPlan &p, const Shape &sh, int family) {
    auto knob = [](const char *name) { const char *v = getenv(name); return v ? atoi(v) : -1; };
    const char *impl = getenv("FJSP_STEP_IMPL"), *lp = getenv("FJSP_LP_IMPL"), *pad = getenv("FJSP_GROUP_LDS_PAD");
    const bool fits = b.single_job && sh.K <= 64 && sh.M <= 8 && sh.J <= 15 &&
                      (b.variant == FJSP_VARIANT_SO_FJSSP || b.variant == FJSP_VARIANT_MO_FJSSP_DISCRETES);
    if (family == 1 && !fits) {
        set_error("fjsp_env_create_family: the batch does not fit the row kernels (one job per kind, one order, <= 64 operation "
                  "types, <= 8 machines, <= 15 jobs, SO_FJSSP / SO_DFJSP / MO_FJSSP_discretes)");
        return FJSP_E_UNSUPPORTED;
    }
    b.grp = (fits && (family == 1 || (family == -1 && !(impl && strcmp(impl, "wave") == 0)))) ? 1 : 0;
    b.kenv_first = knob("FJSP_GROUP_KENV") == 0 ? 0 : 1;
    p.early_forced = knob("FJSP_GROUP_EARLY");
    p.resident_forced = knob("FJSP_GROUP_RESIDENT");
    p.wpb_forced = knob("FJSP_GROUP_WPB");
    p.lds_pad = pad ? (size_t)atol(pad) : 0;
    p.lp_device_forced = lp ? (strcmp(lp, "device") == 0 ? 1 : (strcmp(lp, "global") == 0 ? 2 : 0)) : -1;
    const int ring = knob("FJSP_ASYNC_RING");
    p.async_ring = (ring >= 1 && ring <= 32) ? ring : 32;
    if (b.grp) { p.step = group_build(b, false, p); p.fused = group_build(b, true, p); }
    return FJSP_OK;
}

// Stage 3: the record layouts (fjsp_device.h)
int plan_layout(DevBatch &b, const Shape &sh) {
    const bool dyn = b.variant == FJSP_VARIANT_MO_DFJSP;
    // job words per record: a multiple of 64, or 16 in row-kernel batches (at most 15 jobs) -- the dynamic record of such an
    // environment then spans three 128-byte lines instead of five
    b.JP = b.grp ? 16 : ((sh.J + 63) / 64) * 64;
    b.jcap = std::min(b.JP, (sh.J + 15) / 16 * 16);
    if (step_lds_bytes(b) > 160 * 1024) {
        // four environments per workgroup keep their job tables (8 bytes per job) in the CU's 160 KB of LDS
        char msg[200];
        snprintf(msg, sizeof(msg), "instance too large for the kernels' LDS staging: %d jobs need %zu bytes per workgroup, the limit is "
                 "163840 (about %d jobs at this shape)", sh.J, step_lds_bytes(b), (int)((160 * 1024 / 4 - (30 + 3 * b.KP) * 8 - 256) / 8 / 64 * 64));
        set_error(msg);
        return FJSP_E_UNSUPPORTED;
    }
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP, JP = (size_t)b.JP;
    Layout &L = b.L;
    size_t o = 64;                                   // InstHeader, padded
    auto take = [&](size_t bytes, size_t align) { o = (o + align - 1) / align * align; size_t at = o; o += bytes; return (uint32_t)at; };
    L.i_kA = take(KP * 4, 4); L.i_kB = take(KP * 4, 4); L.i_elig = take(KP * 4, 4); L.i_fmask = take(KP * 4, 4);
    L.i_f4 = take(KP * 4, 4); L.i_rsum = take(KP * 8, 8); L.i_tsum = take(KP * 8, 8);
    L.i_due = take(JP * 4, 4); L.i_jinfo = take(JP * 4, 4); L.i_p = take(MP * KP * 2, 4);
    L.i_x = take(MP * KP * 8, 8); L.i_col = take(MP * KP * 16, 16);
    L.i_ss = take(64, 8); L.i_obs0 = take(128, 8);
    L.i_oarr = take((size_t)sh.S * 4, 4); L.i_ocnt = take((size_t)sh.S * sh.R * 2, 4);
    if (dyn) {
        L.i_pw = take(MP * KP * 2, 4); L.i_ipw = take(MP * 4, 4); L.i_bkoff = take((MP + 1) * 2, 4);
        L.i_bk = take((size_t)sh.B * 8, 8);
    }
    L.i_op = b.grp ? take(2048 + 128, 256) : 0u;
    L.i_colm = b.grp ? take(MP * 64 * 16, 128) : 0u;
    L.i_op8 = b.grp ? take(64 * 8, 128) : 0u;
    L.i_stride = (uint32_t)((o + 255) / 256 * 256);
    o = 192;                                         // EnvScalars (144 B), padded
    L.e_tend = take(MP * 4, 4); L.e_mjob = take(MP * 4, 4); L.e_jst = take(JP * 4, 4); L.e_un = take(b.single_job ? 8 : MP * KP * 8, 8); L.e_asg = take(KP, 4);
    if (b.mord) {
        L.e_q0 = take(KP * 4, 4); L.e_fmask = take(KP * 4, 4); L.e_rsum = take(KP * 8, 8); L.e_tsum = take(KP * 8, 8);
        L.e_col = take(MP * KP * 16, 16); L.e_lpq = take(KP * 4 + 8, 4);
    }
    if (dyn) L.e_dyn = take(sizeof(DynScalars) + MP * 4, 8);
    L.e_stats = b.single_job ? 0u : take(KP * 64, 64);
    L.e_stride = (uint32_t)((o + 127) / 128 * 128);
    // the kernels compute these offsets themselves (FixedOffsets, fjsp_device.h): the two must agree
    using F = FixedOffsets;
    const uint32_t kp = (uint32_t)KP, mp = (uint32_t)MP, jp = (uint32_t)JP;
    const bool same = L.i_kA == F::i_kA(kp) && L.i_kB == F::i_kB(kp) && L.i_elig == F::i_elig(kp) && L.i_fmask == F::i_fmask(kp) &&
                      L.i_f4 == F::i_f4(kp) && L.i_rsum == F::i_rsum(kp) && L.i_tsum == F::i_tsum(kp) && L.i_due == F::i_due(kp) &&
                      L.e_tend == F::e_tend() && L.e_mjob == F::e_mjob(mp) && L.e_jst == F::e_jst(mp) && L.e_un == F::e_un(mp, jp) &&
                      L.e_asg == F::e_asg(mp, jp, kp, b.single_job != 0) &&
                      (b.mord || dyn || L.e_stride == F::e_stride_plain(mp, jp, kp, b.single_job != 0));
    if (!same) { set_error("fjsp_env_create: record layout and FixedOffsets disagree (internal error)"); return FJSP_E_UNSUPPORTED; }
    return FJSP_OK;
}

}  // namespace fjsp

namespace {
// Stage 4, the static state row (i_ss)
void pack_static_state(const Instance &in, int variant, double *ss) {
    if (variant == FJSP_VARIANT_MO_FJSSP_DISCRETES) {
        // MO_FJSSP_discretes.py:55-64 static_state_extract
        long ns = 0, js = 0;
        for (int r = 0; r < in.R; ++r) { ns += in.count[r]; js += in.Jr[r]; }
        const double N_ave = (double)ns / (double)in.R, J_ave = (double)js / (double)in.R;
        double a = 0.0, c2 = 0.0;
        for (int r = 0; r < in.R; ++r) a = a + std::pow((double)in.count[r] - N_ave, 2.0);
        for (int r = 0; r < in.R; ++r) c2 = c2 + std::pow((double)in.Jr[r] - J_ave, 2.0);
        ss[0] = in.ddt; ss[1] = (double)in.M; ss[2] = (double)in.R; ss[3] = N_ave;
        ss[4] = std::sqrt(a / (double)in.R); ss[5] = J_ave; ss[6] = std::sqrt(c2 / (double)in.R);
    }
    // fluid_completed_time = max_k Q_k / rate_k, rate_k summed over machine_rj_dict in FILE order
    // (class_FJSSP.py:276-278); the SO_SFJSP reward divides by it (SO_SFJSP.py:220)
    double best = 0.0;
    bool first_k = true;
    for (int k = 0; k < in.K; ++k) {
        double acc = 0.0;
        for (int q = 0; q < in.elig_n[k]; ++q) {
            const int m = in.elig_list[(size_t)k * in.M + q];
            acc = acc + in.x[(size_t)k * in.M + m] * (1.0 / (double)in.p[(size_t)k * in.M + m]);
        }
        int r_of_k = 0;
        while (in.koff[r_of_k + 1] <= k) ++r_of_k;
        const double v = (double)in.count[r_of_k] / acc;
        if (first_k || v > best) { best = v; first_k = false; }
    }
    ss[7] = best;
}

// Stage 4: the instance record of `in` at rec (zeroed, L.i_stride bytes)
void pack_instance(const Instance &in, const DevBatch &b, bool class_fjsp, unsigned char *rec) {
    const Layout &L = b.L;
    const size_t MP = (size_t)b.MP;
    const bool dyn = b.variant == FJSP_VARIANT_MO_DFJSP;
    const int nj = in.jobs_total();
    *reinterpret_cast<InstHeader *>(rec) = InstHeader{in.K, in.M, in.R | (b.mord ? in.S << 16 : 0), nj};
    int32_t *oarr = reinterpret_cast<int32_t *>(rec + L.i_oarr);
    uint16_t *ocnt = reinterpret_cast<uint16_t *>(rec + L.i_ocnt);
    for (int so = 0; so < in.S; ++so) {
        oarr[so] = in.arrive[so];
        for (int r = 0; r < in.R; ++r) ocnt[(size_t)so * b.RP + r] = (uint16_t)in.count[(size_t)so * in.R + r];
    }
    uint32_t *kA = reinterpret_cast<uint32_t *>(rec + L.i_kA), *kB = reinterpret_cast<uint32_t *>(rec + L.i_kB);
    uint32_t *elig = reinterpret_cast<uint32_t *>(rec + L.i_elig), *first4 = reinterpret_cast<uint32_t *>(rec + L.i_f4);
    uint32_t *jinfo = reinterpret_cast<uint32_t *>(rec + L.i_jinfo);
    int32_t *due = reinterpret_cast<int32_t *>(rec + L.i_due);
    uint16_t *p = reinterpret_cast<uint16_t *>(rec + L.i_p);
    double *x = reinterpret_cast<double *>(rec + L.i_x);
    int jbeg = 0;
    for (int r = 0; r < in.R; ++r) {
        // jobs of kind r over ALL orders, numbered in arrival order (Kind.number_start, class_FJSSP.py:212-217);
        // class_FJSSP.py:214-218: r_due = round(delivery_s * J_r / N_sr); due(n) = round(r_due * n / N_sr) with
        // the ABSOLUTE job number n
        int cnt = 0;
        for (int so = 0; so < in.S; ++so) {
            const int c_s = in.count[(size_t)so * in.R + r];
            const long r_due = py_round((double)((long)in.delivery[so] * in.Jr[r]) / (double)c_s);
            for (int n = cnt; n < cnt + c_s; ++n) {
                due[jbeg + n] = (dyn || class_fjsp) ? in.delivery[so]                 // class_MODFJSP.py:224, class_FJSP.py:229
                                    : (int32_t)py_round((double)(r_due * n) / (double)c_s);
                jinfo[jbeg + n] = (uint32_t)in.koff[r] | ((uint32_t)in.Jr[r] << 16);
            }
            cnt += c_s;
        }
        for (int j = 0; j < in.Jr[r]; ++j) {
            const int k = in.koff[r] + j;
            kA[k] = (uint32_t)jbeg | ((uint32_t)cnt << 16);
            kB[k] = (uint32_t)j | ((uint32_t)in.Jr[r] << 8) | ((uint32_t)(r & 0xFF) << 16) |
                    ((uint32_t)((j == in.Jr[r] - 1 ? 1u : 0u) | 2u) << 24);
            uint32_t em = 0;
            for (int m = 0; m < in.M; ++m) {
                const int pv = in.p[(size_t)k * in.M + m];
                if (pv > 0) em |= 1u << m;
                p[(size_t)k * MP + m] = (uint16_t)pv;
                x[(size_t)k * MP + m] = in.x[(size_t)k * in.M + m];
            }
            elig[k] = em;
            uint32_t f4 = 0;
            for (int q = 0; q < in.elig_n[k] && q < 4; ++q) f4 |= (uint32_t)in.elig_list[(size_t)k * in.M + q] << (8 * q);
            first4[k] = f4;
        }
        jbeg += cnt;
    }
    if (b.grp) {
        // group kernels (fjsp_group.hip): one line of per-lane words behind the packed operation rows -- lane l:
        // len(machine l .kind_task_tuple) (the divisor of Machine.gap_ave, class_FJSSP.py:144-146) | first operation type of
        // job l << 8 | its J_r << 16 | (lanes 0, 1, 2: K, M, jobs) << 24; then the due date of job l (one job per kind: job = kind)
        uint32_t *hw = reinterpret_cast<uint32_t *>(rec + L.i_op + 2048);
        int32_t *dj = reinterpret_cast<int32_t *>(rec + L.i_op + 2048 + 64);
        for (int l = 0; l < 16; ++l) {
            uint32_t w = 0;
            if (l < in.M)
                for (int k = 0; k < in.K; ++k) w += in.p[(size_t)k * in.M + l] > 0 ? 1u : 0u;
            if (l < in.R) { w |= (uint32_t)in.koff[l] << 8; w |= (uint32_t)in.Jr[l] << 16; dj[l] = due[l]; }
            w |= (uint32_t)(l == 0 ? in.K : (l == 1 ? in.M : (l == 2 ? nj : 0))) << 24;
            hw[l] = w;
        }
    }
    if (dyn) {
        uint16_t *pw = reinterpret_cast<uint16_t *>(rec + L.i_pw);
        int32_t *ipw = reinterpret_cast<int32_t *>(rec + L.i_ipw);
        uint16_t *bko = reinterpret_cast<uint16_t *>(rec + L.i_bkoff);
        int32_t *bk = reinterpret_cast<int32_t *>(rec + L.i_bk);
        for (int k = 0; k < in.K; ++k)
            for (int m = 0; m < in.M; ++m) pw[(size_t)k * MP + m] = (uint16_t)in.power[(size_t)k * in.M + m];
        int off = 0;
        for (int m = 0; m < (int)MP; ++m) {
            bko[m] = (uint16_t)off;
            if (m < in.M) { ipw[m] = in.idle_power[m]; off += in.bk_n[m]; }
        }
        bko[MP] = (uint16_t)off;
        for (int q = 0; q < 2 * off; ++q) bk[q] = in.bk[(size_t)q];
        reinterpret_cast<double *>(rec + L.i_ss)[0] = in.ddt;                         // observation[0] = self.DDT
    }
    pack_static_state(in, b.variant, reinterpret_cast<double *>(rec + L.i_ss));
}

// Stage 5: algorithmic HBM bytes of one env-step of `in` (DESIGN.md "bytes per env-step"):
//   static per-k rows (kinfoB, elig, fmask u32; rate_sum, time_sum f64; see per_k below)    K * 28 ..
//   job table read (due, jinfo, jst) + jst write-back                               njobs * 16
//   machine lanes tend/mjob read + write                                            M * 16
//   instance header + EnvScalars read + write                                       16 + 2 * 144
//   column gather at k_sel (p u16, un/arr/rate f64) + un write                      M * 26 + 8
//   actions in, state/reward/done out                                               2 + S*8 + 8 + 1
// (per-k rows: kB, elig, fmask u32 + rate_sum, time_sum f64 = 28 B; + kA when a kind can have several jobs, + first4
//  beyond 8 machines (CPython set order); + the 64-byte statistics row, read and written, in multi-job batches)
//  single-job batches: + the assigned-machine byte; the column gather has no unprocessed entries there (p u16 + {arrival,
//  rate} f64 = 18 B per machine, one byte written) against p + unprocessed + {arrival, rate} = 26 B and 8 B written)
double step_bytes_of(const Instance &in, const DevBatch &b) {
    double bytes = step_bytes(b, in.K, in.jobs_total(), in.M);
    if (b.variant == FJSP_VARIANT_MO_DFJSP) bytes += in.M * 14.0 + 2.0 * sizeof(DynScalars);   // power column, idle power, last-task ends r/w, DynScalars r/w
    return bytes;
}

}  // namespace

namespace fjsp {
// Stage 6 (multi-order batches): the LPs of order arrivals on the device when every tableau this batch can meet
// (t[0, n): its instances', or the one worst case of a generated handle's parameters) fits the LDS of a CU.  Which service: one LP takes the device ~0.3 ms (a 48-pivot tableau of the industrial instances; a host core
// needs ~0.05 ms) but 256 of them run at once, so the device wins when arrivals come in bursts of hundreds -- measured
// (tools/bench_dynamic.py --instances industrial): 4096 envs 32.0 M env-steps/s against the host service's 34.9 M, 32768
// envs 63.1 M against 54.2 M.  Default: the device from 16384 environments on; FJSP_LP_IMPL=device / host decides for
// itself (A/B runs, and the parity test of the two).  FJSP_LP_IMPL=global (opt-in, not measured into a default yet): as device
// when every tableau fits the LDS rule; else, when every tableau is within 256 rows x 1536 columns, the same service with the
// simplex whose tableau lives in a scratch pool in global memory (fjsp_lp_global.hip); else the host.
void choose_lp_service(fjsp_env *e, const LpTableau *t, int n) {
    const DevBatch &b = e->b;
    size_t lds_max = 0, slot_max = 0;
    int K_max = 0, nr_max = 0, nc_max = 0;
    bool in_global = true;
    for (int i = 0; i < n; ++i) {
        const LpTableau &in = t[i];
        const int nr = lp_max_rows(in.K, in.M, in.R), nc = lp_max_columns(in.K, in.M, in.nx, in.R);
        lds_max = std::max(lds_max, (size_t)lp_device_lds_bytes(in.K, in.M, in.nx, in.R, b.MP));
        if (nc > kLpLdsColumns) lds_max = (size_t)1 << 30;
        const size_t slot = (size_t)fjsp_lp_global_bytes(in.K, in.M, in.nx, in.R);
        in_global = in_global && slot > 0;
        slot_max = std::max(slot_max, slot);
        K_max = std::max(K_max, in.K);
        nr_max = std::max(nr_max, nr);
        nc_max = std::max(nc_max, nc);
    }
    const bool want_device = e->plan.lp_device_forced >= 0 ? e->plan.lp_device_forced != 0 : b.N >= 16384;
    e->arr.lp_device = lds_max <= kLpLdsLimit && want_device;
    e->arr.lp_lds = e->arr.lp_device ? lds_max : 0;
    if (!e->arr.lp_device && e->plan.lp_device_forced == 2 && in_global) {
        LpGlobalPool &P = e->arr.lp_pool;
        P.slot_bytes = slot_max;
        P.slots = lp_global_slots((size_t)b.N, slot_max);
        P.lds = lp_global_lds(K_max, b.MP, b.MP, nr_max, nc_max);
        e->arr.lp_device = e->arr.lp_global = true;        // (the pool itself: alloc_arrival_staging)
    }
}

// Staging of the LP services, one slot per env (worst case: every env parks in the same launch)
int alloc_arrival_staging(fjsp_env *e) {
    DevBatch &b = e->b;
    ArrivalService &A = e->arr;
    const size_t N = (size_t)b.N, KP = (size_t)b.KP, MP = (size_t)b.MP;
    if (b.mord && (!dev_alloc(e, (N + 1) * 4, &b.pending_count, "hipMalloc pending list") ||
                   !dev_alloc(e, N * 2 * KP * 2, &b.lp_in, "hipMalloc LP inputs") || !dev_alloc(e, N * KP * MP * 8, &b.lp_x, "hipMalloc LP solutions") ||
                   !host_alloc(e, (N + 1) * 4, &A.h_pending) || !host_alloc(e, N * 2 * KP * 2, &A.h_lp_in) ||
                   !host_alloc(e, N * KP * MP * 8, &A.h_lp_x)))
        return FJSP_E_HIP;
    if (A.lp_global && !dev_alloc(e, (size_t)A.lp_pool.slots * A.lp_pool.slot_bytes, &A.lp_pool.mem, "hipMalloc LP tableau pool")) return FJSP_E_HIP;
    if (A.lp_device && (!dev_alloc(e, 8, &A.d_lp_err, "hipMalloc LP error word") || !dev_alloc(e, 16, &A.d_lp_solved, "hipMalloc LP counters")))
        return FJSP_E_HIP;
    return FJSP_OK;
}
}  // namespace fjsp

namespace {
// Stage 7: every allocation of the batch, the two slabs uploaded, then the first launches
int upload_batch(fjsp_env *e, const std::vector<unsigned char> &islab) {
    DevBatch &b = e->b;
    const size_t N = (size_t)b.N;
    if (!dev_alloc(e, islab.size(), &b.inst, "hipMalloc instance slab") || !dev_alloc(e, N * b.L.e_stride, &b.envs, "hipMalloc env slab") ||
        !dev_alloc(e, N + 16, &e->d_done_scratch, "hipMalloc scratch"))
        return FJSP_E_HIP;
    if (const int rc = alloc_arrival_staging(e)) return rc;
    if (b.grp) {       // operation types of every environment's instance (fjsp_group.hip: large-batch kernels)
        std::vector<uint8_t> kq(N);
        for (size_t q = 0; q < N; ++q) kq[q] = (uint8_t)e->inst_K[q % (size_t)b.n_inst];
        uint8_t *pk = nullptr;
        if (!dev_alloc(e, N, &pk, "hipMalloc K table") || !hip_ok(hipMemcpy(pk, kq.data(), N, hipMemcpyHostToDevice), "upload K table"))
            return FJSP_E_HIP;
        b.kenv = pk;
    }
    // every env starts done so that step() before reset() is flagged, like the
    // reference's uninitialised object would fail
    std::vector<unsigned char> eslab(N * b.L.e_stride, 0);
    for (size_t q = 0; q < N; ++q) reinterpret_cast<EnvScalars *>(eslab.data() + q * b.L.e_stride)->done = 1;
    if (!hip_ok(hipMemcpy(b.inst, islab.data(), islab.size(), hipMemcpyHostToDevice), "upload instance slab") ||
        !hip_ok(hipMemcpy(b.envs, eslab.data(), eslab.size(), hipMemcpyHostToDevice), "upload env slab"))
        return FJSP_E_HIP;
    // the fluid tables, and one reset of every env, which publishes each instance's reset observation (i_obs0, read by the
    // autoreset path of step_kernel); afterwards every env is marked done again
    if (launch_fluid_tables(b, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
        set_error("fluid_tables_kernel launch failed");
        return FJSP_E_HIP;
    }
    std::vector<int32_t> ones(N, 1);
    if (launch_reset(b, nullptr, nullptr, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy2D(b.envs + offsetof(EnvScalars, done), b.L.e_stride, ones.data(), 4, 4, N, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("initial reset failed");
        return FJSP_E_HIP;
    }
    return FJSP_OK;
}
}  // namespace

namespace fjsp {
int usable(const fjsp_env *e, const char *who, unsigned need, const uint8_t *d_actions) {
    if (e->gen_failed) {
        set_error(std::string(who) + ": the last fjsp_env_regenerate of this batch failed; regenerate it from other seeds first");
        return FJSP_E_STATE;
    }
    if ((need & kIntact) && e->failed) {
        set_error(std::string(who) + ": the order-arrival service of this batch failed earlier; destroy the batch");
        return FJSP_E_STATE;
    }
    if ((need & kIdle) && !async_idle(e)) {
        set_error(std::string(who) + ": environments are parked in the asynchronous arrival service; call fjsp_env_arrivals_flush first");
        return FJSP_E_STATE;
    }
    if (reinterpret_cast<uintptr_t>(d_actions) & 1) { set_error(std::string(who) + ": d_actions must be 2-byte aligned"); return FJSP_E_ARG; }
    return FJSP_OK;
}
}  // namespace fjsp

extern "C" {
int fjsp_env_create(const fjsp_instances *s, int32_t first, int32_t n_inst, int32_t n_envs, int32_t variant,
                    int32_t device, uint64_t rng_seed, fjsp_env **out) {
    return fjsp_env_create_family(s, first, n_inst, n_envs, variant, device, rng_seed, -1, out);
}

int fjsp_env_create_family(const fjsp_instances *s, int32_t first, int32_t n_inst, int32_t n_envs, int32_t variant,
                           int32_t device, uint64_t rng_seed, int32_t family, fjsp_env **out) {
    if (family < -1 || family > 1) { set_error("fjsp_env_create_family: family must be -1, 0 or 1"); return FJSP_E_ARG; }
    // SO_DFJSP.py = SO_FJSSP.py over class_FJSP.py: the same kernels, the order's delivery time as every job's due date
    const bool class_fjsp = variant == FJSP_VARIANT_SO_DFJSP;
    if (class_fjsp) variant = FJSP_VARIANT_SO_FJSSP;
    if (!s || !out || first < 0 || n_inst <= 0 || n_envs <= 0 || (size_t)first + (size_t)n_inst > s->v.size()) {
        set_error("fjsp_env_create: bad arguments"); return FJSP_E_ARG;
    }
    const bool dyn = variant == FJSP_VARIANT_MO_DFJSP;
    if (variant != FJSP_VARIANT_SO_FJSSP && variant != FJSP_VARIANT_SO_SFJSP && variant != FJSP_VARIANT_MO_FJSSP_DISCRETES && !dyn) {
        set_error("fjsp_env_create: unknown variant"); return FJSP_E_ARG;
    }
    Shape sh;
    int stages_max = 0;
    for (int i = 0; i < n_inst; ++i) {
        const Instance &in = s->v[(size_t)first + i];
        const int rc = check_instance(in, variant, class_fjsp, sh);
        if (rc != FJSP_OK) return rc;
        for (int r = 0; r < in.R; ++r) stages_max = std::max(stages_max, in.Jr[r]);
    }
    // A batch with order arrivals (an instance of several orders, or MO_DFJSP: plan_batch's mord) marks the jobs of orders
    // still to come with 0xFF in the byte of a job's state word that otherwise holds its next stage (kAbsent,
    // fjsp_kernels.hip), and a finished job of a kind of 255 stages carries 255 there: compute_params would count it as not
    // arrived and finish_rate would divide by too few jobs, by none once all of the kind are finished.
    if ((sh.S > 1 || dyn) && stages_max > 254) {
        set_error("more than 254 operations in a kind of a batch with order arrivals (several orders, MO_DFJSP); 255 in a "
                  "batch of single-order instances");
        return FJSP_E_UNSUPPORTED;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device visible: the environment kernels need an MI355X (there is no CPU path)");
        return FJSP_E_HIP;
    }
    if (device < 0 || device >= ndev) { set_error("fjsp_env_create: device index out of range"); return FJSP_E_ARG; }
    DeviceGuard guard(device);

    // every failing exit from here on tears the handle down with fjsp_env_destroy
    std::unique_ptr<fjsp_env, void (*)(fjsp_env *)> e(new fjsp_env(), fjsp_env_destroy);
    e->device = device; e->src = s; e->first = first;
    DevBatch &b = e->b;
    int rc = plan_batch(b, e->plan, sh, n_inst, n_envs, variant, rng_seed, family);
    if (rc != FJSP_OK) return rc;

    std::vector<unsigned char> islab((size_t)n_inst * b.L.i_stride, 0);
    double bytes = 0.0;
    for (int i = 0; i < n_inst; ++i) {
        const Instance &in = s->v[(size_t)first + i];
        pack_instance(in, b, class_fjsp, islab.data() + (size_t)i * b.L.i_stride);
        bytes += step_bytes_of(in, b);
        e->inst_K.push_back(in.K); e->inst_M.push_back(in.M);
        e->ops_max = std::max(e->ops_max, in.ops_total());
    }
    e->step_bytes = (int64_t)(bytes / (double)n_inst + 0.5);
    uint64_t h = 1469598103934665603ULL;
    for (unsigned char c : islab) h = (h ^ c) * 1099511628211ULL;
    e->inst_hash = h;

    if (b.mord) {
        std::vector<LpTableau> t;
        for (int i = 0; i < n_inst; ++i) {
            const Instance &in = s->v[(size_t)first + i];
            int nx = 0;
            for (int v : in.p) nx += v > 0 ? 1 : 0;
            t.push_back(LpTableau{in.K, in.M, nx, in.R});
        }
        choose_lp_service(e.get(), t.data(), n_inst);
    }
    if ((rc = upload_batch(e.get(), islab)) != FJSP_OK) return rc;
    *out = e.release();
    return FJSP_OK;
}

void fjsp_env_destroy(fjsp_env *e) {
    if (!e) return;
    {
        DeviceGuard guard(e->device);
        arrivals_release(e->arr);           // (first: its LP threads write into pinned memory)
        for (void *p : e->dev_allocs) (void)hipFree(p);
        for (void *p : e->host_allocs) (void)hipHostFree(p);
        if (e->sched.rec) (void)hipFree(e->sched.rec);
    }
    generated_release(e);
    delete e;
}

int fjsp_env_num_envs(const fjsp_env *e) { return e ? e->b.N : 0; }
int fjsp_env_state_size(const fjsp_env *e) { return e ? e->b.state_size : 0; }
int fjsp_env_device(const fjsp_env *e) { return e ? e->device : -1; }
int64_t fjsp_env_step_bytes(const fjsp_env *e) { return e ? e->step_bytes : 0; }
int fjsp_env_kernel_family(const fjsp_env *e) { return e ? e->b.grp : 0; }
int fjsp_env_row_build(const fjsp_env *e, int32_t fused, int32_t *out3) {
    if (!e || !out3) { set_error("fjsp_env_row_build: null argument"); return FJSP_E_ARG; }
    if (!e->b.grp) { set_error("fjsp_env_row_build: the batch is stepped by the one-wave-per-environment kernels"); return FJSP_E_UNSUPPORTED; }
    const GroupBuild &g = fused ? e->plan.fused : e->plan.step;
    out3[0] = g.early; out3[1] = g.mpc; out3[2] = g.resident;
    return FJSP_OK;
}
int fjsp_env_lp_on_device(const fjsp_env *e) { return (e && e->arr.lp_device) ? (e->arr.lp_global ? 2 : 1) : 0; }

int fjsp_env_reset(fjsp_env *e, const uint8_t *d_mask, double *d_state, void *stream) {
    if (!e) { set_error("fjsp_env_reset: null env"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_reset", kIdle)) return rc;
    DeviceGuard guard(e->device);
    if (launch_reset(e->b, d_mask, d_state, (hipStream_t)stream) != 0) { set_error("reset_kernel launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

int fjsp_env_step_traced(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset, double *d_state,
                         double *d_reward, uint8_t *d_done, int16_t *d_trace_km, void *stream) {
    if (!e || !d_actions) { set_error("fjsp_env_step: null argument"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_step", kIntact | kIdle, d_actions)) return rc;
    DeviceGuard guard(e->device);
    if (launch_step(e->b, e->plan, d_actions, d_mo, autoreset ? 1 : 0, d_state, d_reward, d_done, d_trace_km, (hipStream_t)stream, nullptr, e->sched) != 0) {
        set_error("step_kernel launch failed"); return FJSP_E_HIP;
    }
    if (e->b.mord) return service_arrivals(e, d_mo, d_state, d_reward, d_done, d_trace_km, (hipStream_t)stream);
    return FJSP_OK;
}

int fjsp_env_step(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset, double *d_state,
                  double *d_reward, uint8_t *d_done, void *stream) {
    return fjsp_env_step_traced(e, d_actions, d_mo, autoreset, d_state, d_reward, d_done, nullptr, stream);
}

int fjsp_env_rollout(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t T, int16_t *d_trace_km,
                     double *d_reward, double *d_state_last, void *stream) {
    if (!e || !d_actions || T <= 0) { set_error("fjsp_env_rollout: bad arguments"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_rollout", kIntact | kIdle, d_actions)) return rc;
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    if (!e->b.mord && rollout_lds_bytes(e->b) <= 64 * 1024) {
        if (launch_rollout(e->b, e->plan, d_actions, d_mo, T, d_trace_km, d_reward, d_state_last, st, e->sched) != 0) {
            set_error("rollout_kernel launch failed"); return FJSP_E_HIP;
        }
        return FJSP_OK;
    }
    // instance too large for the LDS-resident fused kernel: T step launches on the same stream
    const size_t N = (size_t)e->b.N;
    for (int s2 = 0; s2 < T; ++s2) {
        if (launch_step(e->b, e->plan, d_actions + (size_t)s2 * N * 2, d_mo, 2, d_state_last, d_reward ? d_reward + (size_t)s2 * N : nullptr,
                        e->d_done_scratch, d_trace_km ? d_trace_km + (size_t)s2 * N * 2 : nullptr, st, nullptr, e->sched) != 0) {
            set_error("step_kernel launch failed"); return FJSP_E_HIP;
        }
        if (e->b.mord) {
            const int rc2 = service_arrivals(e, d_mo, d_state_last, d_reward ? d_reward + (size_t)s2 * N : nullptr, e->d_done_scratch,
                                             d_trace_km ? d_trace_km + (size_t)s2 * N * 2 : nullptr, st);
            if (rc2 != FJSP_OK) return rc2;
        }
    }
    return FJSP_OK;
}

namespace {
const char kActorShape[] = "the in-kernel actor is state_size (<= 32) -> 128 -> 128 -> n_actions (<= 32)";
bool actor_ok(const fjsp_actor_params *a) {
    return a && a->w1 && a->b1 && a->w2 && a->b2 && a->w3 && a->b3 && a->hidden == kActorH && a->state_size > 0 &&
           a->state_size <= 32 && a->n_actions > 0 && a->n_actions <= kActorAP;
}
ActorParams actor_of(const fjsp_actor_params *a) {
    ActorParams p;
    p.w1 = a->w1; p.b1 = a->b1; p.w2 = a->w2; p.b2 = a->b2; p.w3 = a->w3; p.b3 = a->b3;
    p.S = a->state_size; p.H = a->hidden; p.A = a->n_actions;
    return p;
}
int refuse(const char *who, const char *why, int rc) { set_error(std::string(who) + ": " + why); return rc; }

// The two routes of the policy kernels through an episode.  kOneLaunch (fjsp_env_rollout_policy, fjsp_env_play_policy,
// fjsp_env_policy_build): a single-order batch, the whole call in one launch.  kSegments (their _orders twins): a batch with
// order arrivals, one launch per segment, the arrival service between the launches.
enum PolicyRoute { kOneLaunch, kSegments };
// What keeps the policy kernels from running this batch on `route`, nullptr where nothing does.  g == nullptr asks about the
// kind of batch alone; otherwise also whether a workgroup exists for an actor of state size S, and *g is the workgroup the
// kernels run then (policy_geometry, fjsp_kernels.hip).
const char *policy_refusal(const fjsp_env *e, PolicyRoute route, int S = 0, PolicyGeometry *g = nullptr) {
    if (route == kOneLaunch && e->b.mord)
        return "the batch has order arrivals (their LPs are served between launches): single-order batches only";
    if (route == kSegments && e->b.variant == FJSP_VARIANT_MO_DFJSP)
        return "MO_DFJSP batches are not played inside the launch (their 12 x 10 actions do not fit the in-kernel actor)";
    if (route == kSegments && !e->b.mord)
        return "the batch has no order arrivals: fjsp_env_play_policy / fjsp_env_rollout_policy run it in one launch";
    if (!g) return nullptr;
    *g = policy_geometry(e->b, S);
    return g->envs > 0 ? nullptr : "one environment's LDS slice does not fit the 160 KB of a CU beside the actor's weights";
}
// The first checks the launching entries share once their own arguments are in order.  Their order decides the text when
// two things are wrong at once: the segmented entries ask about the kind of batch before the actor's shape, the one-launch
// entries after everything else (policy_refusal with the workgroup, which every entry asks last).
int actor_refusal(const fjsp_env *e, const char *who, PolicyRoute route, const fjsp_actor_params *actor) {
    if (route == kSegments)
        if (const char *why = policy_refusal(e, route)) return refuse(who, why, FJSP_E_UNSUPPORTED);
    if (!actor_ok(actor) || actor->state_size != e->b.state_size) return refuse(who, kActorShape, FJSP_E_UNSUPPORTED);
    return FJSP_OK;
}
// Between two segments: the LPs of the envs the last launch parked, then arrival_kernel into the rows given.  *more = false
// where the service knows that nothing parked (the host route fetches the count anyway): every env has finished or reached T.
int serve_segment(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, hipStream_t st, bool *more) {
    const int rc = service_arrivals(e, d_mo, d_state, d_reward, d_done, nullptr, st);
    *more = rc == FJSP_OK && (e->arr.lp_device || e->arr.h_pending[0] != 0);
    return rc;
}
// The rollout's per-env progress between segments: next_t i32[N], the arrival's reward f64[N], parked u8[N]; owned by the
// handle, allocated by the first segmented rollout
int segment_scratch(fjsp_env *e) {
    if (e->d_seg_reward) return FJSP_OK;
    const size_t N = (size_t)e->b.N;
    double *p = nullptr;
    if (!dev_alloc(e, N * 8 + N * 4 + N, &p, "hipMalloc (segment scratch)")) return FJSP_E_HIP;
    e->d_seg_reward = p;
    return FJSP_OK;
}

int rollout_policy(const char *who, PolicyRoute route, fjsp_env *e, fjsp_rollout *buf, const fjsp_actor_params *actor, const float *d_epsilon,
                   const uint64_t *d_seed, int32_t pair_div, int32_t T, const double *d_mo, const double *d_state_in,
                   float *d_flat_actions, float *d_log_prob, double *d_state_last, void *stream) {
    if (!e || !buf || !d_epsilon || !d_seed || !d_state_in || !d_flat_actions || !d_log_prob || !d_state_last || T <= 0 || pair_div < 0)
        return refuse(who, "bad arguments", FJSP_E_ARG);
    if (const int rc = usable(e, who, route == kSegments ? kIntact | kIdle : kIntact)) return rc;
    if (buf->N != e->b.N || buf->S != e->b.state_size || buf->T < T || buf->device != e->device)
        return refuse(who, "the rollout buffer does not match the batch (N, state_size, T, device)", FJSP_E_ARG);
    if (const int rc = actor_refusal(e, who, route, actor)) return rc;
    PolicyGeometry geo{};
    if (const char *why = policy_refusal(e, route, actor->state_size, &geo)) return refuse(who, why, FJSP_E_UNSUPPORTED);
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    PolicyRolloutIO io;
    io.state_in = d_state_in; io.epsilon = d_epsilon; io.seed = d_seed; io.pair_div = pair_div;
    io.o_state = buf->states; io.o_actions = buf->actions; io.o_reward = buf->rewards; io.o_next = buf->next_states;
    io.o_done = buf->dones; io.o_valid = buf->valid; io.o_flat = d_flat_actions; io.o_logp = d_log_prob; io.state_last = d_state_last;
    PolicySegment sg{};
    if (route == kSegments) {
        if (const int rc = segment_scratch(e)) return rc;
        const size_t N = (size_t)e->b.N;
        sg.next_t = reinterpret_cast<int32_t *>(e->d_seg_reward + N); sg.parked = reinterpret_cast<uint8_t *>(sg.next_t + N);
        sg.reward = e->d_seg_reward; sg.done = e->d_done_scratch;
    }
    const ActorParams ap = actor_of(actor);
    const int segments = route == kSegments ? e->b.SP : 1;      // (the one-launch route: one segment, no service)
    for (int seg = 0; seg < segments; ++seg) {
        sg.seg = seg;
        if (launch_rollout_policy(e->b, ap, io, route == kSegments ? &sg : nullptr, d_mo, T, st, e->sched) != 0) {
            set_error(route == kSegments ? "rollout_policy_orders_kernel launch failed" : "rollout_policy_kernel launch failed"); return FJSP_E_HIP;
        }
        if (seg + 1 == segments) break;          // (an env of S orders parks S - 1 times at most: nothing parked in the last launch)
        bool more = false;
        if (const int rc = serve_segment(e, d_mo, d_state_last, e->d_seg_reward, e->d_done_scratch, st, &more)) return rc;
        if (!more) break;
    }
    buf->len = T;
    return FJSP_OK;
}

int play_policy(const char *who, PolicyRoute route, fjsp_env *e, const fjsp_actor_params *actor, int32_t pair_div, int32_t n_greedy,
                const uint64_t *d_seed, int32_t T, const double *d_mo, const double *d_state_in, int32_t n_state_in, const int32_t *d_state_src,
                const uint8_t *d_first, uint8_t *d_actions_out, int32_t *d_steps_out, double *d_state_last, double *d_reward_last,
                uint8_t *d_done_last, void *stream) {
    if (!e || T <= 0 || n_greedy < 0 || pair_div < 0 || !d_state_in || n_state_in <= 0 || !d_steps_out || !d_state_last ||
        !d_reward_last || !d_done_last)
        return refuse(who, "bad arguments", FJSP_E_ARG);
    if (const int rc = usable(e, who, route == kSegments ? kIntact | kIdle : kIntact)) return rc;
    if (const int rc = actor_refusal(e, who, route, actor)) return rc;
    if (pair_div > 0 && actor->n_actions % pair_div != 0) return refuse(who, "pair_div does not divide n_actions", FJSP_E_ARG);
    if (n_greedy < e->b.N && !d_seed) return refuse(who, "sampling envs need d_seed", FJSP_E_ARG);
    if (!d_state_src && n_state_in < e->b.N) return refuse(who, "d_state_in has fewer rows than the batch", FJSP_E_ARG);
    PolicyGeometry geo{};
    if (const char *why = policy_refusal(e, route, actor->state_size, &geo)) return refuse(who, why, FJSP_E_UNSUPPORTED);
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    PolicyPlayIO io;
    io.state_in = d_state_in; io.state_src = d_state_src; io.n_state_in = n_state_in; io.seed = d_seed; io.first = d_first;
    io.pair_div = pair_div; io.n_greedy = n_greedy; io.actions_out = d_actions_out; io.steps_out = d_steps_out;
    io.state_last = d_state_last; io.reward_last = d_reward_last; io.done_last = d_done_last;
    const ActorParams ap = actor_of(actor);
    const int segments = route == kSegments ? e->b.SP : 1;      // (the one-launch route: one segment, no service)
    for (int seg = 0; seg < segments; ++seg) {
        if (launch_play_policy(e->b, ap, io, d_mo, T, seg, st, e->sched) != 0) {
            set_error(route == kSegments ? "play_policy_orders_kernel launch failed" : "play_policy_kernel launch failed"); return FJSP_E_HIP;
        }
        if (seg + 1 == segments) break;          // (an env of S orders parks S - 1 times at most: nothing parked in the last launch)
        bool more = false;
        if (const int rc = serve_segment(e, d_mo, d_state_last, d_reward_last, d_done_last, st, &more)) return rc;
        if (!more) break;
    }
    return FJSP_OK;
}

// out: envs per workgroup, its LDS bytes, KC; the segmented route adds the policy launches of one call at most
int policy_build(const char *who, PolicyRoute route, const fjsp_env *e, int32_t state_size, int32_t *out) {
    if (!e || !out) return refuse(who, "null argument", FJSP_E_ARG);
    if (state_size < 1 || state_size > 32) return refuse(who, "state_size outside 1..32", FJSP_E_ARG);
    PolicyGeometry geo{};
    if (const char *why = policy_refusal(e, route, state_size, &geo)) return refuse(who, why, FJSP_E_UNSUPPORTED);
    out[0] = geo.envs; out[1] = (int32_t)geo.lds; out[2] = e->b.KC;
    if (route == kSegments) out[3] = e->b.SP;
    return FJSP_OK;
}
}  // namespace

int fjsp_actor_forward(const fjsp_actor_params *actor, const double *d_state, int32_t n, float *d_probs, void *stream) {
    if (!d_state || !d_probs || n <= 0) { set_error("fjsp_actor_forward: bad arguments"); return FJSP_E_ARG; }
    if (!actor_ok(actor)) return refuse("fjsp_actor_forward", kActorShape, FJSP_E_UNSUPPORTED);
    if (launch_actor_forward(actor_of(actor), d_state, n, d_probs, (hipStream_t)stream) != 0) { set_error("actor_forward_kernel launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

int fjsp_env_rollout_policy(fjsp_env *e, fjsp_rollout *buf, const fjsp_actor_params *actor, const float *d_epsilon,
                            const uint64_t *d_seed, int32_t pair_div, int32_t T, const double *d_mo, const double *d_state_in,
                            float *d_flat_actions, float *d_log_prob, double *d_state_last, void *stream) {
    return rollout_policy("fjsp_env_rollout_policy", kOneLaunch, e, buf, actor, d_epsilon, d_seed, pair_div, T, d_mo, d_state_in, d_flat_actions,
                          d_log_prob, d_state_last, stream);
}
int fjsp_env_play_policy(fjsp_env *e, const fjsp_actor_params *actor, int32_t pair_div, int32_t n_greedy, const uint64_t *d_seed,
                         int32_t T, const double *d_mo, const double *d_state_in, int32_t n_state_in, const int32_t *d_state_src,
                         const uint8_t *d_first, uint8_t *d_actions_out, int32_t *d_steps_out, double *d_state_last,
                         double *d_reward_last, uint8_t *d_done_last, void *stream) {
    return play_policy("fjsp_env_play_policy", kOneLaunch, e, actor, pair_div, n_greedy, d_seed, T, d_mo, d_state_in, n_state_in, d_state_src,
                       d_first, d_actions_out, d_steps_out, d_state_last, d_reward_last, d_done_last, stream);
}
int fjsp_env_policy_build(const fjsp_env *e, int32_t state_size, int32_t *out3) {
    return policy_build("fjsp_env_policy_build", kOneLaunch, e, state_size, out3);
}

// ---- the same on batches with order arrivals: one policy launch per segment, the arrival service between them
int fjsp_env_rollout_policy_orders(fjsp_env *e, fjsp_rollout *buf, const fjsp_actor_params *actor, const float *d_epsilon,
                                   const uint64_t *d_seed, int32_t pair_div, int32_t T, const double *d_mo, const double *d_state_in,
                                   float *d_flat_actions, float *d_log_prob, double *d_state_last, void *stream) {
    return rollout_policy("fjsp_env_rollout_policy_orders", kSegments, e, buf, actor, d_epsilon, d_seed, pair_div, T, d_mo, d_state_in,
                          d_flat_actions, d_log_prob, d_state_last, stream);
}
int fjsp_env_play_policy_orders(fjsp_env *e, const fjsp_actor_params *actor, int32_t pair_div, int32_t n_greedy, const uint64_t *d_seed,
                                int32_t T, const double *d_mo, const double *d_state_in, int32_t n_state_in, const int32_t *d_state_src,
                                const uint8_t *d_first, uint8_t *d_actions_out, int32_t *d_steps_out, double *d_state_last,
                                double *d_reward_last, uint8_t *d_done_last, void *stream) {
    return play_policy("fjsp_env_play_policy_orders", kSegments, e, actor, pair_div, n_greedy, d_seed, T, d_mo, d_state_in, n_state_in,
                       d_state_src, d_first, d_actions_out, d_steps_out, d_state_last, d_reward_last, d_done_last, stream);
}
int fjsp_env_policy_orders_build(const fjsp_env *e, int32_t state_size, int32_t *out4) {
    return policy_build("fjsp_env_policy_orders_build", kSegments, e, state_size, out4);
}

int fjsp_env_read(fjsp_env *e, int64_t *d_delay_time_sum, int32_t *d_makespan, int32_t *d_completion,
                  int32_t *d_step_time, int32_t *d_step_count, uint8_t *d_done, uint32_t *d_status, void *stream) {
    if (!e) { set_error("fjsp_env_read: null env"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_read", kIntact | kIdle)) return rc;
    DeviceGuard guard(e->device);
    if (launch_read(e->b, d_delay_time_sum, d_makespan, d_completion, d_step_time, d_step_count, d_done, d_status,
                    (hipStream_t)stream) != 0) { set_error("read_kernel launch failed"); return FJSP_E_HIP; }
    if (e->arr.lp_device) {    // a failed device LP surfaces here (read-back is where callers synchronise anyway)
        uint32_t err = 0;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        HIP_TRY(hipMemcpy(&err, e->arr.d_lp_err, 4, hipMemcpyDeviceToHost));
        if (err) { e->failed = true; set_error("an order-arrival LP failed on the device (code " + std::to_string(err) + "); the batch is unusable: destroy it"); return FJSP_E_LP; }
    }
    return FJSP_OK;
}

int fjsp_env_record_schedule(fjsp_env *e, int32_t on) {
    if (!e) { set_error("fjsp_env_record_schedule: null env"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_record_schedule", kIntact | kIdle)) return rc;
    DeviceGuard guard(e->device);
    const size_t N = (size_t)e->b.N;
    // the episode state read below must include every step still queued, on whatever stream the caller used
    HIP_TRY(hipDeviceSynchronize());
    {   // every env must be between episodes: done (as create leaves it) or reset with nothing dispatched yet
        int32_t *d_cnt = nullptr;
        HIP_TRY(hipMalloc(&d_cnt, N * 5));
        uint8_t *d_done = reinterpret_cast<uint8_t *>(d_cnt + N);
        std::vector<int32_t> cnt(N);
        std::vector<uint8_t> done(N);
        const bool ok = launch_read(e->b, nullptr, nullptr, nullptr, nullptr, d_cnt, d_done, nullptr, nullptr) == 0 &&
                        hipDeviceSynchronize() == hipSuccess &&
                        hipMemcpy(cnt.data(), d_cnt, N * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                        hipMemcpy(done.data(), d_done, N, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(d_cnt);
        if (!ok) { set_error("fjsp_env_record_schedule: read-back of the episode state failed"); return FJSP_E_HIP; }
        for (size_t i = 0; i < N; ++i)
            if (!done[i] && cnt[i] != 0) {
                set_error("fjsp_env_record_schedule: env " + std::to_string(i) + " is mid-episode; switch recording after create, after a reset or once every env is done");
                return FJSP_E_STATE;
            }
    }
    if (!on) {
        if (e->sched.rec) HIP_TRY(hipFree(e->sched.rec));
        e->sched = SchedRec{};
        return FJSP_OK;
    }
    if (e->sched.rec) return FJSP_OK;
    if (e->ops_max <= 0) { set_error("fjsp_env_record_schedule: the batch has no operations"); return FJSP_E_STATE; }
    uint4 *d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)e->ops_max * N * sizeof(uint4)));
    if (hipMemset(d, 0, (size_t)e->ops_max * N * sizeof(uint4)) != hipSuccess) {
        (void)hipFree(d);
        set_error("fjsp_env_record_schedule: hipMemset of the record table failed");
        return FJSP_E_HIP;
    }
    e->sched.rec = d;
    e->sched.cap = e->ops_max;
    return FJSP_OK;
}

int fjsp_env_schedule_capacity(const fjsp_env *e) { return (e && e->sched.rec) ? e->sched.cap : 0; }

int fjsp_env_schedule(fjsp_env *e, int32_t *d_table, int32_t *d_len, void *stream) {
    if (!e || !d_table) { set_error("fjsp_env_schedule: null argument"); return FJSP_E_ARG; }
    if (!e->sched.rec) { set_error("fjsp_env_schedule: recording is off (fjsp_env_record_schedule)"); return FJSP_E_STATE; }
    if (const int rc = usable(e, "fjsp_env_schedule", kIdle)) return rc;
    DeviceGuard guard(e->device);
    if (launch_schedule_unpack(e->b, e->sched, d_table, d_len, (hipStream_t)stream) != 0) { set_error("schedule_unpack_kernel launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

int fjsp_env_machine_time_end(fjsp_env *e, int32_t *d_tend, int32_t m_stride, void *stream) {
    if (!e || !d_tend || m_stride < e->b.MP) { set_error("fjsp_env_machine_time_end: bad arguments"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    HIP_TRY(hipMemcpy2DAsync(d_tend, (size_t)m_stride * 4, e->b.envs + e->b.L.e_tend, (size_t)e->b.L.e_stride,
                             (size_t)e->b.MP * 4, (size_t)e->b.N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FJSP_OK;
}

int fjsp_env_energy(fjsp_env *e, int64_t *d_energy, void *stream) {
    if (!e || !d_energy) { set_error("fjsp_env_energy: null argument"); return FJSP_E_ARG; }
    if (e->b.variant != FJSP_VARIANT_MO_DFJSP) { set_error("fjsp_env_energy: not a MO_DFJSP batch"); return FJSP_E_STATE; }
    DeviceGuard guard(e->device);
    HIP_TRY(hipMemcpy2DAsync(d_energy, 8, e->b.envs + e->b.L.e_dyn, (size_t)e->b.L.e_stride, 8, (size_t)e->b.N,
                             hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FJSP_OK;
}

int fjsp_pyset_and_order(uint32_t idle_mask, const int32_t *machines, int32_t n, int32_t ascending, int32_t *out) {
    if (!out || (n > 0 && !machines) || n < 0 || n > 32) { set_error("fjsp_pyset_and_order: bad arguments"); return FJSP_E_ARG; }
    uint32_t bm = 0, f4 = 0;
    for (int q = 0; q < n; ++q) {
        if (machines[q] < 0 || machines[q] > 31) { set_error("fjsp_pyset_and_order: machine index out of range"); return FJSP_E_ARG; }
        bm |= 1u << machines[q];
        if (q < 4) f4 |= (uint32_t)machines[q] << (8 * q);
    }
    const CandList c = pyset_and(idle_mask, bm, f4, ascending != 0);
    for (int i = 0; i < c.n; ++i) out[i] = cand_at(c, i);
    return c.n;
}

int fjsp_env_fluid_tables(fjsp_env *e, int32_t i, double *h_rate, double *h_arr, double *h_rate_sum, double *h_time_sum) {
    if (!e || i < 0 || i >= e->b.N) { set_error("fjsp_env_fluid_tables: bad arguments"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_fluid_tables", 0)) return rc;
    DeviceGuard guard(e->device);
    const int inst = i % e->b.n_inst;
    const int K = e->inst_K[(size_t)inst], M = e->inst_M[(size_t)inst];
    const size_t KP = (size_t)e->b.KP, MP = (size_t)e->b.MP;
    std::vector<double> col(MP * KP * 2), rs(KP), ts(KP);
    HIP_TRY(hipDeviceSynchronize());
    const unsigned char *rec = e->b.inst + (size_t)inst * e->b.L.i_stride;
    HIP_TRY(hipMemcpy(col.data(), rec + e->b.L.i_col, MP * KP * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rs.data(), rec + e->b.L.i_rsum, KP * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ts.data(), rec + e->b.L.i_tsum, KP * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) {
        for (int m = 0; m < M; ++m) {
            if (h_rate) h_rate[(size_t)k * M + m] = col[((size_t)k * MP + m) * 2 + 1];
            if (h_arr) h_arr[(size_t)k * M + m] = col[((size_t)k * MP + m) * 2];
        }
        if (h_rate_sum) h_rate_sum[k] = rs[(size_t)k];
        if (h_time_sum) h_time_sum[k] = ts[(size_t)k];
    }
    return FJSP_OK;
}
}  // extern "C"
