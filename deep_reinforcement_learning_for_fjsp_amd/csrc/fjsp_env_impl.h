// The env handle behind the C ABI, shared by fjsp_env.hip (create, step, read-back), fjsp_arrivals.hip (order-arrival
// services) and fjsp_snapshot.hip (saved states).  Private: not part of include/fjsp_amd.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fjsp_amd.h"
#include "fjsp_device.h"
#include "fjsp_host.h"
#include "fjsp_lp_limits.h"

namespace fjsp {
struct LpCache; struct AsyncRing; struct LpPool;   // fjsp_arrivals.hip; fjsp_lp_pool.h
struct GenState;                                   // fjsp_generate.hip

// largest sizes over the instances of a batch
struct Shape {
    int K = 0, M = 0, J = 0, S = 1, R = 0, B = 1;    // B: breakdown windows of one instance (MO_DFJSP)
    bool single_job = true;                           // one order, one job per kind, in every instance
};

// What only the order-arrival services of multi-order batches use (fjsp_arrivals.hip)
struct ArrivalService {
    // pinned staging of the blocking host service: [0] = count, then env ids | LP inputs per slot | solutions per slot
    uint32_t *h_pending = nullptr;
    uint16_t *h_lp_in = nullptr;
    double *h_lp_x = nullptr;
    LpPool *pool = nullptr;     // host threads of the blocking service and of a generated handle's host LP route (lp_pool_of)
    AsyncRing *ring = nullptr;  // the asynchronous service (fjsp_env_step_async), built by its first call
    LpCache *cache = nullptr;   // solved LPs of the host services
    int lp_threads = 0;         // 0 = default (min(host cores, 16))
    int64_t lp_solves = 0;      // order-arrival LPs solved so far (host services)
    int64_t parked = 0;         // envs currently parked in the asynchronous service (host view)
    // device LP service (fjsp_lp_device.hip): chosen at create time when the largest tableau of the batch fits the CU's LDS
    bool lp_device = false;
    size_t lp_lds = 0;
    // ... or, under FJSP_LP_IMPL=global, when it does not but stays within 256 rows x 1536 columns (fjsp_lp_global.hip: the
    // tableau in a scratch pool in global memory); lp_device is set as well: the service's launches differ in the LP kernel alone
    bool lp_global = false;
    LpGlobalPool lp_pool;
    uint32_t *d_lp_err = nullptr;                // [0] nonzero: an LP failed on the device (reported at the next synchronising call)
    unsigned long long *d_lp_solved = nullptr;   // LPs solved on the device so far, [1] their pivots
};

// The LP shape of one instance of a batch, what a host arrival LP reads of it (lp_shape_of below): the host Instance's arrays,
// or on a generated handle those of its mirror
struct LpShape { int R = 0, M = 0, K = 0; const int *Jr = nullptr, *p = nullptr; };   // Jr[R]; p[K][M] unpadded
// The head of a packed record (pack_instance, generate_pack_kernel) back on the host: of a generated handle's host LP route,
// and the entries of fjsp_env::lp_mirror
struct RecordHead { InstHeader h{}; std::vector<int> Jr, count, p; };      // h.R without the order count; [R], [R] jobs of every kind in order 0, [K][M] unpadded
}  // namespace fjsp

struct fjsp_env {
    fjsp::DevBatch b{};
    fjsp::LaunchPlan plan;             // which build of the kernels the launchers run for this batch, decided at create (plan_launch)
    int device = 0;
    std::vector<void *> dev_allocs, host_allocs;   // device / pinned memory, freed by fjsp_env_destroy
    std::vector<int> inst_K, inst_M;   // per packed instance
    int ops_max = 0;                   // operations of the largest instance, orders that arrive later included (schedule slots)
    fjsp::SchedRec sched;              // dispatch records while recording is on (fjsp_env_record_schedule); rec == nullptr: off
    uint64_t inst_hash = 0;            // FNV-1a of the packed instance slab as uploaded (snapshot compatibility, fjsp_snapshot_*)
    int64_t step_bytes = 0;
    uint8_t *d_done_scratch = nullptr; // scratch for the non-fused rollout fallback
    uint2 *d_decode_kinds = nullptr;   // fjsp_schedule_decode's kind table, [n_inst][KP + 1] (first use; refilled by every call)
    uint2 *d_active_ws = nullptr;      // fjsp_schedule_decode_active's interval entries, [groups][cap][G] (first use; shared by the handle's calls)
    double *d_seg_reward = nullptr;    // fjsp_env_rollout_policy_orders between its segments: reward f64[N] | next_t i32[N] | parked u8[N] (first use)
    const fjsp_instances *src = nullptr;   // the instances [first, first + n_inst) the batch plays (the host LPs read them)
    int first = 0;
    bool failed = false;        // the arrival service failed mid-step: parked envs are in limbo, the handle refuses further steps
    fjsp::ArrivalService arr;
    // handles of fjsp_env_create_generated* only (fjsp_generate.hip): the device generator's buffers and parameters.  Such a
    // handle has no host instance set (src == nullptr); a multi-order one keeps lp_mirror for its host arrival LPs.
    fjsp::GenState *gen = nullptr;
    std::vector<fjsp::RecordHead> lp_mirror;   // [n_inst] the records' heads as of the last regenerate (a masked one regathers its own); empty: not gathered (refresh_lp_mirror)
    bool gen_failed = false;    // the last fjsp_env_regenerate / _regenerate_masked failed: reset / step / rollout are refused until one succeeds
};

namespace fjsp {
inline bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
#define HIP_TRY(expr)                                  \
    do {                                               \
        if (!hip_ok((expr), #expr)) return FJSP_E_HIP; \
    } while (0)

// Zeroed device memory / pinned host memory owned by the handle: fjsp_env_destroy frees it.  (At least 16 bytes: a
// generated handle's lists can be empty.)
template <class T>
bool dev_alloc(fjsp_env *e, size_t bytes, T **d, const char *what) {
    void *p = nullptr;
    bytes = std::max<size_t>(bytes, 16);
    if (!hip_ok(hipMalloc(&p, bytes), what)) return false;
    e->dev_allocs.push_back(p);
    *d = static_cast<T *>(p);
    return hip_ok(hipMemset(p, 0, bytes), "hipMemset");
}
template <class T>
bool host_alloc(fjsp_env *e, size_t bytes, T **h) {
    void *p = nullptr;
    if (!hip_ok(hipHostMalloc(&p, std::max<size_t>(bytes, 16), hipHostMallocDefault), "hipHostMalloc")) return false;
    e->host_allocs.push_back(p);
    *h = static_cast<T *>(p);
    return true;
}

// Algorithmic HBM bytes of one env-step of an instance of K operation types, `jobs` jobs, M machines (the terms: step_bytes_of, fjsp_env.hip)
inline double step_bytes(const DevBatch &b, int K, int jobs, int M) {
    const double per_k = 28.0 + (b.single_job ? 1.0 : 4.0) + (b.MP > 8 ? 4.0 : 0.0) + (b.single_job ? 0.0 : 128.0);
    const double gather = b.single_job ? M * 18.0 + 1.0 : M * 26.0 + 8.0;
    return K * per_k + jobs * 16.0 + M * 16.0 + 304.0 + gather + 2.0 + b.state_size * 8.0 + 9.0;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        // (the common case -- the caller is already on the batch's device -- costs one hipGetDevice: the per-step
        // calls are launch-bound on the host)
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// The refusals the entry points share, after their own argument checks; who names the entry point in the message.
// kIntact: the arrival service has not failed; kIdle: no env is parked in the asynchronous service; d_actions, if
// given, is 2-byte aligned.
enum : unsigned { kIntact = 1, kIdle = 2 };
int usable(const fjsp_env *e, const char *who, unsigned need, const uint8_t *d_actions = nullptr);

// fjsp_arrivals.hip: after a step launch of a multi-order batch, solve the LP of every env it parked at an order arrival
// and let arrival_kernel finish those steps (a failure marks the handle failed)
int service_arrivals(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, int16_t *d_trace,
                     hipStream_t st);
bool async_idle(const fjsp_env *e);
// fjsp_env.hip, stages 2 and 3 of a create: the kernel family and its builds (the library's only reader of the FJSP_*
// environment variables), then the record layouts; both from the batch's largest sizes alone
int plan_batch(DevBatch &b, LaunchPlan &p, const Shape &sh, int n_inst, int n_envs, int variant, uint64_t rng_seed, int family);   // both
int plan_launch(DevBatch &b, LaunchPlan &p, const Shape &sh, int family);
int plan_layout(DevBatch &b, const Shape &sh);
void generated_release(fjsp_env *e);        // fjsp_generate.hip: frees e->gen (its device memory is in e->dev_allocs)
void arrivals_release(ArrivalService &a);   // joins the LP threads first; on the handle's device
void arrivals_forget(ArrivalService &a);    // empties the memo of solved arrival LPs: the instance indices in its keys name other instances now
// fjsp_env.hip, stage 6 of a create of a multi-order batch: which arrival service, from the n tableaus the batch can meet;
// alloc_arrival_staging: the staging and pools of that service (device memory and pinned mirrors, owned by the handle)
void choose_lp_service(fjsp_env *e, const LpTableau *t, int n);
int alloc_arrival_staging(fjsp_env *e);
// fjsp_generate.hip: a generated multi-order handle's lp_mirror from its records (one gather, synchronises)
int refresh_lp_mirror(fjsp_env *e);

// The LP shape of instance i of the batch: one source for every host reader
inline LpShape lp_shape_of(const fjsp_env *e, int i) {
    if (e->src) {
        const Instance &in = e->src->v[(size_t)e->first + (size_t)i];
        return LpShape{in.R, in.M, in.K, in.Jr.data(), in.p.data()};
    }
    const RecordHead &m = e->lp_mirror[(size_t)i];
    return LpShape{m.h.R, m.h.M, m.h.K, m.Jr.data(), m.p.data()};
}
}  // namespace fjsp
