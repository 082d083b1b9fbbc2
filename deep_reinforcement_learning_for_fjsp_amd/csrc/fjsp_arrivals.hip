// Order-arrival services of multi-order batches (DESIGN.md "Order arrivals"): the fluid LP of every env a step parked
// at an order arrival is solved -- by the device LP kernel, by the host before the step call returns (blocking), or by
// host threads while the other envs keep stepping (fjsp_env_step_async) -- and arrival_kernel finishes the step.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "fjsp_env_impl.h"
#include "fjsp_lp_pool.h"

namespace fjsp {
// The device service's LP launch over the handle's staging arrays: the parked environments of the pending list (count_dev,
// read on the device) or the first count_host slots, by the kernel choose_lp_service picked
static int launch_service_lps(const DevBatch &b, const ArrivalService &A, const uint32_t *count_dev, int count_host, unsigned long long *solved,
                              hipStream_t st) {
    return A.lp_global ? launch_lp_global(b, count_dev, count_host, b.pending_count + 1, b.lp_in, b.lp_x, A.d_lp_err, solved, A.lp_pool, st)
                       : launch_lp_device(b, count_dev, count_host, b.pending_count + 1, b.lp_in, b.lp_x, A.d_lp_err, solved, A.lp_lds, st);
}

// Order-arrival LPs repeat: environments that play the same instance and reach an arrival in the same situation (the
// same unprocessed / waiting counts per operation type -- always the case when the shop had run empty and the clock
// jumped to the arrival, SO_FJSSP.py:228-231) pose the same LP.  The LP is a pure function of (instance, Q, n_now), so
// its solution is remembered (same bits as a fresh solve).
struct LpCache {
    std::mutex mu;
    std::unordered_map<std::string, std::vector<double>> map;
    int64_t hits = 0, misses = 0;
    static std::string key(int inst, const uint16_t *lpq, size_t KP, int K) {
        std::string k(sizeof(int) + (size_t)K * 4, '\0');
        std::memcpy(&k[0], &inst, sizeof(int));
        std::memcpy(&k[sizeof(int)], lpq, (size_t)K * 2);
        std::memcpy(&k[sizeof(int) + (size_t)K * 2], lpq + KP, (size_t)K * 2);
        return k;
    }
    bool find(const std::string &k, std::vector<double> &x) {
        std::lock_guard<std::mutex> g(mu);
        auto it = map.find(k);
        if (it == map.end()) { ++misses; return false; }
        ++hits; x = it->second;
        return true;
    }
    // bounded by bytes (keys + solutions; 256 MiB): a full memo stops taking entries -- the LPs it misses are solved
    size_t bytes = 0;
    static constexpr size_t kMaxBytes = (size_t)256 << 20;
    void put(const std::string &k, const std::vector<double> &x) {
        std::lock_guard<std::mutex> g(mu);
        const size_t add = k.size() + x.size() * sizeof(double) + 64;
        if (bytes + add > kMaxBytes) return;
        if (map.emplace(k, x).second) bytes += add;
    }
};

// One launch's parked environments on their way through the asynchronous arrival service.
struct AsyncBatch {
    enum State { FREE, HEAD_COPY, TAIL_COPY, SOLVING, SOLVED, UPLOADING };
    uint32_t *d_count = nullptr;      // device staging the parking waves write: [0] = count, [1 + slot] = env id
    uint16_t *d_lp_in = nullptr;      //                                         [slot][2][KP] LP inputs (Q, n_now)
    uint32_t *h_ids = nullptr;        // pinned mirrors
    uint16_t *h_lp_in = nullptr;
    double *h_x = nullptr;            // pinned [slot][KP][MP] solutions
    hipEvent_t ev_head = nullptr, ev_tail = nullptr, ev_up = nullptr;
    State state = FREE;
    uint32_t n = 0, cap = 0;          // parked envs of this batch; capacity of the pinned mirrors (grown on demand)
    std::atomic<int> solved{0};       // 1 = every LP solved, -1 = a solve failed
    std::atomic<int> left{0}, bad{0};
    std::mutex err_mu;
    std::string err;
};

// Worker threads of the asynchronous service: ONE queue of single LPs across all batches in flight, so that the
// threads stay busy whatever the batch sizes are; a batch is solved when its last LP is.
struct LpWorkers {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<AsyncBatch *, uint32_t>> tasks;
    std::function<bool(AsyncBatch *, uint32_t)> solve;      // false: the LP failed (message left in the batch)
    bool stop = false;
    LpWorkers(int n, std::function<bool(AsyncBatch *, uint32_t)> f) : solve(std::move(f)) {
        for (int t = 0; t < n; ++t) th.emplace_back([this] { loop(); });
    }
    ~LpWorkers() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    void submit(AsyncBatch *a) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (uint32_t q = 0; q < a->n; ++q) tasks.emplace_back(a, q);
        }
        cv.notify_all();
    }
    void loop() {
        for (;;) {
            std::pair<AsyncBatch *, uint32_t> t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !tasks.empty(); });
                if (tasks.empty()) return;              // (stop: drain first)
                t = tasks.front();
                tasks.pop_front();
            }
            if (!solve(t.first, t.second)) t.first->bad.store(1);
            if (t.first->left.fetch_sub(1) == 1) t.first->solved.store(t.first->bad.load() ? -1 : 1);
        }
    }
};

constexpr int kAsyncRing = 32;         // batches in flight: a parked env waits for its LP (0.05 .. 0.8 ms) while calls come every ~0.03 ms
                                       // (LaunchPlan::async_ring, FJSP_ASYNC_RING: fewer, down to 1)
constexpr uint32_t kAsyncHead = 64;    // parked envs whose ids + LP inputs travel with the count (more: a second copy)

// The asynchronous service of one handle: its batches, the worker threads and the copy stream.
struct AsyncRing {
    AsyncBatch batch[kAsyncRing];
    int len = kAsyncRing;               // batches in use: [0, len) (LaunchPlan::async_ring)
    int next = 0;                       // where the search for a free batch starts (the oldest batch in flight)
    // fjsp_env_async_stats: batches handed to the workers, those of them with a tail copy, calls that found no free
    // batch and waited, the largest batch
    int64_t stat_batches = 0, stat_tails = 0, stat_waits = 0, stat_max_n = 0;
    std::unique_ptr<LpWorkers> workers;
    hipStream_t copy_stream = nullptr;  // the parked envs' ids / LP inputs leave on their own stream: the next step launch does not wait for them
    hipEvent_t ev_step = nullptr;
    uint32_t *d_resume_ids = nullptr;   // [N] device list handed to arrival_kernel
    double *d_resume_x = nullptr;       // [N][KP][MP]
    ~AsyncRing() {
        workers.reset();                // (joins: LPs still queued are solved first, into the pinned mirrors freed below)
        for (AsyncBatch &a : batch) {                  // (freeing nullptr does nothing)
            for (void *p : {(void *)a.d_count, (void *)a.d_lp_in}) (void)hipFree(p);
            for (void *p : {(void *)a.h_ids, (void *)a.h_lp_in, (void *)a.h_x}) (void)hipHostFree(p);
            for (hipEvent_t ev : {a.ev_head, a.ev_tail, a.ev_up}) if (ev) (void)hipEventDestroy(ev);
        }
        for (void *p : {(void *)d_resume_ids, (void *)d_resume_x}) (void)hipFree(p);
        if (ev_step) (void)hipEventDestroy(ev_step);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

namespace {
// The host LP of the parked env `env` with inputs lpq ([2][KP]: Q, n_now): from the cache or solved, then written to its
// padded [KP][MP] slot.  Either service calls it from several threads.  false: the LP failed (fjsp_last_error() of the
// calling thread says why).
bool solve_parked_lp(fjsp_env *e, int env, const uint16_t *lpq, double *x_slot) {
    const DevBatch &b = e->b;
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP;
    const LpShape in = lp_shape_of(e, env % b.n_inst);
    std::vector<int> Q(in.K), now(in.K);
    for (int k = 0; k < in.K; ++k) { Q[k] = lpq[(size_t)k]; now[k] = lpq[KP + (size_t)k]; }
    std::vector<double> xk((size_t)in.K * in.M, 0.0);
    double obj = 0.0;
    const std::string ck = LpCache::key(env % b.n_inst, lpq, KP, in.K);
    if (!e->arr.cache->find(ck, xk)) {
        if (solve_fluid_lp(in.R, in.M, in.Jr, in.p, Q.data(), now.data(), xk.data(), &obj) != 0) return false;
        e->arr.cache->put(ck, xk);
    }
    std::fill(x_slot, x_slot + KP * MP, 0.0);
    for (int k = 0; k < in.K; ++k)
        for (int m = 0; m < in.M; ++m) x_slot[(size_t)k * MP + m] = xk[(size_t)k * in.M + m];
    return true;
}

int service_arrivals_impl(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, int16_t *d_trace,
                          hipStream_t st) {
    const DevBatch &b = e->b;
    ArrivalService &A = e->arr;
    if (A.lp_device) {
        // the whole service on the stream: LP kernel (one workgroup per parked env, count read on the device), arrival_kernel,
        // pending list emptied -- no host round trip, fjsp_env_step stays asynchronous
        if (launch_service_lps(b, A, b.pending_count, 0, A.d_lp_solved, st) != 0) {
            set_error("lp_device_kernel launch failed"); return FJSP_E_HIP;
        }
        if (launch_arrival(b, d_mo, 0, b.pending_count + 1, b.lp_x, d_state, d_reward, d_done, d_trace, st, nullptr, false, b.pending_count) != 0) {
            set_error("arrival_kernel launch failed"); return FJSP_E_HIP;
        }
        HIP_TRY(hipMemsetAsync(b.pending_count, 0, 4, st));
        return FJSP_OK;
    }
    // (the sync below also orders this call after the previous call's solution upload, so the pinned staging
    // buffers are free again)
    HIP_TRY(hipMemcpyAsync(A.h_pending, b.pending_count, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t n = A.h_pending[0];
    if (n == 0) return FJSP_OK;
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP;
    // env ids and LP inputs of every parked env: two copies, whatever n is (step_kernel packed them by slot)
    HIP_TRY(hipMemcpyAsync(A.h_pending + 1, b.pending_count + 1, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(A.h_lp_in, b.lp_in, (size_t)n * 2 * KP * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!A.cache) A.cache = new LpCache();
    // one LP per parked env, independent: spread over the host cores
    const LpFailure bad = lp_pool_of(A.pool, A.lp_threads).run(n, [&](uint32_t q) {
        return solve_parked_lp(e, (int)A.h_pending[1 + q], A.h_lp_in + (size_t)q * 2 * KP, A.h_lp_x + (size_t)q * KP * MP);
    }, true);
    if (bad) { set_error(bad.msg); return FJSP_E_LP; }
    HIP_TRY(hipMemcpyAsync(b.lp_x, A.h_lp_x, (size_t)n * KP * MP * 8, hipMemcpyHostToDevice, st));
    if (launch_arrival(b, d_mo, (int)n, b.pending_count + 1, b.lp_x, d_state, d_reward, d_done, d_trace, st) != 0) { set_error("arrival_kernel launch failed"); return FJSP_E_HIP; }
    HIP_TRY(hipMemsetAsync(b.pending_count, 0, 4, st));
    A.lp_solves += n;
    return FJSP_OK;
}

// ------------------------------------------------------------------ asynchronous arrival service

// pinned mirrors of a batch for `need` parked envs (grow-only: a typical launch parks a few dozen envs, a launch right
// after a synchronised reset can park all of them)
int async_reserve(fjsp_env *e, AsyncBatch &a, uint32_t need) {
    if (need <= a.cap) return FJSP_OK;
    const DevBatch &b = e->b;
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP;
    uint32_t cap = std::max<uint32_t>(kAsyncHead, a.cap);
    while (cap < need) cap *= 2;
    cap = std::min<uint32_t>(cap, (uint32_t)b.N);
    uint32_t *ids = nullptr; uint16_t *in = nullptr; double *x = nullptr;
    if (!hip_ok(hipHostMalloc(reinterpret_cast<void **>(&ids), ((size_t)cap + 1) * 4, hipHostMallocDefault), "hipHostMalloc") ||
        !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&in), (size_t)cap * 2 * KP * 2, hipHostMallocDefault), "hipHostMalloc") ||
        !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&x), (size_t)cap * KP * MP * 8, hipHostMallocDefault), "hipHostMalloc")) {
        for (void *p : {(void *)ids, (void *)in, (void *)x}) (void)hipHostFree(p);
        return FJSP_E_HIP;
    }
    if (a.h_ids) {           // keep what the head copy already delivered
        std::memcpy(ids, a.h_ids, ((size_t)std::min(a.cap, cap) + 1) * 4);
        std::memcpy(in, a.h_lp_in, (size_t)std::min(a.cap, cap) * 2 * KP * 2);
        (void)hipHostFree(a.h_ids); (void)hipHostFree(a.h_lp_in); (void)hipHostFree(a.h_x);
    }
    a.h_ids = ids; a.h_lp_in = in; a.h_x = x; a.cap = cap;
    return FJSP_OK;
}

// Builds the asynchronous service of the handle at its first call, completely or not at all (e->arr.ring stays nullptr).
int async_setup(fjsp_env *e) {
    if (e->arr.ring) return FJSP_OK;
    // a generated handle whose blocking service runs on the device has not gathered its records' heads yet
    if (e->gen && e->lp_mirror.empty())
        if (const int rc = refresh_lp_mirror(e)) return rc;
    const DevBatch &b = e->b;
    const size_t N = (size_t)b.N, KP = (size_t)b.KP, MP = (size_t)b.MP;
    std::unique_ptr<AsyncRing> r(new AsyncRing());
    r->len = e->plan.async_ring;
    for (int i = 0; i < r->len; ++i) {
        AsyncBatch &a = r->batch[i];
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a.d_count), (N + 1) * 4));
        HIP_TRY(hipMemset(a.d_count, 0, (N + 1) * 4));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a.d_lp_in), N * 2 * KP * 2));
        if (const int rc = async_reserve(e, a, kAsyncHead)) return rc;
        HIP_TRY(hipEventCreateWithFlags(&a.ev_head, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&a.ev_tail, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&a.ev_up, hipEventDisableTiming));
    }
    HIP_TRY(hipStreamCreateWithFlags(&r->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&r->ev_step, hipEventDisableTiming));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r->d_resume_ids), N * 4));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r->d_resume_x), N * KP * MP * 8));
    if (!e->arr.cache) e->arr.cache = new LpCache();
    // the threads the box gives (16 per GPU); more only oversubscribes a latency-critical wait
    int n_threads = e->arr.lp_threads > 0 ? std::min(e->arr.lp_threads, (int)std::thread::hardware_concurrency())
                                          : std::min((int)std::thread::hardware_concurrency(), 16);
    if (n_threads <= 0) n_threads = 1;
    r->workers.reset(new LpWorkers(n_threads, [e](AsyncBatch *a, uint32_t q) {
        const size_t KP = (size_t)e->b.KP, MP = (size_t)e->b.MP;
        if (solve_parked_lp(e, (int)a->h_ids[1 + q], a->h_lp_in + (size_t)q * 2 * KP, a->h_x + (size_t)q * KP * MP)) return true;
        std::lock_guard<std::mutex> g(a->err_mu);
        a->err = fjsp_last_error();              // (thread-local message of this worker)
        return false;
    }));
    e->arr.ring = r.release();
    return FJSP_OK;
}

// hand a batch's LPs to the worker threads
void async_submit(AsyncRing &r, AsyncBatch *a) {
    ++r.stat_batches;
    r.stat_max_n = std::max<int64_t>(r.stat_max_n, a->n);
    a->solved.store(0); a->bad.store(0); a->left.store((int)a->n);
    a->state = AsyncBatch::SOLVING;
    r.workers->submit(a);
}

// hipSuccess once the event has completed; block: wait for it, else hipErrorNotReady until then
hipError_t poll(hipEvent_t ev, bool block) { return block ? hipEventSynchronize(ev) : hipEventQuery(ev); }

// Advance every batch as far as it can go without waiting (block: with waiting, until the ring is empty).  Batches
// whose LPs are solved are uploaded and finished by arrival_kernel, which writes their outputs and ready = 1.
int async_progress(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, uint8_t *d_ready, hipStream_t st,
                   bool block, bool mark_resumed) {
    const DevBatch &b = e->b;
    AsyncRing &r = *e->arr.ring;
    const size_t KP = (size_t)b.KP, MP = (size_t)b.MP;
    for (;;) {
        bool busy = false;
        for (int off = 0; off < r.len; ++off) {
            AsyncBatch &a = r.batch[(r.next + off) % r.len];       // oldest first
            if (a.state == AsyncBatch::HEAD_COPY) {
                const hipError_t q = poll(a.ev_head, block);
                if (q == hipErrorNotReady) { busy = true; continue; }
                HIP_TRY(q);
                a.n = a.h_ids[0];
                if (a.n > (uint32_t)b.N) a.n = (uint32_t)b.N;
                e->arr.parked += a.n;
                if (a.n == 0) { a.state = AsyncBatch::FREE; continue; }
                if (a.n <= kAsyncHead) { async_submit(r, &a); busy = true; continue; }
                if (const int rc = async_reserve(e, a, a.n)) return rc;
                HIP_TRY(hipMemcpyAsync(a.h_ids + 1 + kAsyncHead, a.d_count + 1 + kAsyncHead, (size_t)(a.n - kAsyncHead) * 4, hipMemcpyDeviceToHost, r.copy_stream));
                HIP_TRY(hipMemcpyAsync(a.h_lp_in + (size_t)kAsyncHead * 2 * KP, a.d_lp_in + (size_t)kAsyncHead * 2 * KP,
                                       (size_t)(a.n - kAsyncHead) * 2 * KP * 2, hipMemcpyDeviceToHost, r.copy_stream));
                HIP_TRY(hipEventRecord(a.ev_tail, r.copy_stream));
                a.state = AsyncBatch::TAIL_COPY;
                ++r.stat_tails;
                busy = true;
            } else if (a.state == AsyncBatch::TAIL_COPY) {
                const hipError_t q = poll(a.ev_tail, block);
                if (q == hipErrorNotReady) { busy = true; continue; }
                HIP_TRY(q);
                async_submit(r, &a);
                busy = true;
            } else if (a.state == AsyncBatch::SOLVING || a.state == AsyncBatch::SOLVED) {
                int sv = a.solved.load();
                if (sv == 0 && block) {
                    while ((sv = a.solved.load()) == 0) std::this_thread::sleep_for(std::chrono::microseconds(20));
                }
                if (sv == 0) { busy = true; continue; }
                if (sv < 0) { set_error("order-arrival LP failed: " + a.err); return FJSP_E_LP; }
                HIP_TRY(hipMemcpyAsync(r.d_resume_ids, a.h_ids + 1, (size_t)a.n * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(r.d_resume_x, a.h_x, (size_t)a.n * KP * MP * 8, hipMemcpyHostToDevice, st));
                if (launch_arrival(b, d_mo, (int)a.n, r.d_resume_ids, r.d_resume_x, d_state, d_reward, d_done, nullptr, st, d_ready,
                                   mark_resumed) != 0) { set_error("arrival_kernel launch failed"); return FJSP_E_HIP; }
                HIP_TRY(hipEventRecord(a.ev_up, st));
                e->arr.lp_solves += a.n;
                e->arr.parked -= a.n;
                a.state = AsyncBatch::UPLOADING;
                busy = true;
            } else if (a.state == AsyncBatch::UPLOADING) {
                const hipError_t q = poll(a.ev_up, block);
                if (q == hipErrorNotReady) { busy = true; continue; }
                HIP_TRY(q);
                a.state = AsyncBatch::FREE;
            }
        }
        if (!block || !busy) return FJSP_OK;
    }
}

// One step launch of the asynchronous service: whatever parks in it goes to `slot`, whose head (count, first ids and
// LP inputs) starts its way to the host behind the launch.
int async_launch(fjsp_env *e, AsyncBatch *slot, const uint8_t *d_actions, const double *d_mo, int32_t autoreset, double *d_state,
                 double *d_reward, uint8_t *d_done, uint8_t *d_ready, hipStream_t st) {
    AsyncRing &r = *e->arr.ring;
    HIP_TRY(hipMemsetAsync(slot->d_count, 0, 4, st));
    DevBatch b2 = e->b;
    b2.pending_count = slot->d_count;
    b2.lp_in = slot->d_lp_in;
    // (a step that parks has dispatched already: its record is written in this launch, arrival_kernel adds none)
    if (launch_step(b2, e->plan, d_actions, d_mo, autoreset ? 1 : 0, d_state, d_reward, d_done, nullptr, st, d_ready, e->sched) != 0) {
        set_error("step_kernel launch failed"); return FJSP_E_HIP;
    }
    const size_t KP = (size_t)e->b.KP;
    const uint32_t head = std::min<uint32_t>(kAsyncHead, (uint32_t)e->b.N);
    HIP_TRY(hipEventRecord(r.ev_step, st));
    HIP_TRY(hipStreamWaitEvent(r.copy_stream, r.ev_step, 0));
    HIP_TRY(hipMemcpyAsync(slot->h_ids, slot->d_count, (size_t)(1 + head) * 4, hipMemcpyDeviceToHost, r.copy_stream));
    HIP_TRY(hipMemcpyAsync(slot->h_lp_in, slot->d_lp_in, (size_t)head * 2 * KP * 2, hipMemcpyDeviceToHost, r.copy_stream));
    HIP_TRY(hipEventRecord(slot->ev_head, r.copy_stream));
    return FJSP_OK;
}
}  // namespace

// A failure inside the service (LP iteration limit, HIP error) leaves envs parked with no way to finish their
// step: the pending list is emptied, so a later launch cannot run its slots past the staging arrays, and the
// handle is marked failed: every later step / rollout returns FJSP_E_STATE until the batch is destroyed.
int service_arrivals(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, int16_t *d_trace,
                     hipStream_t st) {
    const int rc = service_arrivals_impl(e, d_mo, d_state, d_reward, d_done, d_trace, st);
    if (rc != FJSP_OK) {
        const std::string why = fjsp_last_error();
        (void)hipMemsetAsync(e->b.pending_count, 0, 4, st);
        e->failed = true;
        set_error("order-arrival service failed (" + why + "); the batch is unusable: destroy it");
    }
    return rc;
}

bool async_idle(const fjsp_env *e) {
    if (!e->arr.ring) return true;
    for (const AsyncBatch &a : e->arr.ring->batch) if (a.state != AsyncBatch::FREE) return false;
    return true;
}

void arrivals_release(ArrivalService &a) { delete a.ring; delete a.pool; delete a.cache; }

void arrivals_forget(ArrivalService &a) {
    if (!a.cache) return;
    std::lock_guard<std::mutex> g(a.cache->mu);      // (the asynchronous workers are idle: the caller checked async_idle)
    a.cache->map.clear();
    a.cache->bytes = 0;
}
}  // namespace fjsp

using namespace fjsp;

// counter i of the device LP service (0: LPs solved, 1: their pivots); synchronises.  -1: the read failed
static int64_t lp_device_counter(const fjsp_env *e, int i) {
    DeviceGuard guard(e->device);
    unsigned long long dev = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&dev, e->arr.d_lp_solved + i, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)dev;
}

extern "C" {
int fjsp_env_step_async(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset, double *d_state, double *d_reward,
                        uint8_t *d_done, uint8_t *d_ready, void *stream) {
    if (!e || !d_actions || !d_ready) { set_error("fjsp_env_step_async: null argument"); return FJSP_E_ARG; }
    if (const int rc = usable(e, "fjsp_env_step_async", kIntact, d_actions)) return rc;
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    if (!e->b.mord) {                               // nothing ever parks: the plain step, every env ready
        if (launch_step(e->b, e->plan, d_actions, d_mo, autoreset ? 1 : 0, d_state, d_reward, d_done, nullptr, st, nullptr, e->sched) != 0) { set_error("step_kernel launch failed"); return FJSP_E_HIP; }
        HIP_TRY(hipMemsetAsync(d_ready, 1, (size_t)e->b.N, st));
        return FJSP_OK;
    }
    if (const int rc = async_setup(e)) return rc;
    AsyncRing &r = *e->arr.ring;
    int rc = async_progress(e, d_mo, d_state, d_reward, d_done, d_ready, st, false, true);
    if (rc != FJSP_OK) { e->failed = true; return rc; }
    // a free batch for whatever parks in this launch (none free: wait for the oldest ones)
    AsyncBatch *slot = nullptr;
    for (int attempt = 0; attempt < 2 && !slot; ++attempt) {
        for (int off = 0; off < r.len; ++off) {
            AsyncBatch &a = r.batch[(r.next + off) % r.len];
            if (a.state == AsyncBatch::FREE) { slot = &a; r.next = (int)((&a - r.batch) + 1) % r.len; break; }
        }
        if (!slot) {
            ++r.stat_waits;
            rc = async_progress(e, d_mo, d_state, d_reward, d_done, d_ready, st, true, true);
            if (rc != FJSP_OK) { e->failed = true; return rc; }
        }
    }
    if (!slot) { set_error("fjsp_env_step_async: no free batch"); e->failed = true; return FJSP_E_STATE; }
    // From here on environments resumed by async_progress carry their solutions and the launch parks new ones into
    // `slot`: an error on the way leaves them without a path back, so every failing exit marks the batch unusable
    // (as service_arrivals does for the blocking service).
    rc = async_launch(e, slot, d_actions, d_mo, autoreset, d_state, d_reward, d_done, d_ready, st);
    if (rc != FJSP_OK) { e->failed = true; return rc; }
    slot->state = AsyncBatch::HEAD_COPY;
    return FJSP_OK;
}

int fjsp_env_arrivals_flush(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done, uint8_t *d_ready, void *stream) {
    if (!e) { set_error("fjsp_env_arrivals_flush: null env"); return FJSP_E_ARG; }
    if (async_idle(e)) return FJSP_OK;
    DeviceGuard guard(e->device);
    const int rc = async_progress(e, d_mo, d_state, d_reward, d_done, d_ready, (hipStream_t)stream, true, false);
    if (rc != FJSP_OK) e->failed = true;
    return rc;
}

int64_t fjsp_env_parked(const fjsp_env *e) { return e ? e->arr.parked : 0; }
int fjsp_env_async_stats(const fjsp_env *e, int64_t out[4]) {
    if (!e || !out) { set_error("fjsp_env_async_stats: null argument"); return FJSP_E_ARG; }
    const AsyncRing *r = e->arr.ring;
    out[0] = r ? r->stat_batches : 0; out[1] = r ? r->stat_tails : 0;
    out[2] = r ? r->stat_waits : 0;   out[3] = r ? r->stat_max_n : 0;
    return FJSP_OK;
}
int64_t fjsp_env_lp_cache_hits(fjsp_env *e) {
    if (!e || !e->arr.cache) return 0;
    std::lock_guard<std::mutex> g(e->arr.cache->mu);
    return e->arr.cache->hits;
}
int64_t fjsp_env_lp_solves(const fjsp_env *e) {
    if (!e) return 0;
    return e->arr.lp_solves + (e->arr.lp_device ? std::max<int64_t>(lp_device_counter(e, 0), 0) : 0);
}
int64_t fjsp_env_lp_device_pivots(const fjsp_env *e) { return (e && e->arr.lp_device) ? lp_device_counter(e, 1) : 0; }

int fjsp_env_lp_device_solve(fjsp_env *e, int32_t env, const int32_t *Q, const int32_t *n_now, double *x) {
    if (!e || !Q || !n_now || !x || env < 0 || env >= e->b.N) { set_error("fjsp_env_lp_device_solve: bad arguments"); return FJSP_E_ARG; }
    const ArrivalService &A = e->arr;
    if (!A.lp_device) { set_error("fjsp_env_lp_device_solve: this batch keeps the host LP service"); return FJSP_E_UNSUPPORTED; }
    DeviceGuard guard(e->device);
    const DevBatch &b = e->b;
    // (the sizes alone: every handle keeps them per instance, a generated one with no host mirror of its records too)
    const int K = e->inst_K[(size_t)(env % b.n_inst)], M = e->inst_M[(size_t)(env % b.n_inst)];
    std::vector<uint16_t> lpq((size_t)2 * b.KP, 0);
    for (int k = 0; k < K; ++k) {          // the staging arrays hold 16-bit counts (a batch has at most 65535 jobs)
        if (Q[k] < 0 || Q[k] > 65535 || n_now[k] < 0 || n_now[k] > 65535) {
            set_error("fjsp_env_lp_device_solve: Q[k] and n_now[k] must lie in 0 ... 65535"); return FJSP_E_ARG;
        }
        lpq[(size_t)k] = (uint16_t)Q[k]; lpq[(size_t)b.KP + k] = (uint16_t)n_now[k];
    }
    const uint32_t id = (uint32_t)env;
    // (slot 0 of the staging arrays; the batch must be idle: no parked environments)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(b.lp_in, lpq.data(), lpq.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b.pending_count + 1, &id, 4, hipMemcpyHostToDevice));
    if (launch_service_lps(b, A, nullptr, 1, nullptr, nullptr) != 0) {
        set_error("lp_device_kernel launch failed"); return FJSP_E_HIP;
    }
    HIP_TRY(hipDeviceSynchronize());
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, A.d_lp_err, 4, hipMemcpyDeviceToHost));
    if (err) { const uint32_t z = 0; (void)hipMemcpy(A.d_lp_err, &z, 4, hipMemcpyHostToDevice); set_error("fluid LP failed on the device (code " + std::to_string(err) + ")"); return FJSP_E_LP; }
    std::vector<double> xs((size_t)b.KP * b.MP);
    HIP_TRY(hipMemcpy(xs.data(), b.lp_x, xs.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
        for (int m = 0; m < M; ++m) x[(size_t)k * M + m] = xs[(size_t)k * b.MP + m];
    return FJSP_OK;
}

int fjsp_env_set_lp_threads(fjsp_env *e, int32_t n_threads) {
    if (!e || n_threads < 0) { set_error("fjsp_env_set_lp_threads: bad arguments"); return FJSP_E_ARG; }
    e->arr.lp_threads = n_threads;
    return FJSP_OK;
}
}  // extern "C"
