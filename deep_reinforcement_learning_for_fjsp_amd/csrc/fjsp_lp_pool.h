// Host threads for fluid LPs that a call waits for: the blocking order-arrival service (fjsp_arrivals.hip), the generator's
// host route (fjsp_generate.hip) and fjsp_instances_solve_fluid (fjsp_instance.cpp).  Host only: no HIP in here.
// (The asynchronous service's LpWorkers, one queue of single LPs across the batches in flight, is another thing.)
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/fjsp_amd.h"

namespace fjsp {
// Threads for `requested` (fjsp_env_set_lp_threads, solve_fluid's n_threads): that many, or by default the host's cores up to core_cap
inline int lp_thread_count(int requested, int core_cap = 16) {
    return std::max(1, requested > 0 ? requested : std::min((int)std::thread::hardware_concurrency(), core_cap));
}

// The first failure a run reported: its index and the message its thread left in fjsp_last_error()
struct LpFailure { int index = -1; std::string msg; explicit operator bool() const { return index >= 0; } };      // -1: every LP was solved

// Persistent worker threads: run(n, fn) calls fn(q) for q in [0, n) on the workers and the caller, returning when all
// are done.  fn returns false when its LP failed; with skip_rest the LPs not yet begun are then left out.  The workers are
// started by the first run of more than one LP.  Where the system gives no more threads the pool works with those it
// got, the caller among them.
struct LpPool {
    std::vector<std::thread> workers;
    const int wanted;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::function<bool(uint32_t)> fn;
    std::atomic<uint32_t> next{0};
    uint32_t n = 0, generation = 0;
    int active = 0;
    bool stop = false, started = false, skip = false;
    LpFailure failure;
    std::atomic<bool> failed{false};

    explicit LpPool(int n_workers) : wanted(n_workers) {}
    ~LpPool() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv_work.notify_all();
        for (auto &t : workers) t.join();
    }
    void drain() {
        for (;;) {
            const uint32_t q = next.fetch_add(1);
            if (q >= n || (skip && failed.load())) return;
            if (fn(q)) continue;
            std::lock_guard<std::mutex> g(mu);
            if (!failure) { failure.index = (int)q; failure.msg = fjsp_last_error(); }     // thread-local message of this thread
            failed.store(true);
        }
    }
    void loop() {
        uint32_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_work.wait(lk, [&] { return stop || generation != seen; });
            if (stop) return;
            seen = generation;
            lk.unlock();
            drain();
            lk.lock();
            if (--active == 0) cv_done.notify_one();
        }
    }
    LpFailure run(uint32_t count, std::function<bool(uint32_t)> f, bool skip_rest = false) {
        if (count > 1 && !started) {
            started = true;
            try { for (int t = 0; t < wanted; ++t) workers.emplace_back([this] { loop(); }); } catch (const std::system_error &) {}
        }
        const bool alone = workers.empty() || count == 1;       // nobody to wake
        {
            std::lock_guard<std::mutex> g(mu);
            fn = std::move(f); n = count; next.store(0); failure = LpFailure(); failed.store(false); skip = skip_rest;
            if (!alone) { active = (int)workers.size(); ++generation; }
        }
        if (!alone) cv_work.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu);
        if (!alone) cv_done.wait(lk, [&] { return active == 0; });
        return failure;
    }
};

// The pool a handle keeps (ArrivalService::pool) for `requested` threads, the caller counted: rebuilt if the count changed
inline LpPool &lp_pool_of(LpPool *&slot, int requested) {
    const int n_workers = lp_thread_count(requested) - 1;
    if (slot && slot->wanted != n_workers) { delete slot; slot = nullptr; }
    return *(slot ? slot : slot = new LpPool(n_workers));
}
}  // namespace fjsp
