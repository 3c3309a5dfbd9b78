// hq_task_pool.h — internal: the workers of the threaded event encodes (hq_stream16.cpp) and
// their phase clocks. Nothing of the codec: a pool runs fn(0 .. T-1) and answers with a code. No
// exception leaves it and none ends a pool thread: what fn throws becomes the call's code by
// hq_guard.h's table.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "hq_guard.h"

namespace hqs {

inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// phase clocks of the threaded encodes (hq_encode_stats_read)
struct EncodeClocks {
    std::atomic<uint64_t> calls{0}, tasks{0}, helped{0}, wall_ns{0}, encode_ns{0}, copy_ns{0},
        lag_ns{0}, max_lag_ns{0}, run_ns{0};
    void max_lag(uint64_t v) {
        uint64_t m = max_lag_ns.load(std::memory_order_relaxed);
        while (v > m && !max_lag_ns.compare_exchange_weak(m, v, std::memory_order_relaxed)) {
        }
    }
};
inline EncodeClocks g_clk;

// The threaded encodes' workers: created once and kept (a call spawning its T - 1 threads for
// each of its two phases paid tens of microseconds per thread in a process holding the GPU
// runtime's mappings). A call is one Job: indexes 1..T-1 are queued for the pool, the caller runs
// index 0 and then takes its own job's remaining indexes from the job's counter — never another
// call's tasks, so concurrent callers (one per step worker, execengine.go:675-690) do not wait
// behind each other's work. The Job is shared with every queue entry, so a pool thread that
// finishes the last index signals through memory the caller no longer owns alone (the caller
// returns only once every index has finished; an entry popped after that finds no index left).
class TaskPool {
public:
    ~TaskPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    // gang: the T indexes run at the same time (each may wait for the others: a barrier inside
    // fn); the caller runs index 0 only and every other index gets a pool thread of its own (the
    // pool holds a thread per queued index of every live call, so the gang always assembles).
    // The pool holds at most kMaxThreads threads: a call whose indexes would need more waits
    // until earlier calls have finished (T - 1 <= kMaxThreads: callers clamp T).
    // The code: HQ_OK, or the guard's code of the first exception that fn let out (an index that
    // throws still counts as done, so nobody waits for it; a gang's fn must reach its barrier on
    // its own), or of what kept the call from starting (no thread, no queue entry: nothing of
    // the call run). T <= 1 runs fn(0) on the caller as it is.
    static constexpr uint32_t kMaxThreads = 256;
    int parallel_for(uint32_t T, const std::function<void(uint32_t)> &fn, bool gang = false) {
        if (T <= 1) {
            if (T) fn(0);
            return HQ_OK;
        }
        if (T - 1 > kMaxThreads) return HQ_E_INVAL;
        std::shared_ptr<Job> job;
        bool held = false;                     // demand_ holds this call's T - 1
        int rc = hq::guard("parallel_for", [&] {
            job = std::make_shared<Job>();
            job->fn = &fn;
            job->T = T;
            std::unique_lock<std::mutex> lk(mu_);
            room_.wait(lk, [&] { return demand_ + (T - 1) <= kMaxThreads; });
            demand_ += T - 1;
            held = true;
            try {
                while (th_.size() < demand_) th_.emplace_back([this] { loop(); });
                job->queued = now_ns();
                for (uint32_t t = 1; t < T; ++t) q_.push_back(job);
            } catch (...) {
                // (still under mu_: an entry already queued finds no index, so fn, the
                // caller's, is never reached through it)
                job->next = T;
                throw;
            }
            return HQ_OK;
        });
        cv_.notify_all();
        if (!rc) {
            run(*job, 0);
            for (; !gang;) {
                const uint32_t i = job->next.fetch_add(1);
                if (i >= T) break;
                run(*job, i);
            }
            std::unique_lock<std::mutex> l(job->m);
            job->cv.wait(l, [&] { return job->done == job->T; });
            rc = job->rc;
        }
        if (held) {
            std::lock_guard<std::mutex> lk(mu_);
            demand_ -= T - 1;
            room_.notify_all();
        }
        return rc;
    }

private:
    struct Job {
        const std::function<void(uint32_t)> *fn = nullptr;
        uint32_t T = 0;
        std::atomic<uint32_t> next{1};
        uint64_t queued = 0;
        std::mutex m;
        std::condition_variable cv;
        uint32_t done = 0;
        int rc = HQ_OK;                        // of the first index that threw
    };
    static void run(Job &j, uint32_t i) {
        const uint64_t t0 = now_ns();
        const int rc = hq::guard("parallel_for", [&] {
            (*j.fn)(i);
            return HQ_OK;
        });
        g_clk.run_ns += now_ns() - t0;
        g_clk.tasks++;
        std::lock_guard<std::mutex> l(j.m);
        if (rc && !j.rc) j.rc = rc;
        if (++j.done == j.T) j.cv.notify_all();
    }
    void loop() {
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;          // stop_ and nothing left
                job = std::move(q_.front());
                q_.pop_front();
            }
            const uint32_t i = job->next.fetch_add(1);
            if (i >= job->T) continue;           // the caller took it, or the call never started
            const uint64_t lag = now_ns() - job->queued;
            g_clk.lag_ns += lag;
            g_clk.max_lag(lag);
            g_clk.helped++;
            run(*job, i);
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, room_;
    std::deque<std::shared_ptr<Job>> q_;
    std::vector<std::thread> th_;
    size_t demand_ = 0;
    bool stop_ = false;
};

inline TaskPool &task_pool() {
    static TaskPool p;
    return p;
}

}  // namespace hqs
