// Asynchronous prove tickets (capgpu_plonk_prove_batch_async / capgpu_wait): the ticket table and its queue, free of HIP
// so that it also builds for the host alone - tests/cpp/tickets_tsan.cpp runs it under ThreadSanitizer with a stub prover.
//
// A caller with its witnesses in host memory pays a fill and a drain per synchronous call; two callers bound to two
// contexts hide each other's (profiles/phase_trace_r06.md: 0.995 of the resident rate against 0.95-0.97).  A ticket is such
// a bound caller INSIDE the library: the submitter gets a number back at once, a library-owned worker thread proves the
// whole batch on one context, and capgpu_wait collects the result.  Protocol, all under `mu`:
//   * a ticket is QUEUED at submission on the lane of its physical device, RUNNING from the moment a worker of that lane
//     takes it off the front of the lane's queue (tickets of a lane start in submission order), DONE when the run callback
//     has returned, and CONSUMED - gone from the table - once a waiter has taken its result;
//   * a lane has `limit` workers (created with the lane's first ticket), so at most `limit` tickets of a device run at
//     once; later ones queue;
//   * kMaxOutstanding tickets may be in the table (queued, running or done and not yet waited for): the next submission
//     is refused with kBusy instead of blocking;
//   * waiters block on `cv_done`, never spin; of two threads waiting for one ticket one gets the result, the other -
//     like a wait for a ticket that never existed - kUnknown;
//   * drain() (capgpu_shutdown) refuses new tickets, gives every queued ticket `dropped_rc` without running it, lets the
//     running ones finish, joins the workers and discards the results nobody is waiting for; a waiter blocked at that
//     moment still receives its ticket's result.
// The "run" step is a callback, which is what lets the protocol be exercised on the host.  What a ticket borrows from its
// submitter travels in its Job (plonk.hip: AsyncJob - the witnesses, the proof array and, for capgpu_plonk_prove_each_async,
// the outcome array); a ticket that RAN is done with code 0 whatever the outcomes say.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "trace.hpp"

namespace cap {

template <class Job>
struct TicketTable {
  static constexpr size_t kMaxOutstanding = 64;
  static constexpr uint32_t kNoLimit = 0xffffffffu;  // timeout_ms of wait(): no limit
  enum Status { kOk = 0, kBusy = 1, kStopping = 2, kUnknown = 3 };
  enum State { kQueued, kRunning, kDone };

  // proves the job; returns its code and leaves its message in *err.  Called on a worker thread WITHOUT `mu` held.
  using RunFn = std::function<int(Job& job, int lane, std::string* err)>;

  struct Ticket {
    uint64_t id = 0;
    int lane = 0;
    State st = kQueued;
    Job job;
    int rc = 0;
    std::string err;
    uint32_t waiters = 0;  // threads inside wait() for this ticket
  };

  std::mutex mu;
  std::condition_variable cv_work;  // a ticket was queued, or the table is draining
  std::condition_variable cv_done;  // a ticket became done / was consumed, or a running one ended
  std::map<uint64_t, std::unique_ptr<Ticket>> live;  // every ticket not yet consumed
  std::vector<std::deque<Ticket*>> queue;            // [lane]: queued tickets, oldest first
  std::vector<uint32_t> running;                     // [lane]
  std::vector<std::vector<std::thread>> workers;     // [lane]
  uint64_t next_id = 1;
  uint32_t limit = 2;  // tickets of one lane running at once (>= 1); read when a lane's workers are created
  bool stopping = false;
  RunFn run;
  std::function<void(uint64_t id, int lane)> on_start;  // optional; called under `mu` when a ticket starts running (tests)
  // counters since the last reset_stats(): tickets accepted, tickets whose run has ended (dropped ones included), and the
  // most tickets of one lane that were running at the same moment
  uint64_t submitted = 0, completed = 0;
  uint32_t max_running = 0;

  TicketTable() = default;
  TicketTable(const TicketTable&) = delete;
  TicketTable& operator=(const TicketTable&) = delete;
  ~TicketTable() { drain(0, ""); }

  // cv.wait_until on the system clock under ThreadSanitizer (see CoalescerCore::timed_wait: gcc's libtsan does not
  // intercept the steady-clock wait of libstdc++)
  template <class Pred>
  bool timed_wait(std::condition_variable& cv, std::unique_lock<std::mutex>& lk, std::chrono::milliseconds d, Pred pred) {
#if defined(__SANITIZE_THREAD__)
    return cv.wait_until(lk, std::chrono::system_clock::now() + d, pred);
#else
    return cv.wait_for(lk, d, pred);
#endif
  }

  // Queues `job` on `lane` (>= 0).  kOk: *id_out is the ticket (never 0, never reused); kBusy: kMaxOutstanding tickets are
  // in the table; kStopping: the table is being drained.  Never blocks on the device.
  Status submit(Job&& job, int lane, uint64_t* id_out) {
    std::unique_lock<std::mutex> lk(mu);
    if (stopping) return kStopping;
    if (live.size() >= kMaxOutstanding) return kBusy;
    if ((size_t)lane >= queue.size()) {
      queue.resize((size_t)lane + 1);
      running.resize((size_t)lane + 1, 0);
      workers.resize((size_t)lane + 1);
    }
    std::unique_ptr<Ticket> t(new Ticket);
    t->id = next_id++;
    t->lane = lane;
    t->job = std::move(job);
    Ticket* raw = t.get();
    live[raw->id] = std::move(t);
    queue[(size_t)lane].push_back(raw);
    submitted++;
    *id_out = raw->id;
    trace("tk_submit", (int64_t)raw->id, lane);
    if (workers[(size_t)lane].empty()) {
      const uint32_t n = limit ? limit : 1;
      for (uint32_t i = 0; i < n; i++) workers[(size_t)lane].emplace_back([this, lane, i] { work(lane, (int)i); });
    }
    cv_work.notify_all();
    return kOk;
  }

  // Result of ticket `id`.  kUnknown: no such ticket (never issued, or consumed - by another waiter as well).  kOk with
  // *done_out = 0: not done within timeout_ms (0 polls, kNoLimit waits without limit); the ticket stays valid.  kOk with
  // *done_out = 1: *rc_out / *err_out are the run callback's, and the ticket is consumed.
  Status wait(uint64_t id, uint32_t timeout_ms, int* done_out, int* rc_out, std::string* err_out) {
    std::unique_lock<std::mutex> lk(mu);
    *done_out = 0;
    auto it = live.find(id);
    if (it == live.end()) return kUnknown;
    it->second->waiters++;
    // (the ticket may be consumed by another waiter while this one sleeps: looked up again after every wake-up)
    auto settled = [&] {
      auto f = live.find(id);
      return f == live.end() || f->second->st == kDone;
    };
    if (timeout_ms == kNoLimit) cv_done.wait(lk, settled);
    else if (timeout_ms != 0) (void)timed_wait(cv_done, lk, std::chrono::milliseconds(timeout_ms), settled);
    it = live.find(id);
    if (it == live.end()) return kUnknown;
    Ticket& t = *it->second;
    t.waiters--;
    if (t.st != kDone) return kOk;
    *done_out = 1;
    *rc_out = t.rc;
    *err_out = std::move(t.err);
    trace("tk_consumed", (int64_t)id);
    live.erase(it);
    cv_done.notify_all();  // (a second waiter of this ticket, and a submitter's drain, look again)
    return kOk;
  }

  // capgpu_shutdown: see the protocol above.  Afterwards the table accepts tickets again (a later capgpu_init).
  void drain(int dropped_rc, const char* dropped_msg) {
    std::vector<std::thread> join;
    {
      std::unique_lock<std::mutex> lk(mu);
      stopping = true;
      for (auto& q : queue) {
        for (Ticket* t : q) {
          t->st = kDone;
          t->rc = dropped_rc;
          t->err = dropped_msg;
          completed++;
          trace("tk_dropped", (int64_t)t->id);
        }
        q.clear();
      }
      cv_work.notify_all();
      cv_done.notify_all();
      for (auto& lane : workers) {
        for (auto& w : lane) join.push_back(std::move(w));
        lane.clear();
      }
    }
    for (auto& w : join) w.join();  // (a worker finishes the ticket it is running, then sees `stopping`)
    std::unique_lock<std::mutex> lk(mu);
    for (auto it = live.begin(); it != live.end();) {
      if (it->second->waiters == 0) it = live.erase(it);  // (a blocked waiter consumes its own)
      else ++it;
    }
    stopping = false;
  }

  void stats(uint64_t* submitted_out, uint64_t* completed_out, uint32_t* max_running_out) {
    std::lock_guard<std::mutex> lk(mu);
    if (submitted_out) *submitted_out = submitted;
    if (completed_out) *completed_out = completed;
    if (max_running_out) *max_running_out = max_running;
  }
  void reset_stats() {
    std::lock_guard<std::mutex> lk(mu);
    submitted = completed = 0;
    max_running = 0;
  }
  // tickets in the table: queued, running, or done and not yet waited for
  size_t outstanding() {
    std::lock_guard<std::mutex> lk(mu);
    return live.size();
  }

 private:
  void work(int lane, int index) {
    trace("tk_worker", lane, index);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_work.wait(lk, [&] { return stopping || !queue[(size_t)lane].empty(); });
      if (stopping) return;  // (drain has emptied the queues)
      Ticket* t = queue[(size_t)lane].front();
      queue[(size_t)lane].pop_front();
      t->st = kRunning;
      const uint32_t now = ++running[(size_t)lane];
      if (now > max_running) max_running = now;
      trace("tk_start", (int64_t)t->id, lane);
      if (on_start) on_start(t->id, lane);
      lk.unlock();
      std::string err;
      const int rc = run(t->job, lane, &err);  // (a running ticket is never erased: `t` stays valid)
      t->job = Job();  // what the ticket owned is let go before anybody is told, and outside `mu`
      lk.lock();
      t->rc = rc;
      t->err = std::move(err);
      t->st = kDone;
      running[(size_t)lane]--;
      completed++;
      trace("tk_done", (int64_t)t->id, rc);
      cv_done.notify_all();
    }
  }
};

}  // namespace cap
