// Host-only test of the ticket protocol (cap_amd/csrc/tickets.hpp) - the table, queue and waiters behind
// capgpu_plonk_prove_batch_async / capgpu_wait - with a stub prover that sleeps 1-3 ms.  Built with -fsanitize=thread by
// tests/test_tickets_host.py.  Checks: every ticket's result reaches exactly one waiter (two waiters race for each), a
// lane's tickets start in submission order, a lane never runs more tickets than its limit (limits 1 and 2), the 65th
// outstanding ticket is refused, a poll of a queued ticket reports not-done, a second wait finds nothing, and a drain with
// queued tickets releases every blocked waiter; ThreadSanitizer checks the rest.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "../../cap_amd/csrc/tickets.hpp"

struct Job {
  uint64_t input = 0;
  uint64_t* out = nullptr;  // borrowed from the submitter, as a ticket borrows proofs_out
};
using Table = cap::TicketTable<Job>;

static std::atomic<int> failures{0};
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      failures++;                                                  \
      fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #x); \
    }                                                              \
  } while (0)

constexpr int kDropped = -6;

// 4 submitters x 50 tickets over `lanes` lanes, 4 waiter threads that are not submitters; every ticket is waited for twice
static void scenario_stream(uint32_t limit, int lanes) {
  constexpr int kSubmitters = 4, kPer = 50, kWaiters = 4, kTotal = kSubmitters * kPer;
  Table tb;
  tb.limit = limit;
  std::vector<std::atomic<int>> running(lanes);
  for (auto& r : running) r = 0;
  std::atomic<int> over_limit{0};
  tb.run = [&](Job& j, int lane, std::string* err) -> int {
    if (running[(size_t)lane].fetch_add(1) + 1 > (int)limit) over_limit++;
    std::this_thread::sleep_for(std::chrono::milliseconds(1 + j.input % 3));  // "the device is busy"
    *j.out = j.input * 7 + 1;
    running[(size_t)lane].fetch_sub(1);
    if (j.input % 5 == 0) {
      *err = "job " + std::to_string(j.input) + " failed";
      return -7;
    }
    return 0;
  };
  std::vector<std::vector<uint64_t>> started(lanes);  // per lane, in start order (on_start runs under the table's lock)
  tb.on_start = [&](uint64_t id, int lane) { started[(size_t)lane].push_back(id); };

  std::vector<uint64_t> outs(kTotal, 0), id_of(kTotal, 0);
  std::vector<int> lane_of(kTotal, 0);
  std::vector<std::atomic<int>> got(kTotal), unknown(kTotal);
  for (int i = 0; i < kTotal; i++) got[i] = 0, unknown[i] = 0;
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<int> todo;  // job indices handed from submitters to waiters (each twice)
  int closed = 0;
  std::atomic<int> busy_seen{0};

  std::vector<std::thread> th;
  for (int s = 0; s < kSubmitters; s++)
    th.emplace_back([&, s] {
      for (int k = 0; k < kPer; k++) {
        const int idx = s * kPer + k;
        Job j;
        j.input = (uint64_t)idx;
        j.out = &outs[idx];
        lane_of[idx] = idx % lanes;
        uint64_t id = 0;
        for (;;) {
          Job copy = j;
          const Table::Status st = tb.submit(std::move(copy), lane_of[idx], &id);
          if (st == Table::kOk) break;
          CHECK(st == Table::kBusy);
          busy_seen++;
          std::this_thread::sleep_for(std::chrono::milliseconds(1));  // (the caller's move: wait for one, or back off)
        }
        CHECK(id != 0);
        id_of[idx] = id;
        std::lock_guard<std::mutex> g(qmu);
        todo.push_back(idx);
        todo.push_back(idx);
        qcv.notify_all();
      }
      std::lock_guard<std::mutex> g(qmu);
      closed++;
      qcv.notify_all();
    });
  for (int w = 0; w < kWaiters; w++)
    th.emplace_back([&] {
      for (;;) {
        int idx;
        {
          std::unique_lock<std::mutex> lk(qmu);
          qcv.wait(lk, [&] { return !todo.empty() || closed == kSubmitters; });
          if (todo.empty()) return;
          idx = todo.front();
          todo.pop_front();
        }
        int done = 0, rc = 1;
        std::string err;
        // a bounded wait first (not done -> the ticket must still be there), then without limit
        Table::Status st = tb.wait(id_of[idx], 1, &done, &rc, &err);
        if (st == Table::kOk && !done) st = tb.wait(id_of[idx], Table::kNoLimit, &done, &rc, &err);
        if (st == Table::kUnknown) {
          unknown[idx]++;
          continue;
        }
        CHECK(st == Table::kOk && done == 1);
        CHECK(outs[idx] == (uint64_t)idx * 7 + 1);  // the borrowed output was written before the ticket was reported done
        if (idx % 5 == 0) CHECK(rc == -7 && err == "job " + std::to_string(idx) + " failed");
        else CHECK(rc == 0 && err.empty());
        got[idx]++;
      }
    });
  for (auto& x : th) x.join();

  for (int i = 0; i < kTotal; i++) CHECK(got[i].load() == 1 && unknown[i].load() == 1);
  CHECK(over_limit.load() == 0);
  uint64_t sub = 0, comp = 0;
  uint32_t maxr = 0;
  tb.stats(&sub, &comp, &maxr);
  CHECK(sub == (uint64_t)kTotal && comp == (uint64_t)kTotal);
  CHECK(maxr >= 1 && maxr <= limit);
  CHECK(tb.outstanding() == 0);
  size_t n_started = 0;
  for (int l = 0; l < lanes; l++) {
    n_started += started[(size_t)l].size();
    for (size_t i = 1; i < started[(size_t)l].size(); i++) CHECK(started[(size_t)l][i - 1] < started[(size_t)l][i]);  // FIFO
  }
  CHECK(n_started == (size_t)kTotal);
  for (int i = 0; i < kTotal; i++) {  // ... and every ticket ran on the lane it was submitted to
    const auto& v = started[(size_t)lane_of[i]];
    CHECK(std::find(v.begin(), v.end(), id_of[i]) != v.end());
  }
  printf("stream: limit %u, %d lane(s): %d tickets, most running at once %u, busy refusals %d\n", limit, lanes, kTotal, maxr,
         busy_seen.load());
}

// a stub prover that holds every ticket until the test opens the gate
struct Gate {
  std::mutex mu;
  std::condition_variable cv;
  bool open = false;
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return open; });
  }
  void release() {
    std::lock_guard<std::mutex> lk(mu);
    open = true;
    cv.notify_all();
  }
};

template <class Pred>
static void until(Table& tb, Pred p) {  // (test code: the library itself never polls)
  for (;;) {
    {
      std::lock_guard<std::mutex> lk(tb.mu);
      if (p()) return;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

static void scenario_busy_poll_double_wait() {
  Table tb;
  tb.limit = 1;
  Gate gate;
  tb.run = [&](Job& j, int, std::string*) -> int {
    gate.wait();
    *j.out = j.input;
    return 0;
  };
  std::vector<uint64_t> outs(Table::kMaxOutstanding + 1, ~0ull), ids(Table::kMaxOutstanding + 1, 0);
  for (size_t i = 0; i < Table::kMaxOutstanding; i++) {
    Job j{(uint64_t)i, &outs[i]};
    CHECK(tb.submit(std::move(j), 0, &ids[i]) == Table::kOk);
  }
  {
    Job j{99, &outs[Table::kMaxOutstanding]};
    uint64_t id = 0;
    CHECK(tb.submit(std::move(j), 0, &id) == Table::kBusy);  // 64 outstanding: refused, not blocked
  }
  until(tb, [&] { return tb.running[0] == 1; });
  int done = 1, rc = 1;
  std::string err;
  CHECK(tb.wait(ids[63], 0, &done, &rc, &err) == Table::kOk && done == 0);  // queued: a poll reports not-done ...
  CHECK(tb.wait(ids[0], 0, &done, &rc, &err) == Table::kOk && done == 0);   // ... and so does one of the running ticket
  CHECK(tb.wait(ids[63], 2, &done, &rc, &err) == Table::kOk && done == 0);  // a bounded wait comes back, the ticket stays
  CHECK(tb.wait(12345678, 0, &done, &rc, &err) == Table::kUnknown);         // never issued
  gate.release();
  // waited for in the reverse of the submission order
  for (size_t i = Table::kMaxOutstanding; i-- > 0;) {
    CHECK(tb.wait(ids[i], Table::kNoLimit, &done, &rc, &err) == Table::kOk && done == 1 && rc == 0);
    CHECK(outs[i] == (uint64_t)i);
    CHECK(tb.wait(ids[i], 0, &done, &rc, &err) == Table::kUnknown && done == 0);  // consumed: a second wait finds nothing
  }
  {
    Job j{99, &outs[Table::kMaxOutstanding]};  // room again
    uint64_t id = 0;
    CHECK(tb.submit(std::move(j), 0, &id) == Table::kOk);
    CHECK(tb.wait(id, Table::kNoLimit, &done, &rc, &err) == Table::kOk && done == 1 && outs[Table::kMaxOutstanding] == 99);
  }
  printf("busy / poll / double wait: ok\n");
}

static void scenario_drain() {
  constexpr int kTickets = 8;
  Table tb;
  tb.limit = 1;
  Gate gate;
  tb.run = [&](Job& j, int, std::string*) -> int {
    gate.wait();
    *j.out = j.input;
    return 0;
  };
  std::vector<uint64_t> outs(kTickets, ~0ull), ids(kTickets, 0);
  for (int i = 0; i < kTickets; i++) {
    Job j{(uint64_t)i, &outs[i]};
    CHECK(tb.submit(std::move(j), 0, &ids[i]) == Table::kOk);
  }
  until(tb, [&] { return tb.running[0] == 1; });
  std::atomic<int> ran{0}, dropped{0};
  std::vector<std::thread> waiters;
  for (int i = 0; i < kTickets; i++)
    waiters.emplace_back([&, i] {
      int done = 0, rc = 1;
      std::string err;
      CHECK(tb.wait(ids[i], Table::kNoLimit, &done, &rc, &err) == Table::kOk && done == 1);
      if (rc == 0) {
        CHECK(outs[i] == (uint64_t)i);
        ran++;
      } else {
        CHECK(rc == kDropped && err == "dropped" && outs[i] == ~0ull);  // a dropped ticket's output was never written
        dropped++;
      }
    });
  until(tb, [&] {
    uint32_t w = 0;
    for (auto& kv : tb.live) w += kv.second->waiters;
    return w == (uint32_t)kTickets;
  });
  std::thread drainer([&] { tb.drain(kDropped, "dropped"); });
  until(tb, [&] { return tb.stopping; });
  {
    Job j{99, &outs[0]};
    uint64_t id = 0;
    CHECK(tb.submit(std::move(j), 0, &id) == Table::kStopping);  // no new tickets while draining
  }
  gate.release();  // the running ticket finishes; the queued seven never run
  drainer.join();
  for (auto& w : waiters) w.join();
  CHECK(ran.load() == 1 && dropped.load() == kTickets - 1);
  CHECK(tb.outstanding() == 0);
  // results nobody waits for are discarded by a drain, and the table works again afterwards
  uint64_t a = 0, b = 0;
  {
    Job j{5, &outs[5]};
    CHECK(tb.submit(std::move(j), 0, &a) == Table::kOk);
  }
  tb.drain(kDropped, "dropped");
  CHECK(tb.outstanding() == 0);
  int done = 0, rc = 0;
  std::string err;
  CHECK(tb.wait(a, 0, &done, &rc, &err) == Table::kUnknown);
  {
    Job j{6, &outs[6]};
    CHECK(tb.submit(std::move(j), 0, &b) == Table::kOk);
  }
  CHECK(tb.wait(b, Table::kNoLimit, &done, &rc, &err) == Table::kOk && done == 1 && rc == 0 && outs[6] == 6);
  printf("drain: 1 ran, %d dropped, all waiters released\n", dropped.load());
}

int main() {
  scenario_stream(1, 1);  // one at a time: strict submission order
  scenario_stream(2, 1);  // the default: two in flight on a device
  scenario_stream(2, 2);  // two devices, a lane each
  scenario_busy_poll_double_wait();
  scenario_drain();
  if (failures.load()) {
    fprintf(stderr, "%d check(s) failed\n", failures.load());
    return 1;
  }
  printf("OK\n");
  return 0;
}
