// A device buffer pool: buffers that leave a slot are PARKED with the events that must have completed before anyone touches the memory
// again, and handed out to the next taker behind stream waits for those events.  No ctx and no HIP in here: the device side is a backend
// B (share.h's, plus one call), so that test_pool.cpp can run the same code on a backend that only logs.
//
// THE RULE.  A parked buffer carries an event set: its block's `ready` event and every `done` event (share.h), or the one event a ctx
// recorded on its stream when it parked a buffer nobody else used.  The buffers of one block share one set.
//   - acquire() enqueues stream_wait(taker's stream, e) for every event of the set before it returns the buffer: the taker's stream is
//     ordered behind every earlier use, and the host waits for nothing.  (A stream that has already waited for a set does not wait for
//     it again: streams run in order.)  The events are destroyed when the last buffer of their set has left the pool.
//   - a parked buffer is passed to B::free only after every event of its set has COMPLETED: event_query said so (cap pressure, trim),
//     or the host waited for it (overflow, the last release).  So a mistake in the ordering above can produce wrong numbers, never an
//     access to freed memory.
//   - the host waits in two places only: park() of a buffer that does not fit under max_parked_bytes even after every completed parked
//     buffer was freed (today's path: wait, free; counted in overflow_waits and host_waits), and the last release() of the pool
//     (not counted: nothing runs any more).  Under the cap host_waits stays 0.
//
// SIZE POLICY (deterministic: the parked list is scanned oldest first).
//   - EXACT  (pyramid levels, the tiled / planar level-0 copies): the oldest parked buffer of exactly `need` bytes; a miss allocates
//     `need` bytes.
//   - ROUNDED (template levels, which carry cap >= n): the smallest parked buffer with need <= bytes <= 2 * need, the oldest of equal
//     ones; a miss allocates round_up(need): the next multiple of a quarter of need's power of two (never less than 4 KiB), i.e. four
//     size classes per octave and at most 25 % more than asked for, so that templates of similar size land in the same class.
//   A request matches buffers that were parked as the same kind (a template level never takes a pyramid level or a level-0 copy, nor
//   the other way round: a buffer keeps the byte size it was allocated with).  Within a kind buffers are parked by byte size, whoever
//   allocated them and however.
//
// Backend B: share.h's, and
//   int  event_query(Event);           // non-blocking: 1 completed, 0 pending (an error counts as pending)
#pragma once
#include <atomic>
#include <cstddef>
#include <list>
#include <mutex>
#include <vector>

namespace sdso {
namespace pool {

enum Match { EXACT = 0, ROUNDED = 1 };

inline size_t round_up(size_t need) {
  size_t g = 4096;
  while (g * 8 <= need) g *= 2;          // g = 2^floor(log2(need)) / 4 once need >= 32 KiB
  return (need + g - 1) / g * g;
}

struct Stats { long long hits, misses, frees, host_waits, overflow_waits, parked_buffers, parked_bytes; };

template <class B>
class Pool {
 public:
  typedef typename B::Event Event;
  typedef typename B::Stream Stream;

  Pool(int device, size_t max_parked_bytes) : device_(device), max_(max_parked_bytes) {}
  int device() const { return device_; }

  void retain() { refs_.fetch_add(1, std::memory_order_relaxed); }
  // One reference goes (the caller's, a ctx's, a block's).  The last one waits for whatever is pending and frees everything, once.
  void release(B& be) {
    if (refs_.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    for (auto& p : parked_) {
      if (!p.set->complete) { for (auto& e : p.set->ev) { be.event_wait(e); be.event_destroy(e); } p.set->ev.clear(); p.set->complete = true; }
      be.free(p.buf, device_);
      frees_.fetch_add(1, std::memory_order_relaxed);
      if (--p.set->users == 0) delete p.set;
    }
    parked_.clear();
    delete this;
  }

  // Takes n buffers (null entries are skipped) that share `events`, and the events; `kind`: what the buffers were (the size policy
  // above).  Never waits under the cap; over it, the wait and the frees are made outside the lock, so that no other ctx stalls behind
  // them: the bytes of the buffers that fit are reserved first, and the buffers enter the list once the fate of the events is known.
  void park(B& be, Match kind, int n, void* const* bufs, const size_t* bytes, std::vector<Event>&& events) {
    std::vector<void*> victims, over;
    std::vector<int> fit;
    {
      std::lock_guard<std::mutex> g(mu_);
      for (int i = 0; i < n; i++) {
        if (!bufs[i]) continue;
        if (bytes_ + bytes[i] > max_) evict_completed(be, bytes_ + bytes[i] - max_, victims);
        if (bytes_ + bytes[i] > max_) { over.push_back(bufs[i]); continue; }   // no room: today's path for this buffer
        fit.push_back(i);
        bytes_ += bytes[i];                               // reserved: parked_bytes counts it from here on
      }
    }
    for (void* v : victims) { be.free(v, device_); frees_.fetch_add(1, std::memory_order_relaxed); }
    bool complete = events.empty();
    if (!over.empty()) {
      if (!complete) {
        for (auto& e : events) { be.event_wait(e); host_waits_.fetch_add(1, std::memory_order_relaxed); be.event_destroy(e); }
        events.clear(); complete = true;
        overflow_waits_.fetch_add(1, std::memory_order_relaxed);
      }
      for (void* v : over) { be.free(v, device_); frees_.fetch_add(1, std::memory_order_relaxed); }
    }
    if (fit.empty()) { for (auto& e : events) be.event_destroy(e); return; }   // (no buffer relies on them)
    Set* set = new Set();
    set->ev = std::move(events);
    set->complete = complete;
    set->users = (int)fit.size();
    std::lock_guard<std::mutex> g(mu_);
    for (int i : fit) parked_.push_back(Parked{bufs[i], bytes[i], kind, set});
  }
  // a host wait (event_wait / stream_sync) that a caller made on its way into park(), where it could leave no event behind
  void count_host_wait() { host_waits_.fetch_add(1, std::memory_order_relaxed); }

  // A buffer of `need` bytes (EXACT) or of need .. 2 * need bytes (ROUNDED) whose every earlier use is ahead of what `stream` runs from
  // here on; *got is its size.  0 on success.
  int acquire(B& be, size_t need, Match m, Stream stream, void** buf, size_t* got) {
    {
      std::lock_guard<std::mutex> g(mu_);
      auto best = parked_.end();
      for (auto it = parked_.begin(); it != parked_.end(); ++it) {
        if (it->kind != m || (m == EXACT ? it->bytes != need : (it->bytes < need || it->bytes > 2 * need))) continue;
        if (best == parked_.end() || it->bytes < best->bytes) best = it;
        if (m == EXACT) break;
      }
      if (best != parked_.end()) {
        Set* set = best->set;
        if (!set->complete && !(set->has_waiter && set->waiter == stream)) {
          for (auto& e : set->ev)
            if (be.stream_wait(stream, e)) { be.event_wait(e); host_waits_.fetch_add(1, std::memory_order_relaxed); }   // (the enqueue failed: wait here instead)
          set->waiter = stream; set->has_waiter = true;
        }
        *buf = best->buf; *got = best->bytes;
        bytes_ -= best->bytes;
        parked_.erase(best);
        if (--set->users == 0) { for (auto& e : set->ev) be.event_destroy(e); delete set; }
        hits_.fetch_add(1, std::memory_order_relaxed);
        return 0;
      }
    }
    misses_.fetch_add(1, std::memory_order_relaxed);
    const size_t want = m == EXACT ? need : round_up(need);
    const int rc = be.alloc(buf, want);
    if (rc) { *buf = nullptr; return rc; }
    *got = want;
    return 0;
  }

  // frees parked buffers whose events have completed, oldest first, until at most keep_bytes stay parked; no host wait
  void trim(B& be, size_t keep_bytes) {
    std::vector<void*> victims;
    {
      std::lock_guard<std::mutex> g(mu_);
      if (bytes_ > keep_bytes) evict_completed(be, bytes_ - keep_bytes, victims);
    }
    for (void* v : victims) { be.free(v, device_); frees_.fetch_add(1, std::memory_order_relaxed); }
  }

  Stats stats() const {
    std::lock_guard<std::mutex> g(mu_);
    return Stats{hits_.load(), misses_.load(), frees_.load(), host_waits_.load(), overflow_waits_.load(), (long long)parked_.size(), (long long)bytes_};
  }

 private:
  struct Set { std::vector<Event> ev; bool complete = false; int users = 0; bool has_waiter = false; Stream waiter{}; };
  struct Parked { void* buf; size_t bytes; Match kind; Set* set; };

  ~Pool() {}
  // (mu_ held) takes completed buffers off the list, oldest first, until `bytes` are gone or none is left; the caller frees them
  void evict_completed(B& be, size_t bytes, std::vector<void*>& victims) {
    size_t gone = 0;
    for (auto it = parked_.begin(); it != parked_.end() && gone < bytes;) {
      Set* set = it->set;
      if (!set->complete) {
        bool all = true;
        for (auto& e : set->ev) if (be.event_query(e) != 1) { all = false; break; }
        if (all) { for (auto& e : set->ev) be.event_destroy(e); set->ev.clear(); set->complete = true; }
      }
      if (!set->complete) { ++it; continue; }
      victims.push_back(it->buf);
      gone += it->bytes; bytes_ -= it->bytes;
      it = parked_.erase(it);
      if (--set->users == 0) delete set;
    }
  }

  const int device_;
  const size_t max_;
  std::atomic<int> refs_{1};                 // the creator's
  mutable std::mutex mu_;                    // guards parked_, bytes_ and the sets
  std::list<Parked> parked_;                 // oldest first
  size_t bytes_ = 0;
  std::atomic<long long> hits_{0}, misses_{0}, frees_{0}, host_waits_{0}, overflow_waits_{0};
};

}  // namespace pool
}  // namespace sdso
