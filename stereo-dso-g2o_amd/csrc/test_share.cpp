// share.h on a backend that only logs: four threads, each a "ctx" with a stream and a few slots, export, import, write (in place or
// detached) and release blocks in random order, handing handles to each other through one queue.  From the backend's log the program
// asserts that
//   - every buffer is freed exactly once, and every event is destroyed;
//   - no buffer is freed, and no write is granted, while an event recorded into its block has not been waited for;
//   - a block that was never exported is always written in place, and an exported one never is.
// Stand-alone (own main, no HIP): g++ -std=c++17 -pthread test_share.cpp, also under -fsanitize=address,undefined and -fsanitize=thread.
#include "share.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <thread>

using namespace sdso::share;

static void fail(const char* what) { std::fprintf(stderr, "test_share: FAILED: %s\n", what); std::exit(1); }
#define CHECK(c) do { if (!(c)) fail(#c); } while (0)

// ---- the log.  Every fake buffer and event has a number of its own, never reused.  A block is known by the number of its first buffer.
struct Log {
  std::mutex mu;
  long next = 1;
  struct Ev { long block = 0; bool recorded = false, waited = false, destroyed = false; };
  std::map<long, Ev> ev;
  struct Buf { long block = 0; int freed = 0; };
  std::map<long, Buf> buf;
  std::set<long> exported;              // blocks the harness has exported
  long writes_in_place = 0, detaches = 0, frees = 0, stream_waits = 0, host_waits = 0;
  bool events_waited(long block) {      // (mu held)
    for (auto& kv : ev) if (kv.second.block == block && kv.second.recorded && !kv.second.waited) return false;
    return true;
  }
};
static Log g_log;
static thread_local long t_block = 0;   // the block the calling thread is working on: what the backend's events are filed under

struct FakeBackend {
  typedef long Event;
  typedef int Stream;
  int event_create(Event* e) { std::lock_guard<std::mutex> g(g_log.mu); *e = g_log.next++; g_log.ev[*e].block = t_block; return 0; }
  void event_destroy(Event e) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed); CHECK(!E.recorded || E.waited); E.destroyed = true; }
  int event_record(Event e, Stream) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed && !E.recorded); E.recorded = true; return 0; }
  int event_wait(Event e) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed && E.recorded); E.waited = true; g_log.host_waits++; return 0; }
  int stream_wait(Stream, Event e) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed && E.recorded); g_log.stream_waits++; return 0; }
  int stream_sync(Stream) { return 0; }
  int alloc(void** p, size_t) { std::lock_guard<std::mutex> g(g_log.mu); const long id = g_log.next++; g_log.buf[id]; *p = (void*)(intptr_t)id; return 0; }
  void free(void* p, int) {
    std::lock_guard<std::mutex> g(g_log.mu);
    auto& Bf = g_log.buf.at((long)(intptr_t)p);
    CHECK(Bf.freed == 0);                       // exactly once
    CHECK(g_log.events_waited(Bf.block));       // not before every completion event of its block was waited for
    Bf.freed++; g_log.frees++;
  }
};
typedef Block<FakeBackend> Blk;
static long block_id(const Blk* b) { return (long)(intptr_t)b->buf[0]; }

// ---- the handles in transit between the threads
struct Queue {
  std::mutex mu;
  std::vector<Blk*> h;
  void push(Blk* b) { std::lock_guard<std::mutex> g(mu); h.push_back(b); }
  Blk* pop(std::mt19937& rng) {
    std::lock_guard<std::mutex> g(mu);
    if (h.empty()) return nullptr;
    const size_t i = rng() % h.size();
    Blk* b = h[i]; h[i] = h.back(); h.pop_back();
    return b;
  }
};
static Queue g_queue;

static Blk* fresh_block(FakeBackend& be, std::mt19937& rng) {
  void* bufs[kMaxLevels] = {nullptr};
  int d0[kMaxLevels] = {0}, d1[kMaxLevels] = {0};
  const int levels = 1 + (int)(rng() % 4);
  for (int l = 0; l < levels; l++) { CHECK(be.alloc(&bufs[l], 64) == 0); d0[l] = 8 >> l; d1[l] = 8; }
  Blk* b = adopt<FakeBackend>(KIND_PYRAMID, 0, levels, bufs, d0, d1);
  std::lock_guard<std::mutex> g(g_log.mu);
  for (int l = 0; l < levels; l++) g_log.buf.at((long)(intptr_t)bufs[l]).block = block_id(b);
  return b;
}
static void drop_slot(FakeBackend& be, Blk*& b, int stream, bool unsynced) {
  if (!b) return;
  t_block = block_id(b);
  drop(be, b, stream, unsynced);
  b = nullptr;
}

static void worker(int tid, int steps) {
  FakeBackend be;
  std::mt19937 rng(9001u + 77u * (unsigned)tid);
  const int stream = tid;
  Blk* slot[3] = {nullptr, nullptr, nullptr};
  for (int it = 0; it < steps; it++) {
    Blk*& s = slot[rng() % 3];
    switch (rng() % 6) {
      case 0:   // build into the slot: in place, or detached
      case 1: {
        if (!s) { s = fresh_block(be, rng); break; }
        bool was_exported;
        { std::lock_guard<std::mutex> g(g_log.mu); was_exported = g_log.exported.count(block_id(s)) != 0; }
        if (write_in_place(s)) {
          std::lock_guard<std::mutex> g(g_log.mu);
          CHECK(!was_exported);                               // an exported block is never granted to a writer
          CHECK(g_log.events_waited(block_id(s)));            // (and nothing is in flight on one that is)
          g_log.writes_in_place++;
        } else {
          CHECK(was_exported);                                // an unexported block is always written in place
          drop_slot(be, s, stream, true);
          s = fresh_block(be, rng);
          std::lock_guard<std::mutex> g(g_log.mu); g_log.detaches++;
        }
        break;
      }
      case 2: {   // export
        if (!s) break;
        t_block = block_id(s);
        { std::lock_guard<std::mutex> g(g_log.mu); g_log.exported.insert(block_id(s)); }
        CHECK(export_ref(be, s, stream) == 0);
        g_queue.push(s);
        break;
      }
      case 3: {   // import a handle in transit, then pass it on or release it
        Blk* h = g_queue.pop(rng);
        if (!h) break;
        drop_slot(be, s, stream, (rng() & 1) != 0);
        t_block = block_id(h);
        CHECK(import_ref(be, h, stream) == 0);
        s = h;
        if (rng() & 1) g_queue.push(h); else { t_block = block_id(h); drop(be, h, 0, false); }
        break;
      }
      case 4: drop_slot(be, s, stream, (rng() & 1) != 0); break;   // release the slot, with or without work in flight
      case 5: {   // release a handle in transit
        Blk* h = g_queue.pop(rng);
        if (h) { t_block = block_id(h); drop(be, h, 0, false); }
        break;
      }
    }
  }
  for (auto& s : slot) drop_slot(be, s, stream, false);   // (the ctx is destroyed behind a synchronisation)
}

int main() {
  const int kThreads = 4, kSteps = 4000;
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++) th.emplace_back(worker, t, kSteps);
  for (auto& t : th) t.join();
  FakeBackend be;
  std::mt19937 rng(1);
  while (Blk* h = g_queue.pop(rng)) { t_block = block_id(h); drop(be, h, 0, false); }
  std::lock_guard<std::mutex> g(g_log.mu);
  for (auto& kv : g_log.buf) CHECK(kv.second.freed == 1);
  for (auto& kv : g_log.ev) CHECK(kv.second.destroyed);
  CHECK(g_log.writes_in_place > 0 && g_log.detaches > 0 && g_log.stream_waits > 0 && g_log.host_waits > 0);
  std::printf("share ok: %zu buffers, %zu events, %ld writes in place, %ld detaches, %ld stream waits, %ld host waits\n", g_log.buf.size(),
              g_log.ev.size(), g_log.writes_in_place, g_log.detaches, g_log.stream_waits, g_log.host_waits);
  return 0;
}
