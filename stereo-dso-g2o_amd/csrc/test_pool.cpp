// pool.h and share.h's drop_pooled on a backend that only logs: four threads, each a "ctx" with a stream and a few slots, build, export,
// import, detach, drop, acquire, trim and release against ONE pool, handing handles to each other through one queue.  Three of the
// threads are attached to the pool, the fourth is not (its blocks name no pool).  The scenario runs twice: under a cap that is never
// reached, and under one that is sometimes exceeded.  From the backend's log the program asserts that
//   1. no buffer is handed out twice without a park in between;
//   2. every hand-out of a parked buffer comes after a stream_wait on the taker's stream for each event that was attached to it
//      (or after that event was seen completed);
//   3. no free of a buffer comes ahead of the completion (event_query true, or event_wait) of all its events;
//   4. there is no event_wait / stream_sync on any acquire, nor on any park that stayed under the cap (a park that waits frees a buffer
//      it was given, in that very call; the first run, under the cap, counts no wait at all).  How often the random schedule of the
//      second run exceeds its cap is up to the scheduler, so the overflow path is also walked step by step on one thread
//      (overflow_by_hand): a cap filled with buffers whose events are pending, then one more;
//   5. parked_bytes <= max after every operation;
//   6. after the last release every buffer has been freed once and every event destroyed once;
//   7. blocks without a pool take exactly the old drop path (host waits for every event, no event_query, nothing parked).
// Stand-alone (own main, no HIP): g++ -std=c++17 -pthread test_pool.cpp, also under -fsanitize=address,undefined and -fsanitize=thread.
#include "share.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <thread>

using namespace sdso::share;
namespace pl = sdso::pool;

static void fail(const char* what, int line) { std::fprintf(stderr, "test_pool: FAILED (line %d): %s\n", line, what); std::exit(1); }
#define CHECK(c) do { if (!(c)) fail(#c, __LINE__); } while (0)

enum Op { OP_NONE = 0, OP_PARK, OP_ACQUIRE, OP_TRIM, OP_OLD, OP_LAST_RELEASE };

// ---- the log.  Every fake buffer and event has a number of its own, never reused.  An "owner" is one life of a set of buffers between
// two hand-outs: a block, or the buffers of one slot; the events of that life are filed under its serial.
struct Log {
  std::mutex mu;
  long next = 1;
  struct Ev { long owner = 0; bool recorded = false, complete = false, waited = false, destroyed = false; std::set<int> stream_waited; };
  std::map<long, Ev> ev;
  std::map<long, std::vector<long>> owner_ev;
  struct Buf { long owner = 0; size_t bytes = 0; int freed = 0; bool held = true, fresh = true, rounded = false; };
  std::map<long, Buf> buf;
  std::map<long, int> holders;          // shadow holder count per block serial
  long waits_in_pool_ops = 0, waits_old = 0, frees_pool = 0, frees_old = 0, stream_waits = 0, handouts_parked = 0, queries = 0, allocs = 0;
  void reset() { ev.clear(); owner_ev.clear(); buf.clear(); holders.clear(); waits_in_pool_ops = waits_old = frees_pool = frees_old = stream_waits = handouts_parked = queries = allocs = 0; }
};
static Log g_log;
static thread_local long t_owner = 0;       // the owner the calling thread is working on: what the backend's events are filed under
static thread_local Op t_op = OP_NONE;
static thread_local long t_waits = 0, t_frees_given = 0;
static thread_local std::set<long>* t_given = nullptr;   // the buffers the running park was given
static thread_local std::mt19937* t_rng = nullptr;
static int g_query_mode = 0;                // event_query: 0 the device gets on at random; 1 nothing completes; 2 everything has completed

struct FakeBackend {
  typedef long Event;
  typedef int Stream;
  int event_create(Event* e) { std::lock_guard<std::mutex> g(g_log.mu); *e = g_log.next++; g_log.ev[*e].owner = t_owner; g_log.owner_ev[t_owner].push_back(*e); return 0; }
  void event_destroy(Event e) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed); E.destroyed = true; }
  int event_record(Event e, Stream) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed && !E.recorded); E.recorded = true; return 0; }
  int event_wait(Event e) {
    std::lock_guard<std::mutex> g(g_log.mu);
    auto& E = g_log.ev.at(e);
    CHECK(!E.destroyed && E.recorded);
    CHECK(t_op == OP_PARK || t_op == OP_OLD || t_op == OP_LAST_RELEASE);   // never on an acquire or a trim
    E.complete = E.waited = true;
    if (t_op == OP_OLD) g_log.waits_old++; else if (t_op == OP_PARK) { g_log.waits_in_pool_ops++; t_waits++; }
    return 0;
  }
  int event_query(Event e) {   // the device gets on: a pending event is found completed one time in three
    std::lock_guard<std::mutex> g(g_log.mu);
    auto& E = g_log.ev.at(e);
    CHECK(!E.destroyed && E.recorded);
    CHECK(t_op != OP_OLD);
    g_log.queries++;
    if (!E.complete && (g_query_mode == 2 || (g_query_mode == 0 && (*t_rng)() % 3 == 0))) E.complete = true;
    return E.complete ? 1 : 0;
  }
  int stream_wait(Stream s, Event e) { std::lock_guard<std::mutex> g(g_log.mu); auto& E = g_log.ev.at(e); CHECK(!E.destroyed && E.recorded); E.stream_waited.insert(s); g_log.stream_waits++; return 0; }
  int stream_sync(Stream) { CHECK(t_op == OP_OLD); return 0; }
  int alloc(void** p, size_t bytes) { std::lock_guard<std::mutex> g(g_log.mu); const long id = g_log.next++; g_log.buf[id].bytes = bytes; g_log.allocs++; *p = (void*)(intptr_t)id; return 0; }
  void free(void* p, int) {
    std::lock_guard<std::mutex> g(g_log.mu);
    auto& Bf = g_log.buf.at((long)(intptr_t)p);
    CHECK(Bf.freed == 0);                       // exactly once
    for (long e : g_log.owner_ev[Bf.owner]) {   // 3: not before every event of its life completed; on the old path: was waited for
      const auto& E = g_log.ev.at(e);
      CHECK(!E.recorded || (t_op == OP_OLD ? E.waited : E.complete));
    }
    CHECK(t_op != OP_ACQUIRE && t_op != OP_NONE);
    Bf.freed++;
    if (t_op == OP_OLD) g_log.frees_old++; else g_log.frees_pool++;
    if (t_given && t_given->count((long)(intptr_t)p)) t_frees_given++;
  }
};
typedef Block<FakeBackend> Blk;
typedef pl::Pool<FakeBackend> Pool;
static size_t level_bytes(int, int d0, int d1) { return (size_t)d0 * d1; }
static long id_of(void* p) { return (long)(intptr_t)p; }

static Pool* g_pool = nullptr;
static size_t g_max = 0;

struct Queue {
  std::mutex mu;
  std::vector<std::pair<Blk*, long>> h;   // (block, its serial)
  void push(Blk* b, long serial) { std::lock_guard<std::mutex> g(mu); h.emplace_back(b, serial); }
  bool pop(std::mt19937& rng, Blk** b, long* serial) {
    std::lock_guard<std::mutex> g(mu);
    if (h.empty()) return false;
    const size_t i = rng() % h.size();
    *b = h[i].first; *serial = h[i].second; h[i] = h.back(); h.pop_back();
    return true;
  }
};
static Queue g_queue;

struct Slot { Blk* blk = nullptr; long serial = 0; int levels = 0; bool rounded = false; void* own[kMaxLevels] = {nullptr}; size_t bytes[kMaxLevels] = {0}; };
struct Ctx { FakeBackend be; int stream; Pool* pool; std::mt19937 rng; };

static void check_cap(Ctx& c) {   // 5 (while this thread holds a reference)
  if (!c.pool) return;
  const pl::Stats s = c.pool->stats();
  CHECK((size_t)s.parked_bytes <= g_max && s.parked_bytes >= 0 && s.parked_buffers >= 0);
}
static long new_serial() { std::lock_guard<std::mutex> g(g_log.mu); return g_log.next++; }

// a buffer for a slot of `c`: from its pool (EXACT, or ROUNDED), or allocated
static void* get_buffer(Ctx& c, size_t need, bool rounded, size_t* got) {
  void* p = nullptr;
  if (!c.pool) {
    CHECK(c.be.alloc(&p, need) == 0); *got = need;
    std::lock_guard<std::mutex> g(g_log.mu); g_log.buf.at(id_of(p)).fresh = false; g_log.buf.at(id_of(p)).rounded = rounded;
    return p;
  }
  t_op = OP_ACQUIRE;
  CHECK(c.pool->acquire(c.be, need, rounded ? pl::ROUNDED : pl::EXACT, c.stream, &p, got) == 0);
  t_op = OP_NONE;
  std::lock_guard<std::mutex> g(g_log.mu);
  auto& Bf = g_log.buf.at(id_of(p));
  CHECK(Bf.freed == 0 && Bf.bytes == *got);
  if (Bf.fresh) CHECK(rounded ? *got == pl::round_up(need) : *got == need);
  else {
    CHECK(!Bf.held);                                             // 1
    CHECK(Bf.rounded == rounded);                                // a request takes what was parked as its own kind
    CHECK(rounded ? (*got >= need && *got <= 2 * need) : *got == need);
    for (long e : g_log.owner_ev[Bf.owner]) {                    // 2
      const auto& E = g_log.ev.at(e);
      CHECK(!E.recorded || E.complete || E.stream_waited.count(c.stream));
    }
    g_log.handouts_parked++;
  }
  Bf.fresh = false; Bf.held = true; Bf.rounded = rounded;
  return p;
}
static void fill_slot(Ctx& c, Slot& s) {
  static const size_t kSizes[4] = {4096, 16384, 65536, 262144};
  s.levels = 1 + (int)(c.rng() % 4);
  s.serial = new_serial();
  const bool rounded = s.rounded = c.rng() % 4 == 0;
  for (int l = 0; l < s.levels; l++) {
    const size_t need = rounded ? 3000 + c.rng() % 60000 : kSizes[(c.rng() % 4 + l) % 4];
    s.own[l] = get_buffer(c, need, rounded, &s.bytes[l]);
    std::lock_guard<std::mutex> g(g_log.mu);
    g_log.buf.at(id_of(s.own[l])).owner = s.serial;
  }
}
// a park of buffers this thread was given: it waits only where it frees one of them (4)
template <class F>
static void park_op(const std::set<long>& given, bool leave, bool old_path, F f) {
  std::set<long> giv = given;
  if (leave) { std::lock_guard<std::mutex> g(g_log.mu); for (long b : giv) g_log.buf.at(b).held = false; }
  t_given = &giv; t_waits = 0; t_frees_given = 0;
  t_op = old_path ? OP_OLD : OP_PARK;
  f();
  t_op = OP_NONE; t_given = nullptr;
  if (!old_path) CHECK(t_waits == 0 || t_frees_given > 0);
}
// the slot's own buffers leave: parked behind one event on the ctx's stream, or (no pool) freed behind a synchronisation
static void release_own(Ctx& c, Slot& s, bool unsynced) {
  std::set<long> given;
  for (int l = 0; l < s.levels; l++) given.insert(id_of(s.own[l]));
  if (c.pool) {
    t_owner = s.serial;
    std::vector<long> ev;
    if (unsynced) { long e = 0; CHECK(c.be.event_create(&e) == 0 && c.be.event_record(e, c.stream) == 0); ev.push_back(e); }
    park_op(given, true, false, [&] { c.pool->park(c.be, s.rounded ? pl::ROUNDED : pl::EXACT, s.levels, s.own, s.bytes, std::move(ev)); });
  } else {
    park_op(given, true, true, [&] { c.be.stream_sync(c.stream); for (int l = 0; l < s.levels; l++) c.be.free(s.own[l], 0); });
  }
  s = Slot();
  check_cap(c);
}
// one holder of a block leaves, through drop_pooled (fallback: the dropping ctx's pool; a handle has none)
static void drop_block(FakeBackend& be, Blk* b, long serial, int stream, bool unsynced, Pool* fallback) {
  t_owner = serial;
  std::set<long> given;   // (whichever holder turns out to be the last one parks these)
  for (int l = 0; l < kMaxLevels; l++) if (b->buf[l]) given.insert(id_of(b->buf[l]));
  bool last;
  { std::lock_guard<std::mutex> g(g_log.mu); last = --g_log.holders.at(serial) == 0; }
  const bool old_path = !b->pool && !fallback;   // 7
  park_op(given, last, old_path, [&] { drop_pooled(be, b, stream, unsynced, fallback, level_bytes); });
}
static void release_slot(Ctx& c, Slot& s, bool unsynced) {
  if (s.blk) { drop_block(c.be, s.blk, s.serial, c.stream, unsynced, c.pool); s = Slot(); check_cap(c); }
  else if (s.levels) release_own(c, s, unsynced);
}

static void worker(int tid, int steps, bool pooled) {
  Ctx c{FakeBackend(), tid, pooled ? g_pool : nullptr, std::mt19937(4001u + 131u * (unsigned)tid)};
  t_rng = &c.rng;
  Slot slot[3];
  for (int it = 0; it < steps; it++) {
    Slot& s = slot[c.rng() % 3];
    switch (c.rng() % 8) {
      case 0:
      case 1: {   // build into the slot: in place, or detached
        if (!s.blk && s.levels) break;                          // own buffers: written in place
        if (s.blk) {
          if (write_in_place(s.blk)) break;
          release_slot(c, s, true);                             // detach: the frozen block is left to its other holders
        }
        fill_slot(c, s);
        break;
      }
      case 2: {   // export
        if (!s.blk && !s.levels) break;
        if (!s.blk) {
          int d0[kMaxLevels] = {0}, d1[kMaxLevels] = {0};
          for (int l = 0; l < s.levels; l++) { d0[l] = (int)s.bytes[l]; d1[l] = 1; }
          s.blk = adopt<FakeBackend>(s.rounded ? KIND_TEMPLATE : KIND_PYRAMID, 0, s.levels, s.own, d0, d1);
          if (c.pool) { s.blk->pool = c.pool; c.pool->retain(); }
          std::lock_guard<std::mutex> g(g_log.mu); g_log.holders[s.serial] = 1;
        }
        { std::lock_guard<std::mutex> g(g_log.mu); g_log.holders.at(s.serial)++; }
        t_owner = s.serial;
        CHECK(export_ref(c.be, s.blk, c.stream) == 0);
        g_queue.push(s.blk, s.serial);
        break;
      }
      case 3: {   // import a handle in transit, then pass it on or release it
        Blk* h; long serial;
        if (!g_queue.pop(c.rng, &h, &serial)) break;
        release_slot(c, s, (c.rng() & 1) != 0);
        { std::lock_guard<std::mutex> g(g_log.mu); g_log.holders.at(serial)++; }
        t_owner = serial;
        CHECK(import_ref(c.be, h, c.stream) == 0);
        s.blk = h; s.serial = serial; s.rounded = h->kind == KIND_TEMPLATE;
        if (c.rng() & 1) g_queue.push(h, serial); else { drop_block(c.be, h, serial, 0, false, nullptr); check_cap(c); }
        break;
      }
      case 4: release_slot(c, s, (c.rng() & 1) != 0); break;
      case 5: {   // release a handle in transit
        Blk* h; long serial;
        if (g_queue.pop(c.rng, &h, &serial)) { drop_block(c.be, h, serial, 0, false, nullptr); check_cap(c); }
        break;
      }
      case 6: {   // trim
        if (!c.pool) break;
        t_op = OP_TRIM;
        c.pool->trim(c.be, c.rng() % 3 == 0 ? 0 : (size_t)(c.rng() % (1u << 20)));
        t_op = OP_NONE;
        check_cap(c);
        break;
      }
      case 7: {   // a template level that has to grow: its buffer leaves, a rounded one arrives
        if (s.blk || !s.levels || !s.rounded) break;
        const int l = (int)(c.rng() % s.levels);
        Slot one; one.levels = 1; one.rounded = true; one.own[0] = s.own[l]; one.bytes[0] = s.bytes[l]; one.serial = s.serial;
        const long keep_serial = s.serial;
        if (s.levels > 1) {   // (the level leaves under a life of its own, so that its event is not filed under the levels that stay)
          one.serial = new_serial();
          std::lock_guard<std::mutex> g(g_log.mu); g_log.buf.at(id_of(one.own[0])).owner = one.serial;
        } else s.serial = new_serial();
        release_own(c, one, true);
        s.own[l] = get_buffer(c, s.bytes[l] + 1 + c.rng() % 20000, true, &s.bytes[l]);
        { std::lock_guard<std::mutex> g(g_log.mu); g_log.buf.at(id_of(s.own[l])).owner = s.levels > 1 ? keep_serial : s.serial; }
        break;
      }
    }
  }
  for (auto& s : slot) release_slot(c, s, false);   // (the ctx is destroyed behind a synchronisation)
  if (c.pool) {
    if (tid == 0) { const pl::Stats st = c.pool->stats(); std::printf("  thread 0 at its end: hits %lld misses %lld frees %lld host_waits %lld overflow_waits %lld parked %lld\n", st.hits, st.misses, st.frees, st.host_waits, st.overflow_waits, st.parked_buffers); }
    t_op = OP_LAST_RELEASE; c.pool->release(c.be); t_op = OP_NONE;   // the ctx's reference
  }
}

static void scenario(const char* name, size_t max_bytes, bool release_early) {
  const int kThreads = 4, kSteps = 4000;
  { std::lock_guard<std::mutex> g(g_log.mu); g_log.reset(); }
  g_max = max_bytes;
  g_pool = new Pool(0, max_bytes);
  FakeBackend be;
  std::mt19937 rng(1);
  t_rng = &rng;
  for (int t = 0; t < kThreads - 1; t++) g_pool->retain();   // one per attached ctx
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++) th.emplace_back(worker, t, kSteps, t != kThreads - 1);
  pl::Stats st{};
  if (release_early) { t_op = OP_LAST_RELEASE; g_pool->release(be); t_op = OP_NONE; }   // ctxs and blocks still refer to it
  for (auto& t : th) t.join();
  Blk* h; long serial;
  if (!release_early) {
    st = g_pool->stats();
    std::lock_guard<std::mutex> g(g_log.mu);
    CHECK(st.host_waits == 0 && st.overflow_waits == 0 && g_log.waits_in_pool_ops == 0);            // 4: under the cap nobody waits
    CHECK(st.hits == g_log.handouts_parked && st.hits > 0 && st.misses > 0 && st.frees == g_log.frees_pool);
  }
  t_op = OP_LAST_RELEASE;   // (the handles left over: the last of them, or the caller's reference, ends the pool)
  while (g_queue.pop(rng, &h, &serial)) {
    t_owner = serial;
    { std::lock_guard<std::mutex> g(g_log.mu); --g_log.holders.at(serial); }
    const bool old_path = !h->pool;
    t_op = old_path ? OP_OLD : OP_LAST_RELEASE;
    drop_pooled(be, h, 0, false, (Pool*)nullptr, level_bytes);
  }
  t_op = OP_LAST_RELEASE;
  if (!release_early) g_pool->release(be);
  t_op = OP_NONE;
  g_pool = nullptr;
  std::lock_guard<std::mutex> g(g_log.mu);
  for (auto& kv : g_log.buf) CHECK(kv.second.freed == 1);        // 6
  for (auto& kv : g_log.ev) CHECK(kv.second.destroyed);
  CHECK(g_log.handouts_parked > 0 && g_log.stream_waits > 0 && g_log.frees_old > 0 && g_log.waits_old > 0);
  std::printf("pool ok (%s): %zu buffers, %zu events, %ld hand-outs of parked buffers, %ld stream waits, %ld queries, %ld waits in parks, %ld old-path waits\n",
              name, g_log.buf.size(), g_log.ev.size(), g_log.handouts_parked, g_log.stream_waits, g_log.queries, g_log.waits_in_pool_ops, g_log.waits_old);
}

// The overflow path step by step, on one thread: a cap of three buffers, event_query forced to "pending" or "completed".
static void overflow_by_hand() {
  { std::lock_guard<std::mutex> g(g_log.mu); g_log.reset(); }
  const size_t kB = 4096;
  g_max = 3 * kB;
  Pool* p = new Pool(0, g_max);
  FakeBackend be;
  std::mt19937 rng(2);
  t_rng = &rng;
  auto buffer = [&](long serial) { void* b = nullptr; CHECK(be.alloc(&b, kB) == 0); std::lock_guard<std::mutex> g(g_log.mu); g_log.buf.at(id_of(b)).owner = serial; g_log.buf.at(id_of(b)).held = false; return b; };
  auto event = [&](long serial) { long e = 0; t_owner = serial; CHECK(be.event_create(&e) == 0 && be.event_record(e, 0) == 0); return e; };
  auto park = [&](int n, void** bufs, std::vector<long> ev) { const size_t bytes[2] = {kB, kB}; t_op = OP_PARK; p->park(be, pl::EXACT, n, bufs, bytes, std::move(ev)); t_op = OP_NONE; };
  auto expect = [&](long long host_waits, long long overflow_waits, long long frees, long long parked) {
    const pl::Stats s = p->stats();
    CHECK(s.host_waits == host_waits && s.overflow_waits == overflow_waits && s.frees == frees && s.parked_buffers == parked);
    CHECK((size_t)s.parked_bytes == (size_t)parked * kB && (size_t)s.parked_bytes <= g_max);   // 5
  };
  auto freed = [&](void* b) { std::lock_guard<std::mutex> g(g_log.mu); return g_log.buf.at(id_of(b)).freed; };
  auto waited = [&](long e) { std::lock_guard<std::mutex> g(g_log.mu); return g_log.ev.at(e).waited; };
  g_query_mode = 1;                                            // nothing completes
  void* first[3]; long first_ev[3];
  for (int i = 0; i < 3; i++) { const long s = new_serial(); first[i] = buffer(s); first_ev[i] = event(s); park(1, &first[i], {first_ev[i]}); }
  expect(0, 0, 0, 3);                                          // the cap is full of pending buffers, and nobody has waited
  {   // one more: no parked buffer has completed, so it goes today's way: its event is waited for, then it is freed (3: free() checks the order)
    const long s = new_serial(); void* b = buffer(s); const long e = event(s);
    park(1, &b, {e});
    CHECK(waited(e) && freed(b) == 1);
    for (int i = 0; i < 3; i++) CHECK(!waited(first_ev[i]) && freed(first[i]) == 0);   // what is parked was neither waited for nor freed
    expect(1, 1, 1, 3);
  }
  {   // two buffers behind one event: one wait, one overflow, two frees
    const long s = new_serial(); void* b[2] = {buffer(s), buffer(s)}; const long e = event(s);
    park(2, b, {e});
    CHECK(waited(e) && freed(b[0]) == 1 && freed(b[1]) == 1);
    expect(2, 2, 3, 3);
  }
  {   // a buffer without events does not fit either, and there is nothing to wait for
    const long s = new_serial(); void* b = buffer(s);
    park(1, &b, {});
    CHECK(freed(b) == 1);
    expect(2, 2, 4, 3);
  }
  g_query_mode = 2;                                            // the device has caught up
  {   // now the oldest parked buffer makes room: freed after its event was seen completed, without a wait; the new one is parked
    const long s = new_serial(); void* b = buffer(s); const long e = event(s);
    park(1, &b, {e});
    CHECK(freed(first[0]) == 1 && !waited(first_ev[0]) && freed(first[1]) == 0 && freed(b) == 0 && !waited(e));
    expect(2, 2, 5, 3);
  }
  g_query_mode = 1;
  {   // a hand-out: the taker's stream waits for the buffer's event, the host does not
    void* b = nullptr; size_t got = 0;
    t_op = OP_ACQUIRE; CHECK(p->acquire(be, kB, pl::EXACT, 5, &b, &got) == 0); t_op = OP_NONE;
    CHECK(b == first[1] && got == kB);                         // the oldest of its size
    { std::lock_guard<std::mutex> g(g_log.mu); CHECK(g_log.ev.at(first_ev[1]).stream_waited.count(5) == 1 && g_log.ev.at(first_ev[1]).destroyed); }
    CHECK(p->stats().hits == 1);
    expect(2, 2, 5, 2);
    const long life = new_serial();                            // back it goes after a new life of its own, so that the pool ends with it
    { std::lock_guard<std::mutex> g(g_log.mu); g_log.buf.at(id_of(b)).owner = life; }
    park(1, &b, {event(life)});
  }
  t_op = OP_LAST_RELEASE; p->release(be); t_op = OP_NONE;      // the last reference waits for what is pending and frees everything
  g_query_mode = 0;
  std::lock_guard<std::mutex> g(g_log.mu);
  for (auto& kv : g_log.buf) CHECK(kv.second.freed == 1);
  for (auto& kv : g_log.ev) CHECK(kv.second.destroyed);
  std::printf("pool ok (overflow by hand): %zu buffers, %zu events\n", g_log.buf.size(), g_log.ev.size());
}

int main() {
  overflow_by_hand();
  scenario("under the cap", (size_t)1 << 40, false);
  scenario("cap exceeded", (size_t)1 << 19, true);   // two of the largest buffers: exceeded often, though how often is the scheduler's business
  return 0;
}
