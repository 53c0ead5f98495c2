// devbuf.h on a backend that only logs, and whose k-th allocation can be told to fail.  From the log and from the objects' state the
// program asserts the header's contract:
//   1. a reserve within capacity makes no backend call;
//   2. a first reserve allocates without a stream wait;
//   3. a growing reserve logs a wait on the stream it was given, a free, and an alloc of exactly `grown` elements, in that order;
//   4. a failed growth leaves the buffer empty; a following reserve of a smaller need allocates again, and that block is freed once;
//   5. a group of three buffers under one shared count follows the group rule, with the failure at its second and at its third member;
//   6. move construction and move assignment leave the source empty and free the destination's previous block once;
//   7. erasing an entry of a std::map of a struct that holds buffers frees them;
//   8. reset frees behind a wait;
//   9. the pinned space goes through the pinned alloc and free, never the device ones.
// After every scenario each allocation of the log has exactly one free (the blocks are real: the address sanitizer watches as well).
// Stand-alone (own main, no HIP): g++ -std=c++17 test_devbuf.cpp, also under -fsanitize=address,undefined.
#include "devbuf.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

static void fail(const char* what, int line) { std::fprintf(stderr, "test_devbuf: FAILED (line %d): %s\n", line, what); std::exit(1); }
#define CHECK(c) do { if (!(c)) fail(#c, __LINE__); } while (0)

enum Op { SYNC, DEV_ALLOC, DEV_FREE, HOST_ALLOC, HOST_FREE };
struct Rec { Op op; void* p; size_t bytes; int stream; };
static std::vector<Rec> g_log;
static std::map<void*, int> g_live;   // block -> 0 device, 1 pinned
static int g_allocs = 0, g_fail_at = 0;   // the g_fail_at-th allocation from now on fails (0: none)

static void fail_alloc_number(int k) { g_allocs = 0; g_fail_at = k; }

struct FakeBackend {
  typedef int Error;
  typedef int Stream;
  Error alloc(void** p, size_t bytes, int space) {
    if (++g_allocs == g_fail_at) { *p = nullptr; return 2; }
    *p = std::malloc(bytes ? bytes : 1);
    g_live[*p] = space;
    g_log.push_back(Rec{space ? HOST_ALLOC : DEV_ALLOC, *p, bytes, 0});
    return 0;
  }
  void release(void* p, int space) {
    auto it = g_live.find(p);
    CHECK(it != g_live.end());      // allocated, and not freed before
    CHECK(it->second == space);     // by the free of its own space
    g_live.erase(it);
    g_log.push_back(Rec{space ? HOST_FREE : DEV_FREE, p, 0, 0});
    std::free(p);
  }
  Error dev_alloc(void** p, size_t bytes) { return alloc(p, bytes, 0); }
  void dev_free(void* p) { release(p, 0); }
  Error host_alloc(void** p, size_t bytes) { return alloc(p, bytes, 1); }
  void host_free(void* p) { release(p, 1); }
  Error stream_sync(Stream s) { g_log.push_back(Rec{SYNC, nullptr, 0, s}); return 0; }
};
template <class T> using Dev = sdso::devbuf::Buf<FakeBackend, T, sdso::devbuf::DEVICE>;
template <class T> using Pin = sdso::devbuf::Buf<FakeBackend, T, sdso::devbuf::PINNED>;

// every allocation of the log has exactly one free, and nothing is live
static void check_balanced() {
  std::map<void*, int> open;
  for (const Rec& r : g_log) {
    if (r.op == DEV_ALLOC || r.op == HOST_ALLOC) { CHECK(open[r.p] == 0); open[r.p] = 1; }
    if (r.op == DEV_FREE || r.op == HOST_FREE) { CHECK(open[r.p] == 1); open[r.p] = 0; }
  }
  for (auto& kv : open) CHECK(kv.second == 0);
  CHECK(g_live.empty());
}
static void begin() { g_log.clear(); g_fail_at = 0; CHECK(g_live.empty()); }

static void single_buffer() {
  begin();
  {
    Dev<float> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.reserve(7, 0, 0) == 0 && g_log.empty());                       // nothing asked for, nothing done
    CHECK(b.reserve(7, 10, 16) == 0);                                      // 2: the first reserve does not wait
    CHECK(g_log.size() == 1 && g_log[0].op == DEV_ALLOC && g_log[0].bytes == 16 * sizeof(float));
    CHECK(b.get() == g_log[0].p && b.cap() == 16 && (float*)b == b.get());
    CHECK(b.reserve(7, 16, 99) == 0 && b.reserve(7, 3, 99) == 0 && g_log.size() == 1);   // 1: within capacity, no backend call
    void* first = b.get();
    CHECK(b.reserve(9, 17, 40) == 0);                                      // 3: wait on the stream given, free, alloc of `grown`
    CHECK(g_log.size() == 4);
    CHECK(g_log[1].op == SYNC && g_log[1].stream == 9);
    CHECK(g_log[2].op == DEV_FREE && g_log[2].p == first);
    CHECK(g_log[3].op == DEV_ALLOC && g_log[3].bytes == 40 * sizeof(float) && b.get() == g_log[3].p && b.cap() == 40);
    fail_alloc_number(1);                                                  // 4: a failed growth
    CHECK(b.reserve(9, 100, 120) == 2);
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(g_log.size() == 6 && g_log[4].op == SYNC && g_log[5].op == DEV_FREE && g_log[5].p == g_log[3].p);
    CHECK(b.reserve(9, 5, 5) == 0);                                        // a smaller need: no early return on a stale capacity, no wait
    CHECK(g_log.size() == 7 && g_log[6].op == DEV_ALLOC && g_log[6].bytes == 5 * sizeof(float) && b.cap() == 5);
    CHECK(b.reset(4) == 0);                                                // 8: reset frees behind a wait
    CHECK(g_log.size() == 9 && g_log[7].op == SYNC && g_log[7].stream == 4 && g_log[8].op == DEV_FREE && g_log[8].p == g_log[6].p);
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.reset(4) == 0 && g_log.size() == 9);                           // an empty buffer: nothing to wait for
    CHECK(b.reserve(1, 2, 2) == 0);                                        // left to the destructor
  }
  CHECK(g_log.size() == 11 && g_log[10].op == DEV_FREE);                   // (the destructor frees, without a wait)
  check_balanced();
  {
    sdso::devbuf::Buf<FakeBackend, void> bytes;                            // a byte area: capacity in bytes
    CHECK(bytes.reserve(1, 100, 150) == 0 && g_log.back().bytes == 150 && bytes.cap() == 150 && (char*)bytes == bytes.get());
  }
  check_balanced();
}

// three buffers under one count, as every group of the library is written
struct Group {
  Dev<int> a;
  Dev<double> b;
  Pin<char> c;
  int cap = 0;
  int reserve(int stream, int n) {
    if (cap >= n) return 0;
    const size_t grown = (size_t)n + n / 4 + 64;
    cap = 0;
    if (int e = sdso::devbuf::reset_all(stream, a, b, c)) return e;
    if (int e = a.reserve(stream, grown, grown)) return e;
    if (int e = b.reserve(stream, 2 * grown, 2 * grown)) return e;
    if (int e = c.reserve(stream, grown, grown)) return e;
    cap = (int)grown;
    return 0;
  }
  // no member is smaller than the count claims
  bool complete() const { return cap == 0 || (a.cap() == (size_t)cap && b.cap() == 2 * (size_t)cap && c.cap() == (size_t)cap && a.get() && b.get() && c.get()); }
};
static size_t count_ops(size_t from, Op x, Op y) {
  size_t n = 0;
  for (size_t i = from; i < g_log.size(); i++) n += g_log[i].op == x || g_log[i].op == y;
  return n;
}
static void group(int failing_member) {
  begin();
  {
    Group g;
    CHECK(g.reserve(1, 100) == 0 && g.cap == 189 && g.complete());
    CHECK(g_log.size() == 3 && count_ops(0, SYNC, SYNC) == 0);             // fresh members: three allocations, no wait
    CHECK(g.reserve(1, 189) == 0 && g.reserve(1, 7) == 0 && g_log.size() == 3);
    fail_alloc_number(failing_member);
    size_t mark = g_log.size();
    CHECK(g.reserve(5, 1000) == 2);
    CHECK(g.cap == 0);                                                     // 5: the shared count is 0 after the failure
    CHECK(count_ops(mark, DEV_FREE, HOST_FREE) == 3);                      // every member gave up its block, behind a wait on the stream given
    for (size_t i = mark; i < g_log.size(); i++) if (g_log[i].op == DEV_FREE || g_log[i].op == HOST_FREE) CHECK(g_log[i - 1].op == SYNC && g_log[i - 1].stream == 5);
    CHECK(g.a.cap() == 1314 && (failing_member == 2 ? !g.b.get() : g.b.cap() == 2628) && !g.c.get() && g.c.cap() == 0);
    mark = g_log.size();
    CHECK(g.reserve(5, 50) == 0 && g.cap == 126 && g.complete());          // a smaller count: no early return, all three are allocated anew
    CHECK(count_ops(mark, DEV_ALLOC, HOST_ALLOC) == 3);
    CHECK(count_ops(mark, DEV_FREE, HOST_FREE) == (failing_member == 2 ? 1u : 2u));   // (what the failed growth had got as far as allocating)
  }
  check_balanced();
}

static void moves() {
  begin();
  {
    Dev<int> a;
    CHECK(a.reserve(1, 8, 8) == 0);
    void* pa = a.get();
    Dev<int> b(std::move(a));                                              // 6: move construction
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 8 && g_log.size() == 1);
    Dev<int> c;
    CHECK(c.reserve(1, 4, 4) == 0);
    void* pc = c.get();
    const size_t mark = g_log.size();
    c = std::move(b);                                                      // move assignment frees the destination's block, once, and takes the source's
    CHECK(g_log.size() == mark + 1 && g_log[mark].op == DEV_FREE && g_log[mark].p == pc);
    CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 8);
    c = Dev<int>();                                                        // (assigning an empty buffer frees)
    CHECK(g_log.back().op == DEV_FREE && g_log.back().p == pa && c.get() == nullptr);
    CHECK(a.reserve(1, 2, 2) == 0);                                        // a moved-from buffer is an empty one: it serves again
    std::swap(a, c);
    CHECK(a.get() == nullptr && c.cap() == 2);
  }
  check_balanced();
}

struct Holder { Dev<float> x; Pin<int> y; int n = 0; };
static void map_erase() {
  begin();
  {
    std::map<int, Holder> m;
    for (int k = 0; k < 3; k++) { CHECK(m[k].x.reserve(1, 4, 4) == 0 && m[k].y.reserve(1, 1, 1) == 0); }
    Holder h;
    CHECK(h.x.reserve(1, 9, 9) == 0);
    void* old_x = m[0].x.get();
    m[0] = std::move(h);                                                   // (a state replaced by one built aside)
    CHECK(!g_live.count(old_x) && m[0].x.cap() == 9 && m[0].y.get() == nullptr);
    void *x1 = m[1].x.get(), *y1 = m[1].y.get();
    const size_t mark = g_log.size();
    m.erase(1);                                                            // 7
    CHECK(g_log.size() == mark + 2 && !g_live.count(x1) && !g_live.count(y1));
    CHECK(g_live.size() == 3);                                             // m[0].x, m[2].x, m[2].y
  }
  check_balanced();
}

static void pinned() {
  begin();
  {
    Pin<double> p;
    CHECK(p.reserve(3, 4, 6) == 0 && p.reserve(3, 7, 7) == 0 && p.reset(3) == 0 && p.reserve(3, 1, 1) == 0);
  }
  size_t allocs = 0, frees = 0, syncs = 0;
  for (const Rec& r : g_log) {
    CHECK(r.op != DEV_ALLOC && r.op != DEV_FREE);                          // 9
    allocs += r.op == HOST_ALLOC; frees += r.op == HOST_FREE; syncs += r.op == SYNC;
  }
  CHECK(allocs == 3 && frees == 3 && syncs == 2 && g_log[0].bytes == 6 * sizeof(double));
  check_balanced();
}

int main() {
  single_buffer();
  group(2); group(3);
  moves();
  map_erase();
  pinned();
  std::puts("devbuf ok");
  return 0;
}
