// Shared, immutable device blocks: the bookkeeping behind sdso_pyramid_export / sdso_track_export_ref (share.hip).  No ctx and no HIP in
// here: the device side is a backend B, so that test_share.cpp can run the same code on a backend that only logs.
//
// A block is the set of level buffers of one pyramid or one template.  Its holders are the slots that view it (of any ctx on its device)
// and the handles (sdso_shared) that were exported and not yet released; it belongs to them and to nothing else (no registry).  A block
// created by a ctx with a buffer pool (pool.h) also names that pool, and holds a reference to it: drop_pooled() parks there.
//   - exported: set by the first export and never cleared.  From then on the block is FROZEN: no holder writes into it again; a slot
//     that is about to write asks write_in_place() and, on false, detaches (drop() + fresh buffers of its own).
//   - ready: recorded by the first export on the exporter's stream, behind everything that wrote the block; every importer makes its
//     stream wait for it (no host wait).
//   - done: a holder that drops its reference while work it enqueued on the block may still run records an event on its stream into
//     the block.  The holder that drops the LAST reference waits (on the host) for `ready` and for every such event, then frees the
//     buffers: nothing relies on the allocator's free to synchronise anything.
// A block nobody exported has one holder, no events, and is written in place: that path takes no lock, records nothing and waits for
// nothing.
//
// Backend B (an object; the calls return 0 on success):
//   typedef Event, Stream;
//   int  event_create(Event*);         void event_destroy(Event);
//   int  event_record(Event, Stream);  int  event_wait(Event);                 // host wait
//   int  stream_wait(Stream, Event);   int  stream_sync(Stream);               // enqueue a wait / host wait for a whole stream
//   int  alloc(void**, size_t);        void free(void* p, int device);
// (drop_pooled and pool.h also need: int event_query(Event), non-blocking)
#pragma once
#include <atomic>
#include <cstddef>
#include <mutex>
#include <vector>
#include "pool.h"

namespace sdso {
namespace share {

constexpr int kMaxLevels = 6;   // SDSO_PYR_LEVELS
enum Kind { KIND_PYRAMID = 0, KIND_TEMPLATE = 1 };

template <class B>
struct Block {
  int kind = KIND_PYRAMID, device = 0;
  // what a view needs: the level buffers and their sizes (pyramid: w, h; template: n, cap).  Written before the first export only.
  int levels = 0;
  void* buf[kMaxLevels] = {nullptr};
  int dim0[kMaxLevels] = {0}, dim1[kMaxLevels] = {0};
  std::atomic<int> holders{1};          // slots + handles; the creator's slot is the first
  std::atomic<bool> exported{false};
  bool has_ready = false;               // written by the first export, before any other holder exists
  typename B::Event ready{};
  std::mutex mu;                        // guards `done`
  std::vector<typename B::Event> done;
  pool::Pool<B>* pool = nullptr;        // the creator's buffer pool (a reference of the block's own), or null; written before the first export only
};

// the block of buffers a slot owns so far; the slot is its one holder
template <class B>
Block<B>* adopt(int kind, int device, int levels, void* const* bufs, const int* dim0, const int* dim1) {
  Block<B>* b = new Block<B>();
  b->kind = kind; b->device = device; b->levels = levels;
  for (int l = 0; l < kMaxLevels; l++) { b->buf[l] = bufs[l]; b->dim0[l] = dim0[l]; b->dim1[l] = dim1[l]; }
  return b;
}

// may a holder of `b` write into its buffers?  (null: the slot's buffers were never put into a block)
template <class B>
bool write_in_place(const Block<B>* b) { return !b || !b->exported.load(std::memory_order_acquire); }

// One more holder (a handle), taken by a holder on its own thread.  The first export freezes the block and records `ready` on the
// exporter's stream; later ones find the block complete behind the same event.
template <class B>
int export_ref(B& be, Block<B>* b, typename B::Stream s) {
  if (!b->exported.load(std::memory_order_acquire)) {
    typename B::Event e{};
    int rc = be.event_create(&e);
    if (rc) return rc;
    rc = be.event_record(e, s);
    if (rc) { be.event_destroy(e); return rc; }
    b->ready = e; b->has_ready = true;
    b->exported.store(true, std::memory_order_release);
  }
  b->holders.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// One more holder (a slot of the ctx that owns stream `s`), taken through a handle: everything `s` runs from here on comes after `ready`.
template <class B>
int import_ref(B& be, Block<B>* b, typename B::Stream s) {
  if (b->has_ready) { const int rc = be.stream_wait(s, b->ready); if (rc) return rc; }
  b->holders.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// A holder leaves.  `unsynced`: work this holder enqueued on the block may still be running on stream `s` (a handle, or a ctx that has
// just synchronised, passes false).  The last one out waits for every event of the block and frees it, on its own thread.
template <class B>
void drop(B& be, Block<B>* b, typename B::Stream s, bool unsynced) {
  if (unsynced) {
    typename B::Event e{};
    bool recorded = false;
    if (be.event_create(&e) == 0) {
      if (be.event_record(e, s) == 0) recorded = true; else be.event_destroy(e);
    }
    if (recorded) { std::lock_guard<std::mutex> g(b->mu); b->done.push_back(e); }
    else be.stream_sync(s);   // no event to leave behind: wait here instead
  }
  if (b->holders.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  std::vector<typename B::Event> ev;
  { std::lock_guard<std::mutex> g(b->mu); ev.swap(b->done); }
  if (b->has_ready) { be.event_wait(b->ready); be.event_destroy(b->ready); }
  for (auto& e : ev) { be.event_wait(e); be.event_destroy(e); }
  for (int l = 0; l < kMaxLevels; l++) if (b->buf[l]) be.free(b->buf[l], b->device);
  delete b;
}

// drop() for a block that may end in a buffer pool: the block's own, or else `fallback` (the pool of the ctx that drops it; may be
// null).  The last one out does NOT wait: `ready` and the `done` events move into the pool together with the buffers (pool.h: the next
// taker's stream waits for them; nothing is freed before they completed).  bytes(kind, dim0, dim1) is the size of a level buffer.
// Without any pool this is drop().
template <class B, class Bytes>
void drop_pooled(B& be, Block<B>* b, typename B::Stream s, bool unsynced, pool::Pool<B>* fallback, Bytes bytes) {
  pool::Pool<B>* p = b->pool ? b->pool : fallback;
  if (!p) { drop(be, b, s, unsynced); return; }
  if (unsynced) {
    typename B::Event e{};
    bool recorded = false;
    if (be.event_create(&e) == 0) {
      if (be.event_record(e, s) == 0) recorded = true; else be.event_destroy(e);
    }
    if (recorded) { std::lock_guard<std::mutex> g(b->mu); b->done.push_back(e); }
    else { be.stream_sync(s); p->count_host_wait(); }   // no event to leave behind: wait here instead (as drop() does)
  }
  if (b->holders.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  std::vector<typename B::Event> ev;
  { std::lock_guard<std::mutex> g(b->mu); ev.swap(b->done); }
  if (b->has_ready) ev.push_back(b->ready);
  size_t sz[kMaxLevels];
  for (int l = 0; l < kMaxLevels; l++) sz[l] = b->buf[l] ? bytes(b->kind, b->dim0[l], b->dim1[l]) : 0;
  p->park(be, b->kind == KIND_TEMPLATE ? pool::ROUNDED : pool::EXACT, kMaxLevels, b->buf, sz, std::move(ev));
  if (b->pool) b->pool->release(be);   // the block's reference (after the park: the pool may end here)
  delete b;
}

}  // namespace share
}  // namespace sdso
