// A work buffer that one ctx owns alone: one allocation in device or pinned host memory, grown on demand, freed by its destructor.
// Neither pooled (pool.h) nor shared between contexts (share.h).  No ctx and no HIP in here: the memory side is a backend B, so that
// test_devbuf.cpp can run the same code on a backend that only logs.
//
// THE RULE (what `grow` of ba_loop.hip and `map_grow` of map.hip did by hand).  reserve(stream, need, grown):
//   - capacity >= need: nothing, and no backend call;
//   - else: wait for `stream` (only if there is something to free: kernels enqueued on it may still use the block), free, become
//     empty, allocate `grown` elements, and take the new capacity only once that allocation has succeeded.  Contents are not kept.
//   It returns the backend's error.  After any failure the buffer is EMPTY (null pointer, capacity 0), never dangling: the next reserve
//   starts from nothing, and the destructor frees nothing twice.
// How much slack `grown` carries is the call site's business (n + n / 4 + 64, bytes + bytes / 2 + 4096, exact, ...).
// reset(stream) frees behind the same wait and leaves the buffer empty.  The destructor and move assignment free WITHOUT a wait: whoever
// destroys a state or overwrites a buffer has synchronised the stream that used it (sdso_ctx_destroy, sdso_track_release_ref, ...).
//
// GROUPS.  Several buffers that are sized by ONE count or stride kept beside them (TraceBatch::n, InitState::cap, ...): that count is
// 0 whenever any member is not allocated for it.  Zero it before the first member is touched, set it after the last reserve succeeded:
//     if (n <= G.cap) return OK;   G.cap = 0;   reset_all(stream, a ... z);   reserve(a) ... reserve(z), each returning on failure;
//     G.cap = grown;
// reset_all first, so that the members are only ever empty or of one size: a growth that failed half-way is started over by the next
// call, whatever count that call asks for.
//
// Backend B (default-constructible, stateless):
//   typedef ... Error;    // Error() is success
//   typedef ... Stream;
//   Error dev_alloc(void**, size_t bytes);    void dev_free(void*);
//   Error host_alloc(void**, size_t bytes);   void host_free(void*);     // pinned host memory
//   Error stream_sync(Stream);
#pragma once
#include <cstddef>

namespace sdso {
namespace devbuf {

enum Space { DEVICE = 0, PINNED = 1 };
template <class T> struct ElemBytes { static constexpr size_t value = sizeof(T); };
template <> struct ElemBytes<void> { static constexpr size_t value = 1; };   // a byte area that its users carve up

template <class B, class T, Space S = DEVICE>
class Buf {
 public:
  typedef typename B::Error Error;
  typedef typename B::Stream Stream;

  Buf() {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { drop(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~Buf() { drop(); }

  Error reserve(Stream stream, size_t need, size_t grown) {
    if (cap_ >= need) return Error();
    Error e = reset(stream);
    if (e != Error()) return e;
    void* q = nullptr;
    e = S == PINNED ? B().host_alloc(&q, ElemBytes<T>::value * grown) : B().dev_alloc(&q, ElemBytes<T>::value * grown);
    if (e != Error()) return e;
    p_ = (T*)q; cap_ = grown;
    return Error();
  }
  Error reset(Stream stream) {
    if (!p_) return Error();
    const Error e = B().stream_sync(stream);
    drop();   // also where the wait failed: the backend's free is safe at any time, and an empty buffer is the state every caller can handle
    return e;
  }

  operator T*() const { return p_; }                                    // launch sites and copies name the buffer as they named the pointer
  template <class U> explicit operator U*() const { return (U*)p_; }    // (float*)ctx->scratch
  T* get() const { return p_; }
  size_t cap() const { return cap_; }                                   // in elements

 private:
  void drop() {
    if (p_) { if (S == PINNED) B().host_free((void*)p_); else B().dev_free((void*)p_); }
    p_ = nullptr; cap_ = 0;
  }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// every member of a group gives up its block, each behind the wait: the first error, or success
template <class B0, class... Bs>
typename B0::Error reset_all(typename B0::Stream stream, B0& first, Bs&... rest) {
  typename B0::Error e = first.reset(stream);
  ((e = e != typename B0::Error() ? e : rest.reset(stream)), ...);
  return e;
}

}  // namespace devbuf
}  // namespace sdso
