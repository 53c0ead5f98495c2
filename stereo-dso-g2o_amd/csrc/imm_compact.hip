// The wave- and block-wide pieces of the resident set: ordered compaction, and one atomic per wave for a predicate.
// Ordered compaction: items [0, N) in segments of L, one workgroup per segment.  segcount -> scan -> segwrite gives every item that
// satisfies the predicate its rank among them, in item order.
template <class Pred>
__global__ __launch_bounds__(256) void k_imm_segcount(Pred pred, int N, int L, int* __restrict__ cnt) {
  __shared__ int s[4];
  const int base = blockIdx.x * L;
  int c = 0;
  for (int x0 = 0; x0 < L; x0 += 256) {
    const int x = x0 + threadIdx.x, idx = base + x;
    const bool on = x < L && idx < N && pred(idx);
    c += __popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}
// Exclusive scan over the 256 threads of a workgroup (every thread calls): the sum of `sum` over the threads before this one; thread 0
// writes the sum over all of them to *total.  The callers give every thread a chunk of their items and finish inside it.
__device__ __forceinline__ int block_exclusive_scan(int sum, int* __restrict__ total) {
  __shared__ int s[256];
  const int t = threadIdx.x;
  s[t] = sum;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 256; k++) { const int c = s[k]; s[k] = run; run += c; }
    *total = run;
  }
  __syncthreads();
  return s[t];
}
// exclusive scan of cnt[0 .. nseg) in place, one workgroup; *total = the sum
__global__ __launch_bounds__(256) void k_imm_scan(int* __restrict__ cnt, int nseg, int* __restrict__ total) {
  const int t = threadIdx.x, per = (nseg + 255) / 256;
  const int b = t * per, e = min(nseg, b + per);
  int sum = 0;
  for (int k = b; k < e; k++) sum += cnt[k];
  int run = block_exclusive_scan(sum, total);
  for (int k = b; k < e; k++) { const int c = cnt[k]; cnt[k] = run; run += c; }
}
// ordered writes inside a segment: rank = segment offset + items before this chunk + waves before this one + lanes before this one
template <class Pred, class Emit>
__global__ __launch_bounds__(256) void k_imm_segwrite(Pred pred, Emit emit, int N, int L, const int* __restrict__ off) {
  __shared__ int s[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * L;
  int run = off[blockIdx.x];
  for (int x0 = 0; x0 < L; x0 += 256) {
    const int x = x0 + threadIdx.x, idx = base + x;
    const bool on = x < L && idx < N && pred(idx);
    const unsigned long long m = __ballot(on);
    if (lane == 0) s[wv] = __popcll(m);
    __syncthreads();
    int pos = run;
    for (int k = 0; k < wv; k++) pos += s[k];
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (on) emit(idx, pos);
    run += s[0] + s[1] + s[2] + s[3];
    __syncthreads();
  }
}

// counts[k] += the lanes of the wave with `on` (one atomic per wave; every lane of the wave calls)
__device__ __forceinline__ void imm_count(int* __restrict__ counts, int k, bool on) {
  const int c = __popcll(__ballot(on));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[k], c);
}
