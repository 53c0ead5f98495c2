// The Schur part of the BA system: k_ba_sc_host<PLAIN, WPH>, AccumulatedSCHessianSSE::addPoint (AccumulatedSCHessian.cpp:34-103 of the
// reference) and the per-point sums of AccumulatedTopHessianSSE::addPoint<mode> (AccumulatedTopHessian.cpp:160-192) from the residuals'
// records (BaDev::r_rec).  The stitch of its bins is ba_tail.hip's, the back-substitution ba_solve.hip's.
namespace sdso {

// ------------------------------------------------------------------ Schur accumulation, one workgroup per host frame
// AccumulatedSCHessianSSE::addPoint (AccumulatedSCHessian.cpp:34-103) for all points of ONE host frame of ONE window, together with the
// per-point sums addPoint<mode> of the top accumulator leaves in the EFPoint (AccumulatedTopHessian.cpp:160-192).
//
// The four waves of the workgroup share the host's points (64-point slices dealt round-robin, 16-point groups inside a slice).  A group's
// records — the contiguous stretch [p_rbeg[p0], p_rbeg[p0 + 16]) of BaDev::r_rec, 64 bytes per residual, no padding for targets a point does
// not observe — travel straight into LDS by `global_load_lds_dwordx4` (no destination registers, nothing to park), one group ahead of the
// arithmetic, and are split on the way: the DMA takes a global address per lane and writes lane-contiguous LDS, so the JpJdF halves land in
// one buffer (double-buffered: phase 2 of group g reads it while group g + 1 arrives) and the term halves in another (single: phase 1 is
// done with it before the next DMA is issued).  The JpJdF halves also go back out, compact, for the back-substitution (BaDev::r_cj).
//   phase 1  per-point terms on ALL 64 lanes: lane = (point, j), j = 0 {bd, Hdd}, 1 {Hcd0, Hcd1}, 2 {Hcd2, Hcd3}, 3 {flags}.  A lane walks
//            its float pair of the point's (<= 8) records in EFPoint::residualsAll order — which IS the order the records lie in — so Hdd / bd /
//            Hcd, HdiF and bdSumF are the reference's additions one after the other, bit for bit, whatever dropResidual did to that order
//            (EnergyFunctional.cpp:524-533); the eight LDS reads of a lane are independent and issued together.  Lane 3 also builds the
//            point's target -> record map (a word of nibbles) for phase 2.  The quad exchanges H / `any` by DPP and stores the point's 32 bytes
//            of BaDev::p_out ([8..13], the sums of linearised / marginalised residuals, only when such residuals exist or their stale values
//            have to be cleared) and idepth_hessian / the active-record mask / `maxRelBaseline = 0` (:44-48) in BaDev::p_track.
//   phase 2  Z^T diag(HdiF) Z on the matrix cores (v_mfma_f64_16x16x4_f64 since round 6, K = 4 points), Z = [JpJdF of the 7 targets a
//            point can observe (never its host) | Hcd | bdSumF] (61 columns in a 4 x 4 grid of 16-column tiles): only the 10 tiles on and above the
//            diagonal are accumulated (80 accumulator registers in f64); the bins below the
//            diagonal are written as mirror images, which makes accD(i,j,k) == accD(i,k,j)^T hold EXACTLY as it does in the reference
//            (AccumulatorXX::update multiplies a_i * b_j * w: the same product for both, MatrixAccumulators.h:31-80) — the stitch relies on it
//            (ba_tail.hip: S2 = S1^T).  Absent targets, residuals that are not active and points without an active residual are exact zeros.
// The waves' tiles are added through LDS in a fixed order (3+2 -> 1+0 -> 0), laid out the way the bins lie in memory and written by all
// four waves as whole 256-byte blocks straight into the packed accumulator block: no per-item partials in HBM, no fold pass.  Only Hcc / bc
// (sums over ALL hosts) leave a 20-float partial per host.
// PLAIN: no marginalisation pass, no point filter, no linearized residual in the launch (every GN iteration of the reference's live flow):
// all active residuals go to the A sums, and the records of a residual that is not active hold zeros — x + 0 is exact — so no flag is read
// on the value lanes.  clearL: also store zeros into the L sums of p_out (a launch with linearised residuals left values there).
// Two workgroups per CU: 197 / 195 / 190 / 189 VGPRs for <PLAIN, WPH> = <1, 1> / <1, 0> / <0, 1> / <0, 0> in the compiler's report (the f64
// tiles), 51 KB of LDS.
// Its global accesses go through gld / gst (ba_kernels.h): a flat store counts in lgkmcnt too, so an LDS read of phase 1 would wait for
// the r_cj stores issued in front of it (110 against 112 us per 256-window launch, profiles/lin_waits_ab.txt).
constexpr int SCH_REC = 1024;                         // floats of one record buffer: 16 points x 8 records x 8 floats
constexpr int SCH_WAVE = 3 * SCH_REC + 16 * 8;        // two JpJdF buffers (double-buffered), one term buffer, the points' phase-2 operands
// WPH ("wave per host", the form of a large batch): every WAVE takes a whole host frame — all its 16-point groups in a row — and a workgroup
// four hosts of one window.  The host's sums never leave the wave's accumulators: no tree over the waves, no barrier; the bins go from the
// registers straight to memory (every (t1, t2) block of 256 bytes is covered by the four stores of one tile; the blocks below the diagonal
// as float4s of the mirrored tile; the five tiles ON the diagonal are mirrored through 1 KB of the wave's stage first).  A batch of 256
// windows is 2 048 waves on 3 072 slots — one round — where 2 048 workgroups on 768 slots need three: 116 -> see DESIGN.md §4.  A single
// window keeps the workgroup per host (a quarter of the latency).
template <bool PLAIN, bool WPH>
__global__ __launch_bounds__(BA_BLOCK, 2) void k_ba_sc_host(const BaDev* __restrict__ wins, const uint8_t* __restrict__ pflag, int shiftPriorToZero, int margMode, int clearL) {
  constexpr int NW = BA_BLOCK / 64;
  const BaDev& B = wins[blockIdx.y];
  if (ba_finished(B)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nf = B.nf, h = WPH ? (int)blockIdx.x * NW + wv : (int)blockIdx.x;
  if (h >= nf) return;                       // (WPH: a wave of its own — the form has no workgroup barrier)
#ifdef SDSO_SC_STAMPS   // diagnostic build (tools/mk_variant.sh scst -DSDSO_SC_STAMPS): shader-clock ticks of wave 0 of two workgroups per phase, printed
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int stn = 0;
#define SCS() do { if (stn < 8) st[stn++] = __builtin_amdgcn_s_memtime(); } while (0)
  unsigned long long sub[6] = {0, 0, 0, 0, 0, 0}, sub_t = 0;     // inside the group loop: wait for the records | r_cj | phase 1 | DMA issue + inputs | phase 2
#define SCSUB(i) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); sub[i] += tn_ - sub_t; sub_t = tn_; } while (0)
#define SCSUB0() do { sub_t = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SCS() do { } while (0)
#define SCSUB(i) do { } while (0)
#define SCSUB0() do { } while (0)
#endif
  SCS();
  constexpr int SC_NT = 10;                                  // tile t of pair (a <= b) of the 4 x 4 tile grid: sc_ut(a, b)
  constexpr int SC_NEED = 2 * 2 * SC_NT * 256;                // the tree's two tile buffers (f64)
  constexpr int SC_LDS = NW * SCH_WAVE > SC_NEED ? NW * SCH_WAVE : SC_NEED;
  __shared__ __align__(16) float stage_all[SC_LDS];
  float* const bufA = stage_all + wv * SCH_WAVE;             // [2][SCH_REC]
  float* const bufT = bufA + 2 * SCH_REC;
  float (*pt)[8] = reinterpret_cast<float (*)[8]>(bufT + SCH_REC);
  const int pb = B.host_pt_beg[h], pe = B.host_pt_beg[h + 1];     // (in the descriptor itself: no dependent round trip before the first DMA)
  // the sums over the points are carried in f64 like the top sums (top_emit): f64 MFMAs on the float operands converted exactly,
  // (w z_a) z_b with the product w z_a exact; ONE rounding to float when the bins are written
  te_d4 acc[SC_NT];
#pragma unroll
  for (int t = 0; t < SC_NT; t++) acc[t] = (te_d4){0.0, 0.0, 0.0, 0.0};
  auto sc_ut = [](int a, int b) { return a * 4 - (a * (a - 1)) / 2 + (b - a); };   // index of the upper tile (a <= b): 0..9
  const int ci = lane & 15, kq = lane >> 4;
  const int tsub = ci >> 3, asub = ci & 7;
  const int pl = lane >> 2, jq = lane & 3;                   // phase 1: point of the group, float pair of the term record
  // a wave's 16-point groups: 64-point slices dealt round-robin over the waves, four groups per slice
  auto group_p0 = [&](int gidx) { return WPH ? pb + 16 * gidx : pb + 64 * (wv + NW * (gidx >> 2)) + 16 * (gidx & 3); };
  // what a group needs beside its records, fetched one group ahead: the first record of its points (lane L: point min(L, npts), so lane 16
  // and everything past the group's end holds the END of its stretch) and, in the phase-1 layout, prior / delta / order / filter of the point
  struct GroupIn { int rb; float prior, delta; unsigned order; int on; };
  auto fetch_in = [&](int p0, GroupIn& g) {
    const int npts = min(16, pe - p0);
    g.rb = 0; g.prior = 0.f; g.delta = 0.f; g.order = 0xffffffffu; g.on = 0;
    if (npts <= 0) return;
    g.rb = gld(B.p_rbeg + p0 + min(lane, npts));
    if (pl < npts) {
      g.prior = gld(B.p_prior + p0 + pl); g.delta = gld(B.p_delta + p0 + pl); g.order = gld(B.p_order + p0 + pl);
      g.on = pflag ? (int)gld(pflag + p0 + pl) : 1;
    }
  };
  // records [r0, r0 + nrec) -> LDS: 16-byte piece c (record c / 2, half c % 2) of the JpJdF halves lands at float 4 c of dstA, of the term
  // halves at float 4 c of dstT
  auto dma_records = [&](int r0, int nrec, float* dstA, float* dstT) {
    const int npieces = nrec * 2;
    const float* g = B.r_rec + (size_t)r0 * 16;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = lane + 64 * k;
      if (64 * k < npieces) {      // (wave-uniform)
        if (c < npieces) {
          const float* src = g + (size_t)(c >> 1) * 16 + 4 * (c & 1);
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)(dstA + 256 * k), 16, 0, 0);
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 8), (__attribute__((address_space(3))) void*)(dstT + 256 * k), 16, 0, 0);
        }
      }
    }
  };
  GroupIn gcur, gnext;
  fetch_in(group_p0(0), gcur);
  {
    const int r0 = __builtin_amdgcn_readlane(gcur.rb, 0), r1 = __builtin_amdgcn_readlane(gcur.rb, 16);
    if (group_p0(0) < pe) dma_records(r0, r1 - r0, bufA, bufT);
  }
  fetch_in(group_p0(1), gnext);
  SCS();
  for (int gidx = 0;; gidx++) {
    const int p0 = group_p0(gidx);
    if (p0 >= pe) break;
    const int npts = min(16, pe - p0);
    float* const curA = bufA + (gidx & 1) * SCH_REC;
    const int r0 = __builtin_amdgcn_readlane(gcur.rb, 0);
    SCSUB0();
    // this group's records (and the inputs of the next one) have landed; the LDS-DMA is invisible to the compiler's own scoreboard
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    SCSUB(0);
    {  // the JpJdF halves, compact, for the back-substitution: coalesced 1-KB stores straight from the stage
      const int npieces = (__builtin_amdgcn_readlane(gcur.rb, 16) - r0) * 2;
      float* dst = B.r_cj + (size_t)r0 * 8;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = lane + 64 * k;
        if (c < npieces) gst((f32x4*)(dst + (size_t)c * 4), *(const f32x4*)(curA + c * 4));
      }
    }
    SCSUB(1);
    {  // ---- phase 1
      const int base = __shfl(gcur.rb, pl, 64) - r0;           // first record of the lane's point inside the stage
      const int cnt = 8 - (__clz((int)~gcur.order) >> 2);           // its records: the nibbles of `order` that are not 0xF (targets are < 8)
      const bool onp = gcur.on != 0;
      float ax = 0.f, ay = 0.f, lx = 0.f, ly = 0.f;            // A and L sums of the lane's float pair
      int ngood = 0, mbits = 0;
      unsigned inv = 0xffffffffu;                              // nibble t: the record of the point's residual to target t
      float2 v[8];
      float fl[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const float* rec = bufT + (base + (k < cnt ? k : 0)) * 8;
        v[k] = *(const float2*)(rec + 2 * jq);
        fl[k] = PLAIN ? 0.f : rec[RR_FLAGS - 8];
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const bool in = k < cnt;
        const unsigned t = (gcur.order >> (4 * k)) & 15u;
        if (PLAIN) {
          // (jq == 3: v.x is the flags word; the value lanes add records as they are — zeros where the residual is not active)
          const int act = in ? ((int)v[k].x & 1) : 0;
          ngood += act; mbits |= act << k;
          ax += in ? v[k].x : 0.f; ay += in ? v[k].y : 0.f;
        } else {
          const int f = in ? (int)fl[k] : 0;
          const bool m = (f & 1) != 0 && onp;                  // residual active (and the point taking part)
          const bool mA = m && !(f & 2) && !margMode, mL = m && !mA;   // mode 0 vs mode 1 / 2 sums (AccumulatedTopHessian.cpp:54-71)
          if (m) { ngood++; mbits |= 1 << k; }
          // x + 0 is exact: masked-off residuals leave the sums untouched
          ax += mA ? v[k].x : 0.f; ay += mA ? v[k].y : 0.f;
          lx += mL ? v[k].x : 0.f; ly += mL ? v[k].y : 0.f;
        }
        if (in) inv = (inv & ~(15u << (4 * t))) | ((unsigned)k << (4 * t));
      }
      // lane 0 of the quad: bd (x), Hdd (y)
      float H = ay + ly + gcur.prior;
      if (H < 1e-10) H = 1e-10;
      const float hdi = 1.0 / H;
      float bds = ax + lx;
      if (shiftPriorToZero) bds += gcur.prior * gcur.delta;
      const bool any = __builtin_amdgcn_mov_dpp(ngood, 0xff, 0xf, 0xf, true) > 0;     // quad lane 3 counted the active residuals
      const float H0 = quad_bcast<0>(H);
      if (pl < npts && onp) {
        float* po = B.p_out + (size_t)(p0 + pl) * 16;
        if (jq == 0) gst((f32x4*)(po + PO_HDD_A), (f32x4){ay, ax, any ? hdi : 0.f, any ? bds : 0.f});
        else if (jq < 3) gst((f32x2*)(po + PO_HCD_A + 2 * (jq - 1)), (f32x2){ax, ay});
        else {
          float* tr = (float*)(B.p_track + p0 + pl);
          gst((f32x2*)(tr + 2), (f32x2){any ? H0 : 0.f, __int_as_float(mbits)});   // p->data->idepth_hessian (:46, :56); the active records for k_ba_resub*
          if (!any) gst(tr, 0.f);                                                      // p->data->maxRelBaseline = 0 (:47)
        }
        if (!PLAIN || clearL) {
          if (jq == 0) gst((f32x2*)(po + PO_HDD_L), (f32x2){ly, lx});
          else if (jq < 3) gst((f32x2*)(po + PO_HCD_L + 2 * (jq - 1)), (f32x2){lx, ly});
        }
      }
      // the point's operands of phase 2: HdiF, bdSumF, Hcd[4] (zeros without an active residual), the target -> record map, its first record
      float2 o2;
      if (jq == 0) o2 = make_float2(any ? hdi : 0.f, any ? bds : 0.f);
      else if (jq < 3) o2 = make_float2(any ? ax + lx : 0.f, any ? ay + ly : 0.f);
      else o2 = make_float2(__int_as_float((int)inv), __int_as_float(base));
      *(float2*)(&pt[pl][2 * jq]) = o2;
    }
    // the term buffer and (since the last iteration's phase 2) the other JpJdF buffer are free: the next group's records may come
    wave_lds_sync();
    SCSUB(2);
    {
      const int pn = group_p0(gidx + 1);
      if (pn < pe) {
        const int n0 = __builtin_amdgcn_readlane(gnext.rb, 0), n1 = __builtin_amdgcn_readlane(gnext.rb, 16);
        dma_records(n0, n1 - n0, bufA + ((gidx + 1) & 1) * SCH_REC, bufT);
      }
    }
    GroupIn gnn;
    fetch_in(group_p0(gidx + 2), gnn);
    SCSUB(3);
    {  // ---- phase 2: the group's four MFMA operand sets (points 4 u + kq).  Column 16 tt + ci of Z: compact target 2 tt + tsub (the
       // targets without the host itself, which no residual of these points observes), element asub; the last eight columns: Hcd, bdSumF
      float zz[4][4], hx[4];
      // three straight stages — the points' words, the sixteen record words, the products — with the scheduler kept from sinking a read
      // next to its use (left alone it waits for sixteen LDS round trips one after the other instead of two).  Every lane reads ONE word
      // per tile column, unconditionally (a load under a condition becomes a branch with its own wait): the record of its target — any
      // record when the point does not observe it, masked afterwards — or, on the special lanes of the last tile column, the point's
      // Hcd / bdSumF word in pt[]
      unsigned invs[4];
      int bases[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int q = 4 * u + kq;
        hx[u] = pt[q][0];
        const float2 ib = *(const float2*)(&pt[q][6]);
        invs[u] = (unsigned)__float_as_int(ib.x); bases[u] = __float_as_int(ib.y);
      }
      __builtin_amdgcn_sched_barrier(0);
      bool oks[4][4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int q = 4 * u + kq;
        const float* rb = curA + bases[u] * 8 + asub;
#pragma unroll
        for (int tt = 0; tt < 4; tt++) {
          const int tp = 2 * tt + tsub, t = tp + (tp >= h ? 1 : 0);       // (tp = 7 is the special block: its lanes take the other address)
          const unsigned k = (invs[u] >> (4 * (t & 7))) & 15u;
          const float* ad = rb + (k & 7u) * 8;
          bool ok = k != 15u;
          if (tt == 3) { ad = tsub ? &pt[q][asub < 4 ? 2 + asub : 1] : ad; ok = tsub ? asub <= 4 : ok; }
          zz[u][tt] = *ad;
          oks[u][tt] = ok;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int tt = 0; tt < 4; tt++) zz[u][tt] = oks[u][tt] ? zz[u][tt] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        double za[4], zd[4];
#pragma unroll
        for (int tt = 0; tt < 4; tt++) { zd[tt] = (double)zz[u][tt]; za[tt] = (double)hx[u] * zd[tt]; }
#pragma unroll
        for (int a = 0; a < 4; a++) {
#pragma unroll
          for (int b = a; b < 4; b++) acc[sc_ut(a, b)] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[a], zd[b], acc[sc_ut(a, b)], 0, 0, 0);
        }
      }
    }
    gcur = gnext; gnext = gnn;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();          // the next group overwrites pt[]
    SCSUB(4);
  }
  SCS();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ---- the host's bins from ONE wave's accumulators (WPH: this wave's; otherwise wave 0's after the tree), rounded to float: d[v] of lane
  // (kq, ci) = D[16 a + 4 kq + v][16 b + ci] of tile (a, b) — four consecutive rows per lane (the f64 MFMA leaves rows kq + 4 v on a lane;
  // its tiles are turned through 1 KB of LDS into that layout first).  Every (t1, t2) block of 256 bytes is covered by
  // the four stores of its tile; the blocks below the diagonal are float4s of the mirrored tile; a tile ON the diagonal takes its lower
  // triangle from the mirror image too: D(r, c) and D(c, r) differ in the last bit ((w z_r) z_c against (w z_c) z_r), and the stitch relies
  // on accD(h, i, j) == accD(h, j, i)^T exactly.  The blocks of the host's own (absent) target are zeros.
  auto store_bins = [&](float* T /* 16 x 17 floats of LDS of this wave */) {
    const int nf2 = nf * nf;
    float* accD = B.accum + acc_off_D(nf);
    float* accE = B.accum + acc_off_E(nf);
    float* accEB = B.accum + acc_off_EB(nf);
    const int ro = 4 * (kq & 1), cc = ci & 7;                 // row (+ v) and column inside an 8 x 8 block
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int t1p = 2 * a + (kq >> 1), t1 = t1p + (t1p >= h ? 1 : 0);
#pragma unroll
      for (int b = a; b < 4; b++) {
        const int t2p = 2 * b + (ci >> 3), t2 = t2p + (t2p >= h ? 1 : 0);
        f32x4 d;
        const te_d4 dd = acc[sc_ut(a, b)];
#pragma unroll
        for (int v = 0; v < 4; v++) d[v] = (float)dd[v];
        wave_lds_sync();
#pragma unroll
        for (int v = 0; v < 4; v++) T[(kq + 4 * v) * 17 + ci] = d[v];
        wave_lds_sync();
#pragma unroll
        for (int v = 0; v < 4; v++) d[v] = T[(4 * kq + v) * 17 + ci];
        if (a == b) {
#pragma unroll
          for (int v = 0; v < 4; v++) { const float m = T[ci * 17 + 4 * kq + v]; d[v] = (4 * kq + v > ci) ? m : d[v]; }
        }
        if (t1p < 7 && t1 < nf) {
          if (t2p < 7) {
            if (t2 < nf) {
              float* blk = accD + (size_t)(h + t1 * nf + t2 * nf2) * 64 + cc;
#pragma unroll
              for (int v = 0; v < 4; v++) gst(blk + (ro + v) * 8, d[v]);
              if (a != b) gst((f32x4*)(accD + (size_t)(h + t2 * nf + t1 * nf2) * 64 + cc * 8 + ro), (f32x4){d[0], d[1], d[2], d[3]});   // the mirror image
            }
          } else if (cc < 4) {                                 // the special block's columns: Hcd ...
#pragma unroll
            for (int v = 0; v < 4; v++) gst(accE + (size_t)(h + t1 * nf) * 32 + (ro + v) * 4 + cc, d[v]);
          } else if (cc == 4) {                                // ... and bdSumF
#pragma unroll
            for (int v = 0; v < 4; v++) gst(accEB + (size_t)(h + t1 * nf) * 8 + ro + v, d[v]);
          }
        } else if (b == 3 && t1p == 7 && t2p == 7 && ro == 0) {   // special x special: Hcc (16) and bc (4) of this host; the fold adds the hosts
          float* hp = B.sc_part + (size_t)h * 20;
          if (cc < 4) {
#pragma unroll
            for (int v = 0; v < 4; v++) gst(hp + v * 4 + cc, d[v]);
          } else if (cc == 4) {
#pragma unroll
            for (int v = 0; v < 4; v++) gst(hp + 16 + v, d[v]);
          }
        }
      }
    }
    // the host's own target: 2 nf - 1 blocks of accD, one of accE and accEB
    for (int k = 0; k < 2 * nf; k++) {
      const int t = k >> 1;
      if ((k & 1) && t == h) continue;
      const int t1 = (k & 1) ? t : h, t2 = (k & 1) ? h : t;
      gst(accD + (size_t)(h + t1 * nf + t2 * nf2) * 64 + lane, 0.f);
    }
    if (lane < 32) gst(accE + (size_t)(h + h * nf) * 32 + lane, 0.f);
    else if (lane < 40) gst(accEB + (size_t)(h + h * nf) * 8 + lane - 32, 0.f);
  };
  if (WPH) {
    store_bins(bufA);
#ifdef SDSO_SC_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SCS();
    if ((h == 0 || h == 5) && (blockIdx.y == 0 || blockIdx.y == 100) && lane == 0)
      printf("sc_host wave-per-host (%d,%d) ticks: prologue %llu  group loop %llu  bins %llu | total %llu  (points %d)  loop: wait %llu  r_cj %llu  phase 1 %llu  dma + inputs %llu  phase 2 %llu\n",
             h, blockIdx.y, st[1] - st[0], st[2] - st[1], st[3] - st[2], st[3] - st[0], pe - pb, sub[0], sub[1], sub[2], sub[3], sub[4]);
#endif
    return;
  }
  __syncthreads();                            // the tiles lie over the waves' stages
  // ---- fixed-order tree over the four waves: (3 -> 1, 2 -> 0), then (1 -> 0); wave 0 writes the bins
  double (*tiles)[SC_NT * 256] = reinterpret_cast<double (*)[SC_NT * 256]>(stage_all);
  auto put = [&](double* dst) {
#pragma unroll
    for (int t = 0; t < SC_NT; t++)
#pragma unroll
      for (int v = 0; v < 4; v++) dst[(t * 4 + v) * 64 + lane] = acc[t][v];
  };
  auto add = [&](const double* src) {
#pragma unroll
    for (int t = 0; t < SC_NT; t++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[t][v] += src[(t * 4 + v) * 64 + lane];
  };
  if (wv >= 2) put(tiles[wv - 2]);
  __syncthreads();
  if (wv < 2) add(tiles[wv]);
  __syncthreads();
  if (wv == 1) put(tiles[1]);                 // (1 + 3)
  __syncthreads();
  SCS();
  if (wv == 0) {
    // (0 + 2) + (1 + 3): the order the tree always had
#pragma unroll
    for (int t = 0; t < SC_NT; t++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[t][v] += tiles[1][(t * 4 + v) * 64 + lane];
    store_bins((float*)tiles[0]);
  }
#ifdef SDSO_SC_STAMPS
  if (wv == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SCS();
    if ((blockIdx.x == 0 || blockIdx.x == 5) && (blockIdx.y == 0 || blockIdx.y == 100) && lane == 0)
      printf("sc_host (%d,%d) ticks: prologue %llu  group loop %llu  wave tree %llu  bins %llu | total %llu  (points %d)  loop: wait %llu  r_cj %llu  phase 1 %llu  dma + inputs %llu  phase 2 %llu\n",
             blockIdx.x, blockIdx.y, st[1] - st[0], st[2] - st[1], st[3] - st[2], st[4] - st[3], st[4] - st[0], pe - pb, sub[0], sub[1], sub[2], sub[3], sub[4]);
  }
#endif
}

#undef SCS
#undef SCSUB
#undef SCSUB0

}  // namespace sdso
