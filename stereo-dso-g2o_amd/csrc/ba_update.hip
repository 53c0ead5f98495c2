// sdso_ba_window_update: the device form of EnergyFunctional::insertResidual / insertFrame / insertPoint / dropResidual / dropPointsF /
// removePoint (src/OptimizationBackend/EnergyFunctional.cpp:445-533, :739-772) and of the residual drops of FullSystem::marginalizeFrame
// (src/FullSystem/FullSystemMarginalize.cpp:146-198) on an uploaded window.  Included at the end of ba.hip (one translation unit).
//
//   plan_window_edit   host: the integer list surgery on the window's mirrors, O(np + nr) — also sdso_ba_window_plan, without a ctx (ba_layout.h)
//   upload_window_impl host (ba_window.hip): the integer arrays, work lists and tables of the edited window, built by the code that builds an uploaded
//                      one (so the two cannot drift apart), staged in one copy together with the appended entries' payload
//   k_ba_window_gather device: the surviving points' and residuals' rows, old slab -> new slab through the plan's maps
//   k_ba_prior_adopt   device: HM / bM (or the chained prior of sdso_ba_marginalize_frame_dev) into the new dimension (ba_solve.hip)
// sdso_ba_window_update_activated: the same edit with stage 7 taken from the latest sdso_imm_activate of the ctx — the tail of
// optimizeImmaturePoint (FullSystemOptPoint.cpp:196-237) and STEP 4 of activatePointsMT (FullSystem.cpp:919-945).
//   plan_activated_stage7  host (ba_layout.h): stage 7's integers from the records' integer members
//   k_ba_window_fill_activated  device: the float rows of the points that came from a record, record -> new slab

// Rows of the surviving points and residuals, old slab -> new slab.  One thread per 16-byte row: six rows per point (p_geo, p_track, two of
// colour, two of weights), then one thread per residual for its two state bytes.  src < 0: the entry is new, its row came with the staged copy.
struct GatherArgs {
  const float4 *o_geo, *o_track, *o_color, *o_weights; const uint8_t *o_state, *o_isnew;
  float4 *n_geo, *n_track, *n_color, *n_weights; float* n_delta; uint8_t *n_state, *n_isnew;
  const int *psrc, *rsrc; int np, nr;
};
__global__ __launch_bounds__(BA_BLOCK) void k_ba_window_gather(const GatherArgs a) {
  const int t = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (t < a.np * 6) {
    const int p = t / 6, k = t - p * 6, s = a.psrc[p];
    if (s < 0) return;
    if (k == 0) {
      const float4 g = a.o_geo[s];
      a.n_geo[p] = g;
      a.n_delta[p] = g.z - g.w;                        // EFPoint::deltaF = idepth - idepth_zero, as the upload forms it (SCALE_IDEPTH = 1)
    } else if (k == 1) {
      const float4 tr = a.o_track[s];
      a.n_track[p] = make_float4(tr.x, tr.y, 0.f, 0.f);   // maxRelBaseline, numGoodResiduals; idepth_hessian and the target mask start at zero
    } else if (k < 4) {
      a.n_color[2 * p + (k - 2)] = a.o_color[2 * s + (k - 2)];
    } else {
      a.n_weights[2 * p + (k - 4)] = a.o_weights[2 * s + (k - 4)];
    }
    return;
  }
  const int j = t - a.np * 6;
  if (j < a.nr) {
    const int s = a.rsrc[j];
    if (s < 0) return;
    a.n_state[j] = a.o_state[s];
    a.n_isnew[j] = a.o_isnew[s];
  }
}

// Rows of the points that sdso_ba_window_update_activated appended: record asrc[p] of the latest sdso_imm_activate -> point p of the new
// slab (asrc < 0: not such a point).  One thread per 16-byte row, the six rows of k_ba_window_gather: what
// PointHessian::PointHessian(const ImmaturePoint*, ...) copies (HessianBlocks.cpp:35-70) and setIdepthZero / setIdepth(currentIdepth)
// (FullSystemOptPoint.cpp:208-209); maxRelBaseline = numGoodResiduals = 0 (HessianBlocks.cpp:41-42).
struct FillActArgs {
  const ImmActRec* rec; const int* asrc;
  float4 *n_geo, *n_track, *n_color, *n_weights; float* n_delta; int np;
};
__global__ __launch_bounds__(BA_BLOCK) void k_ba_window_fill_activated(const FillActArgs a) {
  const int t = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (t >= a.np * 6) return;
  const int p = t / 6, k = t - p * 6, s = a.asrc[p];
  if (s < 0) return;
  const ImmActRec& r = a.rec[s];
  if (k == 0) {
    const float4 g = make_float4(r.u, r.v, r.idepth, r.idepth);
    a.n_geo[p] = g;
    a.n_delta[p] = g.z - g.w;                          // EFPoint::deltaF as the upload forms it from equal idepths (0, or NaN with them)
  } else if (k == 1) {
    a.n_track[p] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if (k < 4) {
    a.n_color[2 * p + (k - 2)] = ((const float4*)r.color)[k - 2];
  } else {
    a.n_weights[2 * p + (k - 4)] = ((const float4*)r.weights)[k - 4];
  }
}

static void launch_window_gather(sdso_ctx* ctx, const BaWindowDev* W, const WindowCarry& cy, const int* d_psrc, const int* d_rsrc, const int* d_asrc) {
  const BaDev& o = cy.old->d;
  const BaDev& d = W->d;
  GatherArgs a;
  a.o_geo = o.p_geo; a.o_track = o.p_track; a.o_color = (const float4*)o.p_color; a.o_weights = (const float4*)o.p_weights; a.o_state = o.r_state; a.o_isnew = o.r_isnew;
  // (the descriptor holds colour / weights / isNew as const: nothing but the upload and this gather ever writes them)
  a.n_geo = d.p_geo; a.n_track = d.p_track; a.n_color = (float4*)const_cast<float*>(d.p_color); a.n_weights = (float4*)const_cast<float*>(d.p_weights); a.n_delta = d.p_delta;
  a.n_state = d.r_state; a.n_isnew = const_cast<uint8_t*>(d.r_isnew);
  a.psrc = d_psrc; a.rsrc = d_rsrc; a.np = d.np; a.nr = d.nr;
  const long work = (long)d.np * 6 + d.nr;
  if (work > 0) {
    ProfScope ps(ctx, "k_ba_window_gather");
    hipLaunchKernelGGL(k_ba_window_gather, dim3((unsigned)((work + BA_BLOCK - 1) / BA_BLOCK)), dim3(BA_BLOCK), 0, ctx->stream, a);
  }
  if (d_asrc && d.np > 0) {
    FillActArgs f;
    f.rec = cy.act_dev; f.asrc = d_asrc; f.n_geo = a.n_geo; f.n_track = a.n_track; f.n_color = a.n_color; f.n_weights = a.n_weights; f.n_delta = a.n_delta; f.np = d.np;
    ProfScope ps(ctx, "k_ba_window_fill_activated");
    hipLaunchKernelGGL(k_ba_window_fill_activated, dim3((unsigned)(((long)d.np * 6 + BA_BLOCK - 1) / BA_BLOCK)), dim3(BA_BLOCK), 0, ctx->stream, f);
  }
  // HM / bM from the old window's (or from the chained prior of sdso_ba_marginalize_frame_dev): the leading prior_dim rows / columns, zeros for
  // the appended frames (insertFrame, EnergyFunctional.cpp:476-482)
  hipLaunchKernelGGL(k_ba_prior_adopt, dim3(8), dim3(256), 0, ctx->stream, W->dt_HM, W->dt_bM, d.n, cy.prior_H, cy.prior_b, cy.prior_dim);
}

extern "C" int sdso_ba_window_plan(int nf, int np, int nr, const int* host, const int* res_point, const int* res_target,
                                   const sdso_ba_window_edit_t* E, int* nf2, int* np2, int* nr2, int* frame_src, int* point_src, int* res_src) {
  if (!E) return SDSO_ERR_ARG;
  WindowPlan P;
  if (!plan_window_edit(nf, np, nr, host, res_point, res_target, *E, P)) return SDSO_ERR_ARG;
  if (nf2) *nf2 = P.nf2;
  if (np2) *np2 = P.np2;
  if (nr2) *nr2 = P.nr2;
  if (frame_src) std::copy(P.frame_src.begin(), P.frame_src.end(), frame_src);
  if (point_src) std::copy(P.point_src.begin(), P.point_src.end(), point_src);
  if (res_src) std::copy(P.res_src.begin(), P.res_src.end(), res_src);
  return SDSO_OK;
}

// act_rec / act_dev: stage 7 of E came from plan_activated_stage7 — its k-th point is record act_rec[k] of act_dev, whose float rows the
// device fills in (E's stage-7 float arrays are not read); nullptr: sdso_ba_window_update
static int window_update_impl(sdso_ctx* ctx, int win, BaWindowDev* O, const sdso_ba_window_edit_t& E, BaWindowDev** made, const int* act_rec = nullptr,
                              const ImmActRec* act_dev = nullptr) {
  const int nf = O->d.nf, np = O->d.np, nr = O->d.nr;
  if (O->in_batch) return sdso::fail(ctx, SDSO_ERR_STATE, "the window is a member of a batch: update it before sdso_ba_batch_create");
  // ---- the window's own order from its mirrors (h_point / h_target are pair-sorted; perm maps sorted -> window order)
  std::vector<int> o_point(nr), o_target(nr), o_host(np);
  for (int j = 0; j < nr; j++) { o_point[O->perm[j]] = O->h_point[j]; o_target[O->perm[j]] = O->h_target[j]; }
  for (int h = 0; h < nf; h++) for (int p = O->d.host_pt_beg[h]; p < O->d.host_pt_beg[h + 1]; p++) o_host[p] = h;
  WindowPlan P;
  if (!plan_window_edit(nf, np, nr, o_host.data(), o_point.data(), o_target.data(), E, P)) return sdso::fail(ctx, SDSO_ERR_ARG, P.why);
  const int nf2 = P.nf2, np2 = P.np2, nr2 = P.nr2;
  SDSO_REQUIRE(ctx, !E.n_add_frames || (E.evalPT && E.state && E.state_zero && E.ab_exposure && E.frameEnergyTH && E.frameID && E.frame_slot), "null stage-5 frame arrays");
  SDSO_REQUIRE(ctx, !E.n_add_res || E.add_res_state, "null stage-6 residual states");
  SDSO_REQUIRE(ctx, !E.n_add_points || act_rec || (E.pt_u && E.pt_v && E.pt_idepth && E.pt_idepth_zero && E.pt_color && E.pt_weights && E.pt_hasDepthPrior), "null stage-7 point arrays");
  SDSO_REQUIRE(ctx, !E.n_pt_res || E.pt_res_state, "null stage-7 residual states");
  for (int r = 0; r < nr2; r++)
    if (P.res_src[r] >= 0 && O->h_lin[O->inv[P.res_src[r]]])
      return sdso::fail(ctx, SDSO_ERR_STATE, "a surviving residual is linearised (fixLinearizationF only touches points that leave)");
  // ---- the prior (sdso_abi.h)
  WindowCarry cy{O, P.point_src.data(), P.res_src.data(), O->dt_HM, O->dt_bM, O->d.n, act_rec, act_dev};
  if (!E.n_remove_frames && O->marg_chain)
    return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_ba_marginalize_frame_dev has run on this window but the edit removes no frame: its prior would be lost");
  if (E.n_remove_frames) {
    std::vector<int> left;
    for (int f : P.frame_src) if (f >= 0) left.push_back(f);
    if (!(O->marg_chain && O->d_marg && O->marg_frames == left && O->marg_dim == 8 * (int)left.size() + 4))
      return sdso::fail(ctx, SDSO_ERR_STATE, "frames leave: sdso_ba_marginalize_frame_dev must have run for exactly those frames since the last sdso_ba_marginalize_points");
    cy.prior_H = O->d_marg; cy.prior_b = O->d_marg + (size_t)O->marg_dim * O->marg_dim; cy.prior_dim = O->marg_dim;
  }
  // ---- the edited window as an upload would receive it: frames and calibration from the host mirror, the integer arrays from the plan,
  // point / residual payload only for the appended entries (the survivors' rows never leave the device)
  std::vector<double> evalPT((size_t)nf2 * 12), state((size_t)nf2 * 10), state_zero((size_t)nf2 * 10);
  std::vector<float> abx(nf2), fth(nf2);
  std::vector<int> fid(nf2), fslot(nf2);
  for (int f = 0; f < nf2; f++) {
    const int s = P.frame_src[f];
    if (s >= 0) {
      const HostFrame& F = O->frames[s];
      std::memcpy(&evalPT[(size_t)f * 12], F.evalPT.R.data(), 72); std::memcpy(&evalPT[(size_t)f * 12 + 9], F.evalPT.t.data(), 24);
      for (int i = 0; i < 10; i++) { state[(size_t)f * 10 + i] = F.state[i]; state_zero[(size_t)f * 10 + i] = F.state_zero[i]; }
      abx[f] = F.ab_exposure; fth[f] = F.frameEnergyTH; fid[f] = F.frameID; fslot[f] = F.frame_slot;
    } else {
      const int k = -1 - s;
      std::memcpy(&evalPT[(size_t)f * 12], E.evalPT + (size_t)k * 12, 96);
      std::memcpy(&state[(size_t)f * 10], E.state + (size_t)k * 10, 80); std::memcpy(&state_zero[(size_t)f * 10], E.state_zero + (size_t)k * 10, 80);
      abx[f] = E.ab_exposure[k]; fth[f] = E.frameEnergyTH[k]; fid[f] = E.frameID[k]; fslot[f] = E.frame_slot[k];
    }
  }
  std::vector<float> u(np2, 0.f), v(np2, 0.f), idp(np2, 0.f), idz(np2, 0.f), mrb(np2, 0.f), color((size_t)np2 * 8, 0.f), weights((size_t)np2 * 8, 0.f);
  std::vector<int> ngood(np2, 0);
  std::vector<uint8_t> hdp(np2, 0), rstate(nr2, 0), risnew(nr2, 1);
  for (int p = 0; p < np2; p++) {
    const int s = P.point_src[p];
    if (s >= 0) { hdp[p] = O->h_prior[s] > 0.f; continue; }   // (EFPoint::priorF is positive exactly where hasDepthPrior was set)
    const int k = -1 - s;
    if (act_rec) continue;                               // (hasDepthPrior = false, HessianBlocks.cpp:38; the float rows: k_ba_window_fill_activated)
    u[p] = E.pt_u[k]; v[p] = E.pt_v[k]; idp[p] = E.pt_idepth[k]; idz[p] = E.pt_idepth_zero[k]; hdp[p] = E.pt_hasDepthPrior[k];
    std::memcpy(&color[(size_t)p * 8], E.pt_color + (size_t)k * 8, 32); std::memcpy(&weights[(size_t)p * 8], E.pt_weights + (size_t)k * 8, 32);
    if (E.pt_maxRelBaseline) mrb[p] = E.pt_maxRelBaseline[k];
    if (E.pt_numGoodResiduals) ngood[p] = E.pt_numGoodResiduals[k];
  }
  for (int r = 0; r < nr2; r++) {
    const int s = P.res_src[r];
    if (s >= 0) continue;
    const int k = -1 - s;
    if (k < E.n_add_res) { rstate[r] = E.add_res_state[k]; if (E.add_res_isNew) risnew[r] = E.add_res_isNew[k]; }
    else { rstate[r] = E.pt_res_state[k - E.n_add_res]; if (E.pt_res_isNew) risnew[r] = E.pt_res_isNew[k - E.n_add_res]; }
  }
  sdso_ba_window_t Wn;
  std::memset(&Wn, 0, sizeof(Wn));
  Wn.nf = nf2; Wn.np = np2; Wn.nr = nr2; Wn.w = O->d.w; Wn.h = O->d.h;
  for (int i = 0; i < 4; i++) { Wn.calib_value_scaled[i] = O->calib.value_scaled[i]; Wn.calib_value_zero[i] = O->calib.value_zero[i]; }
  Wn.evalPT = evalPT.data(); Wn.state = state.data(); Wn.state_zero = state_zero.data();
  Wn.ab_exposure = abx.data(); Wn.frameEnergyTH = fth.data(); Wn.frameID = fid.data(); Wn.frame_slot = fslot.data();
  Wn.u = u.data(); Wn.v = v.data(); Wn.idepth = idp.data(); Wn.idepth_zero = idz.data(); Wn.color = color.data(); Wn.weights = weights.data();
  Wn.host = P.host.data(); Wn.hasDepthPrior = hdp.data();
  Wn.res_point = P.res_point.data(); Wn.res_target = P.res_target.data(); Wn.res_state = rstate.data();
  Wn.solverMode = O->solverMode; Wn.affineOptModeA = O->affA; Wn.affineOptModeB = O->affB; Wn.forceAcceptStep = O->forceAccept;
  Wn.maxRelBaseline = mrb.data(); Wn.numGoodResiduals = ngood.data(); Wn.res_isNew = risnew.data();
  const int rc = upload_window_impl(ctx, win, &Wn, &cy, made);
  if (rc) return rc;
  BaWindowDev* W = *made;
  W->resInM = O->resInM;                               // EnergyFunctional::resInM keeps counting (:704)
  W->hm_host_valid = false;                            // the prior went device to device
  W->prior_pristine = false;
  W->has_order = true;
  W->ord_frame.swap(P.frame_src); W->ord_point.swap(P.point_src); W->ord_res.swap(P.res_src);
  return SDSO_OK;
}

extern "C" int sdso_ba_window_update(sdso_ctx* ctx, int win, const sdso_ba_window_edit_t* E) {
  GET_WIN();
  SDSO_REQUIRE(ctx, E, "null edit");
  BaWindowDev* made = nullptr;
  const int rc = window_update_impl(ctx, win, W, *E, &made);
  if (rc) {                                            // refused (or failed half-way): the old window stays as it was
    if (made) { const std::string why = ctx->err; free_window(ctx, made); ctx->err = why; }
    return rc;
  }
  ctx->wins[win] = made;
  free_window(ctx, W);                                 // old slab back to the pool: the stream orders its reuse behind the gather
  return SDSO_OK;
}

extern "C" int sdso_ba_window_update_activated(sdso_ctx* ctx, int win, const sdso_ba_window_edit_t* E, const int* act_frame, int* n_points, int* n_res,
                                               int* act_index) {
  GET_WIN();
  SDSO_REQUIRE(ctx, E, "null edit");
  SDSO_REQUIRE(ctx, E->n_add_points == 0 && E->n_pt_res == 0, "stage 7 of the edit must be empty: it is taken from the latest sdso_imm_activate");
  ImmActView A;
  imm_activation_view(ctx, &A);
  if (!A.valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_imm_activate on this ctx yet");
  if (A.consumed) return sdso::fail(ctx, SDSO_ERR_STATE, "the latest sdso_imm_activate has already been taken into a window");
  SDSO_REQUIRE(ctx, act_frame, "null act_frame");
  SDSO_REQUIRE(ctx, A.w == W->d.w && A.h == W->d.h, "the activation's w / h differ from the window's");
  ActStage7 S7;
  const char* why = nullptr;
  if (!plan_activated_stage7(W->d.nf, *E, A.nf, act_frame, A.n, A.h_rec, S7, &why)) return sdso::fail(ctx, SDSO_ERR_ARG, why);
  sdso_ba_window_edit_t E2 = *E;
  E2.n_add_points = (int)S7.pt_host.size(); E2.pt_host = S7.pt_host.data();
  E2.n_pt_res = (int)S7.res_point.size(); E2.pt_res_point = S7.res_point.data(); E2.pt_res_target = S7.res_target.data();
  E2.pt_res_state = S7.res_state.data(); E2.pt_res_isNew = nullptr;   // setState(ResState::IN) (FullSystemOptPoint.cpp:218), isNew as constructed
  BaWindowDev* made = nullptr;
  const bool any = E2.n_add_points > 0;
  const int rc = window_update_impl(ctx, win, W, E2, &made, any ? S7.rec.data() : nullptr, any ? A.d_rec : nullptr);
  if (rc) {
    if (made) { const std::string err = ctx->err; free_window(ctx, made); ctx->err = err; }
    return rc;
  }
  ctx->wins[win] = made;
  free_window(ctx, W);
  imm_activation_consumed(ctx);
  if (n_points) *n_points = E2.n_add_points;
  if (n_res) *n_res = E2.n_pt_res;
  if (act_index) std::copy(S7.rec.begin(), S7.rec.end(), act_index);
  return SDSO_OK;
}

extern "C" int sdso_ba_window_get_order(sdso_ctx* ctx, int win, int* frame_src, int* point_src, int* res_src) {
  GET_WIN();
  if (!W->has_order) return sdso::fail(ctx, SDSO_ERR_STATE, "the window has not been updated since its upload");
  if (frame_src) std::copy(W->ord_frame.begin(), W->ord_frame.end(), frame_src);
  if (point_src) std::copy(W->ord_point.begin(), W->ord_point.end(), point_src);
  if (res_src) std::copy(W->ord_res.begin(), W->ord_res.end(), res_src);
  return SDSO_OK;
}
