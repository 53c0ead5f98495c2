// Frame ingest: Undistort::undistort<T> (src/util/Undistort.cpp:398-489) + FrameHessian::makeImages (HessianBlocks.cpp:141-203) from the
// raw 8- or 16-bit camera images, and the host-only construction of the remap tables (Undistort::readFromFile, :793-949).
#include "sdso_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace sdso;

// ------------------------------------------------------------------ remap construction (host only)
// Behaviour of Undistort::readFromFile behind its parsing (Undistort.cpp:793-949) in this library's own terms: a Lens takes a point of
// the normalised image plane to the raw image (the five distortCoordinates bodies, :974-1236), a Rectifier puts the rectified camera K
// in front of it, and the crop search (makeOptimalK_crop, :586-709) works on two Spans of the normalised plane.  tests/undistort_ref.py
// states the same arithmetic in NumPy; the two are compared bit for bit, so every float / double step below is the reference's.
namespace {
struct Pt { float x, y; };

struct Lens {
  int model;
  Pt f, c;          // focal lengths and principal point of the raw camera in pixels; every parameter is rounded to float once (:976 ff.)
  float k[4];       // FOV: omega, -, -, -; RadTan: k1 k2 r1 r2; Equidistant: k1..k4; KannalaBrandt: k0..k3
  float fov_gain;   // FOV: 2 tan(omega / 2), :977

  Lens(int model_, const double* pars) : model(model_) {
    f = Pt{(float)pars[0], (float)pars[1]};
    c = Pt{(float)pars[2], (float)pars[3]};
    for (int i = 0; i < 4; i++) k[i] = (float)pars[4 + i];
    fov_gain = model == SDSO_CAM_FOV ? 2.0f * tanf(k[0] / 2.0f) : 0.f;
  }

  // the three ways a model ends: plain projection, a radial gain applied to the focal length, a radial gain applied to the product
  Pt project(Pt n) const { return Pt{f.x * n.x + c.x, f.y * n.y + c.y}; }
  Pt project_gain_first(Pt n, float g) const { return Pt{f.x * g * n.x + c.x, f.y * g * n.y + c.y}; }
  Pt project_gain_last(Pt n, float g) const { return Pt{f.x * n.x * g + c.x, f.y * n.y * g + c.y}; }
  static float radius(Pt n) { return sqrtf(n.x * n.x + n.y * n.y); }
  // a + k[0] p[0] + k[1] p[1] + k[2] p[2] + k[3] p[3], summed left to right: the odd polynomials of the two fisheye models
  float series(float a, float p0, float p1, float p2, float p3) const { return a + k[0] * p0 + k[1] * p1 + k[2] * p2 + k[3] * p3; }

  Pt fov(Pt n) const {   // :999-1003
    const float r = radius(n);
    const float g = (r == 0 || k[0] == 0) ? 1.0f : atanf(r * fov_gain) / (k[0] * r);
    return project_gain_first(n, g);
  }
  Pt radtan(Pt n) const {   // :1053-1063.  The reference writes the tangential terms with 2.0 literals, so they, and the sums they join, are double
    const float xx = n.x * n.x, yy = n.y * n.y, xy = n.x * n.y, rr = xx + yy;
    const float radial = k[0] * rr + k[1] * rr * rr;
    const double tx = 2.0 * (double)k[2] * (double)xy, ty = 2.0 * (double)k[3] * (double)xy;
    const double sx = (double)k[3] * ((double)rr + 2.0 * (double)xx), sy = (double)k[2] * ((double)rr + 2.0 * (double)yy);
    return project(Pt{(float)((double)(n.x + n.x * radial) + tx + sx), (float)((double)(n.y + n.y * radial) + ty + sy)});
  }
  Pt equidistant(Pt n) const {   // :1114-1125; even powers 4 and 8 are squares, 6 is 4 times 2
    const float r = radius(n), t = atanf(r);
    const float t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const float td = t * series(1.0f, t2, t4, t6, t8);
    return project_gain_last(n, (double)r > 1e-8 ? td / r : 1.0f);
  }
  Pt kannala_brandt(Pt n) const {   // :1170-1192; each odd power is the one before times theta^2
    const float s = radius(n), t = atan2f(s, 1.0f);
    const float t2 = t * t, t3 = t2 * t, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float r = series(t, t3, t5, t7, t9);
    return (double)s < 1e-6 ? project(n) : project_gain_first(n, r / s);
  }
  Pt apply(Pt n) const {
    switch (model) {
      case SDSO_CAM_PINHOLE: return project(n);   // :1229-1232
      case SDSO_CAM_FOV: return fov(n);
      case SDSO_CAM_RADTAN: return radtan(n);
      case SDSO_CAM_EQUIDISTANT: return equidistant(n);
      default: return kannala_brandt(n);
    }
  }
};

struct Rectifier {
  Lens lens;
  double K[4];   // fx fy cx cy of the rectified camera: the reference's Mat33 K, read as float by every distortCoordinates call

  // rectified pixel coordinates -> raw pixel coordinates, in place
  void map(float* xs, float* ys, size_t n) const {
    const Pt of = {(float)K[0], (float)K[1]}, oc = {(float)K[2], (float)K[3]};
    for (size_t i = 0; i < n; i++) {
      const Pt p = lens.apply(Pt{(xs[i] - oc.x) / of.x, (ys[i] - oc.y) / of.y});
      xs[i] = p.x;
      ys[i] = p.y;
    }
  }
};

// an interval of the normalised image plane along one axis
struct Span {
  float lo = 0, hi = 0;
  float width() const { return hi - lo; }
  float at(int i, int n) const { return lo + (hi - lo) * (float)i / ((float)n - 1.0f); }   // n samples, both ends included
};
// strictly inside the raw image along an axis of `size` pixels (a NaN is not)
inline bool strictly_inside(float v, int size) { return v > 0 && v < (float)(size - 1); }

// The part of the axis through the origin (0 = x, 1 = y) that the lens, with K = identity, sends inside the raw image: 100000 samples
// 1e-4 apart around 0 (:590-624).  The lower end is the first visible sample that is not 0 itself, the upper end the last visible one;
// 0 where there is none.
Span visible_span(const Rectifier& R, int axis, int size) {
  const int n = 100000;
  std::vector<float> t(n), moving(n), fixed(n, 0.f);
  for (int i = 0; i < n; i++) moving[i] = t[i] = ((float)i - 50000.0f) / 10000.0f;
  if (axis == 0) R.map(moving.data(), fixed.data(), n); else R.map(fixed.data(), moving.data(), n);
  int first = -1, last = -1;
  for (int i = 0; i < n; i++) {
    if (!strictly_inside(moving[i], size)) continue;
    if (first < 0 && t[i] != 0) first = i;
    last = i;
  }
  Span s;
  if (first >= 0) s.lo = t[first];
  if (last >= 0) s.hi = t[last];
  return s;
}

// Walk the two edges of the rectified image that bound `axis` (at across.lo and across.hi, n samples along the other axis) through the
// lens: out[e] says whether edge e leaves the raw image somewhere (:637-676).  a, b: work arrays of 2 n floats.
void edges_outside(const Rectifier& R, int axis, const Span& across, const Span& along, int n, int size, bool out[2], float* a, float* b) {
  for (int i = 0; i < n; i++) {
    a[2 * i] = across.lo;
    a[2 * i + 1] = across.hi;
    b[2 * i] = b[2 * i + 1] = along.at(i, n);
  }
  if (axis == 0) R.map(a, b, 2 * (size_t)n); else R.map(b, a, 2 * (size_t)n);
  out[0] = out[1] = false;
  for (int i = 0; i < 2 * n; i++)
    if (!strictly_inside(a[i], size)) out[i & 1] = true;
}

// makeOptimalK_crop (:586-709): the largest K whose w x h image lies inside the raw one.  Starts from the visible spans widened by 1 %,
// then pulls in by 0.5 % per round every edge that leaves the raw image; when edges of both axes do, only the wider span gives way in
// that round.  false = the reference's exit after 500 rounds, which it tests before it looks whether the last round was clean.
bool crop_to_visible(Rectifier& R, int wOrg, int hOrg, int w, int h) {
  R.K[0] = R.K[1] = 1;   // K.setIdentity(), :588
  R.K[2] = R.K[3] = 0;
  Span X = visible_span(R, 0, wOrg), Y = visible_span(R, 1, hOrg);
  for (Span* s : {&X, &Y}) { s->lo *= 1.01; s->hi *= 1.01; }   // float *= double, :626-629
  std::vector<float> a(2 * (size_t)std::max(w, h)), b(a.size());
  for (int round = 1;; round++) {
    bool ox[2], oy[2];
    edges_outside(R, 0, X, Y, h, wOrg, ox, a.data(), b.data());
    edges_outside(R, 1, Y, X, w, hOrg, oy, a.data(), b.data());
    const bool x_out = ox[0] || ox[1], y_out = oy[0] || oy[1];
    const bool x_wider = X.width() > Y.width();
    if (x_out && (!y_out || x_wider)) {
      if (ox[0]) X.lo *= 0.995;
      if (ox[1]) X.hi *= 0.995;
    }
    if (y_out && (!x_out || !x_wider)) {
      if (oy[0]) Y.lo *= 0.995;
      if (oy[1]) Y.hi *= 0.995;
    }
    if (round > 500) return false;
    if (!x_out && !y_out) break;
  }
  R.K[0] = ((float)w - 1.0f) / X.width();   // :705-708: the quotients are float, the products with them double
  R.K[1] = ((float)h - 1.0f) / Y.width();
  R.K[2] = -X.lo * R.K[0];
  R.K[3] = -Y.lo * R.K[1];
  return true;
}

// What a rectified pixel reads (:928-949): the raw coordinate (u, v), moved off the exact first and last row / column ("rounding
// resistant" in the reference), or false = outside.  Two quirks of the reference are part of the rule and are kept:
//   - a v exactly on the last row moves u, not v, and to hOrg - 1.001 (:937);
//   - v is tested against the last COLUMN (:939), so for hOrg > wOrg rows below wOrg - 1 count as outside, and for hOrg < wOrg a v beyond
//     the last row counts as inside (sdso_ingest_calib_create turns those entries into "outside").
bool settle_tap(float& u, float& v, int wOrg, int hOrg) {
  const float last_col = wOrg - 1, last_row = hOrg - 1;
  const float just_inside = 0.001, col_inside = wOrg - 1.001, row_inside = hOrg - 1.001;   // double literals rounded to float
  if (u == 0) u = just_inside;
  if (v == 0) v = just_inside;
  if (u == last_col) u = col_inside;
  if (v == last_row) u = row_inside;
  return u > 0 && v > 0 && u < last_col && v < last_col;
}
}  // namespace

extern "C" int sdso_undistort_make_remap(int model, const double* parsOrg, int wOrg, int hOrg, int w, int h, int out_mode, const float* out_calib,
                                         double* K, float* remapX, float* remapY, int* passthrough) {
  if (model < SDSO_CAM_PINHOLE || model > SDSO_CAM_KANNALABRANDT || !parsOrg || !K || !remapX || !remapY || !passthrough) return SDSO_ERR_ARG;
  if (wOrg < 2 || hOrg < 2 || w < 2 || h < 2 || wOrg > 32768 || hOrg > 32768 || w > 32768 || h > 32768) return SDSO_ERR_ARG;
  double pars[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int npars = (model == SDSO_CAM_PINHOLE || model == SDSO_CAM_FOV) ? 5 : 8;
  for (int i = 0; i < npars; i++) pars[i] = parsOrg[i];
  if (pars[2] < 1 && pars[3] < 1) {   // the "relative" calibration format, :793-809
    pars[0] = pars[0] * wOrg;
    pars[1] = pars[1] * hOrg;
    pars[2] = pars[2] * wOrg - 0.5;
    pars[3] = pars[3] * hOrg - 0.5;
  }
  Rectifier R{Lens(model, pars), {1, 1, 0, 0}};
  *passthrough = 0;
  switch (out_mode) {
    case SDSO_RECTIFY_CROP:
      if (!crop_to_visible(R, wOrg, hOrg, w, h)) return SDSO_ERR_ARG;
      break;
    case SDSO_RECTIFY_NONE:               // :882-895
      if (w != wOrg || h != hOrg) return SDSO_ERR_ARG;
      for (int i = 0; i < 4; i++) R.K[i] = pars[i];
      *passthrough = 1;
      break;
    case SDSO_RECTIFY_EXPLICIT:           // :896-909: the products are float, the - 0.5 double
      if (!out_calib) return SDSO_ERR_ARG;
      R.K[0] = out_calib[0] * w;
      R.K[1] = out_calib[1] * h;
      R.K[2] = out_calib[2] * w - 0.5;
      R.K[3] = out_calib[3] * h - 0.5;
      break;
    default:                              // makeOptimalK_full is assert(false) (:711-714)
      return SDSO_ERR_ARG;
  }
  for (int i = 0; i < 4; i++) K[i] = R.K[i];
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) { remapX[x + y * w] = x; remapY[x + y * w] = y; }
  R.map(remapX, remapY, (size_t)w * h);
  for (size_t i = 0; i < (size_t)w * h; i++)
    if (!settle_tap(remapX[i], remapY[i], wOrg, hOrg)) remapX[i] = remapY[i] = -1;
  return SDSO_OK;
}

// ------------------------------------------------------------------ device side
namespace sdso {

enum { PHOTO_LINEAR = 0, PHOTO_G = 1, PHOTO_G_VIGNETTE = 2 };   // PhotometricUndistorter::processFrame, :231-250

struct IngestCalib {
  int wOrg = 0, hOrg = 0, w = 0, h = 0, pixel_bytes = 1, mode = 0;
  bool passthrough = false, use_exposure = true;
  DevBuf<float2> remap;      // {remapX, remapY} per output pixel; x < 0 = outside
  DevBuf<float> G;           // 256 or 65536 floats; null = the reference's !valid
  DevBuf<float> vinv;        // vignetteMapInv, wOrg*hOrg
};
// Raw images wait in pinned memory for their copy: a StageBuf of this module's own (the double buffer of the window upload), so
// sdso_ingest_frame never waits for the stream.  ctx->pinned cannot serve: the synchronous entry points write it without waiting for
// anything, which would race with a copy still in flight.
struct IngestState {
  std::map<int, IngestCalib> calibs;
  StageBuf stage;
  DevBuf<char> raw;          // the raw images of the ingest in flight on the device; the stream orders its reuse
};

void release_ingest(sdso_ctx* ctx) {
  if (!ctx->ingest) return;
  stage_free(ctx->ingest->stage);
  delete ctx->ingest;
  ctx->ingest = nullptr;
}

struct IngestImage { const void* raw; float4* dst; int kind; };
struct IngestImages { IngestImage img[2]; };

// Level 0 of both eyes from the raw images: per output pixel the remap pair, four raw taps, the response and vignette per tap and the
// bilinear blend of Undistort.cpp:459-472 in its operation order (one rounding per operation: -ffp-contract=off), stored as the
// pyramid's float4 {I, 0, 0, 0}.  The photometric image of :231-250 is never written out: G[raw] * vignetteMapInv of a tap is the same
// product whether it is formed once per raw pixel or once per tap.  blockIdx.y = eye.  The 8-bit response sits in LDS; the 16-bit one
// (256 KB) is read through the cache.  Remap entries are made safe by sdso_ingest_calib_create: x >= 0 implies all four taps exist.
template <typename T, bool PASS>
__global__ __launch_bounds__(256) void k_ingest_level0(IngestImages A, const float2* __restrict__ remap, const float* __restrict__ G,
                                                       const float* __restrict__ vinv, float factor, int wOrg, int npix) {
  __shared__ float sG[256];
  const IngestImage I = A.img[blockIdx.y];
  const int kind = I.kind;
  if (sizeof(T) == 1 && kind != PHOTO_LINEAR) {   // uniform over the block
    sG[threadIdx.x] = G[threadIdx.x];
    __syncthreads();
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const T* __restrict__ raw = (const T*)I.raw;
  auto photo = [&](T r, int idx) -> float {
    if (kind == PHOTO_LINEAR) return factor * r;
    float v;
    if constexpr (sizeof(T) == 1) v = sG[r]; else v = G[r];
    if (kind == PHOTO_G_VIGNETTE) v *= vinv[idx];
    return v;
  };
  float v;
  if (PASS) {
    v = photo(raw[i], i);
  } else {
    const float2 m = remap[i];
    float xx = m.x, yy = m.y;
    if (xx < 0) {
      v = 0;
    } else {
      const int xxi = xx, yyi = yy;
      xx -= xxi;
      yy -= yyi;
      const float xxyy = xx * yy;
      const int b = xxi + yyi * wOrg;
      T r0[2], r1[2];   // the two taps of a row are neighbours: one load per row where the alignment rules let the compiler merge them
      __builtin_memcpy(r0, raw + b, sizeof(r0));
      __builtin_memcpy(r1, raw + b + wOrg, sizeof(r1));
      const float s00 = photo(r0[0], b), s01 = photo(r0[1], b + 1), s10 = photo(r1[0], b + wOrg), s11 = photo(r1[1], b + wOrg + 1);
      v = xxyy * s11 + (yy - xxyy) * s10 + (xx - xxyy) * s01 + (1 - xx - yy + xxyy) * s00;
    }
  }
  I.dst[i] = make_float4(v, 0.f, 0.f, 0.f);
}

template <typename T>
static void launch_level0(sdso_ctx* ctx, const IngestCalib& c, const IngestImages& A, int n_images, float factor) {
  const int npix = c.w * c.h;
  const dim3 grid((npix + 255) / 256, n_images), block(256);
  if (c.passthrough) launch_timed(ctx, "k_ingest_level0", 1, k_ingest_level0<T, true>, grid, block, A, (const float2*)c.remap, (const float*)c.G, (const float*)c.vinv, factor, c.wOrg, npix);
  else launch_timed(ctx, "k_ingest_level0", 1, k_ingest_level0<T, false>, grid, block, A, (const float2*)c.remap, (const float*)c.G, (const float*)c.vinv, factor, c.wOrg, npix);
}

}  // namespace sdso

// ------------------------------------------------------------------ API
extern "C" int sdso_ingest_calib_create(sdso_ctx* ctx, int calib, int wOrg, int hOrg, int w, int h, const float* remapX, const float* remapY, int pixel_bytes,
                                        const float* G, const float* vignetteMapInv, int photometricCalibration, int useExposure) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, wOrg >= 2 && hOrg >= 2 && wOrg <= 32768 && hOrg <= 32768 && w >= 8 && h >= 8 && w <= 32768 && h <= 32768, "image size out of range");
  SDSO_REQUIRE(ctx, (remapX == nullptr) == (remapY == nullptr), "remapX and remapY come together");
  SDSO_REQUIRE(ctx, remapX || (w == wOrg && h == hOrg), "passthrough needs equal input and output sizes");
  SDSO_REQUIRE(ctx, pixel_bytes == 1 || pixel_bytes == 2, "pixel width must be 1 or 2 bytes");
  SDSO_REQUIRE(ctx, photometricCalibration >= 0 && photometricCalibration <= 2, "photometricCalibration must be 0, 1 or 2");
  SDSO_REQUIRE(ctx, !(G && photometricCalibration == 2 && !vignetteMapInv), "mode 2 needs vignetteMapInv");
  for (int l = 0, levels = sdso_pyramid_levels(w, h); l < levels; l++)   // refused here, so that sdso_ingest_frame cannot fail on a slot's shape
    SDSO_REQUIRE(ctx, (w >> l) >= 8 && (h >> l) >= 8, "pyramid level too small");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->ingest) ctx->ingest = new IngestState();
  IngestState& S = *ctx->ingest;
  IngestCalib c;   // built aside: an id in use keeps its tables until the new ones are complete
  c.wOrg = wOrg; c.hOrg = hOrg; c.w = w; c.h = h; c.pixel_bytes = pixel_bytes; c.mode = photometricCalibration;
  c.passthrough = !remapX; c.use_exposure = useExposure != 0;
  const size_t npix = (size_t)w * h, norg = (size_t)wOrg * hOrg;
  hipError_t e = hipSuccess;
  if (remapX) {
    std::vector<float2> m(npix);
    for (size_t i = 0; i < npix; i++) {
      const float x = remapX[i], y = remapY[i];
      // :454 sends x < 0 to 0; any other entry is read at (int)x, (int)y and their right / lower neighbours: where one of those four lies
      // outside wOrg x hOrg (the reference would read out of bounds there) the entry counts as outside, too
      const bool inside = x >= 0 && x < (float)(wOrg - 1) && y > -1.0f && y < (float)(hOrg - 1);
      m[i] = inside ? make_float2(x, y) : make_float2(-1.f, -1.f);
    }
    if ((e = c.remap.reserve(ctx->stream, npix, npix)) == hipSuccess) e = hipMemcpy(c.remap, m.data(), sizeof(float2) * npix, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && G) {
    const size_t gn = pixel_bytes == 1 ? 256 : 65536;
    if ((e = c.G.reserve(ctx->stream, gn, gn)) == hipSuccess) e = hipMemcpy(c.G, G, sizeof(float) * gn, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && G && vignetteMapInv) {
    if ((e = c.vinv.reserve(ctx->stream, norg, norg)) == hipSuccess) e = hipMemcpy(c.vinv, vignetteMapInv, sizeof(float) * norg, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && S.calibs.count(calib)) e = hipStreamSynchronize(ctx->stream);   // an ingest in flight may still read the tables this call replaces
  if (e != hipSuccess) return sdso::fail(ctx, SDSO_ERR_HIP, std::string("sdso_ingest_calib_create: ") + hipGetErrorString(e));   // (c's tables go with it)
  S.calibs[calib] = std::move(c);
  return SDSO_OK;
}

extern "C" int sdso_ingest_calib_release(sdso_ctx* ctx, int calib) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->ingest) return SDSO_OK;
  auto it = ctx->ingest->calibs.find(calib);
  if (it == ctx->ingest->calibs.end()) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ingest->calibs.erase(it);
  return SDSO_OK;
}

extern "C" int sdso_ingest_frame(sdso_ctx* ctx, int calib, int n_images, const int* frame_slots, const void* const* raw, const float* exposure, float factor,
                                 float* exposure_out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, ctx->ingest && ctx->ingest->calibs.count(calib), "unknown ingest calibration");
  SDSO_REQUIRE(ctx, n_images >= 1 && n_images <= 2, "n_images must be 1 or 2");
  SDSO_REQUIRE(ctx, frame_slots && raw && exposure, "null argument");
  for (int i = 0; i < n_images; i++) SDSO_REQUIRE(ctx, raw[i], "null image");
  SDSO_REQUIRE(ctx, n_images == 1 || frame_slots[0] != frame_slots[1], "a frame slot is named twice");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  IngestState& S = *ctx->ingest;
  const IngestCalib& c = S.calibs[calib];
  const size_t img_bytes = ((size_t)c.wOrg * c.hOrg * c.pixel_bytes + 15) & ~(size_t)15, bytes = img_bytes * n_images;
  // the slots first: the calibration's shape was accepted when it was created, so only an allocation can fail from here on
  PyramidDev* P[2] = {nullptr, nullptr};
  for (int i = 0; i < n_images; i++) {
    int rc = pyramid_prepare(ctx, frame_slots[i], c.w, c.h, &P[i]);
    if (rc) return rc;
  }
  // staging: the next pinned buffer, once the copy enqueued from it two calls ago is through; sized for two images whatever n_images is
  char* pin = nullptr;
  { int rc = stage_reserve(ctx, S.stage, 2 * img_bytes, &pin); if (rc) return rc; }
  SDSO_HIP(ctx, S.raw.reserve(ctx->stream, bytes, 2 * img_bytes));
  IngestImages A;
  for (int i = 0; i < 2; i++) A.img[i] = IngestImage{nullptr, nullptr, PHOTO_LINEAR};
  for (int i = 0; i < n_images; i++) {
    std::memcpy(pin + i * img_bytes, raw[i], (size_t)c.wOrg * c.hOrg * c.pixel_bytes);
    const bool linear = !c.G || exposure[i] <= 0 || c.mode == 0;   // :231 (a NaN exposure is not <= 0 there either)
    A.img[i] = IngestImage{S.raw + i * img_bytes, P[i]->d[0], linear ? PHOTO_LINEAR : c.mode == 2 ? PHOTO_G_VIGNETTE : PHOTO_G};
    if (exposure_out) exposure_out[i] = c.use_exposure ? exposure[i] : 1.f;   // :253-259
  }
  SDSO_HIP(ctx, hipMemcpyAsync(S.raw, pin, bytes, hipMemcpyHostToDevice, ctx->stream));
  { int rc = stage_commit(ctx, S.stage); if (rc) return rc; }
  if (c.pixel_bytes == 1) launch_level0<uint8_t>(ctx, c, A, n_images, factor);
  else launch_level0<uint16_t>(ctx, c, A, n_images, factor);
  SDSO_HIP(ctx, hipGetLastError());
  for (int i = 0; i < n_images; i++) {
    int rc = pyramid_finish_levels(ctx, *P[i]);
    if (rc) return rc;
  }
  return SDSO_OK;
}
