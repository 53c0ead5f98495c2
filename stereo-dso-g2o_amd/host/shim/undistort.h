#pragma once
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
// class Undistort (util/Undistort.h:63-104) with the members DatasetReader and main touch: getK, getSize, getOriginalSize, getBl,
// isValid, loadPhotometricCalibration and undistort<T>.  undistort<T> does not return an ImageAndExposure: the undistorted image never
// exists on the host.  It ingests the raw image into a device pyramid slot (Undistort.cpp:398-489 + FrameHessian::makeImages) and
// returns ImageAndExposure::exposure_time; the call only enqueues (sdso_ingest_frame).  Reading the calibration, response and vignette
// files stays with the caller (readFromFile's sscanfs, ImageRW): the class is constructed either from the parsed model parameters or
// from caller-owned remap arrays (the reference's own Undistort::remapX / remapY), and loadPhotometricCalibration takes the tables.
// Mat33T / Vec2iT are the reference's Eigen types (element access (i, j) / [i]).  calib_id names the tables on the device.
template <class Mat33T, class Vec2iT> class Undistort {
 public:
  // from model parameters: model = SDSO_CAM_*, parsOrg = the 5 or 8 numbers of the first line of the calibration file, out_mode =
  // SDSO_RECTIFY_* (line 3), out_calib = the first four numbers of that line (relative fx fy cx cy; its fifth is unused) when it holds an explicit K, else unused,
  // bl = the baseline (line 5)
  Undistort(Device& dev, int calib_id, int model, const double* parsOrg, int wOrg_, int hOrg_, int w_, int h_, int out_mode, const float* out_calib, float bl_)
      : dev_(dev), calib_(calib_id), wOrg(wOrg_), hOrg(hOrg_), w(w_), h(h_), bl(bl_), remapX_((size_t)w_ * h_), remapY_((size_t)w_ * h_) {
    double k[4];
    int pt = 0;
    if (sdso_undistort_make_remap(model, parsOrg, wOrg, hOrg, w, h, out_mode, out_calib, k, remapX_.data(), remapY_.data(), &pt) != SDSO_OK)
      throw Error("Undistort: the reference exits here (rectification mode, sizes, or makeOptimalK_crop does not converge)");
    passthrough = pt != 0;
    setK_(k);
    valid = true;
  }
  // from caller-owned tables (copied): K = fx fy cx cy of the rectified camera; remapX == nullptr: passthrough
  Undistort(Device& dev, int calib_id, const double K4[4], int wOrg_, int hOrg_, int w_, int h_, const float* remapX, const float* remapY, float bl_)
      : dev_(dev), calib_(calib_id), wOrg(wOrg_), hOrg(hOrg_), w(w_), h(h_), bl(bl_) {
    passthrough = remapX == nullptr;
    if (remapX) { remapX_.assign(remapX, remapX + (size_t)w * h); remapY_.assign(remapY, remapY + (size_t)w * h); }
    setK_(K4);
    valid = true;
  }
  ~Undistort() { if (loaded_) sdso_ingest_calib_release(dev_.ctx(), calib_); }
  Undistort(const Undistort&) = delete;
  Undistort& operator=(const Undistort&) = delete;

  const Mat33T getK() const { return K; }
  const Vec2iT getSize() const { Vec2iT v; v[0] = w; v[1] = h; return v; }
  const Vec2iT getOriginalSize() const { Vec2iT v; v[0] = wOrg; v[1] = hOrg; return v; }
  bool isValid() const { return valid; }
  float getBl() const { return bl; }
  const float* remapX() const { return passthrough ? nullptr : remapX_.data(); }
  const float* remapY() const { return passthrough ? nullptr : remapY_.data(); }

  // loadPhotometricCalibration with the tables instead of the file names: G = PhotometricUndistorter::getG() (256 floats for 8-bit
  // images, 65536 for 16-bit ones; nullptr = no valid calibration), vignetteMapInv = wOrg*hOrg floats or nullptr; the two settings are
  // setting_photometricCalibration and setting_useExposure.  Uploads the tables; they stay on the device until the object goes.
  void loadPhotometricCalibration(int pixel_bytes, const float* G, const float* vignetteMapInv, int setting_photometricCalibration, bool setting_useExposure) {
    dev_.check(sdso_ingest_calib_create(dev_.ctx(), calib_, wOrg, hOrg, w, h, remapX(), remapY(), pixel_bytes, G, vignetteMapInv,
                                        setting_photometricCalibration, setting_useExposure ? 1 : 0), "sdso_ingest_calib_create");
    loaded_ = true;
    pixel_bytes_ = pixel_bytes;
  }

  // undistort<T>(image_raw, exposure, timestamp, factor) into pyramid slot `slot`; MinimalImageT carries data / w / h.  Returns exposure_time.
  template <class MinimalImageT>
  float undistort(const MinimalImageT* image_raw, int slot, float exposure = 0, double /*timestamp*/ = 0, float factor = 1) const {
    check_(image_raw);
    const void* raw[1] = {image_raw->data};
    float out = 0;
    dev_.check(sdso_ingest_frame(dev_.ctx(), calib_, 1, &slot, raw, &exposure, factor, &out), "sdso_ingest_frame");
    return out;
  }
  // the two images of a stereo frame in one call (DatasetReader::getImage for the left and the right reader): one level-0 launch
  template <class MinimalImageT>
  void undistortStereo(const MinimalImageT* left, const MinimalImageT* right, int slot_left, int slot_right, const float exposure[2], float factor, float exposure_out[2]) const {
    check_(left); check_(right);
    const void* raw[2] = {left->data, right->data};
    const int slots[2] = {slot_left, slot_right};
    dev_.check(sdso_ingest_frame(dev_.ctx(), calib_, 2, slots, raw, exposure, factor, exposure_out), "sdso_ingest_frame");
  }

 private:
  template <class MinimalImageT> void check_(const MinimalImageT* im) const {
    if (!loaded_) throw Error("Undistort::undistort: loadPhotometricCalibration has not been called");
    if (!im || im->w != wOrg || im->h != hOrg) throw Error("Undistort::undistort: wrong image size");
    if ((int)sizeof(*im->data) != pixel_bytes_) throw Error("Undistort::undistort: pixel type differs from the calibration's");
  }
  void setK_(const double k[4]) { detail::pinholeK(K, k[0], k[1], k[2], k[3]); }
  Device& dev_;
  int calib_;
  int wOrg, hOrg, w, h;
  float bl;
  Mat33T K;
  bool valid = false, passthrough = false, loaded_ = false;
  int pixel_bytes_ = 1;
  std::vector<float> remapX_, remapY_;
};
}  // namespace sdso_shim
