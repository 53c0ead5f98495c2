// The ctx-free rules of the device-resident immature points (imm_*.hip), in plain C++ so that test_imm_layout.cpp checks them with the
// host compiler alone: the members of a point in a host's blob, the order STEP 5 of activatePointsMT (FullSystem.cpp:948-957) leaves
// the survivors in, and that order in closed form, as the kernels of sdso_imm_activate compute it.
#pragma once
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__)
#define IMM_HD __host__ __device__
#else
#define IMM_HD
#endif

namespace sdso {

// ---- the members.  A host's blob is kImmFloats * cap floats, structure of arrays with stride cap: member M starts at IMM_M * cap and
// holds `width` floats per point, point-major (color, weights, gradH and lastTraceUV keep the inner layout of TraceDev, so a blob binds
// to a TraceDev without a copy).  The status byte lives in its own array of cap bytes.
constexpr int kImmFloats = 30;
enum { IMM_U = 0, IMM_V = 1, IMM_TYPE = 2, IMM_IMIN = 3, IMM_IMAX = 4, IMM_QUAL = 5, IMM_COLOR = 6, IMM_WEIGHTS = 14, IMM_GRADH = 22, IMM_ETH = 26,
       IMM_UV = 27, IMM_INTERVAL = 29 };   // offsets in units of cap floats
struct ImmMember { int off, width; };
constexpr int kImmMembers = 12;
IMM_HD constexpr ImmMember imm_member(int m) {   // in blob order; whoever walks the members walks this
  constexpr ImmMember t[kImmMembers] = {{IMM_U, 1},     {IMM_V, 1},       {IMM_TYPE, 1},  {IMM_IMIN, 1}, {IMM_IMAX, 1}, {IMM_QUAL, 1},
                                        {IMM_COLOR, 8}, {IMM_WEIGHTS, 8}, {IMM_GRADH, 4}, {IMM_ETH, 1},  {IMM_UV, 2},   {IMM_INTERVAL, 1}};
  return t[m];
}
constexpr int imm_members_end() {   // the first float past the last member, or -1 where a member does not start at its predecessor's end
  int o = 0;
  for (int m = 0; m < kImmMembers; m++) {
    if (imm_member(m).off != o || imm_member(m).width < 1) return -1;
    o += imm_member(m).width;
  }
  return o;
}
static_assert(imm_members_end() == kImmFloats, "the members fill the blob's kImmFloats columns in order, without a gap");
// The member that holds float c of a point, 0 <= c < kImmFloats (its inner index is c - off), as the gather kernels derive it: a ladder
// written out, which the compiler turns into less code than a walk of imm_member() (the single-float members up to quality answer with
// c itself).  test_imm_layout.cpp holds it against the table for every c.
IMM_HD inline ImmMember imm_member_of_float(int c) {
  if (c < IMM_COLOR) return {c, 1};
  if (c < IMM_WEIGHTS) return {IMM_COLOR, 8};
  if (c < IMM_GRADH) return {IMM_WEIGHTS, 8};
  if (c < IMM_ETH) return {IMM_GRADH, 4};
  if (c < IMM_UV) return {IMM_ETH, 1};
  if (c < IMM_INTERVAL) return {IMM_UV, 2};
  return {IMM_INTERVAL, 1};
}

// ---- one entry of toOptimize as sdso_imm_activate leaves it on the device and sdso_imm_activate_fetch hands it out.  The integer members
// (frame, index, status, lastTraceStatus, res_state) are what the host reads of it; sdso_ba_window_update_activated (ba_update.hip) reads
// the float members where they lie.
struct ImmActRec {
  int frame, index;
  int8_t status; uint8_t lastTraceStatus; uint8_t pad[2];
  float idepth;
  uint8_t res_state[8];
  float u, v, my_type, idepth_min, idepth_max, energyTH;
  float color[8], weights[8];
};
static_assert(sizeof(ImmActRec) == 112, "records are copied as 16-byte aligned blocks");
static_assert(offsetof(ImmActRec, idepth) == 12 && offsetof(ImmActRec, u) == 24 && offsetof(ImmActRec, v) == 28, "k_ba_window_fill_activated reads these as floats 3, 6, 7");
static_assert(offsetof(ImmActRec, color) == 48 && offsetof(ImmActRec, weights) == 80, "colour and weights are read as two float4 each");

// ---- STEP 5: `if (!ph) { immaturePoints[i] = back(); pop_back(); i--; }`.  src[0 .. size) = the old index of every entry of the new
// vector; a flagged entry stands for the reference's null pointer.  Returns size.
inline int imm_remove_order(int n, const uint8_t* flags, int* src) {
  for (int i = 0; i < n; i++) src[i] = i;
  int size = n;
  for (int i = 0; i < size; i++)
    if (flags[src[i]]) { src[i] = src[size - 1]; size--; i--; }
  return size;
}
// The same loop in closed form.  With m = n - nflag survivors of n entries: survivors at indices < m stay; the flagged indices < m,
// ascending, receive the survivors at indices >= m, descending (every `= back(); pop_back()` hands the last live entry to the first hole;
// flagged entries at the back are popped on the way).  pref_i = the number of flagged entries before entry i.
// imm_back_slot: for the survivor at index i >= m, its place k from the back among those survivors (the survivors behind entry i).
IMM_HD inline int imm_back_slot(int n, int nflag, int i, int pref_i) { return (n - 1 - i) - (nflag - pref_i); }
// imm_final_src: the old index of the entry that ends at index i < m: itself, or for the k-th hole (k = pref_i) the k-th survivor from
// the back, back[k] = the i of imm_back_slot(..) == k.
IMM_HD inline int imm_final_src(int i, bool flagged, int pref_i, const int* back) { return flagged ? back[pref_i] : i; }

}  // namespace sdso
