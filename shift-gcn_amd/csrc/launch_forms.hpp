// Which kernel instantiation a (T, V) / (H, W) plane runs: the thresholds, the choosers and,
// per launcher, the (threads, elements per thread) forms it instantiates. Host-only and
// HIP-free: the entry points of bn.hip and tshift.hip call these, tests/launch_forms_dump.cpp
// prints them, and tests/test_launch_forms.py compares that print with the Python mirrors
// (oracle/stream_cases.py, oracle/tshift_cases.py, shiftgcn.ops.ra_fits) plane by plane.
#pragma once
#include <algorithm>
#include <cstddef>
#include <tuple>

namespace sgcn {

constexpr int kThreads = 256;      // the looping / global-tap kernels; widest plane row (V)
constexpr int kBwdThreads = 512;   // the stride-2 LDS backward; the wide stride-1 backward

// largest plane the plane-resident BatchNorm kernels run on 256 threads (512 above): at NTU
// T = 300 (7,500 floats) 256 x 30 measured 0.8 % faster per step than 512 x 15 (same box,
// profiles/r03_bnja/ab_moments_reduce_t256.txt)
constexpr int kJaSplit = 8192;

constexpr int kFwdLdsMax = 8192;    // floats of the staged input plane (32 KiB), 256 threads
constexpr int kFwdLdsMax2 = 16384;  // ... with 512 threads (e.g. MediaPipe T=300: 9,900)
constexpr int kBwdLdsMax = 16384;   // floats of the staged gout + input planes (64 KiB)

// Zero-padded LDS planes (the stride-1 backward and the padded forward kernels): an H x W
// plane is staged with row pitch WP = W + 2 (a zero column each side) between kPadRows
// zero rows above and below, element (h, w) at [(h + kPadRows) * WP + w + 1]; a tap of a
// shift with floor(x) in {-1, 0} and |floor(y)| < kPadRows then needs no range check.
constexpr int kPadRows = 4;
constexpr int ra_pad_floats(int H, int W) { return (H + 2 * kPadRows) * (W + 2); }

// largest stride-1 plane the joint-aligned backward kernels with affine taps (shift_in:
// plain and GBN) run on 256-thread workgroups (up to 32 elements per thread): at NTU T=300
// (7,500 floats) measured 8 % (GBN) / 4 % (plain) faster than 512 threads
constexpr int kRaSplit256 = 8192;
// the shift_out backward (bnin) keeps 512 threads above 4K-float planes: 256 threads at NTU
// T = 300 measured 0.3 % slower per step (profiles/r03_x1b/ab_x1b_bound.txt, variant bnin256)
constexpr int kBninSplit = 4096;
#ifndef SGCN_GBD_SPLIT
#define SGCN_GBD_SPLIT 1
#endif
constexpr size_t kRaLdsMax = 65536;

// elements per thread of the plane-resident joint-aligned kernels on nt threads; 0 = the
// plane does not fit (V > 64 or more than 32 per thread): the looping kernels take it
inline int ja_lpt(int T, int V, int nt) {
  if (V > 64) return 0;
  const int ntj = (nt / V) * V, per = (T * V + ntj - 1) / ntj;
  return per <= 8 ? 8 : (per <= 16 ? 16 : (per <= 24 ? 24 : (per <= 32 ? 32 : 0)));
}

// LDS bytes of the padded stride-1 backward (GBN reuses it for 6*NT partial sums)
inline size_t ra_lds_bytes(int H, int W, int nt, bool gbn) {
  const int f = ra_pad_floats(H, W);
  return (size_t)(gbn ? std::max(f + 1, 6 * nt) : f + 1) * sizeof(float);   // + the spare float
}

// elements per thread of the padded joint-aligned forward kernels (W <= 64) on NT threads;
// 0 when the plane needs more than 32 per thread or more than 64 KiB of LDS
inline int pad_fwd_lpt(int H, int W, int nt) {
  if (W > 64) return 0;
  const int ntj = (nt / W) * W, per = (H * W + ntj - 1) / ntj;
  // 512 threads also at 12 / 20 (as ra_lpt): MediaPipe's 9,900-float planes are 20 per
  // thread, and the eval pre / tail forms held 88-95 VGPRs at 24 (two workgroups per CU)
  int lpt = per <= 8 ? 8 : (per <= 16 ? 16 : (per <= 24 ? 24 : (per <= 32 ? 32 : 0)));
  if (nt == 512 && per > 8 && per <= 12) lpt = 12;
  if (nt == 512 && per > 16 && per <= 20) lpt = 20;
  return (size_t)(ra_pad_floats(H, W) + 1) * sizeof(float) > 65536 ? 0 : lpt;
}

// elements per thread of the joint-aligned stride-1 LDS backward kernels (stride
// (nt / W) * W); 0 = the plane does not fit 32 per thread. 512-thread workgroups also take
// 12 and 20: a thread holds ~5 VGPRs per element, and at 24 the shift_out backward (bnin)
// and the GBD backward held 141-143 VGPRs — one 512-thread workgroup per CU on MediaPipe's
// 9,900-float planes (W = 33, exactly 20 per thread); at 20 two fit (likewise 12 against 16
// for its 4,950-float T = 150 planes: three instead of two)
inline int ra_lpt(int n, int nt, int W) {
  const int nte = (nt / W) * W;
  if (nte <= 0 || W > 64) return 0;
  const int per = (n + nte - 1) / nte;
  if (nt == 512 && per > 8 && per <= 12) return 12;
  if (nt == 512 && per > 16 && per <= 20) return 20;
  return per <= 8 ? 8 : (per <= 16 ? 16 : (per <= 24 ? 24 : (per <= 32 ? 32 : 0)));
}

inline int pick_lpt(int n, int nt) {
  const int per = (n + nt - 1) / nt;
  return per <= 8 ? 8 : (per <= 16 ? 16 : 32);
}

inline int pick_ept(int n) {
  const int per = (n + kThreads - 1) / kThreads;
  return per <= 8 ? 8 : (per <= 16 ? 16 : 32);
}

// ------------------------------------------------------------------------------------
// the whole launch form of one entry point (named after the Python mirrors)
// ------------------------------------------------------------------------------------
enum class Kind {
  refuse,   // SGCN_EINVAL
  empty,    // nothing to launch
  ja,       // plane-resident joint-aligned BatchNorm kernels
  loop,     // looping BatchNorm kernels (kThreads)
  pad,      // tshift_fwd_pad_kernel
  lds,      // tshift_fwd_lds_kernel / tshift_fwd_pre_kernel / tshift_fwd_tail_kernel
  global,   // tshift_fwd_kernel / tshift_bwd_kernel: lpt per thread on kThreads
  ra,       // tshift_bwd_ra_kernel
  s2,       // tshift_bwd_s2_kernel: lpt per thread on kBwdThreads
};
struct LaunchForm {
  Kind kind;
  int nt, lpt;
  bool flag;   // global: more than one pass; s2: joint-aligned walk; gbn: with the down sums
};

// sgcn_moments / sgcn_bn_apply / sgcn_bn_bwd_reduce / sgcn_bn_bwd_apply / sgcn_gcn_dx_finish
inline LaunchForm bn_form(int T, int V) {
  if (V > kThreads) return {Kind::refuse, 0, 0, false};
  const int nt = T * V <= kJaSplit ? kThreads : 512;
  const int lpt = ja_lpt(T, V, nt);
  if (lpt) return {Kind::ja, nt, lpt, false};
  return {Kind::loop, kThreads, 0, false};
}

// the LDS-staged forward of a plane of at most kFwdLdsMax2 floats: padded joint-aligned
// (W <= 64) on 256 threads up to kFwdLdsMax floats, else 512; else the plain staged plane
inline LaunchForm staged_fwd_form(int H, int W) {
  const int n = H * W, nt = n <= kFwdLdsMax ? kThreads : 512;
  const int lpt = pad_fwd_lpt(H, W, nt);
  if (lpt) return {Kind::pad, nt, lpt, false};
  return {Kind::lds, nt, n <= kFwdLdsMax ? pick_lpt(n, kThreads) : 32, false};
}

// sgcn_tshift_fwd
inline LaunchForm tshift_fwd_form(int H, int W, int stride) {
  const int Ho = H / stride;
  if (Ho == 0) return {Kind::empty, 0, 0, false};
  if (H * W <= kFwdLdsMax2) return staged_fwd_form(H, W);
  const int ept = pick_ept(Ho * W);
  return {Kind::global, kThreads, ept, Ho * W > ept * kThreads};
}

// sgcn_tshift_fwd_pre / sgcn_tshift_fwd_tail: LDS-staged planes only (the caller falls back)
inline LaunchForm fwd_fused_form(int H, int W) {
  if (H * W > kFwdLdsMax2 || W > 1024) return {Kind::refuse, 0, 0, false};
  return staged_fwd_form(H, W);
}

// sgcn_tshift_bwd (stride 1 or 2). Stride 1: the padded joint-aligned LDS kernel (W <= 64,
// <= 32 elements per thread, <= 64 KiB of LDS), on 256 threads only where 32 elements per
// thread cover the plane, so fewer lanes idle per workgroup on small planes (T = 150 / 75);
// anything else takes the global-tap kernel
inline LaunchForm bwd_form(int H, int W, int stride) {
  const int n = H * W, Ho = H / stride;
  if (stride == 1 && H > 0) {
    const int nt = n <= kRaSplit256 && ra_lpt(n, 256, W) ? 256 : kBwdThreads;
    const int lpt = ra_lpt(n, nt, W);
    if (lpt && ra_lds_bytes(H, W, nt, false) <= kRaLdsMax) return {Kind::ra, nt, lpt, false};
  }
  if (stride == 2 && H > 0 && (H + Ho) * W <= kBwdLdsMax)
    return {Kind::s2, kBwdThreads, pick_lpt((H + Ho) * W, kBwdThreads), W <= 64};
  const int ept = pick_ept(n);
  return {Kind::global, kThreads, ept, n > ept * kThreads};
}

// sgcn_tshift_bwd_gbn: sgcn_tshift_bwd's stride-1 thread counts. With the down BatchNorm's
// sums (GBD) a 32-element thread holds 183 VGPRs (two 256-thread workgroups per CU): such
// planes take 512 threads x 16 (107 VGPRs, two 512-thread workgroups) (SGCN_GBD_SPLIT=0: 256
// threads as GBN)
inline LaunchForm gbn_form(int H, int W, bool down) {
  const int n = H * W;
  if (W > 64 || n > kBwdLdsMax) return {Kind::refuse, 0, 0, down};
  const int l256 = n <= kRaSplit256 ? ra_lpt(n, 256, W) : 0;
  const int nt = l256 && !(SGCN_GBD_SPLIT && down && l256 > 24) ? 256 : kBwdThreads;
  const int lpt = ra_lpt(n, nt, W);
  if (lpt == 0 || ra_lds_bytes(H, W, nt, true) > kRaLdsMax) return {Kind::refuse, 0, 0, down};
  return {Kind::ra, nt, lpt, down};
}

// sgcn_tshift_bwd_bnin: W <= 64, <= 32 elements per thread, padded plane <= 64 KiB
// (shiftgcn.ops.ra_fits restates the refusals)
inline LaunchForm bnin_form(int H, int W) {
  const int n = H * W;
  if (n > kBwdLdsMax) return {Kind::refuse, 0, 0, false};
  const int nt = n <= kBninSplit ? 256 : 512;
  const int lpt = ra_lpt(n, nt, W);
  if (lpt == 0 || ra_lds_bytes(H, W, nt, false) > kRaLdsMax) return {Kind::refuse, 0, 0, false};
  return {Kind::ra, nt, lpt, false};
}

// ------------------------------------------------------------------------------------
// per launcher: the (nt, lpt) forms its chooser can return, which are the ones instantiated
// ------------------------------------------------------------------------------------
struct Form {
  int nt, lpt;
  constexpr auto fields() const { return std::make_tuple(nt, lpt); }
};
// bn_form's ja: 512 threads only above kJaSplit floats, at least 17 per lane
constexpr Form kJaForms[] = {{256, 8}, {256, 16}, {256, 24}, {256, 32}, {512, 24}, {512, 32}};
// staged_fwd_form's pad (sgcn_tshift_fwd, _pre, _tail): 512 threads above kFwdLdsMax floats
constexpr Form kPadFwdForms[] = {{256, 8},  {256, 16}, {256, 24}, {256, 32},
                                 {512, 20}, {512, 24}, {512, 32}};
// staged_fwd_form's lds
constexpr Form kLdsFwdForms[] = {{256, 8}, {256, 16}, {256, 32}, {512, 32}};
// bwd_form's ra, and gbn_form's without down (the same thread rule): 512 threads only
// where 256 x 32 do not cover the plane
constexpr Form kRaForms[] = {{256, 8},  {256, 16}, {256, 24}, {256, 32},
                             {512, 16}, {512, 20}, {512, 24}, {512, 32}};
// gbn_form's with down: 512 threads from 25 per lane on 256
constexpr Form kGbdForms[] = {{256, 8},  {256, 16}, {256, 24}, {512, 12},
                              {512, 16}, {512, 20}, {512, 24}, {512, 32}};
// bnin_form's: 512 threads above kBninSplit floats (at least 9 per lane); on 256 the
// narrowest joint-aligned stride of any W <= 64 is 208 lanes (W = 52): at most 20 per lane
constexpr Form kBninForms[] = {{256, 8},  {256, 16}, {256, 24}, {512, 12},
                               {512, 16}, {512, 20}, {512, 24}, {512, 32}};

}  // namespace sgcn
