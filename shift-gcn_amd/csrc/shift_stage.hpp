// The temporal shift's tap arithmetic and the zero-padded LDS plane of the stride-1 backward
// (launch_forms.hpp kPadRows / ra_pad_floats), shared by tshift.hip and by the BatchNorm
// backward apply that re-forms shift_in's input gradient while staging (bn.hip
// bn_bwd_apply_tsh_kernel). Every function here disables contraction itself, so a value
// formed through it has the same bits whichever file's kernel calls it.
#pragma once
#include "common.hpp"
#include "launch_forms.hpp"

namespace sgcn {

struct Geom {
  int x1, y1;
  float dx, dy;
};

// `int x1 = floorf(x); dx = x - x1;` (.cu:49-71)
__device__ __forceinline__ Geom make_geom(float x, float y) {
#pragma clang fp contract(off)
  Geom g;
  g.x1 = (int)floorf(x);
  g.y1 = (int)floorf(y);
  g.dx = x - (float)g.x1;
  g.dy = y - (float)g.y1;
  return g;
}

// q11*(1-dx)*(1-dy) + q21*dx*(1-dy) + q12*(1-dx)*dy + q22*dx*dy, left to right (.cu:73)
__device__ __forceinline__ float blend(float q11, float q21, float q12, float q22, float dx,
                                       float dy) {
#pragma clang fp contract(off)
  const float omdx = 1.f - dx, omdy = 1.f - dy;
  return q11 * omdx * omdy + q21 * dx * omdy + q12 * omdx * dy + q22 * dx * dy;
}

// zero the padding of a padded H x W plane (NT threads)
template <int NT>
__device__ __forceinline__ void zero_pad(float* lds, int H, int W) {
  const int WP = W + 2, nprow = 2 * kPadRows * WP;
  for (int i = (int)threadIdx.x; i < nprow + 2 * H; i += NT) {
    int a;
    if (i < nprow) {
      const int r = i / WP, col = i - r * WP;
      a = (r < kPadRows ? r : H + r) * WP + col;
    } else {
      const int j = i - nprow;
      a = ((j >> 1) + kPadRows) * WP + ((j & 1) ? W + 1 : 0);
    }
    lds[a] = 0.f;
  }
}

// whether the input-gradient taps of a shift with reverse geometry r = make_geom(-x, -y) stay
// inside the padding of the staged gout plane
__device__ __forceinline__ bool shift_in_grad_fits(const Geom& r) {
  return r.y1 >= -kPadRows && r.y1 <= kPadRows - 1 && r.x1 >= -1 && r.x1 <= 0;
}

// One element (h, w) of the stride-1 shift's input gradient from the padded LDS image of gout
// (.cu:108-150): the blend of gout at (h + r.y1 + {0,1}, w + r.x1 + {0,1}), a tap outside the
// plane = +0. FITS (shift_in_grad_fits): four unconditional reads at lt + r.y1*WP + r.x1, lt
// the element's own LDS position (the padding supplies the zeros); else range-checked taps.
// Both give the same bits.
template <bool FITS>
__device__ __forceinline__ float shift_in_grad(const float* lds, const Geom& r, int lt, int h,
                                               int w, int H, int W) {
  const int WP = W + 2;
  if (FITS) {
    const int la = lt + r.y1 * WP + r.x1;
    return blend(lds[la], lds[la + 1], lds[la + WP], lds[la + WP + 1], r.dx, r.dy);
  }
  auto tap = [&](int row, int col) {
    const bool in_ = (unsigned)row < (unsigned)H && (unsigned)col < (unsigned)W;
    const int rr = min(max(row, 0), H - 1), cc = min(max(col, 0), W - 1);
    const float v = lds[(rr + kPadRows) * WP + cc + 1];
    return in_ ? v : 0.f;
  };
  const int rq = h + r.y1, cq = w + r.x1;
  return blend(tap(rq, cq), tap(rq, cq + 1), tap(rq + 1, cq), tap(rq + 1, cq + 1), r.dx, r.dy);
}

}  // namespace sgcn
