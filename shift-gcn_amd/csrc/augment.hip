// The feeder's training augmentations (feeders/feeder.py:74-90, feeders/tools.py:32-117:
// normalization, random_shift, random_choose / auto_pading, random_move) for a whole batch in
// ONE streaming launch: the raw (B, C, T, V, M) batch is read once through a per-sample frame
// map and the augmented (B, C, T_out, V, M) batch is written once.
//
// The random draws stay on the host (shiftgcn/augment.py: ClipAugment.draw reproduces the
// reference's `random` / `np.random` streams, whose consumption depends on each sample's
// valid-frame extent); the kernel takes their result as three small per-sample tables:
//   frame_map {src0, dst0, count}: output frame t in [dst0, dst0 + count) is input frame
//     src0 + t - dst0, every other output frame is zero (random_shift composed with the crop
//     or pad of the window);
//   nodes {num_node, node[max_nodes]} and move {A, S, T_x, T_y}[max_nodes] (float64):
//     random_move's segment nodes and the values drawn at them.
//
// Arithmetic, in the reference's order and with its roundings (no contraction anywhere in
// this file's own expressions):
//   1. x = (in - mean[c][v]) / std[c][v], IEEE float32 subtract and divide: bit-exact;
//   2. zero outside the frame map (the zero is NOT normalised: the reference pads after it);
//   3. channels 0/1: per output frame, a, s, t_x, t_y interpolated as np.linspace does
//      (step = (stop - start) / (n - 1); i * step and + start rounded separately; the last
//      element of a segment is `stop`, n = 1 gives `start`), a = a * pi / 180,
//      [x'; y'] = [cos a*s, -sin a*s; sin a*s, cos a*s] [x; y] + [t_x; t_y] in float64,
//      rounded to float32 once. Frames outside every segment keep the reference's zero
//      coefficients (np.zeros(T)), i.e. x' = y' = 0.
// The per-frame coefficients (two float64 sin/cos) are formed once per frame by the first
// lanes of the workgroup that owns the frame tile, and read from LDS by every element.
//
// Launch: one workgroup of 256 threads per (sample, tile of 16 output frames); a thread walks
// the tile's 16*V*M contiguous elements with stride 256 and handles every channel of its
// element, so each load/store instruction of a wave covers 64 consecutive floats of one
// (sample, channel) run. HBM-bound: one read + one write of the batch.
#include "common.hpp"

namespace sgcn {
namespace {

constexpr int kAugThreads = 256;
constexpr int kAugFrames = 16;   // output frames per workgroup

// np.linspace(start, stop, n)[i]
__device__ __forceinline__ double aug_linspace(double start, double stop, int i, int n) {
#pragma clang fp contract(off)
  if (n <= 1) return start;
  if (i == n - 1) return stop;
  const double step = (stop - start) / (double)(n - 1);
  const double y = (double)i * step;
  return y + start;
}

__global__ __launch_bounds__(kAugThreads) void clip_augment_kernel(
    const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ frame_map,
    const int* __restrict__ nodes, const double* __restrict__ move,
    const float* __restrict__ mean, const float* __restrict__ stdv, int C, int T, int T_out,
    int V, int M, int max_nodes, int tiles, int flags) {
#pragma clang fp contract(off)
  __shared__ double coef[kAugFrames][4];   // {cos a*s, sin a*s, t_x, t_y} per frame
  const int b = (int)blockIdx.x / tiles;
  const int f0 = ((int)blockIdx.x - b * tiles) * kAugFrames;
  const int nf = min(kAugFrames, T_out - f0);
  const int VM = V * M;
  const bool norm = (flags & SGCN_AUG_NORMALIZE) != 0;
  const bool mv = (flags & SGCN_AUG_MOVE) != 0;
  const int src0 = frame_map[3 * b], dst0 = frame_map[3 * b + 1], count = frame_map[3 * b + 2];

  if (mv) {
    if ((int)threadIdx.x < nf) {
      const int t = f0 + (int)threadIdx.x;
      const int* nd = nodes + (size_t)b * (max_nodes + 1);
      const double* mp = move + (size_t)b * 4 * max_nodes;
      const int num_node = min(max(nd[0], 0), max_nodes);
      double a = 0.0, s = 0.0, tx = 0.0, ty = 0.0;
      for (int i = 0; i + 1 < num_node; ++i) {
        const int lo = nd[1 + i], hi = nd[2 + i];
        if (t >= lo && t < hi) {
          const int k = t - lo, n = hi - lo;
          a = aug_linspace(mp[i], mp[i + 1], k, n) * 3.141592653589793 / 180.0;
          s = aug_linspace(mp[max_nodes + i], mp[max_nodes + i + 1], k, n);
          tx = aug_linspace(mp[2 * max_nodes + i], mp[2 * max_nodes + i + 1], k, n);
          ty = aug_linspace(mp[3 * max_nodes + i], mp[3 * max_nodes + i + 1], k, n);
        }
      }
      coef[threadIdx.x][0] = cos(a) * s;
      coef[threadIdx.x][1] = sin(a) * s;
      coef[threadIdx.x][2] = tx;
      coef[threadIdx.x][3] = ty;
    }
    __syncthreads();
  }

  const size_t in_plane = (size_t)T * VM, out_plane = (size_t)T_out * VM;
  const float* inb = in + (size_t)b * C * in_plane;
  float* outb = out + (size_t)b * C * out_plane + (size_t)f0 * VM;
  const int n_elem = nf * VM;
  for (int e = (int)threadIdx.x; e < n_elem; e += kAugThreads) {
    const int fl = e / VM, r = e - fl * VM;
    // the host clips the map; a bad device table still never reads out of bounds
    const long long rel = (long long)(f0 + fl) - dst0, sf = src0 + rel;
    const bool inside = rel >= 0 && rel < count && sf >= 0 && sf < T;
    const size_t ioff = (size_t)(inside ? sf : 0) * VM + r;
    const int v = r / M;
    int c = 0;
    if (mv) {
      float x = 0.f, y = 0.f;
      if (inside) {
        x = inb[ioff];
        y = inb[in_plane + ioff];
        if (norm) {
          x = (x - mean[v]) / stdv[v];
          y = (y - mean[V + v]) / stdv[V + v];
        }
      }
      const double m0 = coef[fl][0], m1 = coef[fl][1];
      const double xd = (double)x, yd = (double)y;
      const double nx = (m0 * xd + (-m1) * yd) + coef[fl][2];
      const double ny = (m1 * xd + m0 * yd) + coef[fl][3];
      outb[e] = (float)nx;
      outb[out_plane + e] = (float)ny;
      c = 2;
    }
    for (; c < C; ++c) {
      float x = 0.f;
      if (inside) {
        x = inb[(size_t)c * in_plane + ioff];
        if (norm) x = (x - mean[c * V + v]) / stdv[c * V + v];
      }
      outb[(size_t)c * out_plane + e] = x;
    }
  }
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" {

int sgcn_clip_augment(const float* in, float* out, const int* frame_map, const int* nodes,
                      const double* move, const float* mean, const float* std, int B, int C,
                      int T, int T_out, int V, int M, int max_nodes, int flags, void* stream) {
  SGCN_REQUIRE(in && out && frame_map && in != out);
  SGCN_REQUIRE(B >= 1 && C >= 1 && T >= 1 && T_out >= 1 && V >= 1 && M >= 1);
  SGCN_REQUIRE((flags & ~(SGCN_AUG_NORMALIZE | SGCN_AUG_MOVE)) == 0);
  if (flags & SGCN_AUG_NORMALIZE) SGCN_REQUIRE(mean && std);
  if (flags & SGCN_AUG_MOVE)
    SGCN_REQUIRE(nodes && move && C >= 2 && max_nodes >= 2 && max_nodes <= SGCN_AUG_MAX_NODES);
  // a tile's element index and a plane's mean/std index stay in int
  SGCN_REQUIRE((long long)V * M <= (1 << 26) && (long long)C * V <= 0x7fffffffLL);
  const long long tiles = ((long long)T_out + kAugFrames - 1) / kAugFrames;
  SGCN_REQUIRE(tiles * B <= 0x7fffffffLL);
  clip_augment_kernel<<<(unsigned)(tiles * B), kAugThreads, 0, (hipStream_t)stream>>>(
      in, out, frame_map, nodes, move, mean, std, C, T, T_out, V, M, max_nodes, (int)tiles,
      flags);
  SGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
