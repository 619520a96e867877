// Sequence front and back end of the inference product: every sliding window of a
// landmark sequence cut, zero-padded and pre-normalised in one launch, and the window
// scores averaged back onto the frames in another.
//
// Reference: inference_pipeline.py:252-281 (create_sliding_windows), :167-245
// (pre_normalize = data_gen/preprocess.py:8-91 with the MediaPipe joints; rotation
// helpers :143-164 = data_gen/rotation.py) and :377-386 (aggregate_per_frame). The
// reference pads and normalises on the host with Python loops over window x person x frame;
// the closed form of those loops is in include/shiftgcn.h.
//
// One workgroup of 256 per window. A sequence is small (18,000 MediaPipe frames are 7 MB:
// L2 / Infinity Cache resident, and windows overlap), so the launch is about latency and
// about staying on the device, not about HBM:
//   A  null flag of every (frame, person) of the window into LDS (coalesced pass over the
//      window's real frames);
//   B  per person, a block scan of the flags (wave ballots + per-wave totals) compacts the
//      non-null frames; from it the source-frame map src[t][m] (W*M shorts in LDS);
//   C  the centre of every frame into LDS; lane 0 builds the two float64 rotation matrices;
//   D  every thread takes (t, v, m) points, three channels each: loads and stores are
//      coalesced over (v, m) per channel.
// Steps 1-4 of the closed form are exact (tested bit for bit): no contraction, no
// reassociation in this file.
#include "common.hpp"

#pragma clang fp contract(off)

namespace sgcn {
namespace {

constexpr int kSeqThreads = 256;
constexpr int kSeqWaves = kSeqThreads / kWave;
constexpr int kSeqMaxWM = SGCN_SEQ_MAX_WM;

struct SeqJoints {
  int z_bottom, z_top, x_right, x_left, center_a, center_b;
};

// the reference's joint mask `person.sum(-1) != 0`: (x + y) + z in float32
__device__ __forceinline__ bool joint_present(float x, float y, float z) {
  return (x + y) + z != 0.f;
}

// p <- mat * p in float64, rounded to float32, when the joint is present
// (np.dot(person[mask], matrix.T), preprocess.py:71-72)
__device__ __forceinline__ void rotate_present(const double* mat, float& x, float& y, float& z) {
  if (!joint_present(x, y, z)) return;
  const double dx = x, dy = y, dz = z;
  x = (float)((mat[0] * dx + mat[1] * dy) + mat[2] * dz);
  y = (float)((mat[3] * dx + mat[4] * dy) + mat[5] * dz);
  z = (float)((mat[6] * dx + mat[7] * dy) + mat[8] * dz);
}

// The matrix that turns v onto the unit axis e (2: z, 0: x) about v x e: angle_between
// (rotation.py:28-42: 0 when sum|v| < 1e-6; unit vector in float32, its norm the square root
// of a float32 dot product; arccos in float64) and
// rotation_matrix (rotation.py:5-20: identity when sum|axis| < 1e-6 or |theta| < 1e-6).
__device__ void align_matrix(float vx, float vy, float vz, int e, double* mat) {
  double theta = 0.0;
  const float l1 = (fabsf(vx) + fabsf(vy)) + fabsf(vz);
  if (!((double)l1 < 1e-6)) {
    // |v| as the reference's float32 dot product gives it: the three float32 squares
    // summed exactly (in float64) and rounded once, not once per addition
    const float norm =
        sqrtf((float)(((double)(vx * vx) + (double)(vy * vy)) + (double)(vz * vz)));
    const float u = (e == 2 ? vz : vx) / norm;
    theta = acos(fmin(fmax((double)u, -1.0), 1.0));
  }
  // v x (0,0,1) = (vy, -vx, 0);  v x (1,0,0) = (0, vz, -vy)
  double ax = e == 2 ? (double)vy : 0.0;
  double ay = e == 2 ? -(double)vx : (double)vz;
  double az = e == 2 ? 0.0 : -(double)vy;
  if ((fabs(ax) + fabs(ay)) + fabs(az) < 1e-6 || fabs(theta) < 1e-6) {
    for (int i = 0; i < 9; ++i) mat[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  // unit quaternion (qw; qx, qy, qz) = (cos(theta/2); -sin(theta/2) * axis / |axis|), then
  // its rotation matrix, every entry written out (sums left to right)
  const double len = sqrt((ax * ax + ay * ay) + az * az);
  const double half = theta / 2.0, sh = sin(half);
  const double qw = cos(half);
  const double qx = -(ax / len) * sh, qy = -(ay / len) * sh, qz = -(az / len) * sh;
  mat[0] = qw * qw + qx * qx - qy * qy - qz * qz;
  mat[1] = 2 * (qx * qy + qw * qz);
  mat[2] = 2 * (qx * qz - qw * qy);
  mat[3] = 2 * (qx * qy - qw * qz);
  mat[4] = qw * qw + qy * qy - qx * qx - qz * qz;
  mat[5] = 2 * (qy * qz + qw * qx);
  mat[6] = 2 * (qx * qz + qw * qy);
  mat[7] = 2 * (qy * qz - qw * qx);
  mat[8] = qw * qw + qz * qz - qx * qx - qy * qy;
}

__global__ void __launch_bounds__(kSeqThreads)
window_normalize_kernel(const float* __restrict__ seq, const int* __restrict__ table,
                        float* __restrict__ out, int T, int V, int M, int W, SeqJoints j,
                        int stages) {
  __shared__ unsigned char s_nonnull[kSeqMaxWM];   // [t][m]: raw frame t of person m is not null
  __shared__ short s_src[kSeqMaxWM];               // [t][m]: raw frame the padded frame reads; -1 = 0
  __shared__ short s_comp[kSeqMaxWM];              // one person's non-null frames, in order
  __shared__ float s_centre[3 * kSeqMaxWM];        // [t][c]
  __shared__ double s_mat[18];                     // Z then X, row-major
  __shared__ int s_wtot[kSeqWaves];

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int VM = V * M, WM = W * M;
  // the table is the caller's; a row outside the sequence reads nothing
  const int start = min(max(table[2 * n], 0), T);
  const int nr = min(max(table[2 * n + 1], 0), min(W, T - start));
  const size_t plane = (size_t)T * VM;             // channel stride of seq
  const float* __restrict__ base = seq + (size_t)start * VM;

  // A: null flags
  for (int i = tid; i < WM; i += kSeqThreads) s_nonnull[i] = 0;
  __syncthreads();
  for (int i = tid; i < nr * VM; i += kSeqThreads) {
    const float x = base[i], y = base[plane + i], z = base[2 * plane + i];
    if (x != 0.f || y != 0.f || z != 0.f) s_nonnull[(i / VM) * M + i % M] = 1;
  }
  __syncthreads();

  // B: source-frame map
  if (!(stages & 1)) {
    for (int i = tid; i < WM; i += kSeqThreads) s_src[i] = (i / M) < nr ? (short)(i / M) : (short)-1;
    __syncthreads();
  } else {
    for (int m = 0; m < M; ++m) {
      int count = 0;
      for (int t0 = 0; t0 < W; t0 += kSeqThreads) {
        const int t = t0 + tid;
        const bool f = t < W && s_nonnull[t * M + m];
        const unsigned long long bal = __ballot(f);
        if (lane == 0) s_wtot[wid] = __popcll(bal);
        __syncthreads();
        int off = count, tot = 0;
        for (int w = 0; w < kSeqWaves; ++w) {
          if (w < wid) off += s_wtot[w];
          tot += s_wtot[w];
        }
        if (f) s_comp[off + __popcll(bal & ((1ull << lane) - 1ull))] = (short)t;
        count += tot;
        __syncthreads();
      }
      if (count == 0) {                            // an absent person stays zero
        for (int t = tid; t < W; t += kSeqThreads) s_src[t * M + m] = -1;
      } else {
        // a null first frame compacts the person (then no null frame is left before L)
        const bool compact = !s_nonnull[m];
        const int L = compact ? count : s_comp[count - 1] + 1;   // start of the trailing nulls
        for (int t = tid; t < W; t += kSeqThreads) {
          const int q = t < L ? t : (t - L) % L;
          s_src[t * M + m] = compact ? s_comp[q] : (s_nonnull[q * M + m] ? (short)q : (short)-1);
        }
      }
      __syncthreads();
    }
  }

  // C: centre of every padded frame (person 0), then the two matrices
  if (stages & 2) {
    for (int t = tid; t < W; t += kSeqThreads) {
      const int s = s_src[t * M];
      float c[3] = {0.f, 0.f, 0.f};
      if (s >= 0) {
        const float* f = base + (size_t)s * VM;
        for (int k = 0; k < 3; ++k) {
          c[k] = f[k * plane + (size_t)j.center_a * M];
          if (j.center_b >= 0) c[k] = (c[k] + f[k * plane + (size_t)j.center_b * M]) / 2.f;
        }
      }
      s_centre[3 * t] = c[0];
      s_centre[3 * t + 1] = c[1];
      s_centre[3 * t + 2] = c[2];
    }
    __syncthreads();
  }
  // the padded (and centred) joint v of person m at frame t
  auto point = [&](int t, int r, int m, float& x, float& y, float& z) {
    const int s = s_src[t * M + m];
    x = y = z = 0.f;
    if (s >= 0) {
      const float* f = base + (size_t)s * VM + r;
      x = f[0];
      y = f[plane];
      z = f[2 * plane];
    }
    if (stages & 2) {
      const bool present = joint_present(x, y, z);
      x = present ? x - s_centre[3 * t] : 0.f;
      y = present ? y - s_centre[3 * t + 1] : 0.f;
      z = present ? z - s_centre[3 * t + 2] : 0.f;
    }
  };
  if (stages & 4) {
    if (tid == 0) {
      double mz[9], mx[9];
      float ax, ay, az, bx, by, bz;
      point(0, j.z_top * M, 0, ax, ay, az);
      point(0, j.z_bottom * M, 0, bx, by, bz);
      align_matrix(ax - bx, ay - by, az - bz, 2, mz);
      point(0, j.x_right * M, 0, ax, ay, az);
      point(0, j.x_left * M, 0, bx, by, bz);
      rotate_present(mz, ax, ay, az);
      rotate_present(mz, bx, by, bz);
      align_matrix(ax - bx, ay - by, az - bz, 0, mx);
      for (int i = 0; i < 9; ++i) {
        s_mat[i] = mz[i];
        s_mat[9 + i] = mx[i];
      }
    }
    __syncthreads();
  }

  // D: the points
  const size_t oplane = (size_t)W * VM;
  float* __restrict__ o = out + (size_t)n * 3 * oplane;
  for (int i = tid; i < W * VM; i += kSeqThreads) {
    const int t = i / VM, r = i - t * VM;
    float x, y, z;
    point(t, r, r % M, x, y, z);
    if (stages & 4) {
      rotate_present(s_mat, x, y, z);
      rotate_present(s_mat + 9, x, y, z);
    }
    o[i] = x;
    o[oplane + i] = y;
    o[2 * oplane + i] = z;
  }
}

__global__ void __launch_bounds__(kSeqThreads)
window_aggregate_kernel(const double* __restrict__ scores, const int* __restrict__ table,
                        double* __restrict__ per_frame, int n_windows, int total_frames) {
  const int f = blockIdx.x * kSeqThreads + threadIdx.x;
  if (f >= total_frames) return;
  double sum = 0.0, count = 0.0;
  for (int i = 0; i < n_windows; ++i) {
    const long long start = table[2 * i], nr = table[2 * i + 1];
    if (f >= start && f < start + nr) {
      sum += scores[i];
      count += 1.0;
    }
  }
  per_frame[f] = sum / fmax(count, 1.0);
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_window_normalize(const float* seq, const int* table, float* out,
                                     int n_windows, int T, int V, int M, int W, int z_bottom,
                                     int z_top, int x_right, int x_left, int center_a,
                                     int center_b, int stages, void* stream) {
  SGCN_REQUIRE(n_windows >= 0 && T > 0 && V > 0 && M > 0 && W > 0);
  SGCN_REQUIRE((long long)W * M <= kSeqMaxWM);   // (so t fits the short maps)
  SGCN_REQUIRE((long long)W * V * M < (1ll << 31));
  SGCN_REQUIRE((unsigned)z_bottom < (unsigned)V && (unsigned)z_top < (unsigned)V);
  SGCN_REQUIRE((unsigned)x_right < (unsigned)V && (unsigned)x_left < (unsigned)V);
  SGCN_REQUIRE((unsigned)center_a < (unsigned)V && center_b >= -1 && center_b < V);
  SGCN_REQUIRE(stages >= 0 && stages <= 7);
  if (n_windows == 0) return 0;
  SGCN_REQUIRE(seq && table && out);
  const SeqJoints j = {z_bottom, z_top, x_right, x_left, center_a, center_b};
  window_normalize_kernel<<<(unsigned)n_windows, kSeqThreads, 0, (hipStream_t)stream>>>(
      seq, table, out, T, V, M, W, j, stages);
  SGCN_LAUNCH_CHECK();
  return 0;
}

extern "C" int sgcn_window_aggregate(const double* scores, const int* table, double* per_frame,
                                     int n_windows, int total_frames, void* stream) {
  SGCN_REQUIRE(n_windows >= 0 && total_frames >= 0);
  if (total_frames == 0) return 0;
  SGCN_REQUIRE(per_frame && (n_windows == 0 || (scores && table)));
  const unsigned blocks = (unsigned)(((long long)total_frames + kSeqThreads - 1) / kSeqThreads);
  window_aggregate_kernel<<<blocks, kSeqThreads, 0, (hipStream_t)stream>>>(
      scores, table, per_frame, n_windows, total_frames);
  SGCN_LAUNCH_CHECK();
  return 0;
}
