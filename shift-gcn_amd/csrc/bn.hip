// Training-mode BatchNorm and the elementwise unit tails of the Shift-GCN hot path.
//
// Reference semantics (model/shift_gcn.py): five BatchNorms per TCN_GCN_unit —
//   gcn.bn   = BatchNorm1d(V*C_out) over (n*t) with feature f = v*C_out + d  (:99,:137)
//   down.1, tcn.bn, tcn.bn2, residual.bn = BatchNorm2d over (n, t, v)         (:85,:55-56,:38)
// each followed by the unit's residual add and ReLU (:140-141, :161-162).
//
// Layout stays (N·M, C, T, V). "per_joint" selects the BN1d-over-(d,v) feature set
// (f = d*V + v here, mapped to the reference index v*D + d when reading/writing gamma,
// beta and running stats); otherwise features are channels.
//
// Statistics are deterministic and numerically robust: per-(sample, feature) partial
// moments (mean, M2) from one workgroup per (n·m, c) plane, merged in fixed order with
// Chan's formula in double by the finalize kernels. Running stats follow PyTorch
// (momentum 0.1, unbiased running variance, num_batches_tracked += 1).
#include "common.hpp"
#include "dispatch.hpp"
#include "launch_forms.hpp"
#include "shift_stage.hpp"

namespace sgcn {
namespace {

constexpr int kU = 4;  // elements in flight per thread per loop trip (all loads clamped)

// ------------------------------------------------------------------------------------
// forward statistics: shifted sums per plane (or per joint), no per-element division
// ------------------------------------------------------------------------------------
// part[plane] = {mean, M2} over the plane (per_joint = 0), or part[plane*V + v] over t.
// Shifted data (x - x_first) keeps sum/sum-of-squares well conditioned; the merge over
// the batch is done in double by bn_finalize_kernel.
constexpr int kUM = 8;   // loads in flight per thread (a single-input reduction)

// ZU (per_joint = 3): x holds the Shift_gcn contraction output BEFORE its shift_out, so
// its joint v is the logical joint (v + c) mod V (shift_gcn.py:114-118,136: z[w] =
// y[(w - c) mod V]); the partial goes to the logical feature.
template <bool PER_JOINT, bool ZU = false>
__global__ __launch_bounds__(kThreads) void moments_kernel(const float* __restrict__ x,
                                                            float2* __restrict__ part, int T,
                                                            int V, int C) {
  SGCN_CRIT_PRIO();
  __shared__ float s1[kThreads], s2[kThreads], red[2 * kThreads / 64];
  // planes in REVERSE order: the input was just written front to back by the contraction,
  // so its last planes are still in the die-level (Infinity) cache when this pass starts,
  // and the apply pass that follows (front to back) then meets the planes this pass read
  // last (measured: moments 1.14 -> 0.92 ms per step)
  const int plane = gridDim.x - 1 - blockIdx.x;
  const int P = T * V;
  const float* __restrict__ xp = x + (size_t)plane * P;
  const int i = threadIdx.x;
  if (PER_JOINT) {
    const int G = kThreads / V;  // row groups
    float a = 0.f, q = 0.f;
    const int v = i % V, r = i / V;
    const float k0 = xp[v];      // shift: first row of this joint
    if (i < G * V) {
      for (int t0 = r; t0 < T; t0 += G * kUM) {
        float xv[kUM];
#pragma unroll
        for (int u = 0; u < kUM; ++u) xv[u] = xp[min(t0 + u * G, T - 1) * V + v];
#pragma unroll
        for (int u = 0; u < kUM; ++u) {
          const float d = (t0 + u * G < T) ? xv[u] - k0 : 0.f;
          a += d;
          q += d * d;
        }
      }
    }
    s1[i] = a;
    s2[i] = q;
    __syncthreads();
    if (i < V) {
      float ta = 0.f, tq = 0.f;
      for (int g = 0; g < G; ++g) { ta += s1[g * V + i]; tq += s2[g * V + i]; }
      const float n = (float)T;
      int w = i;
      if (ZU) {
        w = i + (plane % C) % V;
        w = w >= V ? w - V : w;
      }
      part[(size_t)plane * V + w] = make_float2(xp[i] + ta / n, tq - ta * ta / n);
    }
  } else {
    const float k0 = xp[0];
    float a = 0.f, q = 0.f;
    for (int base = 0; base < P; base += kThreads * kUM) {
      float xv[kUM];
#pragma unroll
      for (int u = 0; u < kUM; ++u) xv[u] = xp[min(base + u * kThreads + i, P - 1)];
#pragma unroll
      for (int u = 0; u < kUM; ++u) {
        const float d = (base + u * kThreads + i < P) ? xv[u] - k0 : 0.f;
        a += d;
        q += d * d;
      }
    }
    block_sum2(a, q, red);
    if (i == 0) {
      const float n = (float)P;
      part[plane] = make_float2(k0 + a / n, q - a * a / n);
    }
  }
}

__device__ __forceinline__ int ref_feature(int f, int perm_V, int F) {
  if (perm_V <= 0) return f;
  const int D = F / perm_V;
  const int d = f / perm_V, v = f - d * perm_V;
  return v * D + d;  // BatchNorm1d(V*C) feature index of (d, v)  (shift_gcn.py:135-137)
}

// Plane-resident form of moments_kernel (V <= 64, <= 32 elements per thread): the plane's
// loads all in flight, dealt on the joint-aligned stride NTJ = (NT / V) * V (a thread's
// joint is fixed: the per-joint sums stay in registers and are merged over the GR row
// groups in fixed order). Same shifted sums (shift = the plane's / joint's first element).
template <int NT, int LPT, bool PER_JOINT, bool ZU>
__global__ __launch_bounds__(NT) void moments_ja_kernel(const float* __restrict__ x,
                                                        float2* __restrict__ part, int T,
                                                        int V, int C) {
  SGCN_CRIT_PRIO();
  __shared__ float s1[NT], s2[NT], red[2 * NT / 64];
  const int plane = gridDim.x - 1 - blockIdx.x;   // reverse: see moments_kernel
  const int GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int w = tid % V;
  const int P = T * V;
  const float* __restrict__ xp = x + (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  float xv[LPT];
  {
    const auto xr = make_rsrc(xp, (unsigned)P * 4u);
#pragma unroll
    for (int e = 0; e < LPT; ++e) xv[e] = bload(xr, vo + e * vstep, 0);
  }
  const int nval = own ? (P - tid + NTJ - 1) / NTJ : 0;   // this lane's elements e < nval
  const float k0 = PER_JOINT ? xp[w] : xp[0];
  float a = 0.f, q = 0.f;
#pragma unroll
  for (int e = 0; e < LPT; ++e) {
    const float d = e < nval ? xv[e] - k0 : 0.f;
    a += d;
    q += d * d;
  }
  if (PER_JOINT) {
    s1[tid] = a;
    s2[tid] = q;
    __syncthreads();
    if (tid < V) {
      float ta = 0.f, tq = 0.f;
      for (int g = 0; g < GR; ++g) { ta += s1[g * V + tid]; tq += s2[g * V + tid]; }
      const float n = (float)T;
      int wo = tid;
      if (ZU) {
        wo = tid + (plane % C) % V;
        wo = wo >= V ? wo - V : wo;
      }
      part[(size_t)plane * V + wo] = make_float2(xp[tid] + ta / n, tq - ta * ta / n);
    }
  } else {
    block_sum2(a, q, red);
    if (tid == 0) {
      const float n = (float)P;
      part[plane] = make_float2(k0 + a / n, q - a * a / n);
    }
  }
}

// Per-feature sums over the batch of float2 partials part[b][f]: a workgroup takes 64
// consecutive features (the lanes: each load reads 512 contiguous bytes) and its kFSW waves
// take every kFSW-th sample, 4 rows in flight, then a fixed-order merge through LDS in
// double (deterministic). Lane l of wave 0 returns feature blockIdx.x*64 + l's three double
// sums (x, y, x*x). (One wave per feature with the lanes striding the batch cost a cache
// line per lane and load.)
constexpr int kFW = 4;    // features (waves) per 256-thread block (mask_grad_finalize)
constexpr int kFSW = 8;   // waves per 64 features in the BatchNorm finalizes
__device__ __forceinline__ double wave_dsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ bool feature_sums(const float2* __restrict__ part, int B, int F,
                                             double& sx, double& sy, double& sxx, int& f) {
  __shared__ double red[kFSW - 1][3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  f = blockIdx.x * 64 + lane;
  const int fc = min(f, F - 1);
  double ax = 0.0, ay = 0.0, axx = 0.0;
  int b = w;
  for (; b + 3 * kFSW < B; b += 4 * kFSW) {
    float2 pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pv[u] = part[(size_t)(b + u * kFSW) * F + fc];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ax += pv[u].x;
      ay += pv[u].y;
      axx += (double)pv[u].x * pv[u].x;
    }
  }
  for (; b < B; b += kFSW) {
    const float2 pv = part[(size_t)b * F + fc];
    ax += pv.x;
    ay += pv.y;
    axx += (double)pv.x * pv.x;
  }
  if (w) {
    red[w - 1][0][lane] = ax;
    red[w - 1][1][lane] = ay;
    red[w - 1][2][lane] = axx;
  }
  __syncthreads();
  if (w) return false;
  for (int q = 0; q < kFSW - 1; ++q) {
    ax += red[q][0][lane];
    ay += red[q][1][lane];
    axx += red[q][2][lane];
  }
  sx = ax;
  sy = ay;
  sxx = axx;
  return f < F;
}

// part layout [B][F] of {mean, M2}, each over n_part elements. Equal counts, so
// mean = avg(mean_b), M2 = sum M2_b + n_part * sum (mean_b - mean)^2 (double).
__global__ __launch_bounds__(64 * kFSW) void bn_finalize_kernel(
    const float2* __restrict__ part, int B, int F, int n_part, int perm_V,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    float momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
    long long* __restrict__ num_batches, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ scale_out,
    float* __restrict__ shift_out) {
  SGCN_CRIT_PRIO();
  if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches) *num_batches += 1;
  double smean, sm2, smean2;
  int f;
  if (!feature_sums(part, B, F, smean, sm2, smean2, f)) return;
  const int rf = ref_feature(f, perm_V, F);
  const float g = gamma ? gamma[rf] : 1.f;
  const float bb = beta ? beta[rf] : 0.f;
  const BnCoef k = bn_train_coef(smean, sm2, smean2, B, n_part, eps, g, bb);
  mean_out[f] = k.mean;
  invstd_out[f] = k.invstd;
  scale_out[f] = k.scale;
  shift_out[f] = k.shift;
  if (running_mean) bn_running_update(running_mean, running_var, rf, momentum, k);
}

// eval-mode coefficients from running statistics
__global__ void bn_eval_coef_kernel(int F, int perm_V, const float* __restrict__ gamma,
                                    const float* __restrict__ beta,
                                    const float* __restrict__ running_mean,
                                    const float* __restrict__ running_var, float eps,
                                    float* __restrict__ mean_out,
                                    float* __restrict__ invstd_out,
                                    float* __restrict__ scale_out,
                                    float* __restrict__ shift_out) {
  SGCN_CRIT_PRIO();
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int rf = ref_feature(f, perm_V, F);
  const float invstd = (float)(1.0 / sqrt((double)running_var[rf] + (double)eps));
  const float scale = (gamma ? gamma[rf] : 1.f) * invstd;
  if (mean_out) mean_out[f] = running_mean[rf];
  if (invstd_out) invstd_out[f] = invstd;
  scale_out[f] = scale;
  shift_out[f] = (beta ? beta[rf] : 0.f) - running_mean[rf] * scale;
}

// ------------------------------------------------------------------------------------
// apply: y = act(x*scale[f] + shift[f] + res); res = r*rscale[c] + rshift[c] | r | 0
// ------------------------------------------------------------------------------------
// OUT_STATS: also write the per-plane {mean, M2} of y (moments of the NEXT BatchNorm's
// input, shifted by the plane's first output), saving a separate read pass of y.
// OUTX = 2 instead: also write yg = the NEXT Shift_gcn's gathered, masked input
// yg[c,t,(v - c) mod V] = y[c,t,v] * gm[((v - c) mod V)*C + c] (what sgcn_gcn_gather would
// make from y), saving that kernel's read of y.
// ZU: x is the pre-shift_out contraction output (see moments_kernel): its element (t, v) is
// the logical element (t, (v + c) mod V), where the coefficients, the residual and every
// output live.
template <bool PER_JOINT, int RES, bool RELU, int OUTX, bool ZU = false>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ r,
    const float* __restrict__ rscale, const float* __restrict__ rshift,
    float* __restrict__ y, float2* __restrict__ ystats, const float* __restrict__ gm,
    float* __restrict__ yg, int C, int T, int V) {
  SGCN_CRIT_PRIO();
  constexpr bool OUT_STATS = OUTX == 1, OUT_G = OUTX == 2;
  __shared__ float red[2 * kThreads / 64];
  __shared__ float gm_s[OUT_G ? kThreads : 1];   // this channel's mask column, by joint
  const int plane = blockIdx.x, c = plane % C;
  const int rc = c % V;
  __shared__ float sc_s[PER_JOINT ? kThreads : 1], sh_s[PER_JOINT ? kThreads : 1];
  if (OUT_G && (int)threadIdx.x < V) gm_s[threadIdx.x] = gm[threadIdx.x * C + c];
  if (PER_JOINT && (int)threadIdx.x < V) {
    sc_s[threadIdx.x] = scale[c * V + threadIdx.x];
    sh_s[threadIdx.x] = shift[c * V + threadIdx.x];
  }
  if (OUT_G || PER_JOINT) __syncthreads();
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  float sc = 0.f, sh = 0.f, rsc = 1.f, rsh = 0.f;
  if (!PER_JOINT) { sc = scale[c]; sh = shift[c]; }
  if (RES == 2) { rsc = rscale[c]; rsh = rshift[c]; }
  const int dv = kThreads % V;
  int v = threadIdx.x % V;
  float k0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (OUT_STATS) {  // shift = the plane's first output value (same formula, element 0)
    float a = x[off];
    if (PER_JOINT) a = a * scale[c * V] + shift[c * V];
    else a = a * sc + sh;
    if (RES == 1) a += r[off];
    if (RES == 2) a += r[off] * rsc + rsh;
    if (RELU) a = fmaxf(a, 0.f);
    k0 = a;
  }
  // ZU: logical joint vl of this thread's current element (in-row logical offset vl - v)
  int vl = v;
  if (ZU) {
    vl = v + rc;
    vl = vl >= V ? vl - V : vl;
  }
  for (int base = 0; base < P; base += kThreads * kU) {
    float xv[kU], rv[kU];
    int vq = v, vlq = vl;   // per-u copies for the residual's logical address
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int oc = min(base + u * kThreads + (int)threadIdx.x, P - 1);
      xv[u] = x[off + oc];
      if (RES) rv[u] = r[off + (ZU ? min(max(oc - vq + vlq, 0), P - 1) : oc)];
      if (ZU) {
        vq += dv;
        vq = vq >= V ? vq - V : vq;
        vlq += dv;
        vlq = vlq >= V ? vlq - V : vlq;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int o = base + u * kThreads + threadIdx.x;
      const int ol = ZU ? o - v + vl : o;
      float a = xv[u];
      if (PER_JOINT) a = a * sc_s[vl] + sh_s[vl];
      else a = a * sc + sh;
      if (RES == 1) a += rv[u];
      if (RES == 2) a += rv[u] * rsc + rsh;
      if (RELU) a = fmaxf(a, 0.f);
      if (o < P) y[off + ol] = a;
      if (OUT_G) {
        int u2 = vl - rc;
        u2 = u2 < 0 ? u2 + V : u2;
        if (o < P) yg[off + ol - vl + u2] = a * gm_s[u2];
      }
      if (OUT_STATS) {
        const float d = o < P ? a - k0 : 0.f;
        s1 += d;
        s2 += d * d;
      }
      v += dv;
      if (v >= V) v -= V;
      vl += dv;   // (== v when !ZU)
      if (vl >= V) vl -= V;
    }
  }
  if (OUT_STATS) {
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
      const float n = (float)P;
      ystats[plane] = make_float2(k0 + s1 / n, s2 - s1 * s1 / n);
    }
  }
}

// Plane-resident form of bn_apply_kernel (the product kernel for V <= 64 and planes of
// <= 32 elements per thread): one workgroup per (n·m, c) plane holds the whole plane in
// registers, dealt on the joint-aligned stride NTJ = (NT / V) * V, so a thread's (logical)
// joint w is fixed: the per-joint coefficients, the ZU source offset (the pre-shift_out
// element of logical joint w sits at (w - c) mod V in its row) and the gather target /
// mask of OUTX = 2 are per-thread constants, and every load of the plane is in flight at
// once (buffer descriptors: no clamps, stores past the plane drop). Same expressions as
// bn_apply_kernel, so y / yg are bit-identical; OUTX = 1 takes the plane's {mean, M2} by
// two passes over the registers.
template <int NT, int LPT, bool PER_JOINT, int RES, bool RELU, int OUTX, bool ZU>
__global__ __launch_bounds__(NT) void bn_apply_ja_kernel(
    const float* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ r,
    const float* __restrict__ rscale, const float* __restrict__ rshift,
    float* __restrict__ y, float2* __restrict__ ystats, const float* __restrict__ gm,
    float* __restrict__ yg, int C, int T, int V) {
  SGCN_CRIT_PRIO();
  constexpr bool OUT_STATS = OUTX == 1, OUT_G = OUTX == 2;
  __shared__ float red[2 * NT / 64];
  const int plane = blockIdx.x, c = plane % C, rc = c % V;
  const int GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int w = tid % V;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  const unsigned pb = (unsigned)P * 4u;
  // ZU: the source element of logical joint w; OUT_G: its gather target (both in-row)
  int wz = w - rc;
  wz = wz < 0 ? wz + V : wz;
  const unsigned xo = vo + (unsigned)((ZU ? wz - w : 0) * 4);
  const unsigned go = vo + (unsigned)((wz - w) * 4);
  float xv[LPT], rv[RES ? LPT : 1];
  {
    const auto xr = make_rsrc(x + off, pb);
#pragma unroll
    for (int e = 0; e < LPT; ++e) xv[e] = bload(xr, xo + e * vstep, 0);
    if (RES) {
      const auto rr = make_rsrc(r + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) rv[e] = bload(rr, vo + e * vstep, 0);
    }
  }
  const float sc = PER_JOINT ? scale[c * V + w] : scale[c];
  const float sh = PER_JOINT ? shift[c * V + w] : shift[c];
  const float rsc = RES == 2 ? rscale[c] : 1.f, rsh = RES == 2 ? rshift[c] : 0.f;
  const float gmu = OUT_G ? gm[wz * C + c] : 0.f;
  const auto yr = make_rsrc(y + off, pb);
  const auto ygr = make_rsrc(OUT_G ? yg + off : y + off, OUT_G ? pb : 0u);
  const int nval = own ? (P - tid + NTJ - 1) / NTJ : 0;   // this lane's elements e < nval
  float s1 = 0.f;
#pragma unroll
  for (int e = 0; e < LPT; ++e) {
    float a = xv[e] * sc + sh;
    if (RES == 1) a += rv[e];
    if (RES == 2) a += rv[e] * rsc + rsh;
    if (RELU) a = fmaxf(a, 0.f);
    bstore(yr, a, vo + e * vstep, 0);
    if (OUT_G) bstore(ygr, a * gmu, go + e * vstep, 0);
    if (OUT_STATS) {
      xv[e] = e < nval ? a : 0.f;   // keep y for the second pass
      s1 += xv[e];
    }
  }
  if (OUT_STATS) {
    s1 = block_sum(s1, red);
    const float mean = s1 / (float)P;
    float m2 = 0.f;
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      const float d = xv[e] - mean;
      m2 += e < nval ? d * d : 0.f;
    }
    m2 = block_sum(m2, red);
    if (tid == 0) ystats[plane] = make_float2(mean, m2);
  }
}

// ------------------------------------------------------------------------------------
// backward: reductions of g = dy*(y>0) and g*xhat per feature
// ------------------------------------------------------------------------------------
// DYT: the incoming gradient is itself a BatchNorm input-gradient that was never
// materialised: dy_eff = k1[c]*dy + k2[c]*y + k3[c] with y the tensor read for the ReLU
// mask (the unit's gcn output H, input of Shift_tcn.bn).
// PER_JOINT: x is the Shift_gcn contraction output stored before its shift_out (the
// per_joint = 3 layout); the logical joint v of this thread's column reads it at
// (v - c) mod V.
template <bool PER_JOINT, bool RELU, bool RESBN, bool DYT>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(
    const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ r, const float* __restrict__ rmean,
    const float* __restrict__ rinvstd, const float* __restrict__ dyc, float2* __restrict__ part,
    float2* __restrict__ rpart, int C, int T, int V, int dyp) {
  SGCN_CRIT_PRIO();
  __shared__ float s0[kThreads], s1[kThreads], red[2 * kThreads / 64];
  const int plane = blockIdx.x, c = plane % C;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const int i = threadIdx.x;
  // dyp: dy holds one value per plane (element o of the plane reads dy[plane])
  const float* __restrict__ dyq = dyp ? dy + plane : dy + off;
  const int dys = dyp ? 0 : 1;
  float rm = 0.f, ri = 0.f, d1 = 1.f, d2 = 0.f, d3 = 0.f;
  if (RESBN) { rm = rmean[c]; ri = rinvstd[c]; }
  if (DYT) { d1 = dyc[c]; d2 = dyc[C + c]; d3 = dyc[2 * C + c]; }
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
  if (PER_JOINT) {
    const int G = kThreads / V;
    const int v = i % V, rr = i / V;
    const int vc = min(v, V - 1);
    const float mu = mean[c * V + vc], is = invstd[c * V + vc];
    int vx = v - c % V;   // in-row offset of this column's (pre-rotation) x element
    vx = vx < 0 ? vx + V : vx;
    const int xd = vx - v;
    if (i < G * V) {
      for (int t0 = rr; t0 < T; t0 += G * kU) {
        float gv[kU], yv[kU], xv[kU], rv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int o = min(t0 + u * G, T - 1) * V + v;
          gv[u] = dyq[o * dys];
          if (RELU) yv[u] = y[off + o];
          xv[u] = x[off + o + xd];
          if (RESBN) rv[u] = r[off + o];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          float g = gv[u];
          if (DYT) g = d1 * g + d2 * yv[u] + d3;
          g = (t0 + u * G < T) ? g : 0.f;
          if (RELU) g = yv[u] > 0.f ? g : 0.f;
          a0 += g;
          a1 += g * ((xv[u] - mu) * is);
          if (RESBN) { b0 += g; b1 += g * ((rv[u] - rm) * ri); }
        }
      }
    }
    if (RESBN) block_sum2(b0, b1, red);
    s0[i] = a0;
    s1[i] = a1;
    __syncthreads();
    if (i < V) {
      float t0 = 0.f, t1 = 0.f;
      for (int g = 0; g < G; ++g) { t0 += s0[g * V + i]; t1 += s1[g * V + i]; }
      part[(size_t)plane * V + i] = make_float2(t0, t1);
    }
    if (RESBN && i == 0) rpart[plane] = make_float2(b0, b1);
  } else {
    const float mu = mean[c], is = invstd[c];
    for (int base = 0; base < P; base += kThreads * kU) {
      float gv[kU], yv[kU], xv[kU], rv[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int o = min(base + u * kThreads + i, P - 1);
        gv[u] = dyq[o * dys];
        if (RELU) yv[u] = y[off + o];
        xv[u] = x[off + o];
        if (RESBN) rv[u] = r[off + o];
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float g = gv[u];
        if (DYT) g = d1 * g + d2 * yv[u] + d3;
        g = (base + u * kThreads + i < P) ? g : 0.f;
        if (RELU) g = yv[u] > 0.f ? g : 0.f;
        a0 += g;
        a1 += g * ((xv[u] - mu) * is);
        if (RESBN) { b0 += g; b1 += g * ((rv[u] - rm) * ri); }
      }
    }
    block_sum2(a0, a1, red);
    if (RESBN) block_sum2(b0, b1, red);
    if (i == 0) {
      part[plane] = make_float2(a0, a1);
      if (RESBN) rpart[plane] = make_float2(b0, b1);
    }
  }
}

// Plane-resident form of bn_bwd_reduce_kernel (V <= 64, <= 32 elements per thread): the
// plane's loads all in flight on the joint-aligned stride (a thread's joint is fixed:
// per-joint statistics and the pre-rotation offset of x are per-thread constants).
template <int NT, int LPT, bool PER_JOINT, bool RELU, bool RESBN, bool DYT>
__global__ __launch_bounds__(NT) void bn_bwd_reduce_ja_kernel(
    const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ r, const float* __restrict__ rmean,
    const float* __restrict__ rinvstd, const float* __restrict__ dyc, float2* __restrict__ part,
    float2* __restrict__ rpart, int C, int T, int V, int dyp) {
  SGCN_CRIT_PRIO();
  __shared__ float s0[NT], s1[NT], red[2 * NT / 64];
  const int plane = blockIdx.x, c = plane % C;
  const int GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int w = tid % V;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  const unsigned pb = (unsigned)P * 4u;
  int vx = w - c % V;   // in-row offset of this joint's (pre-rotation) x element
  vx = vx < 0 ? vx + V : vx;
  const unsigned xo = vo + (unsigned)((PER_JOINT ? vx - w : 0) * 4);
  float gv[LPT], yv[RELU ? LPT : 1], xv[LPT], rv[RESBN ? LPT : 1];
  {
    const auto xr = make_rsrc(x + off, pb);
    if (dyp) {   // one value per plane (a lane's elements past the plane are zeroed below)
      const float pv = dy[plane];
#pragma unroll
      for (int e = 0; e < LPT; ++e) gv[e] = pv;
    } else {
      const auto dyr = make_rsrc(dy + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) gv[e] = bload(dyr, vo + e * vstep, 0);
    }
#pragma unroll
    for (int e = 0; e < LPT; ++e) xv[e] = bload(xr, xo + e * vstep, 0);
    if (RELU) {
      const auto yr = make_rsrc(y + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) yv[e] = bload(yr, vo + e * vstep, 0);
    }
    if (RESBN) {
      const auto rr = make_rsrc(r + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) rv[e] = bload(rr, vo + e * vstep, 0);
    }
  }
  float rm = 0.f, ri = 0.f, d1 = 1.f, d2 = 0.f, d3 = 0.f;
  if (RESBN) { rm = rmean[c]; ri = rinvstd[c]; }
  if (DYT) { d1 = dyc[c]; d2 = dyc[C + c]; d3 = dyc[2 * C + c]; }
  const float mu = PER_JOINT ? mean[c * V + w] : mean[c];
  const float is = PER_JOINT ? invstd[c * V + w] : invstd[c];
  const int nval = own ? (P - tid + NTJ - 1) / NTJ : 0;   // this lane's elements e < nval
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
  for (int e = 0; e < LPT; ++e) {
    float g = gv[e];
    if (DYT) g = d1 * g + d2 * yv[e] + d3;
    g = e < nval ? g : 0.f;
    if (RELU) g = yv[e] > 0.f ? g : 0.f;
    a0 += g;
    a1 = fmaf(g, (xv[e] - mu) * is, a1);
    if (RESBN) { b0 += g; b1 = fmaf(g, (rv[e] - rm) * ri, b1); }
  }
  if (PER_JOINT) {
    if (RESBN) block_sum2(b0, b1, red);
    s0[tid] = a0;
    s1[tid] = a1;
    __syncthreads();
    if (tid < V) {
      float t0 = 0.f, t1 = 0.f;
      for (int g = 0; g < GR; ++g) { t0 += s0[g * V + tid]; t1 += s1[g * V + tid]; }
      part[(size_t)plane * V + tid] = make_float2(t0, t1);
    }
    if (RESBN && tid == 0) rpart[plane] = make_float2(b0, b1);
  } else {
    block_sum2(a0, a1, red);
    if (RESBN) block_sum2(b0, b1, red);
    if (tid == 0) {
      part[plane] = make_float2(a0, a1);
      if (RESBN) rpart[plane] = make_float2(b0, b1);
    }
  }
}

// dgamma = sum g*xhat, dbeta = sum g; dx = k1*g + k2*x + k3 with
// k1 = gamma*invstd, k2 = -k1*invstd*mean(g*xhat), k3 = -k1*mean(g) - k2*mean_x
__global__ __launch_bounds__(64 * kFSW) void bn_bwd_finalize_kernel(
    const float2* __restrict__ part, int B, int F, double n_total, int perm_V,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, float* __restrict__ dgamma, float* __restrict__ dbeta,
    int accumulate, int batch_stats, float* __restrict__ coef) {
  SGCN_CRIT_PRIO();
  double sg, sgx, unused;
  int f;
  if (!feature_sums(part, B, F, sg, sgx, unused, f)) return;
  const int rf = ref_feature(f, perm_V, F);
  if (dgamma) dgamma[rf] = accumulate ? dgamma[rf] + (float)sgx : (float)sgx;
  if (dbeta) dbeta[rf] = accumulate ? dbeta[rf] + (float)sg : (float)sg;
  const float g = gamma ? gamma[rf] : 1.f;
  const float3 k = bn_bwd_coef(sg, sgx, g, invstd[f], mean[f], n_total, batch_stats);
  coef[f] = k.x;
  coef[F + f] = k.y;
  coef[2 * F + f] = k.z;
}

// The same from the k-free per-(plane, joint) sums of sgcn_tshift_bwd_gbn:
//   part6[j][b][f], j = {sum dA, sum (H-mu), sum 1, sum dA*zh, sum (H-mu)*zh, sum zh}
// over the active (H > 0) positions, g = k1*dA + k2*(H - mu) + (k3 + k2*mu) with
// k = dyc[3][C] (Shift_tcn.bn's backward coefficients) and mu = dym[C] (its batch mean),
// channel c = f / V. The six sums are merged over b in double: a workgroup takes 64
// consecutive features (the lanes: every load reads 256 contiguous bytes) and its
// kGbnW waves take every kGbnW-th sample (4 rows in flight), merged in fixed order
// through LDS. (The one-wave-per-feature form with lanes striding the batch cost a cache
// line per lane and load: 19 us average per call at F = 1,600-6,400, B = 128.)
// Waves per workgroup: this launch is on the critical path while the side stream's
// weight-gradient contractions hold most CUs; a 1,024-thread workgroup (16 waves, 46 KB of
// LDS) waits for a whole CU to drain (92 us per call in the overlapped trace,
// profiles/r04_gbnfin/), smaller ones fit in beside them.
#ifndef SGCN_GBN_WAVES
#define SGCN_GBN_WAVES 4
#endif
constexpr int kGbnW = SGCN_GBN_WAVES;
__global__ __launch_bounds__(64 * kGbnW) void bn_bwd_finalize_gbn_kernel(
    const float* __restrict__ part6, int B, int F, int V, double n_total,
    const float* __restrict__ dyc, const float* __restrict__ dym, int C,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, float* __restrict__ dgamma, float* __restrict__ dbeta,
    int accumulate, int batch_stats, float* __restrict__ coef) {
  SGCN_CRIT_PRIO();
  __shared__ double red[kGbnW - 1][6][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane;
  const int fc = min(f, F - 1);
  const size_t np = (size_t)B * F;
  double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int b = w;
  for (; b + 3 * kGbnW < B; b += 4 * kGbnW) {
    float pv[6][4];
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) pv[j][u] = part6[j * np + (size_t)(b + u * kGbnW) * F + fc];
#pragma unroll
    for (int j = 0; j < 6; ++j)
      s6[j] += ((double)pv[j][0] + (double)pv[j][1]) + ((double)pv[j][2] + (double)pv[j][3]);
  }
  for (; b < B; b += kGbnW) {
#pragma unroll
    for (int j = 0; j < 6; ++j) s6[j] += (double)part6[j * np + (size_t)b * F + fc];
  }
  if (w) {
#pragma unroll
    for (int j = 0; j < 6; ++j) red[w - 1][j][lane] = s6[j];
  }
  __syncthreads();
  if (w || f >= F) return;
  for (int q = 0; q < kGbnW - 1; ++q) {
#pragma unroll
    for (int j = 0; j < 6; ++j) s6[j] += red[q][j][lane];
  }
  const int c = f / V;
  const double k1 = dyc[c], k2 = dyc[C + c], c3 = (double)dyc[2 * C + c] + k2 * (double)dym[c];
  const double sg = k1 * s6[0] + k2 * s6[1] + c3 * s6[2];
  const double sgx = k1 * s6[3] + k2 * s6[4] + c3 * s6[5];
  const int rf = ref_feature(f, V, F);
  if (dgamma) dgamma[rf] = accumulate ? dgamma[rf] + (float)sgx : (float)sgx;
  if (dbeta) dbeta[rf] = accumulate ? dbeta[rf] + (float)sg : (float)sg;
  const float g = gamma ? gamma[rf] : 1.f;
  const float is = invstd[f];
  const float q1 = g * is;
  // running-statistics (eval) BatchNorm: dx = q1 * g, as bn_bwd_finalize_kernel
  const float q2 = batch_stats ? (float)(-(double)q1 * (double)is * (sgx / n_total)) : 0.f;
  const float q3 = batch_stats ? (float)(-(double)q1 * (sg / n_total) - (double)q2 * (double)mean[f])
                               : 0.f;
  coef[f] = q1;
  coef[F + f] = q2;
  coef[2 * F + f] = q3;
}

// dx = k1[f]*g + k2[f]*x + k3[f]; RES: 1 -> dr = g, 2 -> dr = rk1*g + rk2*r + rk3
// PJM: 0 per-channel, 1 per-joint, 2 per-joint with dx stored GATHERED: element (c, t, v)
// goes to (c, t, (v - c) mod V), i.e. the shift_out gather of the next contraction
// (shift_gcn.py:114-118,136 transposed) is done by this store, not by every GEMM load.
template <int PJM, bool RELU, int RES, bool DYT>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(
    const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
    const float* __restrict__ coef, int F, const float* __restrict__ r,
    const float* __restrict__ rcoef, int RF, const float* __restrict__ dyc,
    float* __restrict__ dx, float* __restrict__ dr, int C, int T, int V) {
  SGCN_CRIT_PRIO();
  // PJM 3: as 2, and x is the pre-shift_out contraction output, read at the same gathered
  // (pre-rotation) index the dx store uses
  constexpr bool PER_JOINT = PJM != 0, GATH = PJM >= 2, XG = PJM == 3;
  const int plane = blockIdx.x, c = plane % C;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const int rc = c % V;
  __shared__ float k_s[PER_JOINT ? 3 * kThreads : 1];   // per-joint {k1, k2, k3} of channel c
  if (PER_JOINT) {
    if ((int)threadIdx.x < V) {
      const int f = c * V + threadIdx.x;
      k_s[threadIdx.x] = coef[f];
      k_s[kThreads + threadIdx.x] = coef[F + f];
      k_s[2 * kThreads + threadIdx.x] = coef[2 * F + f];
    }
    __syncthreads();
  }
  float k1 = 0.f, k2 = 0.f, k3 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
  float d1 = 1.f, d2 = 0.f, d3 = 0.f;
  if (DYT) { d1 = dyc[c]; d2 = dyc[C + c]; d3 = dyc[2 * C + c]; }
  if (!PER_JOINT) { k1 = coef[c]; k2 = coef[F + c]; k3 = coef[2 * F + c]; }
  if (RES == 2) { q1 = rcoef[c]; q2 = rcoef[RF + c]; q3 = rcoef[2 * RF + c]; }
  const int dv = kThreads % V;
  int v = threadIdx.x % V;
  for (int base = 0; base < P; base += kThreads * kU) {
    float gv[kU], yv[kU], xv[kU], rv[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int o = min(base + u * kThreads + (int)threadIdx.x, P - 1);
      gv[u] = dy[off + o];
      if (RELU) yv[u] = y[off + o];
      if (!XG) xv[u] = x[off + o];
      if (RES == 2) rv[u] = r[off + o];
    }
    if (XG) {   // the gathered index of element o (joint v advanced per u as below)
      int vq = v;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int o = min(base + u * kThreads + (int)threadIdx.x, P - 1);
        const int w = vq - rc;
        xv[u] = x[off + min(max(o - vq + (w < 0 ? w + V : w), 0), P - 1)];
        vq += dv;
        if (vq >= V) vq -= V;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int o = base + u * kThreads + threadIdx.x;
      float g = gv[u];
      if (DYT) g = d1 * g + d2 * yv[u] + d3;
      if (RELU) g = yv[u] > 0.f ? g : 0.f;
      if (PER_JOINT) { k1 = k_s[v]; k2 = k_s[kThreads + v]; k3 = k_s[2 * kThreads + v]; }
      if (o < P) {
        int od = o;
        if (GATH) {
          const int w = v - rc;
          od = o - v + (w < 0 ? w + V : w);
        }
        dx[off + od] = k1 * g + k2 * xv[u] + k3;
        if (RES == 1) dr[off + o] = g;
        if (RES == 2) dr[off + o] = q1 * g + q2 * rv[u] + q3;
      }
      v += dv;
      if (v >= V) v -= V;
    }
  }
}

// Plane-resident form of bn_bwd_apply_kernel (V <= 64, <= 32 elements per thread): the
// whole plane in registers on the joint-aligned stride, all loads in flight at once; a
// thread's joint is fixed, so the per-joint coefficients and the PJM 3 gathered index
// (element (c, t, v) at (c, t, (v - c) mod V)) are per-thread constants. Same expressions
// as bn_bwd_apply_kernel: outputs bit-identical.
template <int NT, int LPT, int PJM, bool RELU, int RES, bool DYT>
__global__ __launch_bounds__(NT) void bn_bwd_apply_ja_kernel(
    const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
    const float* __restrict__ coef, int F, const float* __restrict__ r,
    const float* __restrict__ rcoef, int RF, const float* __restrict__ dyc,
    float* __restrict__ dx, float* __restrict__ dr, int C, int T, int V) {
  SGCN_CRIT_PRIO();
  static_assert(PJM == 0 || PJM == 3, "per-channel, or per-joint gathered (ZU)");
  constexpr bool PER_JOINT = PJM == 3;
  const int plane = blockIdx.x, c = plane % C, rc = c % V;
  const int GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int w = tid % V;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  const unsigned pb = (unsigned)P * 4u;
  int wz = w - rc;
  wz = wz < 0 ? wz + V : wz;
  const unsigned go = vo + (unsigned)((PER_JOINT ? wz - w : 0) * 4);   // dx (and x) index
  float gv[LPT], yv[RELU ? LPT : 1], xv[LPT], rv[RES == 2 ? LPT : 1];
  {
    const auto dyr = make_rsrc(dy + off, pb);
    const auto xr = make_rsrc(x + off, pb);
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      gv[e] = bload(dyr, vo + e * vstep, 0);
      xv[e] = bload(xr, go + e * vstep, 0);
    }
    if (RELU) {
      const auto yr = make_rsrc(y + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) yv[e] = bload(yr, vo + e * vstep, 0);
    }
    if (RES == 2) {
      const auto rr = make_rsrc(r + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) rv[e] = bload(rr, vo + e * vstep, 0);
    }
  }
  const int f = PER_JOINT ? c * V + w : c;
  const float k1 = coef[f], k2 = coef[F + f], k3 = coef[2 * F + f];
  float d1 = 1.f, d2 = 0.f, d3 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
  if (DYT) { d1 = dyc[c]; d2 = dyc[C + c]; d3 = dyc[2 * C + c]; }
  if (RES == 2) { q1 = rcoef[c]; q2 = rcoef[RF + c]; q3 = rcoef[2 * RF + c]; }
  const auto dxr = make_rsrc(dx + off, pb);
  const auto drr = make_rsrc(RES ? dr + off : dx + off, RES ? pb : 0u);
#pragma unroll
  for (int e = 0; e < LPT; ++e) {
    float g = gv[e];
    if (DYT) g = d1 * g + d2 * yv[e] + d3;
    if (RELU) g = yv[e] > 0.f ? g : 0.f;
    bstore(dxr, k1 * g + k2 * xv[e] + k3, go + e * vstep, 0);
    if (RES == 1) bstore(drr, g, vo + e * vstep, 0);
    if (RES == 2) bstore(drr, q1 * g + q2 * rv[e] + q3, vo + e * vstep, 0);
  }
}

// bn_bwd_apply_ja_kernel<.., 3, true, RES, true> whose dy is never read from memory: dy =
// shift_inᵀ(gout), the input gradient of Shift_tcn's stride-1 shift_in (positions xpos, ypos),
// re-formed per element from the gout plane staged in the zero-padded LDS image exactly as
// tshift_bwd_ra_kernel stages it, through the same shift_in_grad — so the tensor that kernel
// would store and this one read back never exists, and dx / dr are bit-identical to the pair
// (same expressions in the same order from there on). One workgroup per (b, c) plane on
// the joint-aligned stride; y, x (and r) in registers, every load in flight before the
// barrier. A channel whose taps leave the padding takes a rolled, range-checked loop that
// re-reads its operands (never in a trained model).
template <int NT, int LPT, int RES>
__global__ __launch_bounds__(NT) void bn_bwd_apply_tsh_kernel(
    const float* __restrict__ gout, const float* __restrict__ xpos,
    const float* __restrict__ ypos, const float* __restrict__ y, const float* __restrict__ x,
    const float* __restrict__ coef, int F, const float* __restrict__ r,
    const float* __restrict__ rcoef, int RF, const float* __restrict__ dyc,
    float* __restrict__ dx, float* __restrict__ dr, int C, int T, int V) {
  SGCN_CRIT_PRIO();
  static_assert(RES == 1 || RES == 2, "dr = g, or the down BatchNorm's input gradient");
  extern __shared__ float lds[];   // [(T + 2*kPadRows) * WP] padded gout + 1 spare
  const int plane = blockIdx.x, c = plane % C, rc = c % V;
  const int WP = V + 2, GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int w = tid % V, h0 = tid / V;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  const unsigned pb = (unsigned)P * 4u;
  int wz = w - rc;
  wz = wz < 0 ? wz + V : wz;
  const unsigned go = vo + (unsigned)((wz - w) * 4);   // dx (and x) index
  const auto yr = make_rsrc(y + off, pb);
  const auto xr = make_rsrc(x + off, pb);
  const auto rr = make_rsrc(RES == 2 ? r + off : y + off, RES == 2 ? pb : 0u);
  float yv[LPT], xv[LPT], rv[RES == 2 ? LPT : 1];
  {
    const auto gr = make_rsrc(gout + off, pb);
    float t[LPT];
#pragma unroll
    for (int e = 0; e < LPT; ++e) t[e] = bload(gr, vo + e * vstep, 0);
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      yv[e] = bload(yr, vo + e * vstep, 0);
      xv[e] = bload(xr, go + e * vstep, 0);
    }
    if (RES == 2) {
#pragma unroll
      for (int e = 0; e < LPT; ++e) rv[e] = bload(rr, vo + e * vstep, 0);
    }
    zero_pad<NT>(lds, T, V);
    // element (h, w) at lds[(h + kPadRows) * WP + w + 1]; a lane's elements past the plane go
    // to the spare float after the padded plane (branch-free stores)
    const int lb = (h0 + kPadRows) * WP + w + 1, lspare = ra_pad_floats(T, V);
#pragma unroll
    for (int e = 0; e < LPT; ++e)
      lds[own && e * NTJ + tid < P ? lb + e * GR * WP : lspare] = t[e];
  }
  const int f = c * V + w;
  const float k1 = coef[f], k2 = coef[F + f], k3 = coef[2 * F + f];
  const float d1 = dyc[c], d2 = dyc[C + c], d3 = dyc[2 * C + c];
  float q1 = 0.f, q2 = 0.f, q3 = 0.f;
  if (RES == 2) { q1 = rcoef[c]; q2 = rcoef[RF + c]; q3 = rcoef[2 * RF + c]; }
  const Geom rg = make_geom(-xpos[c], -ypos[c]);
  const auto dxr = make_rsrc(dx + off, pb);
  const auto drr = make_rsrc(dr + off, pb);
  __syncthreads();
  if (!own) return;
  const int lmax = (T - 1 + kPadRows) * WP + V;   // the last element: bases past the plane clamp here
  if (shift_in_grad_fits(rg)) {
    int l0 = (h0 + kPadRows) * WP + w + 1;
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      float g = shift_in_grad<true>(lds, rg, min(l0, lmax), 0, w, T, V);
      g = d1 * g + d2 * yv[e] + d3;
      g = yv[e] > 0.f ? g : 0.f;
      bstore(dxr, k1 * g + k2 * xv[e] + k3, go + e * vstep, 0);
      if (RES == 1) bstore(drr, g, vo + e * vstep, 0);
      if (RES == 2) bstore(drr, q1 * g + q2 * rv[e] + q3, vo + e * vstep, 0);
      // (the next base opaque to the compiler, as in tshift_bwd_ra_kernel: no long-lived
      // address register per element)
      l0 += GR * WP;
      asm volatile("" : "+v"(l0));
    }
  } else {
#pragma unroll 1
    for (int e = 0; e < LPT; ++e) {
      const float yy = bload(yr, vo + e * vstep, 0), xx = bload(xr, go + e * vstep, 0);
      float g = shift_in_grad<false>(lds, rg, 0, h0 + e * GR, w, T, V);
      g = d1 * g + d2 * yy + d3;
      g = yy > 0.f ? g : 0.f;
      bstore(dxr, k1 * g + k2 * xx + k3, go + e * vstep, 0);
      if (RES == 1) bstore(drr, g, vo + e * vstep, 0);
      if (RES == 2) bstore(drr, q1 * g + q2 * bload(rr, vo + e * vstep, 0) + q3, vo + e * vstep, 0);
    }
  }
}

// Plane-resident form of gcn_dx_finish_kernel (V <= 64, <= 32 elements per thread): the
// same one-pass assignment (a thread owns destination joint v' and so source joint
// u = (v' - c) mod V: one mask value, one dmask accumulator), with the whole plane's loads
// in flight at once. dx is bit-identical; the plane sums only change order.
template <int NT, int LPT, bool ADD1, bool ADD2, bool PART, int A2M>
__global__ __launch_bounds__(NT) void gcn_dx_finish_ja_kernel(
    const float* __restrict__ dxt, const float* __restrict__ x0, const float* __restrict__ m,
    const float* __restrict__ add1, const float* __restrict__ add2, float* __restrict__ dx,
    float* __restrict__ dmask_part, const float* __restrict__ ps,
    const float* __restrict__ pmean, const float* __restrict__ pinvstd,
    float2* __restrict__ bn_part, int C, int T, int V, const float* __restrict__ add2m,
    int flags) {
  SGCN_CRIT_PRIO();
  __shared__ float s0[NT];
  __shared__ float red[2 * NT / 64];
  const int plane = blockIdx.x, c = plane % C, rc = c % V;
  const int GR = NT / V, NTJ = GR * V, tid = threadIdx.x;
  const bool own = tid < NTJ;
  const int vd = tid % V;
  int us = vd - rc;
  us = us < 0 ? us + V : us;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const unsigned vo = own ? (unsigned)tid * 4u : 0x80000000u, vstep = (unsigned)NTJ * 4u;
  const unsigned pb = (unsigned)P * 4u;
  const unsigned uo = vo + (unsigned)((us - vd) * 4);
  const bool mdx = flags & SGCN_DXF_MASK_DX;
  constexpr bool A2P = A2M == 2;   // add2 holds one value per plane
  float gv[LPT], xq[LPT], a1[ADD1 ? LPT : 1], a2[ADD2 && !A2P ? LPT : 1], a2q[A2M ? LPT : 1];
  float sv[PART ? LPT : 1];
  {
    const auto gr = make_rsrc(dxt + off, pb), xr = make_rsrc(x0 + off, pb);
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      gv[e] = bload(gr, uo + e * vstep, 0);
      xq[e] = bload(xr, vo + e * vstep, 0);
    }
    if (ADD1) {
      const auto ar = make_rsrc(add1 + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) a1[e] = bload(ar, vo + e * vstep, 0);
    }
    if (ADD2 && !A2P) {
      const auto ar = make_rsrc(add2 + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) a2[e] = bload(ar, vo + e * vstep, 0);
    }
    if (A2M) {
      const auto ar = make_rsrc(add2m + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) a2q[e] = bload(ar, vo + e * vstep, 0);
    }
    if (PART) {
      const auto ar = make_rsrc(ps + off, pb);
#pragma unroll
      for (int e = 0; e < LPT; ++e) sv[e] = bload(ar, vo + e * vstep, 0);
    }
  }
  const float mu = m[us * C + c];
  float pm = 0.f, pi = 0.f, a2v = 0.f;
  if (PART) { pm = pmean[c]; pi = pinvstd[c]; }
  if (A2P) a2v = add2[plane];   // (past the plane its mask a2q is 0)
  const auto dxr = make_rsrc(dx + off, pb);
  float acc = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
  for (int e = 0; e < LPT; ++e) {
    float val = gv[e] * mu;
    if (ADD1) val += a1[e];
    if (ADD2) val += A2M ? (a2q[e] > 0.f ? (A2P ? a2v : a2[e]) : 0.f) : a2[e];
    // mdx: dx leaves with the ReLU mask of x0 (the previous unit's output) already applied
    bstore(dxr, (xq[e] > 0.f || !mdx) ? val : 0.f, vo + e * vstep, 0);
    acc = fmaf(gv[e], xq[e], acc);   // past the plane both loads are 0
    if (PART) {
      const float g = xq[e] > 0.f ? val : 0.f;   // x0 = 0 past the plane
      b0 += g;
      b1 = fmaf(g, (sv[e] - pm) * pi, b1);
    }
  }
  if (PART) {
    block_sum2(b0, b1, red);
    if (tid == 0) bn_part[plane] = make_float2(b0, b1);
  }
  s0[tid] = acc;
  __syncthreads();
  if (tid < V) {   // partial of source joint u = tid: its threads have v' = (u + c) mod V
    int vq = tid + rc;
    vq = vq >= V ? vq - V : vq;
    float sum = 0.f;
    for (int g = 0; g < GR; ++g) sum += s0[g * V + vq];
    dmask_part[(size_t)plane * V + tid] = sum;
  }
}

// ------------------------------------------------------------------------------------
// Shift_gcn input side, forward: shift_in gather + feature mask, materialised once
// ------------------------------------------------------------------------------------
// xg[b,c,t,u] = x0[b,c,t,(u + c) mod V] * m[u][c]   (shift_gcn.py:125-129: index_select
// with shift_in, then * (tanh(Feature_Mask) + 1)). The same fp32 product the contraction
// loaders would form per element; read by the forward contraction and the weight
// gradient as a plain plane (no per-element rotation / mask loads in their main loops).
__global__ __launch_bounds__(kThreads) void gcn_gather_kernel(const float* __restrict__ x0,
                                                              const float* __restrict__ m,
                                                              float* __restrict__ xg, int C,
                                                              int T, int V) {
  SGCN_CRIT_PRIO();
  __shared__ float m_s[kThreads];   // this channel's mask column, by joint
  const int plane = blockIdx.x, c = plane % C;
  const int P = T * V;
  const size_t off = (size_t)plane * P;
  const int rc = c % V;
  if ((int)threadIdx.x < V) m_s[threadIdx.x] = m[threadIdx.x * C + c];
  __syncthreads();
  const int dv = kThreads % V;
  int w = threadIdx.x % V;
  for (int base = 0; base < P; base += kThreads * kU) {
    float xv[kU], mv[kU];
    int ww = w;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int oraw = base + u * kThreads + (int)threadIdx.x;
      int src = ww + rc;
      src = src >= V ? src - V : src;
      xv[u] = x0[off + min(oraw - ww + src, P - 1)];
      mv[u] = m_s[ww];
      ww += dv;
      if (ww >= V) ww -= V;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int o = base + u * kThreads + (int)threadIdx.x;
      if (o < P) xg[off + o] = xv[u] * mv[u];
    }
    w = ww;
  }
}

// ------------------------------------------------------------------------------------
// Shift_gcn input-side backward: undo shift_in and the feature mask
// ------------------------------------------------------------------------------------
// dx[b,c,t,v'] = dxt[b,c,t,u]*m[u][c] (+ add1 + add2), u = (v' - c) mod V  (index_select^T)
// dmask_part[b][c][u] = sum_t dxt[b,c,t,u] * x0[b,c,t,(u+c) mod V]
// PART: also the backward partials of the PREVIOUS unit's tail BatchNorm (bn2, whose
// output after residual + ReLU is x0): bn_part[plane] = {sum g, sum g*(s - mean)*invstd},
// g = dx * (x0 > 0), s = that BatchNorm's input (same layout) — what sgcn_bn_bwd_reduce
// would compute from (dx, x0, s) in another pass over three tensors.
// A2M: add2 enters masked, add2 * (add2m > 0) — the identity-residual gradient of a
// TCN_GCN_unit, g = dout * (out > 0), formed here instead of being written by the tail's
// BatchNorm backward.
// flags (wave-uniform, no instantiation of their own): SGCN_DXF_MASK_DX stores
// dx * (x0 > 0), i.e. the previous unit's output gradient with its ReLU mask applied, so
// none of that unit's backward kernels reads its output for the mask (the same
// `x0 > 0 ? val : 0` PART sums; independent of PART). SGCN_DXF_ADD2_PLANE (the masked form
// only; A2M = 2 in the plane-resident kernel, whose add2 load array it drops): add2 holds
// one value per plane (the gradient of a global average pool).
template <bool ADD1, bool ADD2, bool PART, bool A2M = false>
__global__ __launch_bounds__(kThreads) void gcn_dx_finish_kernel(
    const float* __restrict__ dxt, const float* __restrict__ x0, const float* __restrict__ m,
    const float* __restrict__ add1, const float* __restrict__ add2, float* __restrict__ dx,
    float* __restrict__ dmask_part, const float* __restrict__ ps,
    const float* __restrict__ pmean, const float* __restrict__ pinvstd,
    float2* __restrict__ bn_part, int C, int T, int V, const float* __restrict__ add2m,
    int flags) {
  SGCN_CRIT_PRIO();
  const bool mdx = flags & SGCN_DXF_MASK_DX, a2p = flags & SGCN_DXF_ADD2_PLANE;
  // One pass: thread i owns destination joint v' = i % V of rows t = i / V (mod G), so its
  // source joint u = (v' - c) mod V is fixed: one mask value, one dmask accumulator, and
  // the x0 factor of the mask gradient, x0[t, (u + c) mod V] = x0[t, v'], is the element
  // at the thread's own destination address (read once, with add1/add2).
  __shared__ float s0[kThreads];
  const int plane = blockIdx.x, c = plane % C;
  const size_t off = (size_t)plane * T * V;
  const int rc = c % V;
  const int i = threadIdx.x;
  const int G = kThreads / V;
  const int vd = i % V, rr = i / V;
  int us = vd - rc;
  us = us < 0 ? us + V : us;
  const float mu = m[us * C + c];
  float pm = 0.f, pi = 0.f;
  if (PART) { pm = pmean[c]; pi = pinvstd[c]; }
  float acc = 0.f, b0 = 0.f, b1 = 0.f;
  if (i < G * V) {
    for (int t0 = rr; t0 < T; t0 += G * kU) {
      float gv[kU], xq[kU], a1[kU], a2[kU], sv[kU], a2q[kU];
#pragma unroll
      for (int k = 0; k < kU; ++k) {
        const int row = min(t0 + k * G, T - 1) * V;
        gv[k] = dxt[off + row + us];
        xq[k] = x0[off + row + vd];
        if (ADD1) a1[k] = add1[off + row + vd];
        if (ADD2) a2[k] = a2p ? add2[plane] : add2[off + row + vd];
        if (A2M) a2q[k] = add2m[off + row + vd];
        if (PART) sv[k] = ps[off + row + vd];
      }
#pragma unroll
      for (int k = 0; k < kU; ++k) {
        const int t = t0 + k * G;
        float val = gv[k] * mu;
        if (ADD1) val += a1[k];
        if (ADD2) val += A2M ? (a2q[k] > 0.f ? a2[k] : 0.f) : a2[k];
        if (t < T) dx[off + t * V + vd] = (xq[k] > 0.f || !mdx) ? val : 0.f;
        acc += (t < T) ? gv[k] * xq[k] : 0.f;
        if (PART) {
          const float g = (t < T && xq[k] > 0.f) ? val : 0.f;
          b0 += g;
          b1 += g * ((sv[k] - pm) * pi);
        }
      }
    }
  }
  if (PART) {
    __shared__ float red[2 * kThreads / 64];
    block_sum2(b0, b1, red);
    if (i == 0) bn_part[plane] = make_float2(b0, b1);
  }
  s0[i] = acc;
  __syncthreads();
  if (i < V) {   // partial of source joint u = i: its threads have v' = (i + c) mod V
    int vq = i + rc;
    vq = vq >= V ? vq - V : vq;
    float sum = 0.f;
    for (int g = 0; g < G; ++g) sum += s0[g * V + vq];
    dmask_part[(size_t)plane * V + i] = sum;
  }
}

// m = tanh(mask) + 1   (shift_gcn.py:129)
__global__ void mask_prep_kernel(const float* __restrict__ mask, float* __restrict__ m, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) m[i] = tanhf(mask[i]) + 1.f;
}

// every unit's mask prep in one launch (the entries are kernel arguments); blockIdx.y = entry
struct MaskPrepBatch {
  const float* mask[SGCN_BATCH_MAX];
  float* m[SGCN_BATCH_MAX];
  int n[SGCN_BATCH_MAX];
};
__global__ void mask_prep_many_kernel(const MaskPrepBatch t) {
  const int e = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.n[e]) t.m[e][i] = tanhf(t.mask[e][i]) + 1.f;
}

// dmask[u][c] (+)= (sum_b part[b][c][u]) * (1 - tanh(mask)^2); parallel over b
__device__ __forceinline__ void mask_grad_body(const float* __restrict__ part,
                                               const float* __restrict__ mask, int B, int C,
                                               int V, float* __restrict__ dmask,
                                               int accumulate);
__global__ __launch_bounds__(64 * kFW) void mask_grad_finalize_kernel(
    const float* __restrict__ part, const float* __restrict__ mask, int B, int C, int V,
    float* __restrict__ dmask, int accumulate) {
  mask_grad_body(part, mask, B, C, V, dmask, accumulate);
}
// many (the side stream's deferred ones; the entries are kernel arguments)
struct MaskGradBatch {
  const float* part[SGCN_BATCH_MAX];
  const float* mask[SGCN_BATCH_MAX];
  float* dmask[SGCN_BATCH_MAX];
  int B[SGCN_BATCH_MAX];
  int C[SGCN_BATCH_MAX];
  int V[SGCN_BATCH_MAX];
};
__global__ __launch_bounds__(64 * kFW) void mask_grad_finalize_many_kernel(const MaskGradBatch t) {
  const int i = blockIdx.y;
  if ((int)blockIdx.x * kFW >= t.C[i] * t.V[i]) return;
  mask_grad_body(t.part[i], t.mask[i], t.B[i], t.C[i], t.V[i], t.dmask[i], 0);
}
__device__ __forceinline__ void mask_grad_body(const float* __restrict__ part,
                                               const float* __restrict__ mask, int B, int C,
                                               int V, float* __restrict__ dmask,
                                               int accumulate) {
  const int F = C * V;  // part feature f = c*V + u
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * kFW + (int)(threadIdx.x >> 6);
  const int fc = min(f, F - 1);
  double a = 0.0;
  for (int b0 = lane; b0 < B; b0 += 64 * 4) {
    float pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + u * 64;
      pv[u] = b < B ? part[(size_t)b * F + fc] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) a += pv[u];
  }
  const double s = wave_dsum(a);
  if (f >= F || lane != 0) return;
  const int c = f / V, u = f - c * V;
  const int i = u * C + c;
  const float t = tanhf(mask[i]);
  const float g = (float)s * (1.f - t * t);
  dmask[i] = accumulate ? dmask[i] + g : g;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

#define SGCN_PLANE_CHECK() \
  SGCN_REQUIRE(B >= 0 && C > 0 && T >= 0 && V > 0 && V <= kThreads)

// One launch of a BatchNorm plane kernel: the plane-resident joint-aligned kernel `ja` on
// bn_form's (threads, elements per thread), else the looping kernel `loop`; `a` are the
// kernel's flags (dispatch.hpp). False: a flag value outside its set, nothing launched.
template <class J, class L, class... A>
static bool launch_plane(int T, int V, J&& ja, L&& loop, A... a) {
  const LaunchForm f = bn_form(T, V);
  if (f.kind == Kind::ja) return with_form<kJaForms>({f.nt, f.lpt}, ja, a...);
  return with_consts(loop, a...);
}

extern "C" {

size_t sgcn_moments_ws_bytes(int B, int C, int V, int per_joint) {
  return (size_t)B * C * (per_joint ? V : 1) * sizeof(float2);
}

int sgcn_moments(const float* x, float* part, int B, int C, int T, int V, int per_joint,
                 void* stream) {
  SGCN_PLANE_CHECK();
  if (B == 0) return 0;
  SGCN_REQUIRE(x && part && T > 0);
  hipStream_t st = (hipStream_t)stream;
  SGCN_REQUIRE(per_joint == 0 || per_joint == 3);
  auto ja = [&](auto NT, auto LPT, auto PJ) {
    moments_ja_kernel<NT, LPT, PJ, PJ><<<B * C, int(NT), 0, st>>>(x, (float2*)part, T, V, C);
  };
  auto loop = [&](auto PJ) {
    moments_kernel<PJ, PJ><<<B * C, kThreads, 0, st>>>(x, (float2*)part, T, V, C);
  };
  const bool ok = launch_plane(T, V, ja, loop, per_joint == 3);
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_finalize(const float* part, int B, int F, int n_part, int perm_V,
                     const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, long long* num_batches,
                     float* mean, float* invstd, float* scale, float* shift, void* stream) {
  SGCN_REQUIRE(part && B > 0 && F > 0 && n_part > 0 && mean && invstd && scale && shift);
  SGCN_REQUIRE((running_mean == nullptr) == (running_var == nullptr));
  SGCN_REQUIRE(perm_V <= 0 || F % perm_V == 0);
  hipStream_t st = (hipStream_t)stream;
  bn_finalize_kernel<<<(F + 63) / 64, 64 * kFSW, 0, st>>>(
      (const float2*)part, B, F, n_part, perm_V, gamma, beta, eps, momentum, running_mean,
      running_var, num_batches, mean, invstd, scale, shift);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_eval_coef(int F, int perm_V, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, float eps,
                      float* mean, float* invstd, float* scale, float* shift, void* stream) {
  SGCN_REQUIRE(F > 0 && running_mean && running_var && scale && shift);
  SGCN_REQUIRE(perm_V <= 0 || F % perm_V == 0);
  bn_eval_coef_kernel<<<(F + 255) / 256, 256, 0, (hipStream_t)stream>>>(
      F, perm_V, gamma, beta, running_mean, running_var, eps, mean, invstd, scale, shift);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_apply(const float* x, const float* scale, const float* shift, int per_joint,
                  const float* r, const float* rscale, const float* rshift, int relu,
                  float* y, float* y_stats, const float* gather_m, float* y_gathered, int B,
                  int C, int T, int V, void* stream) {
  SGCN_PLANE_CHECK();
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(x && scale && shift && y);
  SGCN_REQUIRE((gather_m == nullptr) == (y_gathered == nullptr));
  SGCN_REQUIRE(!(y_stats && y_gathered) && y_gathered != y);
  SGCN_REQUIRE((rscale == nullptr) == (rshift == nullptr) && (r || !rscale));
  SGCN_REQUIRE(per_joint == 0 || per_joint == 3);
  hipStream_t st = (hipStream_t)stream;
  const int res = r == nullptr ? 0 : (rscale ? 2 : 1);
  dim3 g(B * C);
  float2* ys = (float2*)y_stats;
  if (per_joint == 3) SGCN_REQUIRE(relu && !y_gathered);
  // per_joint == 3: the Shift_gcn tail on the pre-shift_out contraction output (ZU)
  const OneOf<0, 1, 2> rs{res};
  const int ox = ys ? 1 : (y_gathered ? 2 : 0);
  auto ja = [&](auto NT, auto LPT, auto PJ, auto RS, auto RL, auto OX) {
    bn_apply_ja_kernel<NT, LPT, PJ, RS, RL, OX, PJ><<<g, int(NT), 0, st>>>(
        x, scale, shift, r, rscale, rshift, y, ys, gather_m, y_gathered, C, T, V);
  };
  auto loop = [&](auto PJ, auto RS, auto RL, auto OX) {
    bn_apply_kernel<PJ, RS, RL, OX, PJ><<<g, kThreads, 0, st>>>(
        x, scale, shift, r, rscale, rshift, y, ys, gather_m, y_gathered, C, T, V);
  };
  const bool ok =
      per_joint == 3
          ? launch_plane(T, V, ja, loop, Const<true>{}, rs, Const<true>{}, OneOf<0, 1>{ox})
          : launch_plane(T, V, ja, loop, Const<false>{}, rs, relu != 0, OneOf<0, 1, 2>{ox});
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_bwd_reduce(const float* dy, const float* y, int relu, const float* x,
                       const float* mean, const float* invstd, int per_joint, const float* r,
                       const float* rmean,
                       const float* rinvstd, const float* dy_coef, float* part, float* rpart,
                       int B, int C, int T, int V, int dy_plane, void* stream) {
  SGCN_PLANE_CHECK();
  SGCN_REQUIRE(B > 0 && T > 0 && dy && x && mean && invstd && part && (y || !relu));
  const int dyp = dy_plane != 0;
  SGCN_REQUIRE(!dy_coef || (y && relu));
  SGCN_REQUIRE((r == nullptr) == (rpart == nullptr) && (!r || (rmean && rinvstd)));
  SGCN_REQUIRE(per_joint == 0 || per_joint == 3);
  hipStream_t st = (hipStream_t)stream;
  dim3 g(B * C);
  const bool rb = r != nullptr;
  if (per_joint == 3) SGCN_REQUIRE(relu);
  // per_joint == 3: x = the pre-shift_out contraction output (see the kernels)
  const bool dyt = dy_coef != nullptr;
  auto ja = [&](auto NT, auto LPT, auto PJ, auto RL, auto RB, auto DYT) {
    bn_bwd_reduce_ja_kernel<NT, LPT, PJ, RL, RB, DYT><<<g, int(NT), 0, st>>>(
        dy, y, x, mean, invstd, r, rmean, rinvstd, dy_coef, (float2*)part, (float2*)rpart, C, T,
        V, dyp);
  };
  auto loop = [&](auto PJ, auto RL, auto RB, auto DYT) {
    bn_bwd_reduce_kernel<PJ, RL, RB, DYT><<<g, kThreads, 0, st>>>(
        dy, y, x, mean, invstd, r, rmean, rinvstd, dy_coef, (float2*)part, (float2*)rpart, C, T,
        V, dyp);
  };
  const bool ok = per_joint == 3
                      ? launch_plane(T, V, ja, loop, Const<true>{}, Const<true>{}, rb, dyt)
                      : launch_plane(T, V, ja, loop, Const<false>{}, relu != 0, rb, dyt);
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_bwd_finalize(const float* part, int B, int F, long long n_total, int perm_V,
                         const float* mean, const float* invstd, const float* gamma,
                         float* dgamma, float* dbeta, int accumulate, int batch_stats,
                         float* coef, void* stream) {
  SGCN_REQUIRE(part && B > 0 && F > 0 && n_total > 0 && mean && invstd && coef);
  SGCN_REQUIRE(perm_V <= 0 || F % perm_V == 0);
  bn_bwd_finalize_kernel<<<(F + 63) / 64, 64 * kFSW, 0, (hipStream_t)stream>>>(
      (const float2*)part, B, F, (double)n_total, perm_V, mean, invstd, gamma, dgamma, dbeta,
      accumulate, batch_stats, coef);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_bwd_finalize_gbn(const float* part6, int B, int C, int V, long long n_total,
                             const float* dy_coef, const float* dy_mean, const float* mean,
                             const float* invstd, const float* gamma, float* dgamma,
                             float* dbeta, int accumulate, int batch_stats, float* coef,
                             void* stream) {
  SGCN_REQUIRE(part6 && B > 0 && C > 0 && V > 0 && n_total > 0 && dy_coef && dy_mean && mean &&
               invstd && coef);
  const int F = C * V;
  bn_bwd_finalize_gbn_kernel<<<(F + 63) / 64, 64 * kGbnW, 0, (hipStream_t)stream>>>(
      part6, B, F, V, (double)n_total, dy_coef, dy_mean, C, mean, invstd, gamma, dgamma, dbeta,
      accumulate, batch_stats, coef);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_bwd_apply(const float* dy, const float* y, int relu, const float* x,
                      const float* coef, int per_joint, const float* r, const float* rcoef,
                      const float* dy_coef, float* dx, float* dr, int B, int C, int T, int V,
                      void* stream) {
  SGCN_PLANE_CHECK();
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(dy && x && coef && dx && (y || !relu));
  SGCN_REQUIRE(!dy_coef || (y && relu));
  SGCN_REQUIRE(!rcoef || (r && dr));
  SGCN_REQUIRE(per_joint == 0 || per_joint == 3);
  hipStream_t st = (hipStream_t)stream;
  const int res = dr == nullptr ? 0 : (rcoef ? 2 : 1);
  const int F = per_joint ? C * V : C;
  dim3 g(B * C);
  if (per_joint == 3) SGCN_REQUIRE(relu);
  const OneOf<0, 1, 2> rs{res};
  const bool dyt = dy_coef != nullptr;
  auto ja = [&](auto NT, auto LPT, auto PJM, auto RL, auto RS, auto DYT) {
    bn_bwd_apply_ja_kernel<NT, LPT, PJM, RL, RS, DYT><<<g, int(NT), 0, st>>>(
        dy, y, x, coef, F, r, rcoef, C, dy_coef, dx, dr, C, T, V);
  };
  auto loop = [&](auto PJM, auto RL, auto RS, auto DYT) {
    bn_bwd_apply_kernel<PJM, RL, RS, DYT><<<g, kThreads, 0, st>>>(
        dy, y, x, coef, F, r, rcoef, C, dy_coef, dx, dr, C, T, V);
  };
  const bool ok = per_joint == 3
                      ? launch_plane(T, V, ja, loop, Const<3>{}, Const<true>{}, rs, dyt)
                      : launch_plane(T, V, ja, loop, Const<0>{}, relu != 0, rs, dyt);
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_bn_bwd_apply_tsh(const float* gout, const float* xpos, const float* ypos,
                          const float* y, const float* x, const float* coef, const float* r,
                          const float* rcoef, const float* dy_coef, float* dx, float* dr, int B,
                          int C, int T, int V, void* stream) {
  SGCN_REQUIRE(B > 0 && C > 0 && T > 0 && V > 0);
  SGCN_REQUIRE(gout && xpos && ypos && y && x && coef && dy_coef && dx && dr);
  SGCN_REQUIRE((r == nullptr) == (rcoef == nullptr));
  SGCN_REQUIRE((long long)B * C < (1LL << 31));
  // the planes and the (threads, elements per thread) of sgcn_tshift_bwd_gbn, whose staging
  // this is (caller falls back to the stored gradient: ops.ra_fits)
  const LaunchForm f = gbn_form(T, V, r != nullptr);
  SGCN_REQUIRE(f.kind == Kind::ra);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = ra_lds_bytes(T, V, f.nt, false);
  auto go = [&](auto NT, auto LPT, auto RES) {
    bn_bwd_apply_tsh_kernel<NT, LPT, RES><<<B * C, int(NT), lds, st>>>(
        gout, xpos, ypos, y, x, coef, C * V, r, rcoef, C, dy_coef, dx, dr, C, T, V);
  };
  const bool ok = r ? with_form<kGbdForms>({f.nt, f.lpt}, go, Const<2>{})
                    : with_form<kRaForms>({f.nt, f.lpt}, go, Const<1>{});
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_mask_prep(const float* mask, float* m, int n, void* stream) {
  SGCN_REQUIRE(mask && m && n > 0);
  mask_prep_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(mask, m, n);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_mask_prep_many(const float* const* mask, float* const* m, const int* count, int n,
                        void* stream) {
  SGCN_REQUIRE(n >= 0 && n <= SGCN_BATCH_MAX);
  if (n == 0) return 0;
  SGCN_REQUIRE(mask && m && count);
  MaskPrepBatch t{};
  int mx = 0;
  for (int i = 0; i < n; ++i) {
    SGCN_REQUIRE(mask[i] && m[i] && count[i] > 0);
    t.mask[i] = mask[i];
    t.m[i] = m[i];
    t.n[i] = count[i];
    mx = max(mx, count[i]);
  }
  mask_prep_many_kernel<<<dim3((mx + 255) / 256, n), 256, 0, (hipStream_t)stream>>>(t);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_mask_grad_finalize_many(const float* const* part, const float* const* mask,
                                 float* const* dmask, const int* B, const int* C,
                                 const int* V, int n, void* stream) {
  SGCN_REQUIRE(n >= 0 && n <= SGCN_BATCH_MAX);
  if (n == 0) return 0;
  SGCN_REQUIRE(part && mask && dmask && B && C && V);
  MaskGradBatch t{};
  int mf = 0;
  for (int i = 0; i < n; ++i) {
    SGCN_REQUIRE(part[i] && mask[i] && dmask[i] && B[i] > 0 && C[i] > 0 && V[i] > 0);
    t.part[i] = part[i];
    t.mask[i] = mask[i];
    t.dmask[i] = dmask[i];
    t.B[i] = B[i];
    t.C[i] = C[i];
    t.V[i] = V[i];
    mf = max(mf, C[i] * V[i]);
  }
  mask_grad_finalize_many_kernel<<<dim3((mf + kFW - 1) / kFW, n), 64 * kFW, 0,
                                   (hipStream_t)stream>>>(t);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_gcn_gather(const float* x0, const float* m, float* xg, int B, int C, int T, int V,
                    void* stream) {
  SGCN_PLANE_CHECK();
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(x0 && m && xg && x0 != xg);
  gcn_gather_kernel<<<B * C, kThreads, 0, (hipStream_t)stream>>>(x0, m, xg, C, T, V);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_gcn_dx_finish(const float* dxt, const float* x0, const float* m, const float* add1,
                       const float* add2, const float* add2_mask, float* dx, float* dmask_part,
                       const float* prev_s, const float* prev_mean, const float* prev_invstd,
                       float* prev_part, int B,
                       int C, int T, int V, int flags, void* stream) {
  SGCN_PLANE_CHECK();
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(dxt && x0 && m && dx && dmask_part);
  SGCN_REQUIRE((flags & ~(SGCN_DXF_MASK_DX | SGCN_DXF_ADD2_PLANE)) == 0);
  SGCN_REQUIRE(!(flags & SGCN_DXF_ADD2_PLANE) || add2_mask);   // the masked (identity-unit) form
  SGCN_REQUIRE(!prev_part || (prev_s && prev_mean && prev_invstd));
  SGCN_REQUIRE(!add2_mask || add2);
  hipStream_t st = (hipStream_t)stream;
  float2* pp = (float2*)prev_part;
  if (add2_mask) SGCN_REQUIRE(add1);
  // add2_mask: the identity-unit form (add1 given, add2 masked by add2_mask). (Plane-resident,
  // it holds ~200 VGPRs at 256 x 32 — two workgroups per CU — but 512 x 16, twice the waves,
  // measured 2 % slower: profiles/r05_ar/ab_dx_finish_512.txt)
  const bool a1 = add1 != nullptr, a2 = add2 != nullptr, pt = pp != nullptr;
  auto ja = [&](auto NT, auto LPT, auto A1, auto A2, auto PT, auto A2M) {
    gcn_dx_finish_ja_kernel<NT, LPT, A1, A2, PT, A2M><<<B * C, int(NT), 0, st>>>(
        dxt, x0, m, add1, add2, dx, dmask_part, prev_s, prev_mean, prev_invstd, pp, C, T, V,
        add2_mask, flags);
  };
  auto loop = [&](auto A1, auto A2, auto PT, auto A2M) {
    gcn_dx_finish_kernel<A1, A2, PT, A2M != 0><<<B * C, kThreads, 0, st>>>(
        dxt, x0, m, add1, add2, dx, dmask_part, prev_s, prev_mean, prev_invstd, pp, C, T, V,
        add2_mask, flags);
  };
  // A2M: 0 no mask, 1 add2 masked per element, 2 add2 holds one value per plane
  const bool ok = add2_mask ? launch_plane(T, V, ja, loop, Const<true>{}, Const<true>{}, pt,
                                           OneOf<1, 2>{flags & SGCN_DXF_ADD2_PLANE ? 2 : 1})
                            : launch_plane(T, V, ja, loop, a1, a2, pt, Const<0>{});
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_mask_grad_finalize(const float* part, const float* mask, int B, int C, int V,
                            float* dmask, int accumulate, void* stream) {
  SGCN_REQUIRE(part && mask && dmask && B > 0 && C > 0 && V > 0);
  mask_grad_finalize_kernel<<<(C * V + kFW - 1) / kFW, 64 * kFW, 0,
                              (hipStream_t)stream>>>(part, mask, B, C, V, dmask, accumulate);
  SGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
