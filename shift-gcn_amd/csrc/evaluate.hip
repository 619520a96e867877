// The evaluation phase on the device (main.py:450-515, ensemble.py:18-32): from a batch of
// class scores and its labels, ONE launch forms per sample the weighted score fusion, the
// cross-entropy loss, the prediction and the rank of the label, and counts top-k hits, the
// confusion matrix and out-of-range labels; a second small launch sums the batch's losses.
// sgcn_ce_bwd is the loss's backward. Every expression is written here (nothing borrowed
// from a library kernel), with no contraction anywhere in this file's own arithmetic.
//
// Per sample i (r = the row the metrics are taken of, C values):
//   fusion  S == 1: r = scores[0][i]. S > 1: r[c] = ((s0*a0 + s1*a1) + s2*a2) + ..., left to
//           right, every product and sum rounded once in the scores' type (a_k = alpha[k]
//           rounded to that type): ensemble.py:27 evaluated on numpy arrays of that type.
//   loss    loss = logsumexp(r) - r[label], the maximum subtracted first, with exp, the sum and
//           log in float64 whatever the scores' type: m = max_c r[c] at p = pred,
//           s = sum_{c != p} exp(r[c] - m), lse = m + log1p(s), loss = log1p(s) + (m - r[l]).
//           log(1 + s) is taken as log1p and the label's own term as the exact difference
//           m - r[l] >= 0, so no term cancels and the loss keeps its relative accuracy down
//           to the smallest values (a confident, correct row at scores of +-1e4 has a loss
//           far below the spacing of lse). The sum runs over a lane's classes c = lane,
//           lane + 64, ... in order, then a fixed xor tree over the lanes: the same bits on
//           every run.
//   pred    the FIRST index of the maximum (np.argmax, torch.max on the CPU).
//   rank    #{c : r[c] > r[l]} + #{c > l : r[c] == r[l]}: the position of the label from the
//           top of np.argsort(r, kind="stable"), so `rank < k` is
//           `label in np.argsort(r, kind="stable")[-k:]`. Feeder.top_k (feeder.py:92-95) sorts
//           with numpy's default, unstable kind: the two agree on rows without ties, and may
//           differ where the label ties with the k-th score.
//   a label outside [0, C) indexes nothing: loss = NaN, rank = C, no confusion entry, one more
//           in bad_labels (lse and pred are still those of the row).
// NaN or Inf scores are outside the contract (the values stored are then unspecified), but
// every index is clamped, so nothing is read or written out of bounds.
//
// Launch: one wavefront per sample, 4 per workgroup; a lane walks the classes lane,
// lane + 64, ... (C = 60: one value per lane; C = 2 leaves lanes idle). The integer counters
// are summed per workgroup in LDS and added with one device atomic per counter (integer
// adds commute: the totals do not depend on arrival order); confusion[label][pred] takes one
// atomic per sample. No floating-point atomics anywhere.
#include "common.hpp"

#include <limits.h>

namespace sgcn {
namespace {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / kWave;
constexpr int kLossThreads = 256;

struct EvalArgs {
  double alpha[SGCN_EVAL_MAX_STREAMS];
  int k[SGCN_EVAL_MAX_K];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// r[c] of one sample: `row` points at scores[0][i][0], `stride` is the stream stride
template <typename T>
__device__ __forceinline__ T fused_at(const T* __restrict__ row, long long stride, int S,
                                      const EvalArgs& a, int c) {
#pragma clang fp contract(off)
  if (S == 1) return row[c];
  T r = row[c] * (T)a.alpha[0];
  for (int s = 1; s < S; ++s) {
    const T p = row[(size_t)s * stride + c] * (T)a.alpha[s];
    r = r + p;
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(kEvalThreads) void score_metrics_kernel(
    const T* __restrict__ scores, long long stride, int S, EvalArgs args,
    const long long* __restrict__ labels, int n, int C, long long off, T* __restrict__ fused,
    double* __restrict__ loss, double* __restrict__ lse, int* __restrict__ pred,
    int* __restrict__ rank, int nk, int* __restrict__ hits, int* __restrict__ confusion,
    int* __restrict__ bad_labels) {
#pragma clang fp contract(off)
  __shared__ int cnt[SGCN_EVAL_MAX_K + 1];   // this workgroup's hits per k, then bad labels
  if (threadIdx.x <= SGCN_EVAL_MAX_K) cnt[threadIdx.x] = 0;
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * kEvalWaves + wid;
  if (i < n) {   // wave-uniform
    const T* row = scores + (size_t)i * C;
    const long long l = labels[i];
    const bool valid = l >= 0 && l < C;
    const int lc = valid ? (int)l : 0;   // never indexes with a bad label

    // pass 1: the fused row (stored when asked for), its maximum and the first index of it
    T best = (T)0;
    int bidx = INT_MAX;
    for (int c = lane; c < C; c += kWave) {
      const T r = fused_at(row, stride, S, args, c);
      if (fused) fused[(size_t)(off + i) * C + c] = r;
      if (bidx == INT_MAX || r > best) {
        best = r;
        bidx = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const T ob = __shfl_xor(best, o, kWave);
      const int oi = __shfl_xor(bidx, o, kWave);
      // a lane without a class holds INT_MAX and loses; equal values keep the lower index
      if (oi != INT_MAX && (bidx == INT_MAX || ob > best || (ob == best && oi < bidx))) {
        best = ob;
        bidx = oi;
      }
    }
    // (NaN scores can leave the lanes disagreeing: take lane 0's, clamped into the row)
    const int p = min(max(__shfl(bidx, 0, kWave), 0), C - 1);
    const double m = (double)__shfl(best, 0, kWave);
    const T rl = fused_at(row, stride, S, args, lc);

    // pass 2: sum of exp(r - m) over c != p in float64, and the label's rank
    double se = 0.0;
    int above = 0;
    for (int c = lane; c < C; c += kWave) {
      const T r = fused_at(row, stride, S, args, c);
      if (c != p) se += exp((double)r - m);
      above += (r > rl || (r == rl && c > lc)) ? 1 : 0;
    }
    se = wave_sum_f64(se);
    above = wave_sum_i32(above);

    if (lane == 0) {
      const double l1p = log1p(se);
      const int rk = valid ? above : C;
      lse[off + i] = m + l1p;
      loss[off + i] = valid ? l1p + (m - (double)rl) : __builtin_nan("");
      if (pred) pred[off + i] = p;
      if (rank) rank[off + i] = rk;
      if (valid) {
        if (confusion) atomicAdd(&confusion[(size_t)lc * C + p], 1);
        for (int j = 0; j < nk; ++j)
          if (rk < args.k[j]) atomicAdd(&cnt[j], 1);
      } else {
        atomicAdd(&cnt[SGCN_EVAL_MAX_K], 1);
      }
    }
  }
  __syncthreads();
  // one device-scope integer atomic per counter and workgroup
  const int t = threadIdx.x;
  if (t < nk && hits && cnt[t]) atomicAdd(&hits[t], cnt[t]);
  if (t == SGCN_EVAL_MAX_K && bad_labels && cnt[t]) atomicAdd(bad_labels, cnt[t]);
}

// mean of loss[0..n) in a fixed tree: thread t sums t, t + 256, ... in order, the lanes of a
// wave in an xor tree, the 4 waves in order
__global__ __launch_bounds__(kLossThreads) void batch_loss_kernel(
    const double* __restrict__ loss, int n, double* __restrict__ out,
    float* __restrict__ out_f32) {
#pragma clang fp contract(off)
  __shared__ double red[kLossThreads / kWave];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kLossThreads) s += loss[i];
  s = wave_sum_f64(s);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = red[0];
    for (int w = 1; w < kLossThreads / kWave; ++w) tot += red[w];
    const double mean = tot / (double)n;
    if (out) *out = mean;
    if (out_f32) *out_f32 = (float)mean;
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(
    const float* __restrict__ logits, const double* __restrict__ lse,
    const long long* __restrict__ labels, const float* __restrict__ g,
    float* __restrict__ dlogits, int n, int C) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * C) return;
  const int i = (int)(e / C), c = (int)(e - (long long)i * C);
  const long long l = labels[i];
  float d = 0.f;
  if (l >= 0 && l < C) {
    const double p = exp((double)logits[e] - lse[i]);
    d = (float)((p - (c == l ? 1.0 : 0.0)) * (double)g[0] / (double)n);
  }
  dlogits[e] = d;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" {

int sgcn_score_metrics(const void* scores, long long stream_stride, int S, const double* alpha,
                       int f64, const long long* labels, int n, int C, long long row_offset,
                       void* fused, double* loss, double* lse, int* pred, int* rank,
                       const int* k, int nk, int* hits, int* confusion, int* bad_labels,
                       void* stream) {
  SGCN_REQUIRE(scores && labels && loss && lse);
  SGCN_REQUIRE(C >= 1 && n >= 0 && row_offset >= 0);
  SGCN_REQUIRE(S >= 1 && S <= SGCN_EVAL_MAX_STREAMS);
  SGCN_REQUIRE(nk >= 0 && nk <= SGCN_EVAL_MAX_K);
  if (S > 1) SGCN_REQUIRE(alpha && stream_stride >= (long long)n * C);
  if (nk > 0) SGCN_REQUIRE(k && hits);
  SGCN_REQUIRE(f64 == 0 || f64 == 1);
  // confusion's (C, C) index stays in int range
  SGCN_REQUIRE((long long)C * C <= 0x7fffffffLL);
  if (n == 0) return 0;
  EvalArgs args = {};
  for (int s = 0; s < S && alpha; ++s) args.alpha[s] = alpha[s];
  for (int j = 0; j < nk; ++j) args.k[j] = k[j];
  const unsigned grid = (unsigned)(((long long)n + kEvalWaves - 1) / kEvalWaves);
  if (f64)
    score_metrics_kernel<double><<<grid, kEvalThreads, 0, (hipStream_t)stream>>>(
        (const double*)scores, stream_stride, S, args, labels, n, C, row_offset, (double*)fused,
        loss, lse, pred, rank, nk, hits, confusion, bad_labels);
  else
    score_metrics_kernel<float><<<grid, kEvalThreads, 0, (hipStream_t)stream>>>(
        (const float*)scores, stream_stride, S, args, labels, n, C, row_offset, (float*)fused,
        loss, lse, pred, rank, nk, hits, confusion, bad_labels);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_batch_loss(const double* loss, long long row_offset, int n, double* batch_loss,
                    long long batch_idx, float* mean_f32, void* stream) {
  SGCN_REQUIRE(loss && (batch_loss || mean_f32));
  SGCN_REQUIRE(n >= 0 && row_offset >= 0 && batch_idx >= 0);
  if (n == 0) return 0;
  batch_loss_kernel<<<1, kLossThreads, 0, (hipStream_t)stream>>>(
      loss + row_offset, n, batch_loss ? batch_loss + batch_idx : nullptr, mean_f32);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_ce_bwd(const float* logits, const double* lse, const long long* labels, const float* g,
                float* dlogits, int n, int C, void* stream) {
  SGCN_REQUIRE(logits && lse && labels && g && dlogits);
  SGCN_REQUIRE(C >= 1 && n >= 0);
  if (n == 0) return 0;
  const long long blocks = ((long long)n * C + 255) / 256;
  SGCN_REQUIRE(blocks <= 0x7fffffffLL);
  ce_bwd_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(logits, lse, labels, g,
                                                                    dlogits, n, C);
  SGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
