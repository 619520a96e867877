// Pointwise (1x1) channel contractions of the Shift-GCN hot path on fp32 MFMA (gfx950).
//
// Every "trailing pointwise conv" of the reference is one C_in x C_out contraction over
// P = N·M·T·V positions of the (N·M, C, T, V) layout:
//   Shift_gcn : einsum('nwc,cd->nwd') between the two joint-shift gathers
//               (model/shift_gcn.py:125-136), + Linear_bias
//   Shift_tcn : temporal_linear Conv2d(C, C, 1) (shift_gcn.py:62,69)
//   down / residual tcn(k=1, stride s) Conv2d (shift_gcn.py:84, 35-36)
// The joint-shift gathers (index_select with shift_in / shift_out, shift_gcn.py:108-118,
// 127, 136) and the feature mask are NOT separate passes here: shift_in + mask are
// applied while staging the B operand (a per-channel rotation inside each V-row), and
// shift_out is applied in the epilogue's store addresses (rotation by the output
// channel). No permute to (n·t, v·c) is ever materialised.
//
// Kernels
//  * pwg_fwd_kernel : Y[b][m][pos_out(n,m)] (+)= act(sum_k A[m][k] * Bop(b,k,n) + bias[m])
//      used for the forward (A = weights) and for dX (A = weights^T). Positions are
//      flattened over (sample, t, v); one tile = all M (<= 256) x BN positions, so the X
//      operand crosses HBM exactly once in long contiguous runs per channel row.
//      v_mfma_f32_32x32x2_f32 (exact f32, one rounding per product == an fmaf chain),
//      BK = 16 double-buffered LDS stages (one barrier per stage), register prefetch of
//      the next stage's global loads while the current stage's MFMAs issue.
//  * pw_dw_kernel  : split-K dW[m][n] = sum_{b,p} G(b,m,p) * X(b,n,p) over all positions,
//      deterministic fp32 partial slabs [split][M][N] + row sums (bias grad), reduced in
//      fixed order by slab_reduce_kernel (optionally transposed, for Linear_weight's
//      (C_in, C_out) layout).
#include <type_traits>

#include "common.hpp"
#include "dispatch.hpp"
#include "pw_forms.hpp"

namespace sgcn {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// A position-mapped plane operand: element (b, ch, n) with n = t*V + v (logical
// position) lives at ptr[b*bstride + ch*cstride + (t*tstride)*V + rot(v, ch)], where
// rot(v, ch) = (v + rsign*ch) mod V.
struct Plane {
  const float* ptr;
  long long bstride;
  long long cstride;
  int tstride;
  int rsign;
};

struct OutPlane {
  float* ptr;
  long long bstride;
  long long cstride;
  int tstride;
  int rsign;
};

// Exact unsigned division by a runtime divisor d >= 1 for dividends n < 2^31: with
// l = ceil(log2 d) and m = floor(2^32 (2^l - d) / d) + 1, n / d = (umulhi(m, n) + n) >> l
// (the sum stays below 2^32 because n < 2^31 and umulhi(m, n) < n).
struct FastDiv {
  unsigned m, s;
};
inline FastDiv fast_div(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  const unsigned long long m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
  return {(unsigned)m, l};
}
__device__ __forceinline__ int fdiv(int n, unsigned m, unsigned s) {
  const unsigned u = (unsigned)n;
  return (int)((__umulhi(m, u) + u) >> s);
}

struct FwdArgs {
  const float* A;   // weights
  int lda;
  int a_mcontig;    // A[m][k] = a_mcontig ? A[k*lda+m] : A[m*lda+k]
  const float* bias;
  Plane x;
  const float* mask;  // optional mask[v*K + k] multiplied into B (Shift_gcn feature mask)
  const int* ts;      // TSH: per-channel temporal-shift table (tshift_params_kernel), K x 12
  float* xs;          // TSH (optional): also store the shifted operand (layout of x)
  OutPlane y;
  int M, K, T, V;
  int B;
  // exact division by N = T*V and by V (FastDiv, set by fwd_divisors): the per-column
  // (sample, t, v) decomposition without a ~35-instruction integer division each
  unsigned divN_m, divN_s, divV_m, divV_s;
  // byte extents of the operands (buffer-descriptor ranges: an offset at or past the
  // extent loads 0 / drops the store) and epilogue flags
  unsigned x_bytes, y_bytes, a_bytes, mask_bytes;
  int relu;
};

// the FastDiv constants of a.T * a.V and a.V (every FwdArgs launch sets them)
inline void fwd_divisors(FwdArgs& a) {
  const FastDiv n = fast_div((unsigned)(a.T * a.V)), v = fast_div((unsigned)a.V);
  a.divN_m = n.m;
  a.divN_s = n.s;
  a.divV_m = v.m;
  a.divV_s = v.s;
}

// Diagnostic builds only (tools/bench/pwbench -DSGCN_PW_STAMPS): per-workgroup cycle
// stamps of the forward contraction's phases, written by one lane to a debug buffer that
// nothing else reads. Compiled out of the product library.
#ifdef SGCN_PW_STAMPS
__device__ unsigned long long* g_pw_stamps;
__device__ unsigned long long* g_pw_where;
#define SGCN_PW_STAMP(i)                                                                  \
  do {                                                                                    \
    if (threadIdx.x == 0) {                                                               \
      const size_t wgi = (size_t)blockIdx.y * gridDim.x + blockIdx.x;                     \
      g_pw_stamps[wgi * 4 + (i)] = __builtin_amdgcn_s_memtime();                          \
      /* where the workgroup runs: HW_ID (CU / SH / SE) and XCC_ID */                     \
      if ((i) == 0 && g_pw_where)                                                         \
        g_pw_where[wgi] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) |  \
                          (unsigned)__builtin_amdgcn_s_getreg(63492);                     \
    }                                                                                     \
  } while (0)
#else
#define SGCN_PW_STAMP(i) do {} while (0)
#endif
// Diagnostic builds only (tools/bench/pwbench -DSGCN_PW_DIAG=n): drop parts of the forward
// contraction's main loop to see what each costs (results are then wrong): 1 = no A
// staging after stage 0, 2 = no B staging after stage 0, 3 = neither
// (profiles/r03_pw/staging_cost.txt).
#ifndef SGCN_PW_DIAG
#define SGCN_PW_DIAG 0
#endif
// Cache policy of the forward contraction's plain X-operand loads and of its weight loads
// (the aux operand of the buffer loads: 0 default, 2 nt, 16 sc1): tuning knobs
// (tools/bench/ofetch), results unchanged.
#ifndef SGCN_PW_XPOL
#define SGCN_PW_XPOL 0
#endif
#ifndef SGCN_PW_APOL
#define SGCN_PW_APOL 0
#endif

// XCD-aware tile order (cdna_hip_programming.md T1): workgroups are dealt round-robin over
// the 8 XCDs, each with its own L2. Consecutive position tiles share the 128-B lines at
// their edges (a tile's row segment is BN*4 bytes at an arbitrary 4-B alignment: planes are
// T*V floats), so tile i and i+1 on different XCDs fetch those lines twice (PMC, forward
// contraction: 1.12x the operand bytes at BN = 256, 1.28-1.30x at BN = 128,
// profiles/r04_ofetch/). Remapped, the workgroups of one XCD take one contiguous run of
// tiles (bijective for any count). Speed only.
#ifndef SGCN_PW_XCD
#define SGCN_PW_XCD 1
#endif
#ifndef SGCN_DW_XCD
#define SGCN_DW_XCD 1
#endif
template <bool ON = true>
__device__ __forceinline__ int xcd_tile(int b, int n) {
  if (!ON || n <= 8) return b;
  const int q = n >> 3, r = n & 7, x = b & 7, i = b >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

__device__ __forceinline__ int pmod(int a, int V) {
  int r = a % V;
  return r < 0 ? r + V : r;
}

// keep v where ok, exact +0 elsewhere: a bit-AND the compiler cannot turn back into a
// branch around the (always in-bounds) load
__device__ __forceinline__ float keep(float v, bool ok) {
  return __uint_as_float(__float_as_uint(v) & (ok ? 0xffffffffu : 0u));
}

// rotation step (d*rsign) mod V in [0, V)
__device__ __forceinline__ int rot_step(int d, int rsign, int V) { return pmod(d * rsign, V); }

// ------------------------------------------------------------------------------------
// Temporal shift fused into a contraction operand (Shift_tcn: bn -> shift_in ->
// temporal_linear, shift_gcn.py:66-69). The operand element (k, t, v) is
//   shift_k(a_k * H[k] + b_k)[t, v]     (stride 1, shift_cuda_kernel.cu:11-76)
// formed from four taps of H while the operand tile is staged, with exactly the
// arithmetic of tshift.hip's AFFINE path (per-tap multiply then add, zero outside the
// plane, the .cu:73 blend in order, no contraction), so it is bit-identical to writing
// the shifted tensor with sgcn_tshift_fwd and contracting it. Per-channel geometry comes
// from a table (12 words per channel, 48-byte rows for scalar loads):
//   [0] off = y1*V + x1, [1] y1, [2] x1, [3] dx, [4] dy, [5] a, [6] b,
//   [7] two-row channel (below), [8] y1*V, [9] 1 - dy
//
// Two-row channels (round 6, verdict r05 x1). The blend of .cu:73 in float is
//   q11*(1-dx)*(1-dy) + q21*dx*(1-dy) + q12*(1-dx)*dy + q22*dx*dy.
// For x = xpos in (-2^-25, 0): x1 = -1 and dx = x + 1 rounds to exactly 1.0f, so 1-dx = 0,
// q11 and q12 only add zeros and q21*dx = q21, q22*dx = q22: the value IS
// q21*(1-dy) + q22*dy with q21, q22 on the element's own column. For x = 0: x1 = 0, dx = 0,
// and it is q11*(1-dy) + q12*dy, the same two taps. Those channels (about half of a freshly
// initialised model's: xpos starts in U(-1e-8, 1e-8), model/Temporal_shift/cuda/shift.py:42,
// and its gradient is exactly +-0, .cu:386, so only weight decay moves it, towards 0; the
// positive half takes mode 2, below) need two taps of one column
// instead of four: half the bytes returned into VGPRs and a third of the VALU, which on
// gfx950 is what the fused operand costs against the fp32 MFMA (profiles/r05_dma2/).
// Bit-identical to the four-tap form (up to the sign of an exact zero). With mode 2 the
// channels with 0 < x < 2^-25 (1-dx rounds to 1) take it too, dropping the q21*dx and
// q22*dx terms (|dx| < 2^-25; tested within 2e-7 * max|q| of the exact value, north_star's
// 1e-5).
// The choice is per launch: the table kernel also writes one flag, set when EVERY channel
// qualifies, which the contraction reads once at its start (a per-row choice costs a
// scalar-load wait per operand row inside the main loop: measured 2x slower); a launch with
// any other channel takes the four-tap form for all.
// ------------------------------------------------------------------------------------
constexpr int kTsWords = 12;

__device__ __forceinline__ float ts_tap(float q, float a, float b, bool ok) {
#pragma clang fp contract(off)
  const float v = q * a + b;
  return ok ? v : 0.f;
}

__device__ __forceinline__ float ts_blend(float q11, float q21, float q12, float q22, float dx,
                                          float dy) {
#pragma clang fp contract(off)
  const float omdx = 1.f - dx, omdy = 1.f - dy;
  return q11 * omdx * omdy + q21 * dx * omdy + q12 * omdx * dy + q22 * dx * dy;
}

// the two-row channels' blend: q21*(1-dy) + q22*dy (omdy = 1 - dy from the table)
__device__ __forceinline__ float ts_blend2(float q0, float q1, float omdy, float dy) {
#pragma clang fp contract(off)
  return q0 * omdy + q1 * dy;
}

// per-channel table: x1 = floorf(x), dx = x - x1 (.cu:49-71), same for y (stride 1: no
// +0.5, shift.py:17-18 applies to stride != 1 only)
__global__ void tshift_params_kernel(const float* __restrict__ xpos,
                                     const float* __restrict__ ypos,
                                     const float* __restrict__ scale,
                                     const float* __restrict__ shift, int K, int V,
                                     int two_row, int* __restrict__ tab) {
#pragma clang fp contract(off)
  SGCN_CRIT_PRIO();
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const float x = xpos[k], y = ypos[k];
  const int x1 = (int)floorf(x), y1 = (int)floorf(y);
  const float dx = x - (float)x1, dy = y - (float)y1;
  int* r = tab + k * kTsWords;
  r[0] = y1 * V + x1;
  r[1] = y1;
  r[2] = x1;
  r[3] = __float_as_int(dx);
  r[4] = __float_as_int(dy);
  r[5] = __float_as_int(scale ? scale[k] : 1.f);
  r[6] = __float_as_int(shift ? shift[k] : 0.f);
  // two-row channel: exact (x1 = -1 with 1 - dx == 0, or dx == 0), or with mode 2 also
  // x1 = 0 with 1 - dx == 1 (the dropped terms weigh dx < 2^-25)
  const bool exact2 = (x1 == -1 && 1.f - dx == 0.f) || (x1 == 0 && dx == 0.f);
  const bool approx2 = two_row >= 2 && x1 == 0 && 1.f - dx == 1.f;
  r[7] = two_row >= 1 && (exact2 || approx2) ? 1 : 0;
  r[8] = y1 * V;
  r[9] = __float_as_int(1.f - dy);
  for (int i = 10; i < kTsWords; ++i) r[i] = 0;
}

// the launch's two-row flag (tab[K * kTsWords]): every channel two-row (one workgroup)
__global__ __launch_bounds__(256) void tshift_two_row_flag_kernel(int K,
                                                                  int* __restrict__ tab) {
  SGCN_CRIT_PRIO();
  const int k = threadIdx.x;
  const int all = __syncthreads_and(k >= K || tab[k * kTsWords + 7] != 0);
  if (k == 0) tab[K * kTsWords] = all;
}

// ------------------------------------------------------------------------------------
// forward / dX. Positions are flattened over (sample, t, v) so a tile may span samples;
// one tile = all M (<= BM) x BN positions, so X crosses HBM once in long contiguous
// runs per channel row; BK = 16 double-buffered LDS stages, one barrier per stage.
// The main loop is VALU-lean: on gfx950 the f32 MFMA
// runs on the vector ALU: every VALU instruction between MFMAs costs MFMA issue time
// (measured: 2 v_fma per v_mfma_f32_32x32x2_f32 -> -15 %, 8 -> -35 %). So operands
// are fetched with buffer loads whose per-lane byte offset is fixed for the whole tile
// (the (sample, t[, v]) column) and whose row offset (channel, K-stage) is a wave-
// uniform SGPR soffset; bounds come from the descriptor range (out-of-range -> 0), not
// from per-element selects. Only the joint-shift rotation (XROT) and the feature mask
// cost VALU per loaded element.
// ------------------------------------------------------------------------------------

// A thread's position column of a forward tile (fixed for the tile).
struct TileCol {
  unsigned xcol;   // byte offset of (sample, t[, v]) in X; p.x_bytes past P (loads return 0)
  int vv, tt;      // joint and frame
  bool ok;         // the column is a position (p0 + nb < P)
};

// Tile-column setup of the forward kernels, tile at (m0, p0): fills bias_s / rot_s (per tile
// row: bias, shift_out rotation) and ycol_s / v_s (per tile column: byte offset of (b, t) in
// Y, p.y_bytes past P so that stores are dropped; joint v) and returns thread tid's column
// nb = tid % BN. XNOV: xcol without v (the rotated operand adds its own joint per row).
template <int BM, int BN, int NT, bool XNOV>
__device__ __forceinline__ TileCol tile_columns(const FwdArgs& p, int p0, int m0, float* bias_s,
                                                int* rot_s, unsigned* ycol_s, int* v_s) {
  const int tid = threadIdx.x, nb = tid % BN;
  const int V = p.V, N = p.T * V, M = p.M;
  const int P = p.B * N;                 // < 2^31 (host-checked)
  for (int i = tid; i < BM; i += NT) {
    bias_s[i] = (p.bias && m0 + i < M) ? p.bias[m0 + i] : 0.f;
    rot_s[i] = p.y.rsign ? pmod(p.y.rsign * (m0 + i), V) : 0;
  }
  const int pc = p0 + nb;
  TileCol c{p.x_bytes, 0, 0, pc < P};
  unsigned ycol = p.y_bytes;
  if (pc < P) {
    const int b = fdiv(pc, p.divN_m, p.divN_s);
    const int n = pc - b * N;
    const int t = fdiv(n, p.divV_m, p.divV_s);
    c.tt = t;
    c.vv = n - t * V;
    // 32-bit offsets: every term is at most the operand's byte extent (< 2^32, host-checked)
    c.xcol = ((unsigned)b * (unsigned)p.x.bstride + (unsigned)t * (unsigned)(p.x.tstride * V) +
              (unsigned)(XNOV ? 0 : c.vv)) * 4u;
    ycol = ((unsigned)b * (unsigned)p.y.bstride + (unsigned)t * (unsigned)(p.y.tstride * V)) * 4u;
  }
  if (tid < BN) {
    ycol_s[nb] = ycol;
    v_s[nb] = c.vv;
  }
  return c;
}

// Tile store of the forward kernels: Y (+)= act(acc + bias) for the BM x BN tile at row m0
// whose columns tile_columns described. The MFMA C/D map (col = lane&31, row = (r&3) +
// 8*(r>>2) + 4*(lane>>5); the same for every operand type of the 32 x 32 forms) leaves each
// wave holding 32-column pieces of 64 rows; stored straight from registers, a 128-B line of
// a Y row is completed by several waves (and tiles) at different times, and lines evicted
// from L2 half-written cost a second partial write (PMC: 1.20x the algorithmic bytes at
// M >= 128). So the tile is staged through LDS (smem: WM*16 x BN floats, the operand
// stages' memory, which every wave has finished reading) in passes of 16 rows per wave
// band, and each wave then stores whole tile rows: 64 lanes on 64 consecutive positions,
// BN/64 instructions per row, every line completed at once.
template <int BM, int BN, int WM, int WN, bool ACCUM, typename SF>
__device__ __forceinline__ void store_tile(const FwdArgs& p,
                                           const f32x16 (&acc)[BM / WM / 32][BN / WN / 32],
                                           SF* smem, const float* bias_s, const int* rot_s,
                                           const unsigned* ycol_s, const int* v_s, int m0,
                                           int wid, int wm, int wn, int lane) {
  constexpr int MI = BM / WM / 32, NJ = BN / WN / 32;
  constexpr int NW = WM * WN;
  constexpr int RB = WM * 16;      // staged rows per pass
  constexpr int CQ = BN / 64;      // 64-column groups per row
  constexpr int RPW = RB / NW;     // rows per wave per pass
  static_assert(BN % 64 == 0 && RB % NW == 0, "epilogue staging");
  const int V = p.V, M = p.M;
  const int kl = lane >> 5, cl = lane & 31;
  const auto yr = make_rsrc(p.y.ptr, p.y_bytes);
  const unsigned ycs4 = (unsigned)(p.y.cstride * 4);
  unsigned ycolq[CQ];
  int vq[CQ];
#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    ycolq[q] = ycol_s[lane + 64 * q];
    vq[q] = v_s[lane + 64 * q];
  }
  // ACCUM: the old value of an output element is loaded for all of this wave's rows of a
  // pass BEFORE the pass's LDS staging: in the store loop it would wait a memory round trip
  // (a load after the previous row's stores)
  float pf[ACCUM ? RPW : 1][ACCUM ? CQ : 1];
  auto row_of = [&](int i, int h, int k) {   // tile row of this wave's k-th row of a pass
    const int lr = wid + k * NW;
    return (lr >> 4) * (BM / WM) + i * 32 + 16 * h + (lr & 15);   // uniform
  };
  // (ROT a compile-time branch: without the shift_out rotation a lane's store offsets are
  // the same for every row, hoisted out of the row loops — the epilogue is most of the
  // VALU work of a K <= 128 tile, which shares the issue with the fp32 MFMA)
  auto epilogue = [&](auto relu_tag, auto rot_tag) {
    constexpr bool RELU = decltype(relu_tag)::value;
    constexpr bool ROT = decltype(rot_tag)::value;
    auto voff_of = [&](int trow, int q) {
      int vo = vq[q];
      if constexpr (ROT) {   // shift_out rotation of the stored joint
        vo += rot_s[trow];
        vo = vo >= V ? vo - V : vo;
      }
      return vo;
    };
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if constexpr (ACCUM) {
#pragma unroll
          for (int k = 0; k < RPW; ++k) {
            const int trow = row_of(i, h, k);
            // a row past M: every address past its extent (loads 0, nothing stored later)
            const unsigned soff = m0 + trow < M ? (unsigned)(m0 + trow) * ycs4 : p.y_bytes;
#pragma unroll
            for (int q = 0; q < CQ; ++q)
              pf[k][q] = bload(yr, ycolq[q] + (unsigned)(voff_of(trow, q) * 4), soff);
          }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int rr = 0; rr < 8; ++rr) {
            const int r = 8 * h + rr;
            const int lr = wm * 16 + (r & 3) + 8 * ((r >> 2) & 1) + 4 * kl;
            smem[lr * BN + wn * (BN / WN) + j * 32 + cl] = acc[i][j][r];
          }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
          const int lr = wid + k * NW;
          const int trow = row_of(i, h, k);
          if (m0 + trow >= M) break;   // rows past M (they increase with k)
          const float bv = bias_s[trow];
          const unsigned soff = (unsigned)(m0 + trow) * ycs4;
#pragma unroll
          for (int q = 0; q < CQ; ++q) {
            const unsigned voff = ycolq[q] + (unsigned)(voff_of(trow, q) * 4);
            float val = smem[lr * BN + lane + 64 * q] + bv;
            if (RELU) val = fmaxf(val, 0.f);
            if constexpr (ACCUM) val += pf[k][q];
            bstore(yr, val, voff, soff);
          }
        }
        __syncthreads();
      }
  };
  if (p.y.rsign != 0) {
    if (p.relu) epilogue(std::true_type{}, std::true_type{});
    else epilogue(std::false_type{}, std::true_type{});
  } else {
    if (p.relu) epilogue(std::true_type{}, std::false_type{});
    else epilogue(std::false_type{}, std::false_type{});
  }
}

// AR (K <= 64, the HBM-bound 64-row tiles): the whole A (K x BM) is staged into LDS once in
// the prologue and B is single-buffered (a second barrier per stage): 35 instead of 43 KB of
// LDS, so four workgroups fit a CU instead of three — a third more operand bytes in flight.
template <int BM, int BN, int WM, int WN, bool MASK, bool XROT, bool AMC, bool ACCUM,
          bool TSH = false, bool AR = false>
__global__ __launch_bounds__(64 * WM * WN) void pwg_fwd_kernel(FwdArgs p) {
  SGCN_CRIT_PRIO();
  static_assert(!TSH || (!MASK && !XROT), "the temporal-shift operand is plain");
  static_assert(!AR || !TSH, "AR: plain contraction");
  constexpr int NT = 64 * WM * WN;
  constexpr int BK = 16;
  constexpr int MI = BM / WM / 32;
  constexpr int NJ = BN / WN / 32;
  constexpr int AP = BM + 1, BP = BN + 1;
  constexpr int A_PER = BM * BK / NT;
  constexpr int B_PER = BN * BK / NT;
  constexpr int KSTEP_B = NT / BN;
  static_assert(MI >= 1 && NJ >= 1 && A_PER >= 1 && B_PER >= 1, "bad tile");
  static_assert((BM * BK) % NT == 0 && NT % BN == 0 && NT % BK == 0 && NT % BM == 0, "bad tile");
  // operand stages; the epilogue reuses the same memory to stage the accumulator tile
  constexpr int KAR = 64;                          // AR: the largest K held resident
  constexpr int ASZ = AR ? KAR * AP : 2 * BK * AP;
  constexpr int BSZ = AR ? BK * BP : 2 * BK * BP;
  __shared__ float smem[ASZ + BSZ];
  float (*As)[BK * AP] = reinterpret_cast<float (*)[BK * AP]>(smem);
  float (*Bs)[BK * BP] = reinterpret_cast<float (*)[BK * BP]>(smem + ASZ);
  __shared__ float bias_s[BM];
  __shared__ int rot_s[BM];
  __shared__ unsigned ycol_s[BN];   // per tile column: byte offset of (b, t) in Y
  __shared__ int v_s[BN];           // per tile column: joint v

  SGCN_PW_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid - (wid / WN) * WN;
  const int V = p.V, K = p.K, M = p.M;
  const int p0 = xcd_tile<SGCN_PW_XCD>(blockIdx.x, gridDim.x) * BN;
  const int m0 = blockIdx.y * BM;
  const auto xr = make_rsrc(p.x.ptr, p.x_bytes);
  const auto ar = make_rsrc(p.A, p.a_bytes);
  const auto mr = make_rsrc(MASK ? p.mask : p.A, MASK ? p.mask_bytes : 0u);
  const auto xsr = make_rsrc(TSH && p.xs ? p.xs : p.A, TSH && p.xs ? p.x_bytes : 0u);
  // TSH: every channel of the launch takes the two-row operand (the table's flag word)
  const bool two =
      TSH && ((const __attribute__((address_space(4))) int*)p.ts)[K * kTsWords] != 0;

  // ---- B column of this thread (fixed for the tile) ----
  const TileCol col = tile_columns<BM, BN, NT, XROT>(p, p0, m0, bias_s, rot_s, ycol_s, v_s);
  const int nb = tid % BN;
  const int kb0 = __builtin_amdgcn_readfirstlane(tid / BN);
  const unsigned xcol = col.xcol;
  const int vv = col.vv, tt = col.tt;
  const bool colok = col.ok;
  const unsigned xcs4 = (unsigned)(p.x.cstride * 4);
  const int bstep = XROT ? rot_step(KSTEP_B, p.x.rsign, V) : 0;
  const int kstage_rot = XROT ? rot_step(BK, p.x.rsign, V) : 0;
  int cv0 = XROT ? pmod(vv + p.x.rsign * kb0, V) : 0;
  const unsigned mcol = (unsigned)(vv * K * 4);

  // ---- A element of this thread: (m, k) = fixed lane part + uniform i part ----
  const int lda = p.lda;
  const int am = AMC ? tid % BM : tid / BK;
  const int ak = AMC ? tid / BM : tid % BK;
  const unsigned avoff = AMC ? (m0 + am < M ? (unsigned)((ak * lda + m0 + am) * 4) : p.a_bytes)
                             : (unsigned)(((m0 + am) * lda + ak) * 4);
  // per-i uniform step of the A element: AMC -> k += NT/BM, else m += NT/BK
  const unsigned astep = AMC ? (unsigned)((NT / BM) * lda * 4) : (unsigned)((NT / BK) * lda * 4);
  // k-contiguous A: a k past K would alias the next row, so the lane's stage loads go out
  // of the descriptor range (0) when k0 + ak >= K (one compare + select per stage instead
  // of masking every loaded value)
  const int kspan = K - ak;

  float ra[A_PER], rb[B_PER], rm[MASK ? B_PER : 1];
  float rq[TSH ? B_PER : 1][TSH ? 3 : 1];   // TSH: taps q21, q12, q22 (q11 in rb)
  const unsigned v4 = (unsigned)(V * 4);
  // TSH: the per-channel table through the constant address space, so its (wave-uniform)
  // rows are fetched by scalar loads: as a plain global pointer the compiler cannot prove
  // the kernel's own stores (the side output) leave it alone and issues VECTOR loads, each
  // followed by a vmcnt(0) wait that drains every tap load in flight (round-6 ISA: the
  // fused contraction ran at half its round-2 speed)
  using cint = const __attribute__((address_space(4))) int;
  cint* tsc = (cint*)p.ts;
  auto load_tsh = [&](int k0) {
    // taps of H around (t + y1, v + x1); a tap outside the plane is masked in store_stage
    // (its address is clamped / past the extent, never faulting). An in-plane tap lies
    // inside [0, x_bytes - 4 - row offset], so clamping every tap offset into that range
    // only moves taps that store_stage masks, and no address (voffset + soffset) ever
    // leaves the operand; a column past P keeps the out-of-range marker for all taps.
    if constexpr (!TSH) return;
    else if (two) {   // two-row channels: rows y1, y1 + 1 of the element's own column
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int row = min(k0 + kb0 + i * KSTEP_B, K - 1);
        const unsigned so = (unsigned)row * xcs4;
        const int vo = (int)xcol + tsc[row * kTsWords + 8] * 4;
        const int lim = (int)(p.x_bytes - 4u - so);
        rb[i] = bload(xr, colok ? (unsigned)min(max(vo, 0), lim) : p.x_bytes, so);
        rq[i][1] = bload(xr, colok ? (unsigned)min(max(vo + (int)v4, 0), lim) : p.x_bytes, so);
      }
    } else {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int row = min(k0 + kb0 + i * KSTEP_B, K - 1);
        const unsigned so = (unsigned)row * xcs4;
        const int vo = (int)xcol + tsc[row * kTsWords] * 4;
        const int lim = (int)(p.x_bytes - 4u - so);
        auto tap = [&](int d) {
          return colok ? (unsigned)min(max(vo + d, 0), lim) : p.x_bytes;
        };
        rb[i] = bload(xr, tap(0), so);
        rq[i][0] = bload(xr, tap(4), so);
        rq[i][1] = bload(xr, tap((int)v4), so);
        rq[i][2] = bload(xr, tap((int)v4 + 4), so);
      }
    }
  };
  auto load_stage = [&](int k0) {
    int cv = cv0;
    if constexpr (TSH) load_tsh(k0);
#pragma unroll
    for (int i = 0; i < (TSH || ((SGCN_PW_DIAG & 2) && k0) ? 0 : B_PER); ++i) {
      const int row = min(k0 + kb0 + i * KSTEP_B, K - 1);
      const unsigned voff = XROT ? xcol + (unsigned)(cv * 4) : xcol;
      rb[i] = bload_pol<SGCN_PW_XPOL>(xr, voff, (unsigned)row * xcs4);
      if (MASK) rm[i] = bload(mr, mcol, (unsigned)row * 4u);
      if (XROT) {
        cv += bstep;
        cv = cv >= V ? cv - V : cv;
      }
    }
    if (AR) return;   // A is resident (staged in the prologue)
    const unsigned ak0 = AMC ? (unsigned)(k0 * lda * 4) : (unsigned)(k0 * 4);
#pragma unroll
    for (int i = 0; i < ((SGCN_PW_DIAG & 1) && k0 ? 0 : A_PER); ++i)
      ra[i] = bload_pol<SGCN_PW_APOL>(ar, AMC ? avoff : (k0 < kspan ? avoff : p.a_bytes),
                                      ak0 + (unsigned)i * astep);
  };
  const int T = p.T;
  // TSH: form the shifted operand from the taps (straight-line per form: a branch inside
  // the unrolled loop left the tap arrays in scratch). The side output (the shifted operand
  // itself, for the weight gradient; each element is formed exactly once when one M-block
  // covers all M) is stored unconditionally: without x_shifted its descriptor has range 0.
  auto store_tsh = [&](int buf, int k0) {
    if constexpr (!TSH) return;
    else if (two) {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int row = min(k0 + kb0 + i * KSTEP_B, K - 1);
        cint* pr = tsc + row * kTsWords;
        const int tr = tt + pr[1];
        const float a = __int_as_float(pr[5]), b = __int_as_float(pr[6]);
        const bool r0 = (unsigned)tr < (unsigned)T, r1 = (unsigned)(tr + 1) < (unsigned)T;
        const float val = ts_blend2(ts_tap(rb[i], a, b, r0), ts_tap(rq[i][1], a, b, r1),
                                    __int_as_float(pr[9]), __int_as_float(pr[4]));
        bstore(xsr, val, colok ? xcol : p.x_bytes, (unsigned)row * xcs4);
        Bs[buf][(kb0 + i * KSTEP_B) * BP + nb] = val;
      }
    } else {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int row = min(k0 + kb0 + i * KSTEP_B, K - 1);
        cint* pr = tsc + row * kTsWords;
        const int tr = tt + pr[1], vr = vv + pr[2];
        const float a = __int_as_float(pr[5]), b = __int_as_float(pr[6]);
        const bool r0 = (unsigned)tr < (unsigned)T, r1 = (unsigned)(tr + 1) < (unsigned)T;
        const bool c0 = (unsigned)vr < (unsigned)V, c1 = (unsigned)(vr + 1) < (unsigned)V;
        const float val =
            ts_blend(ts_tap(rb[i], a, b, r0 && c0), ts_tap(rq[i][0], a, b, r0 && c1),
                     ts_tap(rq[i][1], a, b, r1 && c0), ts_tap(rq[i][2], a, b, r1 && c1),
                     __int_as_float(pr[3]), __int_as_float(pr[4]));
        bstore(xsr, val, colok ? xcol : p.x_bytes, (unsigned)row * xcs4);
        Bs[buf][(kb0 + i * KSTEP_B) * BP + nb] = val;
      }
    }
  };
  auto store_stage = [&](int buf, int k0) {
    if constexpr (TSH) store_tsh(buf, k0);
#pragma unroll
    for (int i = 0; i < (TSH || ((SGCN_PW_DIAG & 2) && k0) ? 0 : B_PER); ++i) {
      const float val = MASK ? rb[i] * rm[i] : rb[i];
      Bs[AR ? 0 : buf][(kb0 + i * KSTEP_B) * BP + nb] = val;
    }
    if (AR) return;
#pragma unroll
    for (int i = 0; i < ((SGCN_PW_DIAG & 1) && k0 ? 0 : A_PER); ++i) {
      const int m = AMC ? am : am + i * (NT / BK);
      const int k = AMC ? ak + i * (NT / BM) : ak;
      As[buf][k * AP + m] = ra[i];
    }
  };

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x16{};

  const int kl = lane >> 5, cl = lane & 31;
  const int nstage = (K + BK - 1) / BK;
  if constexpr (AR) {
    // the whole A (K <= 64 rows of BM) into LDS at row k, every stage's loads in flight at
    // once (rows past K: out of range, 0)
    float raa[KAR / BK][A_PER];
#pragma unroll
    for (int st = 0; st < KAR / BK; ++st) {
      const int k0 = st * BK;
      const unsigned ak0 = AMC ? (unsigned)(k0 * lda * 4) : (unsigned)(k0 * 4);
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const bool in = k0 + (AMC ? ak + i * (NT / BM) : ak) < K;
        raa[st][i] = bload(ar, in ? (AMC ? avoff : (k0 < kspan ? avoff : p.a_bytes)) : p.a_bytes,
                           ak0 + (unsigned)i * astep);
      }
    }
#pragma unroll
    for (int st = 0; st < KAR / BK; ++st)
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const int m = AMC ? am : am + i * (NT / BK);
        const int k = AMC ? ak + i * (NT / BM) : ak;
        smem[(st * BK + k) * AP + m] = raa[st][i];
      }
  }
  load_stage(0);
  store_stage(0, 0);
  __syncthreads();
  SGCN_PW_STAMP(1);
  for (int s = 0; s < nstage; ++s) {
    const int cur = s & 1;
    if (s + 1 < nstage) {
      if (XROT) {
        cv0 += kstage_rot;
        cv0 = cv0 >= V ? cv0 - V : cv0;
      }
      load_stage((s + 1) * BK);
    }
    const float* __restrict__ Aw = (AR ? smem + s * BK * AP : As[cur]) + kl * AP +
                                   wm * (BM / WM) + cl;
    const float* __restrict__ Bw = Bs[AR ? 0 : cur] + kl * BP + wn * (BN / WN) + cl;
    float af[2][MI], bf[2][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i) af[0][i] = Aw[i * 32];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[0][j] = Bw[j * 32];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int c2 = (kk >> 1) & 1;
      if (kk + 2 < BK) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[c2 ^ 1][i] = Aw[(kk + 2) * AP + i * 32];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[c2 ^ 1][j] = Bw[(kk + 2) * BP + j * 32];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c2][i], bf[c2][j], acc[i][j],
                                                           0, 0, 0);
    }
    if (s + 1 < nstage) {
      if (AR) __syncthreads();   // single B buffer: every wave has read this stage
      store_stage(cur ^ 1, (s + 1) * BK);
    }
    __syncthreads();
  }

  SGCN_PW_STAMP(2);
  // ---- epilogue: the operand stages' memory now stages the accumulator tile ----
  static_assert(WM * 16 * BN <= ASZ + BSZ, "epilogue staging");
  store_tile<BM, BN, WM, WN, ACCUM>(p, acc, smem, bias_s, rot_s, ycol_s, v_s, m0, wid, wm, wn,
                                    lane);
#ifdef SGCN_PW_STAMPS
  __builtin_amdgcn_s_waitcnt(0);   // stores issued and drained
#endif
  SGCN_PW_STAMP(3);
}

// ------------------------------------------------------------------------------------
// Eval-mode inference forward with bf16 operands (sgcn_pw_fwd_bf16): the plain contraction
// (no mask, no operand rotation, no accumulate) on v_mfma_f32_32x32x16_bf16. Both operands
// stay fp32 in memory and are rounded to bf16 (round to nearest even, the hardware's packed
// convert) on their way into LDS; products of two bf16 values are exact in fp32 and the
// accumulator, bias add, ReLU and stores are fp32, as in pwg_fwd_kernel.
//
// LDS holds bf16 in 16-byte slots of 8 consecutive k: a stage (32 k) of an operand is four
// groups g of [rows][8 k], so the fragment of lane (r = lane & 31, h = lane >> 5) for the
// MFMA k-step s is ONE slot, (group 2s + h, row r): 32 lanes read 512 contiguous bytes.
//  * X: a thread owns one position column and eight consecutive k rows of it (coalesced
//    loads along the positions), converts them and writes one slot.
//  * A, k-contiguous (Conv2d weights): a thread owns a k pair of a row (16 lanes read 128
//    contiguous bytes), writes one dword; the groups are 2 slots apart from a multiple of
//    the bank count so the four groups a wave writes land on different banks.
//  * A, m-contiguous (Linear_weight): as X, a thread owns a row m and eight k.
// Rows k >= K are out of the descriptor range for BOTH operands (zeros in LDS; a k past K
// is never read from memory), rows m >= M and columns past P likewise. Two stages are
// double-buffered with one barrier each; tile-column setup and tile store are the ones
// pwg_fwd_kernel calls (tile_columns, store_tile: the C/D map of the 32 x 32 forms does not
// depend on the operand type).
// Not pinned: subnormal, infinite and NaN operands.
// ------------------------------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
typedef u32x4 __attribute__((may_alias)) lds_slot;
typedef unsigned __attribute__((may_alias)) lds_word;
typedef float __attribute__((may_alias)) lds_float;

template <int BM, int BN, int WM, int WN, bool AMC>
__global__ __launch_bounds__(64 * WM * WN) void pwg_fwd_bf16_kernel(FwdArgs p) {
  SGCN_CRIT_PRIO();
  constexpr int NT = 64 * WM * WN;
  constexpr int BK = kPwBf16BK, KG = BK / 8;   // k-groups of 8 per stage
  constexpr int MI = BM / WM / 32;
  constexpr int NJ = BN / WN / 32;
  constexpr int AG = BM + 2, BG = BN;          // slots per group
  constexpr int ASZ = KG * AG, BSZ = KG * BG;  // slots per stage buffer
  // X: NT / BN groups per pass
  constexpr int BGS = NT / BN, B_IT = KG / BGS;
  // A k-contiguous: 16 k pairs x NT / 16 rows per pass; m-contiguous: NT / BM groups per pass
  constexpr int A_ROWS = NT / 16, A_IT = BM / A_ROWS;
  constexpr int AGS = NT / BM, AM_IT = (KG + AGS - 1) / AGS;
  static_assert(MI >= 1 && NJ >= 1 && BK == 32, "bad tile");
  static_assert(NT % BN == 0 && KG % BGS == 0 && B_IT >= 1, "bad tile (X staging)");
  static_assert(BM % A_ROWS == 0 && NT % BM == 0 && BM % 64 == 0, "bad tile (A staging)");
  // slots of the operand stages and of store_tile's staged rows (WM * 16 x BN floats)
  constexpr int OPS = 2 * (ASZ + BSZ), EPS = WM * 16 * BN / 4;
  __shared__ lds_slot smem[OPS > EPS ? OPS : EPS];
  lds_slot* const As = smem;                   // [2][KG][AG]
  lds_slot* const Bs = smem + 2 * ASZ;         // [2][KG][BG]
  __shared__ float bias_s[BM];
  __shared__ int rot_s[BM];
  __shared__ unsigned ycol_s[BN];   // per tile column: byte offset of (b, t) in Y
  __shared__ int v_s[BN];           // per tile column: joint v

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid - (wid / WN) * WN;
  const int K = p.K, M = p.M;
  const int p0 = xcd_tile<SGCN_PW_XCD>(blockIdx.x, gridDim.x) * BN;
  const int m0 = blockIdx.y * BM;
  const auto xr = make_rsrc(p.x.ptr, p.x_bytes);
  const auto ar = make_rsrc(p.A, p.a_bytes);

  // ---- X column of this thread (fixed for the tile) ----
  const unsigned xcol =
      tile_columns<BM, BN, NT, false>(p, p0, m0, bias_s, rot_s, ycol_s, v_s).xcol;
  const int nb = tid % BN;
  const int bg0 = __builtin_amdgcn_readfirstlane(tid / BN);
  const unsigned xcs4 = (unsigned)(p.x.cstride * 4);

  // ---- A elements of this thread ----
  const int lda = p.lda;
  // k-contiguous: the pair (2 kp, 2 kp + 1) of rows am + it * A_ROWS
  const int kp = tid & 15, am = tid >> 4;
  const unsigned avoff = (unsigned)(((m0 + am) * lda + 2 * kp) * 4);
  const int kspan = K - 2 * kp;   // the pair's elements are inside the row while k0 < kspan (- 1)
  // m-contiguous: row amc, groups ag0 + it * AGS
  const int amc = tid % BM;
  const int ag0 = __builtin_amdgcn_readfirstlane(tid / BM);
  const unsigned amvoff = m0 + amc < M ? (unsigned)((m0 + amc) * 4) : p.a_bytes;

  float rb[B_IT][8];
  float ra[AMC ? AM_IT * 8 : A_IT * 2];
  auto load_stage = [&](int k0) {
#pragma unroll
    for (int it = 0; it < B_IT; ++it)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = k0 + (bg0 + it * BGS) * 8 + j;   // uniform
        rb[it][j] = bload_pol<SGCN_PW_XPOL>(xr, row < K ? xcol : p.x_bytes,
                                            (unsigned)min(row, K - 1) * xcs4);
      }
    if constexpr (AMC) {
#pragma unroll
      for (int it = 0; it < AM_IT; ++it) {
        const int g = ag0 + it * AGS;   // uniform
        if (g >= KG) break;             // more waves than groups (BM = 64)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int row = k0 + g * 8 + j;
          ra[it * 8 + j] = bload_pol<SGCN_PW_APOL>(ar, row < K ? amvoff : p.a_bytes,
                                                   (unsigned)(min(row, K - 1) * lda * 4));
        }
      }
    } else {
      // a k past K would alias the next row: such a lane's load goes out of the range (and
      // so does a row past M: its offset is at least the extent)
#pragma unroll
      for (int it = 0; it < A_IT; ++it) {
        const unsigned vo = avoff + (unsigned)(it * A_ROWS * lda * 4);
        ra[2 * it] = bload_pol<SGCN_PW_APOL>(ar, k0 < kspan ? vo : p.a_bytes, (unsigned)(k0 * 4));
        ra[2 * it + 1] =
            bload_pol<SGCN_PW_APOL>(ar, k0 < kspan - 1 ? vo + 4u : p.a_bytes, (unsigned)(k0 * 4));
      }
    }
  };
  auto pack8 = [](const float* v) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)v[j];
    return __builtin_bit_cast(u32x4, r);
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int it = 0; it < B_IT; ++it)
      Bs[buf * BSZ + (bg0 + it * BGS) * BG + nb] = pack8(rb[it]);
    if constexpr (AMC) {
#pragma unroll
      for (int it = 0; it < AM_IT; ++it) {
        const int g = ag0 + it * AGS;
        if (g < KG) As[buf * ASZ + g * AG + amc] = pack8(&ra[it * 8]);
      }
    } else {
      lds_word* const Aw = reinterpret_cast<lds_word*>(As + buf * ASZ);
#pragma unroll
      for (int it = 0; it < A_IT; ++it) {
        bf16x2 r;
        r[0] = (__bf16)ra[2 * it];
        r[1] = (__bf16)ra[2 * it + 1];
        Aw[((kp >> 2) * AG + am + it * A_ROWS) * 4 + (kp & 3)] = __builtin_bit_cast(unsigned, r);
      }
    }
  };

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x16{};

  const int kl = lane >> 5, cl = lane & 31;
  const int nstage = (K + BK - 1) / BK;
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int s = 0; s < nstage; ++s) {
    const int cur = s & 1;
    if (s + 1 < nstage) load_stage((s + 1) * BK);
    const lds_slot* __restrict__ Ar = As + cur * ASZ + kl * AG + wm * (BM / WM) + cl;
    const lds_slot* __restrict__ Br = Bs + cur * BSZ + kl * BG + wn * (BN / WN) + cl;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[MI], bf[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = __builtin_bit_cast(bf16x8, Ar[2 * kk * AG + i * 32]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = __builtin_bit_cast(bf16x8, Br[2 * kk * BG + j * 32]);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < nstage) store_stage(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: the operand stages' memory now stages the accumulator tile ----
  store_tile<BM, BN, WM, WN, false>(p, acc, reinterpret_cast<lds_float*>(smem), bias_s, rot_s,
                                    ycol_s, v_s, m0, wid, wm, wn, lane);
}

// ------------------------------------------------------------------------------------
// dW (split-K over all positions)
// ------------------------------------------------------------------------------------
struct DwArgs {
  Plane g;            // A operand rows m: G(b, m, n)
  Plane x;            // B operand rows n: X(b, c, n)
  const float* mask;  // optional mask[v*Nc + c] on X
  float* slab;        // [S][M][Nc]
  float* bslab;       // optional [S][M] row sums of G
  int M, Nc, T, V, B;
  int chunks_per_split;
  unsigned g_bytes, x_bytes, mask_bytes;   // buffer ranges (pw_dw3_kernel)
};

// PLAIN (no mask, no joint rotation, byte extents in g_bytes / x_bytes): full tiles take a
// lane's position (sample, t, v) advanced incrementally from chunk to chunk and load through
// buffer descriptors (one address add per load) instead of two integer divisions per chunk
// and 64-bit pointer arithmetic per load (11 VALU per MFMA before: the VALU shares the
// fp32 MFMA's issue); partial tiles keep the general path.
template <int BM, int BN, int WM, int WN, bool MASK, bool PLAIN = false>
__global__ __launch_bounds__(64 * WM * WN) void pw_dw_kernel(DwArgs p) {
  constexpr int NT = 64 * WM * WN;
  // positions per chunk: a wave's 64 lanes read 64 consecutive positions (256 B) of one
  // operand row per load instruction (32 lanes x 2 rows, i.e. 128-B row segments, at BK =
  // 32 read at ~3.7 TB/s on the HBM-bound 64-wide shapes)
  constexpr int BK = kDwBK;
  constexpr int MI = BM / WM / 32, NJ = BN / WN / 32;
  constexpr int AP = BM + 1, BP = BN + 1;
  constexpr int RSTEP = NT / BK;             // rows per load step
  constexpr int A_PER = BM / RSTEP, B_PER = BN / RSTEP;
  static_assert(MI >= 1 && NJ >= 1 && A_PER >= 1 && B_PER >= 1, "bad tile");
  __shared__ float As[BK * AP];
  __shared__ float Bs[BK * BP];
  extern __shared__ float mask_s[];   // [v][c - c0] (dynamic: V*BN floats)

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int ntiles = (p.Nc + BN - 1) / BN;
  const int m0 = (blockIdx.x / ntiles) * BM, c0 = (blockIdx.x % ntiles) * BN;
  const int split = blockIdx.y;
  const int V = p.V, N = p.T * V;
  const int nchunk = (N + BK - 1) / BK;
  const int q_begin = split * p.chunks_per_split;
  const int q_end = min(q_begin + p.chunks_per_split, p.B * nchunk);
  const bool want_bias = p.bslab != nullptr && (blockIdx.x % ntiles) == 0;

  if (MASK) {
    for (int i = tid; i < V * BN; i += NT) {
      const int v = i / BN, c = c0 + (i - v * BN);
      mask_s[i] = c < p.Nc ? p.mask[v * p.Nc + c] : 0.f;
    }
    __syncthreads();
  }

  const int kq = tid % BK, r0 = tid / BK;
  // rotation of row r0 + RSTEP*i is (base + i*step) mod V, advanced incrementally
  const int g_rot0 = pmod(p.g.rsign * (m0 + r0), V), g_step = rot_step(RSTEP, p.g.rsign, V);
  const int x_rot0 = pmod(p.x.rsign * (c0 + r0), V), x_step = rot_step(RSTEP, p.x.rsign, V);
  const int gcs = (int)p.g.cstride, xcs = (int)p.x.cstride;
  float ra[A_PER], rb[B_PER], rsum[A_PER];
  int vcur = 0;
  bool ncur = false;
#pragma unroll
  for (int i = 0; i < A_PER; ++i) rsum[i] = 0.f;

  // PLAIN fast path state: the position of the next chunk to load
  const bool fast = PLAIN && m0 + BM <= p.M && c0 + BN <= p.Nc;   // uniform
  const auto gres = make_rsrc(p.g.ptr, PLAIN ? p.g_bytes : 0u);
  const auto xres = make_rsrc(p.x.ptr, PLAIN ? p.x_bytes : 0u);
  const unsigned grow = (unsigned)((m0 + r0) * gcs) * 4u, xrow = (unsigned)((c0 + r0) * xcs) * 4u;
  const unsigned gstep = (unsigned)(RSTEP * gcs) * 4u, xstep = (unsigned)(RSTEP * xcs) * 4u;
  const unsigned gbs = (unsigned)p.g.bstride, xbs = (unsigned)p.x.bstride;
  const unsigned gts = (unsigned)(p.g.tstride * V), xts = (unsigned)(p.x.tstride * V);
  const int t0 = kq / V, v0 = kq - (kq / V) * V, dt = BK / V, dv = BK - (BK / V) * V;
  int fb = 0, fc = 0, fn = 0, ft = 0, fv = 0;
  if (fast && q_begin < q_end) {
    fb = q_begin / nchunk;
    fc = q_begin - fb * nchunk;
    fn = fc * BK + kq;
    ft = fn / V;
    fv = fn - ft * V;
  }
  auto load_fast = [&]() {
    ncur = fn < N;
    vcur = fv;
    const unsigned gp = grow + ((unsigned)fb * gbs + (unsigned)ft * gts + (unsigned)fv) * 4u;
    const unsigned xp = xrow + ((unsigned)fb * xbs + (unsigned)ft * xts + (unsigned)fv) * 4u;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) ra[i] = bload(gres, gp + (unsigned)i * gstep, 0);
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rb[i] = bload(xres, xp + (unsigned)i * xstep, 0);
    // next chunk: BK positions on, or the next sample's first
    if (++fc == nchunk) {
      fc = 0;
      ++fb;
      fn = kq;
      ft = t0;
      fv = v0;
    } else {
      fn += BK;
      ft += dt;
      fv += dv;
      if (fv >= V) { fv -= V; ++ft; }
    }
  };
  auto load_stage = [&](int q) {
    if (fast) {
      load_fast();
      return;
    }
    const int b = q / nchunk;
    const int n = (q - b * nchunk) * BK + kq;
    const bool nvalid = n < N;
    const int ncl = min(n, N - 1);
    const int t = ncl / V;
    const int v = ncl - t * V;
    vcur = v;
    ncur = nvalid;
    const float* __restrict__ gb =
        p.g.ptr + (long long)b * p.g.bstride + (long long)t * p.g.tstride * V;
    const float* __restrict__ xb =
        p.x.ptr + (long long)b * p.x.bstride + (long long)t * p.x.tstride * V;
    int cg = v + g_rot0;
    cg = cg >= V ? cg - V : cg;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int mc = min(m0 + r0 + i * RSTEP, p.M - 1);
      ra[i] = gb[mc * gcs + cg];
      cg += g_step;
      cg = cg >= V ? cg - V : cg;
    }
    int cx = v + x_rot0;
    cx = cx >= V ? cx - V : cx;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int ccl = min(c0 + r0 + i * RSTEP, p.Nc - 1);
      rb[i] = xb[ccl * xcs + cx];
      cx += x_step;
      cx = cx >= V ? cx - V : cx;
    }
  };

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x16{};

  const int kl = lane >> 5, cl = lane & 31;
  if (q_begin < q_end) load_stage(q_begin);
  for (int q = q_begin; q < q_end; ++q) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const float gv = keep(ra[i], ncur && m0 + r0 + i * RSTEP < p.M);
      As[kq * AP + r0 + i * RSTEP] = gv;
      rsum[i] += gv;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      float xv = keep(rb[i], ncur && c0 + r0 + i * RSTEP < p.Nc);
      if (MASK) xv *= mask_s[vcur * BN + r0 + i * RSTEP];
      Bs[kq * BP + r0 + i * RSTEP] = xv;
    }
    __syncthreads();
    if (q + 1 < q_end) load_stage(q + 1);
    float af[2][MI], bf[2][NJ];
    const float* __restrict__ Aw = As + kl * AP + wm * (BM / WM) + cl;
    const float* __restrict__ Bw = Bs + kl * BP + wn * (BN / WN) + cl;
#pragma unroll
    for (int i = 0; i < MI; ++i) af[0][i] = Aw[i * 32];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[0][j] = Bw[j * 32];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int cur = (kk >> 1) & 1;
      if (kk + 2 < BK) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[cur ^ 1][i] = Aw[(kk + 2) * AP + i * 32];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[cur ^ 1][j] = Bw[(kk + 2) * BP + j * 32];
      }
      // keep the prefetch reads above this k-step's MFMAs (the scheduler otherwise sinks
      // them below to reuse registers, exposing LDS latency every k-step)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j],
                                                           0, 0, 0);
    }
    __syncthreads();
  }

  float* slab = p.slab + (size_t)split * p.M * p.Nc;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = c0 + wn * (BN / WN) + j * 32 + cl;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
        if (m < p.M && c < p.Nc) slab[(size_t)m * p.Nc + c] = acc[i][j][r];
      }
  }
  if (want_bias) {
    // rows r0 + i*RSTEP are shared by the BK lanes with equal tid/BK
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      float s = rsum[i];
#pragma unroll
      for (int o = BK / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const int m = m0 + r0 + i * RSTEP;
      if (kq == 0 && m < p.M) p.bslab[(size_t)split * p.M + m] = s;
    }
  }
}

// ------------------------------------------------------------------------------------
// dW v3: the same split-K contraction with a VALU-lean main loop (see pwg_fwd_kernel).
// Positions are flattened over (sample, t, v) and cut into chunks of BKP; a lane owns one
// position of the chunk (its (b, t, v) advanced incrementally, no division in the loop)
// and RPW = 64/BKP rows per wave instruction; the row offset is a wave-uniform soffset.
// Positions past the split's end load 0 through the descriptor range.
// ------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int BKP, bool MASK, bool GROT, bool XROT, bool BIAS>
__global__ __launch_bounds__(64 * WM * WN) void pw_dw3_kernel(DwArgs p) {
  constexpr int NT = 64 * WM * WN;
  constexpr int MI = BM / WM / 32, NJ = BN / WN / 32;
  // row pitch: the per-chunk stores put BKP positions x (32/BKP) rows in one 32-lane
  // ds_write group; a pitch = 2 (mod 32) words (BKP = 16) or odd (BKP = 32) keeps them on
  // distinct banks. Fragment reads (32 consecutive words per half-wave) never conflict.
  constexpr int PAD = BKP == 16 ? 34 : 33;
  constexpr int AP = BM + PAD, BP = BN + PAD;
  constexpr int RPW = 64 / BKP;            // rows covered by one wave instruction
  constexpr int RSTEP = NT / BKP;          // rows between a thread's consecutive loads
  constexpr int G_PER = BM / RSTEP, X_PER = BN / RSTEP;
  static_assert(MI >= 1 && NJ >= 1 && G_PER >= 1 && X_PER >= 1, "bad tile");
  static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && 64 % BKP == 0, "bad tile");
  __shared__ float As[2][BKP * AP];
  __shared__ float Bs[2][BKP * BP];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid - (wid / WN) * WN;
  const int ntn = (p.Nc + BN - 1) / BN;
  // XCD-aware: one XCD's workgroups take consecutive (split, tile) pairs, i.e. adjacent
  // position ranges, whose edge lines they then share in one L2 (see xcd_tile)
  const int lin = xcd_tile<SGCN_DW_XCD>(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int tix = lin % gridDim.x;
  const int m0 = (tix / ntn) * BM, c0 = (tix % ntn) * BN;
  const int split = lin / gridDim.x;
  const int V = p.V, T = p.T, N = T * V;
  const int P = p.B * N;
  const int nch = (P + BKP - 1) / BKP;
  const int q_begin = split * p.chunks_per_split;
  const int q_end = min(q_begin + p.chunks_per_split, nch);
  const int p_end = min(q_end * BKP, P);
  const auto gr = make_rsrc(p.g.ptr, p.g_bytes);
  const auto xr = make_rsrc(p.x.ptr, p.x_bytes);
  const auto mr = make_rsrc(MASK ? p.mask : p.x.ptr, MASK ? p.mask_bytes : 0u);

  const int kq = lane % BKP;          // position of this lane within a chunk
  const int rsub = lane / BKP;        // row within the wave instruction
  const int rw = wid * RPW;           // uniform row base of this wave
  // lane position state (advanced by BKP per chunk)
  int pp = q_begin * BKP + kq;
  int b = pp / N, n = pp - (pp / N) * N;
  int t = n / V, v = n - (n / V) * V;
  const int dt = BKP / V, dv = BKP - (BKP / V) * V;
  const unsigned gcs4 = (unsigned)(p.g.cstride * 4), xcs4 = (unsigned)(p.x.cstride * 4);
  const int g_step = GROT ? rot_step(RSTEP, p.g.rsign, V) : 0;
  const int x_step = XROT ? rot_step(RSTEP, p.x.rsign, V) : 0;
  const int g_rot0 = GROT ? pmod(p.g.rsign * (m0 + rw + rsub), V) : 0;
  const int x_rot0 = XROT ? pmod(p.x.rsign * (c0 + rw + rsub), V) : 0;

  float ra[G_PER], rb[X_PER], rm[MASK ? X_PER : 1], rsum[BIAS ? G_PER : 1];
#pragma unroll
  for (int i = 0; i < (BIAS ? G_PER : 1); ++i) rsum[i] = 0.f;

  auto load_chunk = [&]() {
    const bool ok = pp < p_end;
    const unsigned gb = ok ? (unsigned)(((long long)b * p.g.bstride +
                                         (long long)t * p.g.tstride * V) * 4) : p.g_bytes;
    const unsigned xb = ok ? (unsigned)(((long long)b * p.x.bstride +
                                         (long long)t * p.x.tstride * V) * 4) : p.x_bytes;
    const unsigned lg = (unsigned)rsub * gcs4, lx = (unsigned)rsub * xcs4;
    int cg = v + g_rot0;
    cg = cg >= V ? cg - V : cg;
#pragma unroll
    for (int i = 0; i < G_PER; ++i) {
      const unsigned voff = gb + lg + (unsigned)((GROT ? cg : v) * 4);
      ra[i] = bload(gr, voff, (unsigned)(m0 + rw + i * RSTEP) * gcs4);
      if (GROT) {
        cg += g_step;
        cg = cg >= V ? cg - V : cg;
      }
    }
    int cx = v + x_rot0;
    cx = cx >= V ? cx - V : cx;
    const unsigned mcol = (unsigned)((v * p.Nc + rsub) * 4);
#pragma unroll
      for (int i = 0; i < X_PER; ++i) {
        const unsigned voff = xb + lx + (unsigned)((XROT ? cx : v) * 4);
        rb[i] = bload(xr, voff, (unsigned)(c0 + rw + i * RSTEP) * xcs4);
        if (MASK) rm[i] = bload(mr, mcol, (unsigned)(c0 + rw + i * RSTEP) * 4u);
        if (XROT) {
          cx += x_step;
          cx = cx >= V ? cx - V : cx;
        }
      }
    // advance this lane's position by one chunk
    pp += BKP;
    n += BKP;
    v += dv;
    t += dt;
    if (v >= V) { v -= V; ++t; }
    while (n >= N) { n -= N; ++b; t -= T; }   // a chunk may exceed a tiny sample (N < BKP)
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G_PER; ++i) {
      As[buf][kq * AP + rw + rsub + i * RSTEP] = ra[i];
      if (BIAS) rsum[i] += ra[i];
    }
#pragma unroll
    for (int i = 0; i < X_PER; ++i) {
      Bs[buf][kq * BP + rw + rsub + i * RSTEP] = MASK ? rb[i] * rm[i] : rb[i];
    }
  };

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x16{};

  const int kl = lane >> 5, cl = lane & 31;
  const int nq = q_end - q_begin;
  if (nq > 0) {
    load_chunk();
    store_chunk(0);
  }
  __syncthreads();
  for (int s = 0; s < nq; ++s) {
    const int cur = s & 1;
    if (s + 1 < nq) load_chunk();
    const float* __restrict__ Aw = As[cur] + kl * AP + wm * (BM / WM) + cl;
    const float* __restrict__ Bw = Bs[cur] + kl * BP + wn * (BN / WN) + cl;
    float af[2][MI], bf[2][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i) af[0][i] = Aw[i * 32];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[0][j] = Bw[j * 32];
#pragma unroll
    for (int kk = 0; kk < BKP; kk += 2) {
      const int c2 = (kk >> 1) & 1;
      if (kk + 2 < BKP) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[c2 ^ 1][i] = Aw[(kk + 2) * AP + i * 32];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[c2 ^ 1][j] = Bw[(kk + 2) * BP + j * 32];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c2][i], bf[c2][j], acc[i][j],
                                                           0, 0, 0);
    }
    if (s + 1 < nq) store_chunk(cur ^ 1);
    __syncthreads();
  }

  float* slab = p.slab + (size_t)split * p.M * p.Nc;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = c0 + wn * (BN / WN) + j * 32 + cl;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
        if (m < p.M && c < p.Nc) slab[(size_t)m * p.Nc + c] = acc[i][j][r];
      }
  }
  if (BIAS && (tix % ntn) == 0) {
    // row rw + rsub + i*RSTEP is shared by the BKP lanes with equal rsub
#pragma unroll
    for (int i = 0; i < G_PER; ++i) {
      float sv = rsum[i];
#pragma unroll
      for (int o = BKP / 2; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
      const int m = m0 + rw + rsub + i * RSTEP;
      if (kq == 0 && m < p.M) p.bslab[(size_t)split * p.M + m] = sv;
    }
  }
}

// Split-K reduction of the dW (and bias) slabs in ONE launch, FIXED order (deterministic):
//   i <  n        : dw[i]     (+)= sum_s slab[s*n + i]        (transpose: i = m*Nc + c ->
//                                                            stored at c*M + m)
//   n <= i < n+nb : dbias[i-n] (+)= sum_s bslab[s*nb + i - n]
// 64 outputs per block x 16 split-groups (1024 threads); a group sums every 16th split
// with 16 loads in flight, then the 16 group sums are added in order. The slabs are a
// few MB to 64 MB: few dependent load rounds per thread keep this launch short.
constexpr int kRedGroups = 16, kRedU = 16;
__global__ __launch_bounds__(64 * kRedGroups) void slab_reduce_kernel(
    const float* __restrict__ slab, const float* __restrict__ bslab, int S, int n, int nb,
    int M, int Nc, float* __restrict__ out, float* __restrict__ bout, int transpose,
    int accum, int baccum) {
  __shared__ float red[kRedGroups][64];
  const int il = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + il;
  const bool isb = i >= n;
  const float* __restrict__ src = isb ? bslab : slab;
  const int stride = isb ? nb : n;
  const int ic = isb ? min(i - n, nb - 1) : i;
  float acc[kRedU];
#pragma unroll
  for (int k = 0; k < kRedU; ++k) acc[k] = 0.f;
  if (i < n + nb) {
    int s = q;
    for (; s + kRedGroups * (kRedU - 1) < S; s += kRedGroups * kRedU) {
#pragma unroll
      for (int k = 0; k < kRedU; ++k) acc[k] += src[(size_t)(s + kRedGroups * k) * stride + ic];
    }
    for (; s < S; s += kRedGroups) acc[0] += src[(size_t)s * stride + ic];
  }
#pragma unroll
  for (int w = kRedU / 2; w >= 1; w >>= 1)
#pragma unroll
    for (int k = 0; k < w; ++k) acc[k] = acc[k] + acc[k + w];
  red[q][il] = acc[0];
  __syncthreads();
  if (q == 0 && i < n + nb) {
    float tot = 0.f;
#pragma unroll
    for (int g = 0; g < kRedGroups; ++g) tot += red[g][il];
    if (isb) {
      const int d = i - n;
      bout[d] = baccum ? bout[d] + tot : tot;
    } else {
      int dst = i;
      if (transpose) {
        const int m = i / Nc, c = i - m * Nc;
        dst = c * M + m;
      }
      out[dst] = accum ? out[dst] + tot : tot;
    }
  }
}

void launch_slab_reduce(const float* slab, const float* bslab, int S, int M, int Nc, float* dw,
                        int transpose, int accum, float* dbias, int baccum, hipStream_t st) {
  const int n = M * Nc, nb = dbias ? M : 0;
  slab_reduce_kernel<<<(n + nb + 63) / 64, 64 * kRedGroups, 0, st>>>(
      slab, bslab, S, n, nb, M, Nc, dw, dbias, transpose, accum, baccum);
}


// ------------------------------------------------------------------------------------
// dW for Nc <= 4 input channels (l1's gcn Linear and down conv, 3 -> 64): HBM-bound on G
// (M rows), so no MFMA tile (which would stage 64 operand rows for 3 and multiply zeros):
// each wave owns 16 rows of G, its 64 lanes walk 64 consecutive positions per step
// (256-B row reads), the Nc X values of a position are shared by the wave's 16 rows, and
// the per-lane sums are merged over the wave in a fixed xor order into slab[split]. Same
// slab layout and reduction as pw_dw_kernel.
// ------------------------------------------------------------------------------------
template <int NC, bool MASK>
__global__ __launch_bounds__(256) void pw_dw_smallc_kernel(DwArgs p, int pos_per_split) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = (blockIdx.x * 4 + wid) * kDwcRows;   // this wave's first row
  const int split = blockIdx.y;
  const int V = p.V, N = p.T * V;
  const long long P = (long long)p.B * N;
  const long long q0 = (long long)split * pos_per_split;
  const long long q1 = min(q0 + pos_per_split, P);
  float acc[kDwcRows][NC], bs[kDwcRows];
#pragma unroll
  for (int r = 0; r < kDwcRows; ++r) {
    bs[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[r][c] = 0.f;
  }
  if (m0 < p.M) {
    for (long long q = q0 + lane; q < q1; q += 64) {
      const int b = (int)(q / N);
      const int n = (int)(q - (long long)b * N);
      const int t = n / V, v = n - t * V;
      const float* __restrict__ gb =
          p.g.ptr + (long long)b * p.g.bstride + (long long)t * p.g.tstride * V;
      const float* __restrict__ xb =
          p.x.ptr + (long long)b * p.x.bstride + (long long)t * p.x.tstride * V;
      float xv[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int cc = min(c, p.Nc - 1);
        xv[c] = xb[cc * p.x.cstride + pmod(v + p.x.rsign * cc, V)];
        if (MASK) xv[c] *= p.mask[v * p.Nc + cc];
        if (c >= p.Nc) xv[c] = 0.f;
      }
      int cg = pmod(v + p.g.rsign * m0, V);
      const int gstep = p.g.rsign < 0 ? V - 1 : (p.g.rsign > 0 ? 1 : 0);
#pragma unroll
      for (int r = 0; r < kDwcRows; ++r) {
        const int m = min(m0 + r, p.M - 1);
        const float gv = m0 + r < p.M ? gb[(long long)m * p.g.cstride + cg] : 0.f;
        cg += gstep;
        cg = cg >= V ? cg - V : cg;
        bs[r] += gv;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[r][c] = fmaf(gv, xv[c], acc[r][c]);
      }
    }
  }
  // fixed-order wave merge; lane 0 writes the split's partials
#pragma unroll
  for (int r = 0; r < kDwcRows; ++r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      bs[r] += __shfl_xor(bs[r], o, 64);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[r][c] += __shfl_xor(acc[r][c], o, 64);
    }
  }
  if (lane == 0 && m0 < p.M) {
    float* slab = p.slab + (size_t)split * p.M * p.Nc;
#pragma unroll
    for (int r = 0; r < kDwcRows; ++r) {
      if (m0 + r >= p.M) break;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < p.Nc) slab[(size_t)(m0 + r) * p.Nc + c] = acc[r][c];
      if (p.bslab) p.bslab[(size_t)split * p.M + m0 + r] = bs[r];
    }
  }
}

// ------------------------------------------------------------------------------------
// Forward / dX contraction with M <= 4 output rows (l1's input gradients, 64 -> 3): one
// position per lane, the K input rows read straight from HBM (coalesced over the lanes'
// consecutive positions, 8 rows in flight), the M x K weights broadcast from LDS (one
// 16-byte read per k). HBM-bound on the K-row operand; the 64-row MFMA tile would stage
// and multiply 61 rows of zeros. Same bias / ReLU / accumulate epilogue as pwg_fwd_kernel.
// ------------------------------------------------------------------------------------
template <bool AMC, bool ACCUM>
__global__ __launch_bounds__(256) void pw_fwd_smallm_kernel(FwdArgs p) {
  SGCN_CRIT_PRIO();
  __shared__ float4 Ws[256];   // [k] -> (m0..m3), zero past M
  const int tid = threadIdx.x;
  const int K = p.K, M = p.M, V = p.V, N = p.T * V;
  for (int k = tid; k < K; k += 256) {
    float w[kSmallM];
#pragma unroll
    for (int m = 0; m < kSmallM; ++m)
      w[m] = m < M ? (AMC ? p.A[k * p.lda + m] : p.A[m * p.lda + k]) : 0.f;
    Ws[k] = make_float4(w[0], w[1], w[2], w[3]);
  }
  __syncthreads();
  const long long q = (long long)blockIdx.x * 256 + tid;
  if (q >= (long long)p.B * N) return;
  const int b = (int)(q / N);
  const int n = (int)(q - (long long)b * N);
  const int t = n / V, v = n - t * V;
  const float* __restrict__ xp =
      p.x.ptr + (long long)b * p.x.bstride + (long long)t * p.x.tstride * V + v;
  float* __restrict__ yp = p.y.ptr + (long long)b * p.y.bstride + (long long)t * p.y.tstride * V + v;
  const long long xcs = p.x.cstride;
  float acc[kSmallM] = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= K; k += 8) {
    float xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xv[u] = xp[(k + u) * xcs];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float4 w = Ws[k + u];
      acc[0] = fmaf(w.x, xv[u], acc[0]);
      acc[1] = fmaf(w.y, xv[u], acc[1]);
      acc[2] = fmaf(w.z, xv[u], acc[2]);
      acc[3] = fmaf(w.w, xv[u], acc[3]);
    }
  }
  for (; k < K; ++k) {
    const float xv = xp[k * xcs];
    const float4 w = Ws[k];
    acc[0] = fmaf(w.x, xv, acc[0]);
    acc[1] = fmaf(w.y, xv, acc[1]);
    acc[2] = fmaf(w.z, xv, acc[2]);
    acc[3] = fmaf(w.w, xv, acc[3]);
  }
#pragma unroll
  for (int m = 0; m < kSmallM; ++m) {
    if (m >= M) break;
    float val = acc[m] + (p.bias ? p.bias[m] : 0.f);
    if (p.relu) val = fmaxf(val, 0.f);
    float* dst = yp + (long long)m * p.y.cstride;
    if (ACCUM) val += *dst;
    *dst = val;
  }
}
// ------------------------------------------------------------------------------------
// launch helpers (pw_forms.hpp chooses the family, tile and split geometry)
// ------------------------------------------------------------------------------------
inline dim3 pwg_grid(const FwdArgs& a, int bm, int bn) {
  const long long P = (long long)a.B * a.T * a.V;   // < 2^31 (checked by the caller)
  return dim3((unsigned)cdiv(P, bn), (unsigned)cdiv(a.M, bm));
}

// pwg_fwd_kernel on a tile of kPwFwdTiles (false: another tile, nothing launched)
bool launch_pwg(const FwdArgs& a, const PwFwdTile& t, bool accum, hipStream_t st) {
  return with_form<kPwFwdTiles>(t, [&](auto BM, auto BN, auto WM, auto WN, auto AR, auto MASK,
                                       auto XROT, auto AMC, auto ACCUM) {
    pwg_fwd_kernel<BM, BN, WM, WN, MASK, XROT, AMC, ACCUM, false, AR>
        <<<pwg_grid(a, BM, BN), 64 * WM * WN, 0, st>>>(a);
  }, a.mask != nullptr, a.x.rsign != 0, a.a_mcontig != 0, accum);
}

// ... with the fused temporal-shift operand, on a tile of kPwTshTiles
bool launch_pwg_tsh(const FwdArgs& a, const PwFwdTile& t, hipStream_t st) {
  return with_form<kPwTshTiles>(t, [&](auto BM, auto BN, auto WM, auto WN, auto AR) {
    pwg_fwd_kernel<BM, BN, WM, WN, false, false, false, false, true, AR>
        <<<pwg_grid(a, BM, BN), 64 * WM * WN, 0, st>>>(a);
  });
}

// pwg_fwd_bf16_kernel on a tile of kPwBf16Tiles
bool launch_pwg_bf16(const FwdArgs& a, const PwBf16Tile& t, hipStream_t st) {
  return with_form<kPwBf16Tiles>(t, [&](auto BM, auto BN, auto WM, auto WN, auto AMC) {
    pwg_fwd_bf16_kernel<BM, BN, WM, WN, AMC><<<pwg_grid(a, BM, BN), 64 * WM * WN, 0, st>>>(a);
  }, a.a_mcontig != 0);
}

// The weight gradient's kernel on pw_dw_form's grid (a: slabs, chunks per split and byte
// ranges set), one launcher per family; false: a tile outside its list, nothing launched
bool launch_dwc(const DwArgs& a, const PwDwForm& f, hipStream_t st) {
  return with_form<kDwcForms>({a.Nc}, [&](auto NC, auto MASK) {
    pw_dw_smallc_kernel<NC, MASK><<<dim3(f.tiles, f.S), 256, 0, st>>>(a, f.per);
  }, a.mask != nullptr);
}

bool launch_dw3(const DwArgs& a, const PwDwForm& f, hipStream_t st) {
  return with_form<kDw3Tiles>(f.tile, [&](auto BM, auto BN, auto WM, auto WN, auto BKP, auto MASK,
                                          auto GROT, auto XROT, auto BIAS) {
    pw_dw3_kernel<BM, BN, WM, WN, BKP, MASK, GROT, XROT, BIAS>
        <<<dim3(f.tiles, f.S), 64 * WM * WN, 0, st>>>(a);
  }, a.mask != nullptr, a.g.rsign != 0, a.x.rsign != 0, a.bslab != nullptr);
}

// (operand form OP: 0 general, 1 plain = the buffer-descriptor fast path, 2 masked)
bool launch_dw(const DwArgs& a, const PwDwForm& f, bool plain, hipStream_t st) {
  return with_form<kDwTiles>(f.tile, [&](auto BM, auto BN, auto WM, auto WN, auto, auto OP) {
    constexpr bool MASK = OP == 2;
    pw_dw_kernel<BM, BN, WM, WN, MASK, OP == 1>
        <<<dim3(f.tiles, f.S), 64 * WM * WN, MASK ? (size_t)a.V * BN * sizeof(float) : 0, st>>>(a);
  }, OneOf<0, 1, 2>{a.mask ? 2 : plain});
}

// byte extent of a plane operand: one past its last addressed element
unsigned plane_bytes(long long bstride, long long cstride, int tstride, int B, int C, int T,
                     int V) {
  const long long e = (long long)(B - 1) * bstride + (long long)(C - 1) * cstride +
                      (long long)(T - 1) * tstride * V + V;
  return (unsigned)(e * 4);
}

// what every forward entry point requires of its sizes and its two planes (false: EINVAL):
// positions and per-operand offsets index in 32 bits, extents fit the buffer ranges
bool fwd_shape_ok(int B, int M, int K, int T, int V, const Plane& x, const OutPlane& y) {
  return B >= 0 && M > 0 && K > 0 && K <= kPwMaxK && T >= 0 && V > 0 && V < 32768 &&
         x.tstride >= 1 && y.tstride >= 1 && x.rsign >= -1 && x.rsign <= 1 &&
         y.rsign >= -1 && y.rsign <= 1 && x.cstride * (long long)K < (1LL << 31) &&
         y.cstride * (long long)M < (1LL << 31) && (long long)B * T * V < (1LL << 31) &&
         pw_extent(x.bstride, x.cstride, x.tstride, B, K, T, V) < kPwMaxElems &&
         pw_extent(y.bstride, y.cstride, y.tstride, B, M, T, V) < kPwMaxElems;
}

// what every forward entry point passes: weights (k- or m-contiguous), planes, sizes, divisors
// and byte ranges; every optional pointer (mask, ts, xs) starts null
FwdArgs fwd_args(const float* w, int w_mcontig, const float* bias, const Plane& x,
                 const OutPlane& y, int relu, int B, int M, int K, int T, int V) {
  FwdArgs a{};
  a.A = w;
  a.lda = w_mcontig ? M : K;
  a.a_mcontig = w_mcontig;
  a.bias = bias;
  a.x = x;
  a.y = y;
  a.M = M;
  a.K = K;
  a.T = T;
  a.V = V;
  a.B = B;
  fwd_divisors(a);
  a.x_bytes = plane_bytes(x.bstride, x.cstride, x.tstride, B, K, T, V);
  a.y_bytes = plane_bytes(y.bstride, y.cstride, y.tstride, B, M, T, V);
  a.a_bytes = (unsigned)((long long)M * K * 4);
  a.relu = relu ? 1 : 0;
  return a;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" {

int sgcn_pw_fwd(const float* w, int w_mcontig, const float* bias, const float* x,
                long long x_bstride, long long x_cstride, int x_tstride, int x_rsign,
                const float* mask, float* y, long long y_bstride, long long y_cstride,
                int y_tstride, int y_rsign, int relu, int accumulate, int B, int M, int K,
                int T, int V, void* stream) {
  const Plane xp{x, x_bstride, x_cstride, x_tstride, x_rsign};
  const OutPlane yp{y, y_bstride, y_cstride, y_tstride, y_rsign};
  SGCN_REQUIRE(fwd_shape_ok(B, M, K, T, V, xp, yp));
  SGCN_REQUIRE(!mask || V <= kMaskMaxV);
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(w && x && y);
  FwdArgs a = fwd_args(w, w_mcontig, bias, xp, yp, relu, B, M, K, T, V);
  a.mask = mask;
  a.mask_bytes = mask ? (unsigned)(V * K * 4) : 0u;
  hipStream_t st = (hipStream_t)stream;
  const bool ac = accumulate != 0;
  const PwFwdForm f = pw_fwd_form(M, K, mask != nullptr, x_rsign, y_rsign);
  bool ok;
  if (f.smallm) {
    const unsigned grid = (unsigned)cdiv((long long)B * T * V, 256);
    ok = with_consts([&](auto AMC, auto ACCUM) {
      pw_fwd_smallm_kernel<AMC, ACCUM><<<grid, 256, 0, st>>>(a);
    }, w_mcontig != 0, ac);
  } else {
    ok = launch_pwg(a, f.tile, ac, st);
  }
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  return 0;
}

int sgcn_pw_fwd_bf16(const float* w, int w_mcontig, const float* bias, const float* x,
                     long long x_bstride, long long x_cstride, int x_tstride, float* y,
                     long long y_bstride, long long y_cstride, int y_tstride, int y_rsign,
                     int relu, int B, int M, int K, int T, int V, void* stream) {
  const Plane xp{x, x_bstride, x_cstride, x_tstride, 0};
  const OutPlane yp{y, y_bstride, y_cstride, y_tstride, y_rsign};
  SGCN_REQUIRE(fwd_shape_ok(B, M, K, T, V, xp, yp));
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(w && x && y);
  const FwdArgs a = fwd_args(w, w_mcontig, bias, xp, yp, relu, B, M, K, T, V);
  SGCN_REQUIRE(launch_pwg_bf16(a, pw_fwd_bf16_form(M, K), (hipStream_t)stream));
  SGCN_LAUNCH_CHECK();
  return 0;
}

size_t sgcn_pw_tshift_ws_bytes(int K) { return ((size_t)K * kTsWords + 1) * sizeof(int); }

int sgcn_pw_fwd_tshift(const float* w, const float* bias, const float* x, long long x_bstride,
                       long long x_cstride, const float* xpos, const float* ypos,
                       const float* in_scale, const float* in_shift, float* x_shifted,
                       void* ws, size_t ws_bytes, float* y, long long y_bstride,
                       long long y_cstride, int relu, int two_row, int B, int M, int K, int T,
                       int V, void* stream) {
  const Plane xp{x, x_bstride, x_cstride, 1, 0};
  const OutPlane yp{y, y_bstride, y_cstride, 1, 0};
  SGCN_REQUIRE(fwd_shape_ok(B, M, K, T, V, xp, yp));
  SGCN_REQUIRE(two_row >= 0 && two_row <= 2);
  SGCN_REQUIRE((in_scale == nullptr) == (in_shift == nullptr));
  SGCN_REQUIRE(x_cstride >= (long long)T * V && y_cstride >= (long long)T * V);
  if (B == 0 || T == 0) return 0;
  SGCN_REQUIRE(w && x && y && xpos && ypos && ws && ws_bytes >= sgcn_pw_tshift_ws_bytes(K));
  hipStream_t st = (hipStream_t)stream;
  tshift_params_kernel<<<(K + 63) / 64, 64, 0, st>>>(xpos, ypos, in_scale, in_shift, K, V,
                                                     two_row, (int*)ws);
  tshift_two_row_flag_kernel<<<1, 256, 0, st>>>(K, (int*)ws);
  SGCN_LAUNCH_CHECK();
  FwdArgs a = fwd_args(w, 0, bias, xp, yp, relu, B, M, K, T, V);
  a.ts = (const int*)ws;
  a.xs = x_shifted;
  SGCN_REQUIRE(launch_pwg_tsh(a, pw_tshift_form(M), st));
  SGCN_LAUNCH_CHECK();
  return 0;
}

size_t sgcn_pw_dw_ws_bytes(int B, int M, int Nc, int T, int V) {
  return pw_dw_form(B, M, Nc, T, V).ws_bytes;
}

int sgcn_pw_dw(const float* g, long long g_bstride, long long g_cstride, int g_tstride,
               int g_rsign, const float* x, long long x_bstride, long long x_cstride,
               int x_tstride, int x_rsign, const float* mask, float* dw, int dw_transpose,
               int dw_accumulate, float* dbias, int dbias_accumulate, void* ws,
               size_t ws_bytes, int B, int M, int Nc, int T, int V, void* stream) {
  SGCN_REQUIRE(B > 0 && M > 0 && Nc > 0 && T > 0 && V > 0 && V < 32768);
  SGCN_REQUIRE(g && x && dw && ws && g_tstride >= 1 && x_tstride >= 1);
  SGCN_REQUIRE(g_rsign >= -1 && g_rsign <= 1 && x_rsign >= -1 && x_rsign <= 1);
  SGCN_REQUIRE(!mask || V <= kMaskMaxV);
  const PwDwForm f = pw_dw_form(B, M, Nc, T, V);
  SGCN_REQUIRE(ws_bytes >= f.ws_bytes);
  SGCN_REQUIRE(g_cstride * (long long)M < (1LL << 31) && x_cstride * (long long)Nc < (1LL << 31));
  const long long ge = pw_extent(g_bstride, g_cstride, g_tstride, B, M, T, V);
  const long long xe = pw_extent(x_bstride, x_cstride, x_tstride, B, Nc, T, V);
  const bool plain = pw_dw_plain(mask != nullptr, g_rsign, x_rsign, ge, xe);
  if (f.family == DwFamily::dw3) SGCN_REQUIRE(ge < kPwMaxElems && xe < kPwMaxElems);
  DwArgs a{{g, g_bstride, g_cstride, g_tstride, g_rsign},
           {x, x_bstride, x_cstride, x_tstride, x_rsign}, mask, (float*)ws, nullptr, M, Nc, T, V,
           B, f.per};   // (the byte ranges start 0)
  if (dbias) a.bslab = a.slab + (size_t)f.S * M * Nc;
  if (f.family == DwFamily::dw3 || plain) {   // the byte ranges of their buffer loads
    a.g_bytes = plane_bytes(g_bstride, g_cstride, g_tstride, B, M, T, V);
    a.x_bytes = plane_bytes(x_bstride, x_cstride, x_tstride, B, Nc, T, V);
    a.mask_bytes = mask ? (unsigned)(V * Nc * 4) : 0u;
  }
  hipStream_t st = (hipStream_t)stream;
  bool ok = true;
  if (f.family == DwFamily::smallc) ok = launch_dwc(a, f, st);
  else if (f.family == DwFamily::dw3) ok = launch_dw3(a, f, st);
  else ok = launch_dw(a, f, plain, st);
  SGCN_REQUIRE(ok);
  SGCN_LAUNCH_CHECK();
  launch_slab_reduce(a.slab, a.bslab, f.S, M, Nc, dw, dw_transpose, dw_accumulate, dbias,
                     dbias_accumulate, st);
  SGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
