// Which kernel, tile and split geometry a pointwise contraction (pwconv.hip) runs: the
// constants its choosers and kernels share, the build-time knobs, one function per entry
// point that returns the whole decision and, per launcher, the tiles it instantiates.
// Host-only and HIP-free like launch_forms.hpp: the entry points call these and nothing else
// decides a form, tests/launch_forms_dump.cpp prints them, and tests/test_launch_forms.py
// compares that print with the Python mirrors (oracle/pw_cases.py, shiftgcn.ops.PW_MAX_ELEMS).
#pragma once
#include <cstddef>
#include <tuple>

namespace sgcn {

constexpr int kMaskMaxV = 64;                  // joints per row supported by the mask tables
constexpr int kPwMaxK = 256;                   // contraction length of the forward kernels
constexpr long long kPwMaxElems = 1LL << 29;   // operand extent (elements) a buffer range holds
constexpr int kSmallM = 4;                     // pw_fwd_smallm_kernel output rows
constexpr int kDwBK = 64;                      // pw_dw_kernel positions per chunk
#ifndef SGCN_DWC_ROWS
#define SGCN_DWC_ROWS 16
#endif
constexpr int kDwcRows = SGCN_DWC_ROWS;        // pw_dw_smallc_kernel G rows per wave (4 waves)
constexpr int kDwcMaxC = 4;                    // ... and its input channels

constexpr long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// the bound on a plane operand's extent (elements) the entry points hold below kPwMaxElems
inline long long pw_extent(long long bstride, long long cstride, int tstride, int B, int C, int T,
                           int V) {
  return (long long)(B - 1) * bstride + (long long)C * cstride + (long long)T * tstride * V;
}

// ------------------------------------------------------------------------------------
// sgcn_pw_fwd / sgcn_pw_fwd_tshift: BM x BN tile on WM x WN waves; ar = A resident in LDS
// ------------------------------------------------------------------------------------
struct PwFwdTile {
  int bm, bn, wm, wn;
  bool ar;
  constexpr auto fields() const { return std::make_tuple(bm, bn, wm, wn, ar); }
};
// 64 < M <= 128: 128 x 128 tiles on 8 waves (32 x 64 per wave, twice the workgroups of the
// 128 x 256 tile): pw_fwd class -1.8 %, step +0.1..0.25 % same-box (profiles/r04_tiles/;
// 64 x 128 / 4-wave tiles at M <= 64 and 128 x 128 / 256 x 64 tiles at M > 128 measured
// there too, not better)
constexpr PwFwdTile kPwFwdTiles[] = {{64, 256, 2, 4, false}, {64, 256, 2, 4, true},
                                     {128, 128, 4, 2, false}, {256, 128, 4, 2, false}};
// (the plain path's 128 x 128 tile at 64 < M <= 128 measured no better for the fused
// temporal-shift operand, profiles/r06_x1/tshbench_tile128x128.txt)
constexpr PwFwdTile kPwTshTiles[] = {{64, 256, 2, 4, false}, {128, 256, 2, 4, false},
                                     {256, 128, 4, 2, false}};

#ifndef SGCN_SMALLM
#define SGCN_SMALLM 1   // A/B knob: pw_fwd_smallm_kernel at M <= kSmallM
#endif
#ifndef SGCN_PW_AR
#define SGCN_PW_AR 1    // A/B knob: the A-resident K <= 64 forward tile (pwg_fwd_kernel AR)
#endif
struct PwFwdForm {
  bool smallm;      // pw_fwd_smallm_kernel (no tile); else pwg_fwd_kernel on tile
  PwFwdTile tile;
};
inline PwFwdForm pw_fwd_form(int M, int K, bool mask, int x_rsign, int y_rsign) {
  if (M <= kSmallM && SGCN_SMALLM && !mask && x_rsign == 0 && y_rsign == 0) return {true, {}};
  // 16 < K <= 64 (HBM-bound): A resident in LDS, one B buffer -> four workgroups per CU
  // (one K stage, K <= 16, gains nothing from it: l1's K = 3 measured 4 % slower)
  if (M <= 64) return {false, kPwFwdTiles[K > 16 && K <= 64 && SGCN_PW_AR ? 1 : 0]};
  return {false, kPwFwdTiles[M <= 128 ? 2 : 3]};
}
inline PwFwdTile pw_tshift_form(int M) { return kPwTshTiles[M <= 64 ? 0 : (M <= 128 ? 1 : 2)]; }

// ------------------------------------------------------------------------------------
// sgcn_pw_fwd_bf16 (eval-mode inference, bf16 operands on v_mfma_f32_32x32x16_bf16):
// BM x BN tile on WM x WN waves, 32 k per LDS stage. The fp32 forward's tile footprints; M
// past 256 takes more row blocks of the 256-row tile. K does not enter the choice.
// ------------------------------------------------------------------------------------
struct PwBf16Tile {
  int bm, bn, wm, wn;
  constexpr auto fields() const { return std::make_tuple(bm, bn, wm, wn); }
};
constexpr int kPwBf16BK = 32;                  // k per stage (two MFMA k-steps of 16)
constexpr PwBf16Tile kPwBf16Tiles[] = {{64, 256, 2, 4}, {128, 128, 4, 2}, {256, 128, 4, 2}};
inline PwBf16Tile pw_fwd_bf16_form(int M, int K) {
  (void)K;
  return kPwBf16Tiles[M <= 64 ? 0 : (M <= 128 ? 1 : 2)];
}

// ------------------------------------------------------------------------------------
// sgcn_pw_dw: family, tile and split-K geometry
// ------------------------------------------------------------------------------------
struct PwDwTile {
  int bm, bn, wm, wn, bkp;   // bkp: positions per chunk
  constexpr auto fields() const { return std::make_tuple(bm, bn, wm, wn, bkp); }
};
struct PwDwcForm {
  int nc;
  constexpr auto fields() const { return std::make_tuple(nc); }
};
// positions per chunk of the 256-row weight-gradient tiles (A/B knob: 8 halves their LDS,
// 74 -> 37 KB at 256 x 256, leaving room on the CU for the critical path's kernels while
// the side stream runs them)
#ifndef SGCN_DW3_BKP_BIG
#define SGCN_DW3_BKP_BIG 16
#endif
constexpr PwDwTile kDw3Tiles[] = {{128, 128, 2, 2, 16},
                                  {256, 128, 4, 2, SGCN_DW3_BKP_BIG},
                                  {256, 256, 4, 2, SGCN_DW3_BKP_BIG}};
constexpr PwDwTile kDwTiles[] = {{64, 64, 2, 2, kDwBK}, {64, 128, 2, 2, kDwBK},
                                 {128, 64, 4, 2, kDwBK}, {128, 128, 4, 2, kDwBK}};
constexpr PwDwcForm kDwcForms[] = {{1}, {2}, {3}, {4}};

// pw_dw_smallc_kernel: Nc <= 4; ~1,024 workgroups of 4 x 16 rows over position splits
#ifndef SGCN_DWC
#define SGCN_DWC 1
#endif
inline bool use_dwc(int Nc) { return SGCN_DWC && Nc <= kDwcMaxC; }
inline int dwc_splits(int M, long long P) {
  const long long mg = cdiv(M, 4 * kDwcRows);
  long long S = cdiv(1024, mg);
  if (cdiv(P, S) < 256) S = cdiv(P, 256);   // at least four 64-position steps per split
  return (int)(S < 1 ? 1 : S);
}

// pw_dw3 measured faster from 128x128 contractions up (tools/bench/pwbench: l5/l6 tcn,
// l9 tcn/gcn), equal or slower on the 64-wide masked/rotated ones
#ifndef SGCN_DW3_MIN
#define SGCN_DW3_MIN (128 * 128)
#endif
static_assert(SGCN_DW3_MIN >= 128 * 128,
              "pw_dw3_kernel's 64 x 64, 128 x 64 and 64 x 128 tiles were removed as unreachable "
              "(M * Nc >= 128 * 128 excludes them): a smaller SGCN_DW3_MIN needs them back");
inline bool use_dw3(int M, int Nc) { return (long long)M * Nc >= SGCN_DW3_MIN; }

struct Dw3Cfg {
  PwDwTile tile;
  int target;   // workgroups aimed at
};
inline Dw3Cfg dw3_cfg(int M, int Nc) {
  if (M <= 128 && Nc <= 128) return {kDw3Tiles[0], 1024};
  return {kDw3Tiles[Nc <= 128 ? 1 : 2], 512};
}
// split count for pw_dw3: ~target workgroups, slab <= 64 MiB, >= 1 chunk per split
inline int dw3_splits(int M, int Nc, long long P, int bkp, int tiles, int target) {
  long long S = cdiv(target, tiles);
  const long long cap = (64LL << 20) / (4LL * M * Nc), nch = cdiv(P, bkp);
  if (S > cap) S = cap;
  if (S > nch) S = nch;
  return (int)(S < 1 ? 1 : S);
}

inline PwDwTile dw_tile(int M, int Nc) { return kDwTiles[(M > 64 ? 2 : 0) + (Nc > 64 ? 1 : 0)]; }
// ~512 workgroups (2 per CU at pw_dw_kernel's register budget); slab <= 16 MiB
inline int dw_splits(int M, int Nc, int B, int N, int tiles) {
  const long long total = B * cdiv(N, kDwBK);
  long long S = cdiv(512, tiles);
  const long long cap = (16LL << 20) / (4LL * M * Nc);
  if (S > cap) S = cap;
  if (S > total) S = total;
  return (int)(S < 1 ? 1 : S);
}

enum class DwFamily { smallc, dw3, dw };
struct PwDwForm {
  DwFamily family;
  PwDwTile tile;     // smallc: a workgroup's 4 waves x kDwcRows rows by Nc, 64 positions a step
  int tiles, S;      // the launch grid: tiles x splits
  int per;           // chunks (smallc: positions) per split
  size_t ws_bytes;   // S slabs of M x Nc partial sums and M row sums
};
inline PwDwForm pw_dw_form(int B, int M, int Nc, int T, int V) {
  const long long P = (long long)B * T * V;
  const Dw3Cfg c = dw3_cfg(M, Nc);
  PwDwForm f{DwFamily::dw, dw_tile(M, Nc)};
  if (use_dwc(Nc)) f = {DwFamily::smallc, {4 * kDwcRows, Nc, 4, 1, 64}};
  else if (use_dw3(M, Nc)) f = {DwFamily::dw3, c.tile};
  f.tiles = (int)(cdiv(M, f.tile.bm) * cdiv(Nc, f.tile.bn));
  long long work = P;   // what the splits divide: positions, or chunks of them
  if (f.family == DwFamily::smallc) {
    f.S = dwc_splits(M, P);
  } else if (f.family == DwFamily::dw3) {   // ... of the positions flattened over the samples
    work = cdiv(P, f.tile.bkp);
    f.S = dw3_splits(M, Nc, P, f.tile.bkp, f.tiles, c.target);
  } else {                                  // ... of each sample's plane
    work = B * cdiv((long long)T * V, kDwBK);
    f.S = dw_splits(M, Nc, B, T * V, f.tiles);
  }
  f.per = (int)cdiv(work, f.S);
  f.ws_bytes = (size_t)f.S * ((size_t)M * Nc + M) * sizeof(float);
  return f;
}

// pw_dw_kernel's buffer-descriptor fast path: plain operands whose extents fit a range
#ifndef SGCN_DW_PLAIN
#define SGCN_DW_PLAIN 1   // A/B knob
#endif
inline bool pw_dw_plain(bool mask, int g_rsign, int x_rsign, long long g_extent,
                        long long x_extent) {
  return !mask && g_rsign == 0 && x_rsign == 0 && SGCN_DW_PLAIN && g_extent < kPwMaxElems &&
         x_extent < kPwMaxElems;
}

}  // namespace sgcn
