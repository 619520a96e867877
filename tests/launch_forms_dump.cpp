// Prints what shift-gcn_amd/csrc/launch_forms.hpp and pw_forms.hpp decide, for
// tests/test_launch_forms.py to compare with the Python mirrors (oracle/stream_cases.py,
// oracle/tshift_cases.py, oracle/pw_cases.py): the shared constants, every form and tile list,
// then one line per plane and chooser over the ranges the mirrors' reachable() enumerate, one
// per contraction size, and one per "B M Nc T V" line of standard input. Host-only: builds
// with any C++17 compiler, needs no GPU.
//
//   const <name> <value>
//   list <name> <nt> <lpt>
//   tile <name> <bm> <bn> <wm> <wn> <ar | bkp>      (kDwcForms: tile <name> <nc>)
//   <chooser> <H> <W> <stride | down | 0> <kind> <nt> <lpt> <flag>
//   pwfwd <M> <K> <mask> <x_rsign> <y_rsign> <smallm | pwg> <bm> <bn> <ar>
//   pwtsh <M> <bm> <bn>
//   pwdw <B> <M> <Nc> <T> <V> <smallc | dw3 | dw> <bm> <bn> <bkp> <tiles> <S> <per> <ws bytes>
//        <use_dwc> <use_dw3>
#include <cstdio>

#include "../shift-gcn_amd/csrc/launch_forms.hpp"
#include "../shift-gcn_amd/csrc/pw_forms.hpp"

using namespace sgcn;

static const char* kind_name(Kind k) {
  switch (k) {
    case Kind::refuse: return "refuse";
    case Kind::empty: return "empty";
    case Kind::ja: return "ja";
    case Kind::loop: return "loop";
    case Kind::pad: return "pad";
    case Kind::lds: return "lds";
    case Kind::global: return "global";
    case Kind::ra: return "ra";
    case Kind::s2: return "s2";
  }
  return "?";
}

template <int N>
static void list(const char* name, const Form (&forms)[N]) {
  for (const Form& f : forms) std::printf("list %s %d %d\n", name, f.nt, f.lpt);
}

static void plane(const char* chooser, int H, int W, int arg, const LaunchForm& f) {
  std::printf("%s %d %d %d %s %d %d %d\n", chooser, H, W, arg, kind_name(f.kind), f.nt, f.lpt,
              (int)f.flag);
}

template <class T, int N>
static void tiles(const char* name, const T (&list)[N]) {
  for (const T& t : list) {
    const auto [bm, bn, wm, wn, x] = t.fields();
    std::printf("tile %s %d %d %d %d %d\n", name, bm, bn, wm, wn, (int)x);
  }
}

static void contractions() {
  std::printf("const kMaskMaxV %d\nconst kPwMaxK %d\nconst kPwMaxElems %lld\n", kMaskMaxV,
              kPwMaxK, kPwMaxElems);
  std::printf("const kSmallM %d\nconst kDwBK %d\nconst kDwcRows %d\nconst kDwcMaxC %d\n",
              kSmallM, kDwBK, kDwcRows, kDwcMaxC);
  std::printf("const SGCN_DW3_MIN %d\nconst SGCN_DW3_BKP_BIG %d\n", SGCN_DW3_MIN,
              SGCN_DW3_BKP_BIG);
  tiles("kPwFwdTiles", kPwFwdTiles);
  tiles("kPwTshTiles", kPwTshTiles);
  tiles("kDw3Tiles", kDw3Tiles);
  tiles("kDwTiles", kDwTiles);
  for (const PwDwcForm& f : kDwcForms) std::printf("tile kDwcForms %d\n", f.nc);
  for (int M = 1; M <= 300; ++M) {
    for (int K = 1; K <= kPwMaxK; ++K)
      for (int flags = 0; flags < 8; ++flags) {
        const int mask = flags >> 2, xr = (flags >> 1) & 1, yr = flags & 1;
        const PwFwdForm f = pw_fwd_form(M, K, mask != 0, xr, yr);
        std::printf("pwfwd %d %d %d %d %d %s %d %d %d\n", M, K, mask, xr, yr,
                    f.smallm ? "smallm" : "pwg", f.tile.bm, f.tile.bn, (int)f.tile.ar);
      }
    const PwFwdTile t = pw_tshift_form(M);
    std::printf("pwtsh %d %d %d\n", M, t.bm, t.bn);
  }
  int B, M, Nc, T, V;
  while (std::scanf("%d %d %d %d %d", &B, &M, &Nc, &T, &V) == 5) {
    const PwDwForm f = pw_dw_form(B, M, Nc, T, V);
    const char* family[] = {"smallc", "dw3", "dw"};
    std::printf("pwdw %d %d %d %d %d %s %d %d %d %d %d %d %zu %d %d\n", B, M, Nc, T, V,
                family[(int)f.family], f.tile.bm, f.tile.bn, f.tile.bkp, f.tiles, f.S, f.per,
                f.ws_bytes, (int)use_dwc(Nc), (int)use_dw3(M, Nc));
  }
}

int main() {
  list("kJaForms", kJaForms);
  list("kPadFwdForms", kPadFwdForms);
  list("kLdsFwdForms", kLdsFwdForms);
  list("kRaForms", kRaForms);
  list("kGbdForms", kGbdForms);
  list("kBninForms", kBninForms);
  // past the largest threshold nothing new can appear
  const int n_max = kFwdLdsMax2 + 2 * kThreads;
  // the stream_cases choosers: V <= kThreads, and one column past it (bn_form refuses)
  for (int V = 1; V <= kThreads + 1; ++V)
    for (int T = 1; T < n_max / V + 2; ++T) {
      plane("bn", T, V, 0, bn_form(T, V));
      plane("fused", T, V, 0, fwd_fused_form(T, V));
      plane("bnin", T, V, 0, bnin_form(T, V));
    }
  // the tshift_cases choosers: W <= 130
  for (int W = 1; W <= 130; ++W)
    for (int H = 1; H < n_max / W + 2; ++H) {
      for (int stride = 1; stride <= 2; ++stride) {
        plane("fwd", H, W, stride, tshift_fwd_form(H, W, stride));
        plane("bwd", H, W, stride, bwd_form(H, W, stride));
      }
      for (int down = 0; down <= 1; ++down) plane("gbn", H, W, down, gbn_form(H, W, down != 0));
    }
  contractions();
  return 0;
}
