// Prints what shift-gcn_amd/csrc/pw_forms.hpp decides for sgcn_pw_fwd_bf16, for
// tests/test_bf16_forms.py to compare with the Python mirror (tests/bf16_cases.py): the
// constants, the tile list, then one line per contraction size M <= 300, K <= kPwMaxK.
// Host-only: builds with any C++17 compiler, needs no GPU.
//
//   const <name> <value>
//   tile kPwBf16Tiles <bm> <bn> <wm> <wn>
//   pwbf16 <M> <K> <bm> <bn> <wm> <wn>
#include <cstdio>

#include "../shift-gcn_amd/csrc/pw_forms.hpp"

using namespace sgcn;

int main() {
  std::printf("const kPwBf16BK %d\n", kPwBf16BK);
  std::printf("const kPwMaxK %d\n", kPwMaxK);
  std::printf("const kSmallM %d\n", kSmallM);
  for (const PwBf16Tile& t : kPwBf16Tiles)
    std::printf("tile kPwBf16Tiles %d %d %d %d\n", t.bm, t.bn, t.wm, t.wn);
  for (int M = 1; M <= 300; ++M)
    for (int K = 1; K <= kPwMaxK; ++K) {
      const PwBf16Tile t = pw_fwd_bf16_form(M, K);
      std::printf("pwbf16 %d %d %d %d %d %d\n", M, K, t.bm, t.bn, t.wm, t.wn);
    }
  return 0;
}
