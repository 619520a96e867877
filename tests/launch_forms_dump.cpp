// Prints what shift-gcn_amd/csrc/launch_forms.hpp decides, for tests/test_launch_forms.py to
// compare with the Python mirrors (oracle/stream_cases.py, oracle/tshift_cases.py): every
// form list, then one line per plane and chooser over the ranges the mirrors' reachable()
// enumerate. Host-only: builds with any C++17 compiler, needs no GPU.
//
//   list <name> <nt> <lpt>
//   <chooser> <H> <W> <stride | down | 0> <kind> <nt> <lpt> <flag>
#include <cstdio>

#include "../shift-gcn_amd/csrc/launch_forms.hpp"

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
  return 0;
}
