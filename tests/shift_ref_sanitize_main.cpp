// Stand-alone sanitizer run of the reference temporal-shift kernels as oracle/ref_build.py
// builds them for the host. Run BY HAND on a CPU machine that has the reference tree, never
// by pytest and never on a GPU machine:
//
//   python oracle/ref_build.py          (or build(): writes oracle/_ref/shift_ref_tu.cpp)
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I oracle/_ref tests/shift_ref_sanitize_main.cpp \
//       -o /tmp/shift_ref_sanitize && /tmp/shift_ref_sanitize
//
// It drives every entry point of the generated translation unit over the plane and position
// range of tests/test_oracle_shift_ref.py's sweep (H 0..12 x W 1..9, stride 1, 2 and 3,
// float and double, |pos| up to 2^20, the doubles that round to a float across an integer),
// with every buffer allocated at its exact extent so that an out-of-bounds tap is a
// heap-buffer-overflow. A clean exit (status 0, "clean" printed) is what justifies using the
// host build in place of the CUDA one inside that position range: no float -> int conversion
// out of range, no signed overflow in the index sums, no read or write outside a plane.
#include "shift_ref_tu.cpp"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
struct Lcg {
  uint64_t s;
  double next() {  // uniform in (-2, 2)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(s >> 11) / 9007199254740992.0) * 4.0 - 2.0;
  }
};

template <typename T>
std::vector<T> filled(size_t n, Lcg& r) {
  std::vector<T> v(n);
  for (auto& e : v) e = (T)r.next();
  return v;
}

template <typename T>
double sweep(bool edges) {
  const int B = 2, C = 16;
  const double big = 1048576.0;
  double sum = 0;
  Lcg rng{sizeof(T) * 977u + (edges ? 1u : 0u)};
  for (int H = 0; H <= 12; ++H)
    for (int W = 1; W <= 9; ++W) {
      const double xs[16] = {0.0, 1e-8, -1e-8, 1.0, -2.0, 3.0, 0.5, -1.5, 0.3, -0.7, W + 1.25,
                             -(W + 2.5), big, -big + 0.5, 2.5, -0.25};
      const double ys[16] = {0.0, -1e-8, 1e-8, -1.0, 2.0, -4.0, -0.5, 3.5, 1.3, -2.75,
                             -(H + 1.5), H + 2.25, -big, big - 0.5, 5.0, 0.75};
      const double edge[6] = {1.0 - 1e-12, -1e-50, -1.0 - 1e-12, 1e-50, 3.0 - 1e-13,
                              -(2.0 + 1e-12)};
      for (int rot = 0; rot < 16; rot += 5) {
        std::vector<T> xp(C), yp(C);
        for (int c = 0; c < C; ++c) {
          xp[c] = (T)xs[c];
          yp[c] = (T)ys[(c + rot) % 16];
          if (edges && c < 6) xp[c] = (T)edge[c];
          if (edges && c >= 6 && c < 12) yp[c] = (T)edge[c - 6];
        }
        auto in = filled<T>((size_t)B * C * H * W, rng);
        for (int stride = 1; stride <= 3; ++stride) {
          const size_t nout = (size_t)B * C * (H / stride) * W;
          std::vector<T> out(nout, (T)0);
          drv_forward<T>(in.data(), out.data(), xp.data(), yp.data(), B, C, H, W, stride);
          for (T e : out) sum += (double)e;
          if (stride > 2) continue;
          auto g = filled<T>(nout, rng);
          std::vector<T> gin(in.size(), (T)0), gxb(nout, (T)0), gyb(nout, (T)0);
          if (stride == 1)
            drv_bottom_s1<T>(g.data(), gin.data(), xp.data(), yp.data(), B, C, H, W);
          else
            drv_bottom_s2<T>(g.data(), gin.data(), xp.data(), yp.data(), B, C, H, W);
          drv_position<T>(in.data(), g.data(), xp.data(), yp.data(), gxb.data(), gyb.data(), B,
                          C, H, W, stride);
          for (T e : gin) sum += (double)e;
          std::vector<T> gx(C, (T)0), gy(C, (T)0);
          for (size_t i = 0; i < nout; ++i) {
            gx[(i / ((size_t)(H / stride) * W)) % C] += gxb[i];
            gy[(i / ((size_t)(H / stride) * W)) % C] += gyb[i];
          }
          drv_constraint<T>(gx.data(), gy.data(), C);
          for (T e : gy) sum += (double)e;
        }
      }
    }
  return sum;
}
}  // namespace

int main() {
  const double a = sweep<float>(false), b = sweep<double>(false), c = sweep<double>(true);
  std::printf("checksums %.9g %.9g %.9g\nclean\n", a, b, c);
  return 0;
}
