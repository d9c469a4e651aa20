// Host check of the visual-odometry arithmetic (csrc/odometry_math.h, the text the kernels of csrc/odometry.hip compile): the
// bilinear sample and the weight at their edge values, a pixel's validity tests on NaN, infinities and footprints that leave
// the image (nothing is converted to int before it is compared; every image is read through a checked size), the 29 sums of
// identical images, the exponents' bound, the 6x6 solve against a known system, the Cayley matrix's orthogonality, a step
// composed with its inverse, and the formation of G.  Plain C++, no device, no HIP header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <package>/csrc \
//       tools/odometry_math_check.cpp -o odometry_check && ./odometry_check
// Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "odometry_math.h"

namespace {

int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++failures;                                         \
    }                                                     \
  } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNan = std::numeric_limits<float>::quiet_NaN();
const float kEye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

OmLevel level(int H, int W) {
  OmLevel L = {40.f, (W - 1) * 0.5f, (H - 1) * 0.5f, 0.f, 0.0625f, 64.f, 0.125f, {1, 1, 1, 1, 1, 1}, H, W, 4, 2048};
  int e[6];
  om_exponents(40.0, (W - 1) * 0.5, (H - 1) * 0.5, 0.0, 64.0, H, W, e);
  for (int i = 0; i < 6; ++i) L.scale[i] = ldexpf(1.f, e[i]);
  return L;
}

void check_sample_and_weight() {
  const unsigned char I[4] = {10, 250, 0, 255};                     // 2 x 2
  CHECK(om_bilinear16(I, 2, 0, 0, 0, 0) == 2560 && om_bilinear16(I, 2, 0, 0, 15, 0) == 16 * (10 + 15 * 250), "along the row");
  CHECK(om_bilinear16(I, 2, 0, 0, 15, 15) == 10 + 15 * 250 + 0 + 225 * 255, "the far corner has weight 225 / 256");
  const unsigned char full[4] = {255, 255, 255, 255};
  for (int fx = 0; fx < 16; ++fx)
    for (int fy = 0; fy < 16; ++fy) CHECK(om_bilinear16(full, 2, 0, 0, fx, fy) == 255 * 256, "a constant stays one");
  CHECK(om_weight(0, 2048) == 64 && om_weight(-2048, 2048) == 64 && om_weight(2049, 2048) == 63 && om_weight(-65280, 2048) == 2 &&
            om_weight(65280, 1) == 0 && om_weight(65280, 65280) == 64,
        "the weight");
}

void check_pixels() {
  const int H = 9, W = 13;
  const OmLevel L = level(H, W);
  std::vector<unsigned char> Ip((size_t)H * W), Ic((size_t)H * W);
  std::vector<float> D((size_t)H * W, 5.f);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) Ip.at((size_t)v * W + u) = Ic.at((size_t)v * W + u) = (unsigned char)(17 * u + 5 * v * v);
  long long S[OM_SUMS] = {0};
  OmPixel p;
  for (int v = 1; v < H - 1; ++v)
    for (int u = 1; u < W - 1; ++u) {
      CHECK(om_pixel(L, kEye, Ip.data(), Ic.data(), D.data(), u, v, &p), "u %d v %d", u, v);
      CHECK(p.r == 0 && p.w == 64, "identical images: r %d", p.r);
      for (int i = 0; i < 6; ++i) CHECK(std::abs(p.q[i]) < (1 << 18), "q[%d] = %d", i, p.q[i]);
      om_accumulate(S, p);
    }
  CHECK(S[OM_N] == (H - 2) * (W - 2) && S[OM_RR] == 0 && S[0] > 0, "the count");
  for (int i = 0; i < 6; ++i) CHECK(S[OM_B + i] == 0, "w q r of identical images");
  for (float d : {kNan, kInf, -kInf, 0.f, -3.f, 0.06f, 64.f, 1e30f}) {
    D.at(4 * W + 6) = d;
    CHECK(!om_pixel(L, kEye, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "d %g", (double)d);
  }
  D.at(4 * W + 6) = 5.f;
  // the footprint leaves the image on every side, and by far; the last admitted position is 16 (W - 1) - 1 sixteenths
  for (float shift : {-6.1f, 6.f, -1e30f, 1e30f, kInf, kNan}) {
    float g[12];
    memcpy(g, kEye, sizeof g);
    g[2] = shift;
    CHECK(!om_pixel(L, g, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "column shift %g", (double)shift);
    memcpy(g, kEye, sizeof g);
    g[6] = shift < 0 ? shift + 2.f : shift - 2.f;
    CHECK(!om_pixel(L, g, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "row shift %g", (double)shift);
  }
  float g[12];
  memcpy(g, kEye, sizeof g);
  g[2] = 5.9375f;                                                   // 6 + 5.9375 = 11.9375 = 16 * 12 - 1 sixteenths: x0 = 11, fx = 15
  CHECK(om_pixel(L, g, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "the last position inside");
  g[2] = -6.f;
  CHECK(om_pixel(L, g, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "column 0");
  for (float z : {0.1f, 0.f, -1.f, kNan}) {
    memcpy(g, kEye, sizeof g);
    g[10] = z;
    CHECK(!om_pixel(L, g, Ip.data(), Ic.data(), D.data(), 6, 4, &p), "ratio %g", (double)z);
  }
  std::vector<unsigned char> flat((size_t)H * W, 77);
  CHECK(!om_pixel(L, kEye, flat.data(), Ic.data(), D.data(), 6, 4, &p), "no gradient");
}

void check_exponents() {
  int e[6];
  om_exponents(700.0, 620.5, 187.0, 0.0, 192.0, 375, 1242, e);
  const double A = 620.5, Bv = 187.0, Dn = 192.0, f = 700.0;
  const double B[6] = {Dn, Dn, A * Dn / f, f + Bv * Bv / f, f + A * A / f, A};
  for (int i = 0; i < 6; ++i) {
    const double top = 510.0 * B[i] * std::ldexp(1.0, e[i]);
    CHECK(top <= 131072.0 && top > 65536.0 * 0.999, "e[%d] = %d: %g", i, e[i], top);
  }
  double fl, cxl, cyl, dl;
  om_level_camera(700.0, 620.5, 187.0, 3.0, 2, &fl, &cxl, &cyl, &dl);
  CHECK(fl == 175.0 && cxl == 154.75 && cyl == 46.375 && dl == 0.75, "the camera of level 2");
}

void check_solve() {
  // A = M M^T + I for a fixed M, x known: the solve returns it to rounding
  double M[6][6], A[6][6], x0[6], c[6], x[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) M[i][j] = std::sin(1.0 + 3.0 * i + 7.0 * j);
  for (int i = 0; i < 6; ++i) {
    x0[i] = 1.5 - i;
    for (int j = 0; j < 6; ++j) {
      A[i][j] = i == j ? 1.0 : 0.0;
      for (int k = 0; k < 6; ++k) A[i][j] += M[i][k] * M[j][k];
    }
  }
  for (int i = 0; i < 6; ++i) {
    c[i] = 0.0;
    for (int j = 0; j < 6; ++j) c[i] += A[i][j] * x0[j];
  }
  CHECK(om_ldl_solve(A, c, x), "a positive definite system");
  for (int i = 0; i < 6; ++i) CHECK(std::fabs(x[i] - x0[i]) < 1e-12, "x[%d] = %.17g", i, x[i]);
  A[3][3] = -1.0;
  CHECK(!om_ldl_solve(A, c, x), "a pivot that is not positive");
  A[3][3] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!om_ldl_solve(A, c, x), "a NaN pivot");
  long long S[OM_SUMS] = {0};
  const int e[6] = {2, 2, 5, 3, 3, 8};
  double xi[6], R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tau[3] = {0, 0, 0};
  CHECK(!om_step(S, e, xi) && !om_update(S, e, 6, R, tau), "no pixel: no pivot");
  for (int i = 0; i < 6; ++i) S[om_upper(i, i)] = (1LL << 40) + i, S[OM_B + i] = (long long)(i - 2) * (1LL << 30);
  S[OM_N] = 100, S[OM_RR] = 1LL << 30;
  CHECK(om_upper(0, 0) == 0 && om_upper(0, 5) == 5 && om_upper(1, 1) == 6 && om_upper(5, 5) == 20, "the order of the 21");
  CHECK(om_step(S, e, xi), "a diagonal system");
  for (int i = 0; i < 6; ++i) {
    const double want = (double)S[OM_B + i] * std::ldexp(1.0, e[i] - 7) / ((double)S[om_upper(i, i)] * (1.0 + 1.0 / 1024.0));
    CHECK(std::fabs(xi[i] - want) <= 1e-14 * std::fabs(want), "xi[%d]", i);
  }
  CHECK(!om_update(S, e, 101, R, tau) && R[0] == 1.0 && tau[0] == 0.0, "fewer than min_pixels: nothing changes");
  CHECK(om_residual(S) == 256.0 / 100.0, "the residual");
}

void check_motion() {
  for (double s : {0.0, 1e-9, 0.01, 0.3, 2.0}) {
    const double w[3] = {0.3 * s, -0.7 * s, 0.2 * s};
    double R[9];
    om_cayley(w, R);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double d = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2];
        CHECK(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-15, "R R^T [%d][%d] = %.17g at %g", i, j, d, s);
      }
    if (s == 0.0)
      for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1.0 : 0.0), "the identity, exactly");
    if (s == 1e-9) CHECK(std::fabs(R[1] + w[2]) < 1e-17 && std::fabs(R[2] - w[1]) < 1e-17, "I + [w]x to first order");
    // a step composed with its inverse: T X^-1 (X^-1)^-1 = T, where (R | t)^-1 = (R^T | -R^T t)
    const double tw[3] = {0.1 * s, 0.02, -0.3};
    double T[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tau[3] = {0.5, -0.25, 2.0}, Ri[9], ti[3];
    om_compose(T, tau, R, tw);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Ri[3 * i + j] = R[3 * j + i];
      ti[i] = -((R[i] * tw[0] + R[3 + i] * tw[1]) + R[6 + i] * tw[2]);
    }
    om_compose(T, tau, Ri, ti);
    for (int i = 0; i < 9; ++i) CHECK(std::fabs(T[i] - (i % 4 == 0 ? 1.0 : 0.0)) <= 4e-15, "T[%d] = %.17g at %g", i, T[i], s);
    const double t0[3] = {0.5, -0.25, 2.0};
    for (int i = 0; i < 3; ++i) CHECK(std::fabs(tau[i] - t0[i]) <= 1e-13 * (1.0 + s), "tau[%d] = %.17g at %g", i, tau[i], s);
  }
  // the world pose: chained by a motion and then by its inverse it returns; the identity motion leaves it to the bit
  {
    const double w[3] = {0.02, -0.3, 0.01};
    double R[9], T[12], Ti[12], Wd[12] = {0, 0, 1, 3.0, 0, 1, 0, -1.0, -1, 0, 0, 7.5}, W0[12];
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(W0, Wd, sizeof W0);
    om_chain(Wd, eye);
    for (int i = 0; i < 12; ++i) CHECK(Wd[i] == W0[i], "the identity motion: W[%d]", i);
    om_cayley(w, R);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j], Ti[4 * i + j] = R[3 * j + i];
      T[4 * i + 3] = 0.25 * (i + 1);
    }
    for (int i = 0; i < 3; ++i) Ti[4 * i + 3] = -((R[i] * T[3] + R[3 + i] * T[7]) + R[6 + i] * T[11]);
    om_chain(Wd, T);
    CHECK(std::fabs(Wd[3] - W0[3]) > 0.1, "the motion moves the world pose");
    om_chain(Wd, Ti);
    for (int i = 0; i < 12; ++i) CHECK(std::fabs(Wd[i] - W0[i]) <= 1e-14, "W T^-1 T: W[%d] = %.17g", i, Wd[i]);
  }
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0}, fwd[3] = {0, 0, -0.5};
  float g[12];
  om_form_g(I3, zero, 721.5377, 609.5593, 172.854, g);
  for (int i = 0; i < 12; ++i) CHECK(g[i] == kEye[i], "the identity gives [I | 0] exactly: g[%d] = %g", i, (double)g[i]);
  om_form_g(I3, fwd, 100.0, 50.0, 20.0, g);
  CHECK(g[3] == -0.25f && g[7] == -0.1f && g[11] == -0.005f && g[0] == 1.f && g[10] == 1.f, "K tau / f");
}

}  // namespace

int main() {
  check_sample_and_weight();
  check_pixels();
  check_exponents();
  check_solve();
  check_motion();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
