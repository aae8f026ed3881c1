// The gradient with respect to the free derivatives through the C++ compat veneer
// (include/compat/mav_trajectory_generation/polynomial_optimization_linear.h):
//   host:   PolynomialOptimizationBatch<N>::freeGradientHost over mtg_free_gradient_host (no object, no device) -- the N = 2 case by
//           hand, and N = 4, K = 2 at unit times against the closed-form columns of the cubic Hermite map (integers: exact);
//   device: PolynomialOptimizationBatch<N>::freeGradient with device pointers over mtg_free_gradient, bit for bit against the host
//           form, and with host pointers through the object.
// Usage: test_free_gradient_veneer host | device
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <mav_trajectory_generation/polynomial_optimization_linear.h>

using mav_trajectory_generation::PolynomialOptimizationBatch;

static int failures = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static unsigned long long state = 88172645463325252ull;
static double uniform(double lo, double hi) {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return lo + (hi - lo) * (double)(state >> 11) / 9007199254740992.0;
}

static void host_tests() {
  {  // N = 2, K = 1, T = 2: g_S = G_0 - G_1 / 2 (vertex 0, fixed), g_E = G_1 / 2 (vertex 1, free)
    const std::vector<uint32_t> mask = {1u, 0u};
    const double times[1] = {2.0}, G[4] = {0.75, -2.5, 3.0, 0.625};
    double gfree[2] = {-1, -1}, gfixed[2] = {-1, -1};
    PolynomialOptimizationBatch<2>::freeGradientHost(2, mask, 0, 1, times, G, nullptr, 1.0, gfree, gfixed);
    EXPECT(gfixed[0] == 0.75 + 1.25 && gfixed[1] == 3.0 - 0.3125);
    EXPECT(gfree[0] == -1.25 && gfree[1] == 0.3125);
    double only[2] = {-1, -1};
    PolynomialOptimizationBatch<2>::freeGradientHost(2, mask, 0, 1, times, G, nullptr, 1.0, only);   // grad_fixed not wanted
    EXPECT(only[0] == -1.25 && only[1] == 0.3125);
  }
  {  // N = 4, K = 2, unit times, cubic Hermite: c = (x0, v0, 3(x1 - x0) - 2 v0 - v1, 2(x0 - x1) + v0 + v1); free: v at the middle vertex
    const std::vector<uint32_t> mask = {3u, 1u, 3u};
    const double times[2] = {1.0, 1.0};
    double w[8];
    for (double& x : w) x = std::floor(uniform(-9.0, 10.0));
    double gfree[1], gfixed[5];
    PolynomialOptimizationBatch<4>::freeGradientHost(1, mask, 1, 1, times, w, nullptr, 1.0, gfree, gfixed);
    // d c / d v1: segment 0 (end velocity): (0, 0, -1, 1); segment 1 (start velocity): (0, 1, -2, 1)
    EXPECT(gfree[0] == (-w[2] + w[3]) + (w[5] - 2 * w[6] + w[7]));
    // d c / d x1 (fixed column 2): segment 0 (end position): (0, 0, 3, -2); segment 1 (start position): (1, 0, -3, 2)
    EXPECT(gfixed[2] == (3 * w[2] - 2 * w[3]) + (w[4] - 3 * w[6] + 2 * w[7]));
    EXPECT(gfixed[0] == w[0] - 3 * w[2] + 2 * w[3] && gfixed[1] == w[1] - 2 * w[2] + w[3]);
    EXPECT(gfixed[3] == 3 * w[6] - 2 * w[7] && gfixed[4] == -w[6] + w[7]);
  }
}

static void device_tests() {
  constexpr int N = 10;
  const int D = 3, K = 4, B = 37;
  std::vector<uint32_t> mask(K + 1, 1u);
  mask[0] = mask[K] = 31u;
  PolynomialOptimizationBatch<N> opt(D, mask, 3);
  const size_t n_free = opt.getNumberFreeConstraints(), n_fixed = opt.getNumberFixedConstraints();
  std::vector<double> times(B * K), G(B * K * D * N), c(B * K * D * N);
  for (double& t : times) t = uniform(0.3, 4.0);
  for (double& x : G) x = uniform(-1.0, 1.0);
  for (double& x : c) x = uniform(-1.0, 1.0);
  std::vector<double> hf(B * D * n_free), hx(B * D * n_fixed), of(hf.size()), ox(hx.size()), df(hf.size()), dx(hx.size());
  PolynomialOptimizationBatch<N>::freeGradientHost(D, mask, 3, B, times.data(), G.data(), c.data(), 0.5, hf.data(), hx.data());
  opt.freeGradient(B, times.data(), G.data(), c.data(), 0.5, of.data(), ox.data());   // host pointers through the object
  EXPECT(std::memcmp(hf.data(), of.data(), hf.size() * 8) == 0 && std::memcmp(hx.data(), ox.data(), hx.size() * 8) == 0);
  mtg_context* ctx = mav_trajectory_generation::mtg_compat_detail::context();
  void *d_t, *d_g, *d_c, *d_f, *d_x;
  EXPECT(mtg_device_malloc(ctx, times.size() * 8, &d_t) == MTG_OK && mtg_device_malloc(ctx, G.size() * 8, &d_g) == MTG_OK &&
         mtg_device_malloc(ctx, c.size() * 8, &d_c) == MTG_OK && mtg_device_malloc(ctx, hf.size() * 8, &d_f) == MTG_OK &&
         mtg_device_malloc(ctx, hx.size() * 8, &d_x) == MTG_OK);
  EXPECT(mtg_copy_to_device(ctx, d_t, times.data(), times.size() * 8) == MTG_OK && mtg_copy_to_device(ctx, d_g, G.data(), G.size() * 8) == MTG_OK &&
         mtg_copy_to_device(ctx, d_c, c.data(), c.size() * 8) == MTG_OK);
  opt.freeGradient(B, (const double*)d_t, (const double*)d_g, (const double*)d_c, 0.5, (double*)d_f, (double*)d_x, true);
  opt.sync();
  EXPECT(mtg_copy_to_host(ctx, df.data(), d_f, df.size() * 8) == MTG_OK && mtg_copy_to_host(ctx, dx.data(), d_x, dx.size() * 8) == MTG_OK);
  EXPECT(std::memcmp(hf.data(), df.data(), hf.size() * 8) == 0 && std::memcmp(hx.data(), dx.data(), hx.size() * 8) == 0);
  for (void* p : {d_t, d_g, d_c, d_f, d_x}) mtg_device_free(ctx, p);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  host_tests();
  if (mode == "device") device_tests();
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("FREE-GRADIENT VENEER TESTS PASSED (%s)\n", mode == "device" ? "host + device" : "host");
  return 0;
}
