// mtg_pullback_host.cpp -- host build (plain g++, no HIP) of the gradient with respect to the free derivatives: the lane code
// of mtg_pullback_lane.h run one (trajectory, vertex, dimension) after the other.  Nothing in the rule depends on the launch
// geometry, so both forms agree bit for bit.  The masks and column offsets come from the plan description: no context, no
// device, no factorisation (structurally rank-deficient plans are plans like any other here).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mtg_hip.h"
#include "mtg_pullback_lane.h"

extern "C" int mtg_free_gradient_host(const mtg_plan_desc* desc, int64_t batch, const mtg_layout* layout, const double* times,
                                      const double* grad_coeffs, const double* coeffs, double smoothness_weight, double* grad_free,
                                      double* grad_fixed) {
  if (!desc || !desc->fixed_mask || !mtgp::arguments_ok(batch, layout, times, grad_coeffs, coeffs, grad_free, grad_fixed))
    return MTG_ERR_INVALID_ARGUMENT;
  const int N = desc->n_coeffs, D = desc->dimension, K = desc->n_segments, d = desc->derivative_to_optimize;
  if (N < 2 || N > MTG_MAX_N || (N & 1) || D < 1 || K < 1 || d < 0 || d > N / 2 - 1) return MTG_ERR_INVALID_ARGUMENT;
  const int H = N / 2, full = (1 << H) - 1;
  std::vector<int> mask(K + 1), offF(K + 2, 0), offP(K + 2, 0);
  for (int v = 0; v <= K; ++v) {
    mask[v] = (int)(desc->fixed_mask[v] & (uint32_t)full);
    const int nf = __builtin_popcount((unsigned)mask[v]);
    offF[v + 1] = offF[v] + nf;
    offP[v + 1] = offP[v] + (H - nf);
  }
  mtgp::Params P;
  P.times = times; P.ts_b = layout->times_stride_b; P.ts_k = layout->times_stride_k;
  P.grad = grad_coeffs; P.coeffs = coeffs; P.w = smoothness_weight;
  P.gfree = grad_free; P.ps_b = layout->free_stride_b; P.ps_d = layout->free_stride_d; P.ps_c = layout->free_stride_c;
  P.gfixed = grad_fixed; P.fs_b = layout->fixed_stride_b; P.fs_d = layout->fixed_stride_d; P.fs_c = layout->fixed_stride_c;
  P.mask = mask.data(); P.offF = offF.data(); P.offP = offP.data();
  P.B = batch; P.K = K; P.D = D; P.deriv = d; P.q1off = mtgp::q1_offset(N, d);
  mtgs::with_instance<mtgp::kMinInstance>(N, [&](auto nc) {
    for (int64_t b = 0; b < batch; ++b)
      for (int v = 0; v <= K; ++v)
        for (int dim = 0; dim < D; ++dim) mtgp::vertex_lane<decltype(nc)::value>(P, b, v, dim);
  });
  return MTG_OK;
}
