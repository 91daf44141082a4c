// Pieces the two coordinate-head sources share: the exact erf GELU, and the
// launchers of the H = 64 kernels (pair_coord_h64.hip).  The entries and every
// host check live in pair_coord.hip, which dispatches here on pair.size(1) ==
// 64 with tensors it has already validated (L % 8 == 0, L >= 8, 16 B-aligned
// bases).
#pragma once

#include <torch/extension.h>

#include <hip/hip_runtime.h>

#if defined(__HIPCC__)
constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;

static __device__ __forceinline__ float gelu_exact(float x) {
  return 0.5f * x * (1.f + erff(x * kRsqrt2));
}

// y = gelu(x), dy = gelu'(x)
static __device__ __forceinline__ void gelu_exact_grad(float x, float& y,
                                                       float& dy) {
  const float cdf = 0.5f * (1.f + erff(x * kRsqrt2));
  y = x * cdf;
  dy = cdf + x * kRsqrt2Pi * expf(-0.5f * x * x);
}
#endif

// columns of a weight-gradient row: dW1 (o-major, H*H) | db1 (H) | dW2 (H) | db2
static inline int64_t pair_coord_wgrad_cols(int64_t H) {
  return H * H + 2 * H + 1;
}

// pad: (B, L) bytes, true = padded, or null.  out (B, L, 3) fp32.
void pair_coord_h64_forward_launch(at::Tensor& out, const at::Tensor& pair,
                                   const at::Tensor& pair0,
                                   const at::Tensor& coords,
                                   const at::Tensor& inv_n, const uint8_t* pad,
                                   const at::Tensor& W1, const at::Tensor& b1,
                                   const at::Tensor& W2, const at::Tensor& b2);

// dpair as pair; fold: pair_coord_wgrad_cols(64) fp32, the folded gradients
void pair_coord_h64_backward_launch(at::Tensor& dpair, at::Tensor& fold,
                                    const at::Tensor& grad,
                                    const at::Tensor& pair,
                                    const at::Tensor& pair0,
                                    const at::Tensor& coords,
                                    const at::Tensor& inv_n, const uint8_t* pad,
                                    const at::Tensor& W1, const at::Tensor& b1,
                                    const at::Tensor& W2);
