// Launchers of the Uni-Mol pair embedding kernels at K = 128 gaussians and
// H = 64 heads (pair_gauss_h64.hip). The entries and every host check live in
// bindings.cpp, which calls these with tensors it has already validated (bf16
// Linear tensors, fp32 everything else, L % 8 == 0, L >= 8, contiguous, 16 B-
// aligned bases, pad 8 B-aligned).
#pragma once

#include <torch/extension.h>

// columns of a weight-gradient row:
// dW1 (o-major, 128*128) | db1 (128) | dW2 (h-major, 64*128) | db2 (64)
int64_t pair_gauss_h64_wgrad_cols();

// pad: (B, L) bytes, true = padded, or null. out (B, 64, L, L) bf16; a padded
// key j holds the bits of fill in every head and row.
void pair_gauss_h64_forward_launch(at::Tensor& out, const at::Tensor& coords,
                                   const at::Tensor& a, const at::Tensor& b,
                                   const uint8_t* pad, const at::Tensor& means,
                                   const at::Tensor& stds, const at::Tensor& W1,
                                   const at::Tensor& b1, const at::Tensor& W2,
                                   const at::Tensor& b2, float fill);

// grad as out. d_a, d_b (B, L, L) fp32; stat_fold: 256 fp32, d_means | d_stds;
// w_fold: pair_gauss_h64_wgrad_cols() fp32
void pair_gauss_h64_backward_launch(at::Tensor& d_a, at::Tensor& d_b,
                                    at::Tensor& stat_fold, at::Tensor& w_fold,
                                    const at::Tensor& grad,
                                    const at::Tensor& coords,
                                    const at::Tensor& a, const at::Tensor& b,
                                    const uint8_t* pad, const at::Tensor& means,
                                    const at::Tensor& stds, const at::Tensor& W1,
                                    const at::Tensor& b1, const at::Tensor& W2);
