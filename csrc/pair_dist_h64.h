// Launchers of the pair distance head kernels at H = 64 (pair_dist_h64.hip).
// The entries and every host check live in bindings.cpp, which calls these
// with tensors it has already validated (H == 64, L % 8 == 0, L >= 8,
// contiguous, 16 B-aligned bases, fp32 parameters on the device of pair).
#pragma once

#include <torch/extension.h>

// columns of a weight-gradient row:
// dW1 (o-major, 64*64) | db1 (64) | dgamma (64) | dbeta (64) | dw2 (64) | db2
int64_t pair_dist_h64_wgrad_cols();

// pad: (B, L) bytes, true = padded, or null. F (B, L, L) fp32, the
// unsymmetrised f_ij; rows of a padded i are left unwritten.
void pair_dist_h64_forward_launch(at::Tensor& F, const at::Tensor& pair,
                                  const uint8_t* pad, const at::Tensor& W1,
                                  const at::Tensor& b1, const at::Tensor& gamma,
                                  const at::Tensor& beta, const at::Tensor& w2,
                                  const at::Tensor& b2, float eps);

// out = 0.5 * (in + in^T) over the last two axes, 0 where i or j is padded;
// in, out (B, L, L) fp32, distinct
void pair_dist_sym_launch(at::Tensor& out, const at::Tensor& in,
                          const uint8_t* pad);

// dF: the symmetrised, masked output gradient (B, L, L) fp32. dpair as pair;
// fold: pair_dist_h64_wgrad_cols() fp32, the folded gradients
void pair_dist_h64_backward_launch(at::Tensor& dpair, at::Tensor& fold,
                                   const at::Tensor& dF, const at::Tensor& pair,
                                   const uint8_t* pad, const at::Tensor& W1,
                                   const at::Tensor& b1,
                                   const at::Tensor& gamma,
                                   const at::Tensor& beta, const at::Tensor& w2,
                                   float eps);
