// Launchers of the norm regulariser kernels (pair_norm.hip). The entries and
// every host check live in bindings.cpp, which calls these with tensors it
// has already validated (bf16 or fp32, contiguous, 16 B-aligned bases,
// H % 4 == 0, L % 8 == 0, E % 8 == 0, unit counts that fit 31 bits).
#pragma once

#include <torch/extension.h>

// widest row the one-wave-per-row kernels take
constexpr int64_t kRowNormMaxE = 8192;

// pair, bias (B, H, L, L); pad (B, L) bytes, true = padded, 8 B-aligned, or
// null. coef (B, L, L) fp32; uerr (B, L, L/8) fp32, the error summed over
// each 8-position unit.
void pair_norm_forward_launch(at::Tensor& coef, at::Tensor& uerr,
                              const at::Tensor& pair, const at::Tensor& bias,
                              const uint8_t* pad);

// d_pair = gscale[b] * coef * (pair - bias), d_bias = -d_pair, both as pair;
// gscale (B) fp32
void pair_norm_backward_launch(at::Tensor& d_pair, at::Tensor& d_bias,
                               const at::Tensor& gscale, const at::Tensor& coef,
                               const at::Tensor& pair, const at::Tensor& bias);

// x (N, E); pad (N) bytes or null. coef, err (N) fp32.
void row_norm_forward_launch(at::Tensor& coef, at::Tensor& err,
                             const at::Tensor& x, const uint8_t* pad);

// dx = g_row[n] * coef[n] * x, as x; g_row (N) fp32
void row_norm_backward_launch(at::Tensor& dx, const at::Tensor& g_row,
                              const at::Tensor& coef, const at::Tensor& x);
