// Launchers of the head-dim-8 pair-track attention (pair_attn_d8.hip).  The
// entries and every host check live in pair_attn.hip, which dispatches here
// on q.size(2) == 8 with tensors it has already validated.
#pragma once

#include <torch/extension.h>

// dropout scalars as pair_attn.hip's Drop: pinv = 1 / (1 - p), pthresh =
// keep16_threshold(p); drop == false ignores them
struct Pair8Drop {
  bool drop;
  float pinv;
  uint32_t pthresh;
  uint64_t seed;
};

void pair8_forward_launch(at::Tensor& o, at::Tensor& logits, at::Tensor& lse,
                          const at::Tensor& q, const at::Tensor& k,
                          const at::Tensor& v, const at::Tensor& bias,
                          const Pair8Drop& dr);

// d_logits may be null
void pair8_backward_launch(at::Tensor& dq, at::Tensor& dk, at::Tensor& dv,
                           at::Tensor& dbias, const at::Tensor& d_out,
                           const at::Tensor* d_logits, const at::Tensor& q,
                           const at::Tensor& k, const at::Tensor& v,
                           const at::Tensor& o, const at::Tensor& lse,
                           const at::Tensor& logits, const Pair8Drop& dr);
