// Fused dropout(x [+ bias]) + residual add for gfx950:
// out = residual + keep*pinv*(x [+ bias]).
// Replaces the torch dropout kernel + add kernel pair (saves one full
// read+write of the hidden tensor per site; two sites per transformer
// layer).  Bitfield keep-mask, Philox keyed by PyTorch's generator.
// Backward: dx = g * keep * pinv (one pass); d_residual = g (pass-through,
// no kernel).
//
// One kernel family serves the plain and the shared-axis (row-/column-wise)
// join: the kernels are templated on the mask map (dropout_mask.h), which
// says where a unit's keep byte lives and what keys its Philox draw. The
// dropout_add_* entries use the flat map, the shared_dropout_add_* entries
// the (outer, shared, inner) map over a contiguous (B, R, T, C) tensor. One
// launch either way, no extra pass, and the shared mask is never
// activation-sized. Backward reads the byte through the same map and never
// touches Philox.
#include "common.h"
#include "dispatch.h"
#include "dropout_mask.h"
#include "fold.h"

#include <optional>
#include <vector>

namespace {

template <typename T, typename Map, bool DROP, bool HAS_BIAS>
__global__ void dropout_add_fwd_kernel(T* __restrict__ out,
                                       uint8_t* __restrict__ dmask,
                                       const T* __restrict__ x,
                                       const T* __restrict__ res,
                                       const T* __restrict__ bias, int C,
                                       int64_t n8, Map map, float pinv,
                                       uint32_t pthresh, uint64_t rngkey) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n8; i += stride) {
    float fx[8], fr[8];
    load8(x + i * 8, fx);
    load8(res + i * 8, fr);
    if constexpr (HAS_BIAS) {
      float fb[8];
      load8(bias + (int)((i * 8) % C), fb);
#pragma unroll
      for (int j = 0; j < 8; ++j) fx[j] += fb[j];
    }
    if constexpr (DROP) {
      bool first;
      const int64_t m = mask_index(map, i, first);
      bool keep[8];
      keep16x8(rngkey, (uint64_t)m, 0, pthresh, keep);
      uint8_t bits = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bits |= (uint8_t)(keep[j] ? 1u : 0u) << j;
        fx[j] = fr[j] + drop_scale<Map::kExact>(keep[j], fx[j], pinv);
      }
      if (first) dmask[m] = bits;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) fx[j] += fr[j];
    }
    store8(out + i * 8, fx);
  }
}

template <typename T, typename Map, bool DROP, bool BGRAD>
__global__ void dropout_add_bwd_kernel(T* __restrict__ dx, const T* __restrict__ g,
                                       const uint8_t* __restrict__ dmask,
                                       float* __restrict__ partials, int C,
                                       int64_t n8, Map map, float pinv) {
  extern __shared__ float s_col[];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  int c0 = -1;
  for (int64_t i = tid; i < n8; i += stride) {
    if (BGRAD && c0 < 0) c0 = (int)((i * 8) % C);
    float f[8];
    load8(g + i * 8, f);
    if constexpr (DROP) {
      bool first;
      const uint8_t bits = dmask[mask_index(map, i, first)];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = (bits >> j) & 1 ? f[j] * pinv : 0.f;
      store8(dx + i * 8, f);
    }
    if constexpr (BGRAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
  if constexpr (BGRAD) {
    colsum_block_fold(acc, c0, C, s_col,
                      partials + (int64_t)blockIdx.x * C);
  }
}

// Shared maps come with dropout only: their entries require p in (0, 1).
template <typename Map>
constexpr bool kMayPassThrough = std::is_same_v<Map, FlatMap>;

// bc undefined: no bias
template <typename Map>
void launch_fwd(const char* name, at::Tensor& out, at::Tensor& dmask,
                const at::Tensor& x, const at::Tensor& res,
                const at::Tensor& bc, int C, const Map& map, bool drop,
                float pinv, uint32_t pthresh, uint64_t rngkey) {
  TORCH_INTERNAL_ASSERT(drop || kMayPassThrough<Map>);
  const int64_t n8 = x.numel() / 8;
  const bool has_bias = bc.defined();
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = unicore_grid((n8 + 255) / 256);
  DISPATCH_FTYPES(x.scalar_type(), name, {
    auto launch = [&](auto drop_tag, auto bias_tag) {
      constexpr bool DROP = decltype(drop_tag)::value;
      constexpr bool HB = decltype(bias_tag)::value;
      dropout_add_fwd_kernel<scalar_t, Map, DROP, HB><<<grid, 256, 0, stream>>>(
          reinterpret_cast<scalar_t*>(out.data_ptr()),
          DROP ? dmask.data_ptr<uint8_t>() : nullptr,
          reinterpret_cast<const scalar_t*>(x.data_ptr()),
          reinterpret_cast<const scalar_t*>(res.data_ptr()),
          HB ? reinterpret_cast<const scalar_t*>(bc.data_ptr()) : nullptr, C,
          n8, map, pinv, pthresh, rngkey);
    };
    auto pick = [&](auto drop_tag) {
      if (has_bias) launch(drop_tag, std::true_type{});
      else launch(drop_tag, std::false_type{});
    };
    if (drop) pick(std::true_type{});
    else if constexpr (kMayPassThrough<Map>) pick(std::false_type{});
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// dx = grad through the mask (drop) and dbias = its column sums (bgrad);
// !drop: dx is grad itself and only the column sum runs
template <typename Map>
void launch_bwd(const char* name, at::Tensor& dx, at::Tensor& dbias,
                const at::Tensor& grad, const at::Tensor& dmask, int C,
                const Map& map, bool drop, float pinv) {
  TORCH_INTERNAL_ASSERT(drop || kMayPassThrough<Map>);
  const int64_t n8 = grad.numel() / 8;
  const bool bgrad = dbias.numel() > 0;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = bgrad ? colsum_grid(n8, C) : unicore_grid((n8 + 255) / 256);
  at::Tensor partials;
  if (bgrad) partials = at::empty({grid, (int64_t)C}, dbias.options());
  const size_t lds = bgrad ? (size_t)C * sizeof(float) : 0;
  DISPATCH_FTYPES(grad.scalar_type(), name, {
    auto launch = [&](auto drop_tag, auto bg_tag) {
      constexpr bool DROP = decltype(drop_tag)::value;
      constexpr bool BG = decltype(bg_tag)::value;
      dropout_add_bwd_kernel<scalar_t, Map, DROP, BG>
          <<<grid, 256, lds, stream>>>(
              reinterpret_cast<scalar_t*>(dx.data_ptr()),
              reinterpret_cast<const scalar_t*>(grad.data_ptr()),
              DROP ? dmask.data_ptr<uint8_t>() : nullptr,
              BG ? partials.data_ptr<float>() : nullptr, C, n8, map, pinv);
    };
    if (drop) {
      if (bgrad) launch(std::true_type{}, std::true_type{});
      else launch(std::true_type{}, std::false_type{});
    } else if constexpr (kMayPassThrough<Map>) {
      if (bgrad) launch(std::false_type{}, std::true_type{});
    }
  });
  if (bgrad) {
    unicore_fold_columns(partials.data_ptr<float>(), dbias.data_ptr<float>(),
                         grid, C, partials.options(), stream);
  }
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

}  // namespace

// returns {out, dmask}
std::vector<at::Tensor> dropout_add_forward(at::Tensor x, at::Tensor res,
                                            std::optional<at::Tensor> bias,
                                            double p, bool is_training) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && res.is_contiguous(),
              "dropout_add: contiguous CUDA");
  TORCH_CHECK(x.sizes() == res.sizes() && x.scalar_type() == res.scalar_type(),
              "dropout_add: x/res mismatch");
  TORCH_CHECK(x.numel() % 8 == 0, "dropout_add: numel % 8 == 0");
  const int64_t n8 = x.numel() / 8;
  const bool drop = is_training && p > 0.0;
  auto out = at::empty_like(x);
  auto dmask = at::empty({drop ? n8 : 0}, x.options().dtype(at::kByte));
  float pinv = 1.f;
  uint32_t pthresh = 0;
  uint64_t rngkey = 0;
  if (drop) {
    const double pc = std::min(p, 0.999999);
    pinv = (float)(1.0 / (1.0 - pc));
    pthresh = keep16_threshold(pc);
    rngkey = reserve_dropout_key(n8);
  }
  at::Tensor bc;
  int C = 0;
  if (bias.has_value()) {
    bc = bias->contiguous();
    C = (int)bc.numel();
    TORCH_CHECK(C > 0 && C % 8 == 0 && x.size(-1) == C &&
                    bc.scalar_type() == x.scalar_type(),
                "dropout_add: bad bias");
  }
  launch_fwd("dropout_add_forward", out, dmask, x, res, bc, C, FlatMap{}, drop,
             pinv, pthresh, rngkey);
  return {out, dmask};
}

// returns {out, dmask}
std::vector<at::Tensor> shared_dropout_add_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias, double p,
    int64_t shared_dim) {
  const char* name = "shared_dropout_add_forward";
  check_operand(name, x, shared_dim);
  check_pair(name, x, res);
  check_p(name, p);
  at::Tensor bc = check_bias(name, bias, x);
  auto out = at::empty_like(x);
  const int64_t nmask = mask_units(x, shared_dim);
  auto dmask = at::empty({nmask}, x.options().dtype(at::kByte));
  if (x.numel() == 0) return {out, dmask};
  // the generator draw of the unshared entry, sized by the mask units
  launch_fwd(name, out, dmask, x, res, bc, (int)x.size(3),
             unit_map(x, shared_dim), true, (float)(1.0 / (1.0 - p)),
             keep16_threshold(p), reserve_dropout_key(nmask));
  return {out, dmask};
}

// returns {dx, dbias (fp32, bias_dim elements or empty)}
std::vector<at::Tensor> dropout_add_backward(at::Tensor grad, at::Tensor dmask,
                                             double p, int64_t bias_dim) {
  TORCH_CHECK(grad.is_cuda() && grad.is_contiguous(), "dropout_add_backward");
  const bool drop = dmask.numel() > 0;
  TORCH_CHECK(!drop || dmask.numel() == grad.numel() / 8,
              "dropout_add_backward: mask mismatch");
  const bool bgrad = bias_dim > 0;
  const int C = (int)bias_dim;
  TORCH_CHECK(!bgrad || colsum_supported(C), "dropout_add_backward: bad bias dim");
  const float pinv = (float)(1.0 / (1.0 - std::min(p, 0.999999)));
  // !drop: dx == grad, the caller aliases it; only the colsum runs
  auto dx = drop ? at::empty_like(grad) : grad;
  auto dbias = at::empty({bgrad ? (int64_t)C : 0},
                         grad.options().dtype(at::kFloat));
  launch_bwd("dropout_add_backward", dx, dbias, grad, dmask, C, FlatMap{},
             drop, pinv);
  return {dx, dbias};
}

// returns {dx, dbias (fp32, bias_dim elements or empty)}
std::vector<at::Tensor> shared_dropout_add_backward(at::Tensor grad,
                                                    at::Tensor dmask, double p,
                                                    int64_t shared_dim,
                                                    int64_t bias_dim) {
  const char* name = "shared_dropout_add_backward";
  check_operand(name, grad, shared_dim);
  check_p(name, p);
  const int64_t nmask = mask_units(grad, shared_dim);
  TORCH_CHECK(dmask.device() == grad.device() &&
                  dmask.scalar_type() == at::kByte && dmask.is_contiguous(),
              name, ": mask must be a contiguous uint8 tensor on ",
              grad.device(), ", got ", dmask.scalar_type(), " on ",
              dmask.device());
  TORCH_CHECK(dmask.numel() == nmask, name, ": mask has ", dmask.numel(),
              " bytes, shared_dim ", shared_dim, " of sizes ", grad.sizes(),
              " needs ", nmask);
  const bool bgrad = bias_dim > 0;
  const int C = (int)grad.size(3);
  TORCH_CHECK(!bgrad || (bias_dim == C && colsum_supported(C)), name,
              ": bias_dim must be 0 or the channel width ", C,
              " (with a supported column sum), got ", bias_dim);
  auto dx = at::empty_like(grad);
  auto dbias = at::zeros({bgrad ? (int64_t)C : 0},
                         grad.options().dtype(at::kFloat));
  if (grad.numel() == 0) return {dx, dbias};
  launch_bwd(name, dx, dbias, grad, dmask, C, unit_map(grad, shared_dim), true,
             (float)(1.0 / (1.0 - p)));
  return {dx, dbias};
}
