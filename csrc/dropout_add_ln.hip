// Fused dropout(x [+ bias]) + residual add + LayerNorm for gfx950.
//
// The post-LN residual join (out = LN(res + dropout(x + b))) is two kernels
// today (dropout_add, then LN) with the summed tensor making a full HBM
// round-trip between them. This kernel computes the sum in registers, writes
// it ONCE (saved for backward / the next residual), reduces mean/var from
// the registers, and writes the normed output — one launch, one read of
// x+res instead of two reads + an extra intermediate read.
//
// Backward reuses the existing kernels unchanged: layernorm_backward on the
// saved sum produces d_sum (+ dgamma/dbeta), and dropout_add_backward maps
// d_sum through the keep-mask (+ folded-bias column sum); d_res = d_sum.
//
// Like dropout_add.hip the kernel is templated on the mask map
// (dropout_mask.h), here applied per row: the map is evaluated once per row
// and the lanes add their unit. With the flat map (dropout_add_ln_forward)
// the dmask layout and Philox keying are IDENTICAL to dropout_add.hip (flat
// 8-element index), with the shared map (shared_dropout_add_ln_forward) to
// its shared-axis entries, so the matching backward entry consumes the mask
// as-is.
#include "common.h"
#include "dispatch.h"
#include "dropout_mask.h"

#include <optional>
#include <vector>

namespace {

template <typename T, typename Map, int NV, bool DROP, bool HAS_BIAS>
__global__ void dropout_add_ln_fwd_kernel(
    T* __restrict__ normed, T* __restrict__ summed,
    uint8_t* __restrict__ dmask, float* __restrict__ mean,
    float* __restrict__ invvar, const T* __restrict__ x,
    const T* __restrict__ res, const T* __restrict__ bias,
    const T* __restrict__ gamma, const T* __restrict__ beta, int64_t n1,
    int n2, Map map, float eps, float pinv, uint32_t pthresh,
    uint64_t rngkey) {
  const int lane = threadIdx.x;
  const int wid = threadIdx.y;
  const int row8 = n2 / 8;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.y + wid; row < n1;
       row += (int64_t)gridDim.x * blockDim.y) {
    const int64_t rbase = row * (int64_t)n2;
    bool first = true;
    int64_t mbase = 0;
    if constexpr (DROP) mbase = mask_index(map, row, first) * (int64_t)row8;
    float vals[NV][8];
    float sum = 0.f, sumsq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e0 = (lane + i * 64) * 8;
      if (e0 < n2) {
        float fx[8], fr[8];
        load8(x + rbase + e0, fx);
        load8(res + rbase + e0, fr);
        if constexpr (HAS_BIAS) {
          float fb[8];
          load8(bias + e0, fb);
#pragma unroll
          for (int j = 0; j < 8; ++j) fx[j] += fb[j];
        }
        if constexpr (DROP) {
          const int64_t m = mbase + lane + i * 64;
          bool keep[8];
          keep16x8(rngkey, (uint64_t)m, 0, pthresh, keep);
          uint8_t bits = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            bits |= (uint8_t)(keep[j] ? 1u : 0u) << j;
            fx[j] = drop_scale<Map::kExact>(keep[j], fx[j], pinv);
          }
          if (first) dmask[m] = bits;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float s = fr[j] + fx[j];
          vals[i][j] = s;
          sum += s;
          sumsq += s * s;
        }
        store8(summed + rbase + e0, vals[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[i][j] = 0.f;
      }
    }
    const float mu = wave_sum(sum) / n2;
    const float var = wave_sum(sumsq) / n2 - mu * mu;
    const float iv = rsqrtf(var + eps);
    if (lane == 0) {
      mean[row] = mu;
      invvar[row] = iv;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e0 = (lane + i * 64) * 8;
      if (e0 < n2) {
        float g[8], b[8], o[8];
        load8(gamma + e0, g);
        load8(beta + e0, b);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = (vals[i][j] - mu) * iv * g[j] + b[j];
        store8(normed + rbase + e0, o);
      }
    }
  }
}

// Allocates the outputs beside dmask and launches; bc undefined: no bias.
// Shared maps come with dropout only: their entry requires p in (0, 1).
// returns {normed, summed, dmask, mean, invvar}
template <typename Map>
std::vector<at::Tensor> launch_ln_fwd(
    const char* name, const at::Tensor& x, const at::Tensor& res,
    const at::Tensor& bc, const at::Tensor& gamma, const at::Tensor& beta,
    at::Tensor dmask, const Map& map, bool drop, double eps, float pinv,
    uint32_t pthresh, uint64_t rngkey) {
  constexpr bool kMayPassThrough = std::is_same_v<Map, FlatMap>;
  TORCH_INTERNAL_ASSERT(drop || kMayPassThrough);
  const int n2 = (int)x.size(-1);
  const int64_t n1 = x.numel() / n2;
  const bool has_bias = bc.defined();
  auto normed = at::empty_like(x);
  auto summed = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({n1}, fopt);
  auto invvar = at::empty({n1}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 block(64, 4);
  const dim3 grid(unicore_grid((n1 + 3) / 4));
  DISPATCH_FTYPES(x.scalar_type(), name, {
    auto launch = [&](auto nv_tag, auto drop_tag, auto bias_tag) {
      constexpr int NV = decltype(nv_tag)::value;
      constexpr bool DROP = decltype(drop_tag)::value;
      constexpr bool HB = decltype(bias_tag)::value;
      dropout_add_ln_fwd_kernel<scalar_t, Map, NV, DROP, HB>
          <<<grid, block, 0, stream>>>(
              reinterpret_cast<scalar_t*>(normed.data_ptr()),
              reinterpret_cast<scalar_t*>(summed.data_ptr()),
              DROP ? dmask.data_ptr<uint8_t>() : nullptr,
              mean.data_ptr<float>(), invvar.data_ptr<float>(),
              reinterpret_cast<const scalar_t*>(x.data_ptr()),
              reinterpret_cast<const scalar_t*>(res.data_ptr()),
              HB ? reinterpret_cast<const scalar_t*>(bc.data_ptr()) : nullptr,
              reinterpret_cast<const scalar_t*>(gamma.data_ptr()),
              reinterpret_cast<const scalar_t*>(beta.data_ptr()), n1, n2, map,
              (float)eps, pinv, pthresh, rngkey);
    };
    auto pick_bias = [&](auto nv_tag, auto drop_tag) {
      if (has_bias) launch(nv_tag, drop_tag, std::true_type{});
      else launch(nv_tag, drop_tag, std::false_type{});
    };
    auto pick = [&](auto nv_tag) {
      if (drop) pick_bias(nv_tag, std::true_type{});
      else if constexpr (kMayPassThrough) pick_bias(nv_tag, std::false_type{});
    };
    if (n2 <= 512)
      pick(std::integral_constant<int, 1>{});
    else if (n2 <= 1024)
      pick(std::integral_constant<int, 2>{});
    else
      pick(std::integral_constant<int, 4>{});
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {normed, summed, dmask, mean, invvar};
}

}  // namespace

// returns {normed, summed, dmask, mean, invvar}
std::vector<at::Tensor> dropout_add_ln_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias,
    at::Tensor gamma, at::Tensor beta, double p, bool is_training,
    double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && res.is_contiguous(),
              "dropout_add_ln: contiguous CUDA");
  TORCH_CHECK(x.sizes() == res.sizes() && x.scalar_type() == res.scalar_type(),
              "dropout_add_ln: x/res mismatch");
  const int n2 = (int)x.size(-1);
  TORCH_CHECK(n2 % 8 == 0 && n2 <= 2048,
              "dropout_add_ln: hidden must be %%8==0 and <= 2048");
  TORCH_CHECK(gamma.numel() == n2 && beta.numel() == n2 &&
                  gamma.is_contiguous() && beta.is_contiguous(),
              "dropout_add_ln: bad gamma/beta");
  const bool drop = is_training && p > 0.0;
  const int64_t n8 = x.numel() / 8;
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
  if (bias.has_value()) {
    bc = bias->contiguous();
    TORCH_CHECK((int)bc.numel() == n2 && bc.scalar_type() == x.scalar_type(),
                "dropout_add_ln: bad bias");
  }
  return launch_ln_fwd("dropout_add_ln_forward", x, res, bc, gamma, beta,
                       dmask, FlatMap{}, drop, eps, pinv, pthresh, rngkey);
}

std::vector<at::Tensor> shared_dropout_add_ln_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias,
    at::Tensor gamma, at::Tensor beta, double p, int64_t shared_dim,
    double eps) {
  const char* name = "shared_dropout_add_ln_forward";
  check_operand(name, x, shared_dim);
  check_pair(name, x, res);
  check_p(name, p);
  const int n2 = (int)x.size(3);
  TORCH_CHECK(x.size(3) <= 2048, name,
              ": channel width must be at most 2048, got ", x.size(3));
  TORCH_CHECK(gamma.numel() == n2 && beta.numel() == n2, name,
              ": gamma/beta have ", gamma.numel(), "/", beta.numel(),
              " elements, the channel width is ", n2);
  TORCH_CHECK(gamma.is_contiguous() && beta.is_contiguous() &&
                  gamma.scalar_type() == x.scalar_type() &&
                  beta.scalar_type() == x.scalar_type() &&
                  gamma.device() == x.device() && beta.device() == x.device(),
              name, ": gamma/beta must be contiguous ", x.scalar_type(),
              " on ", x.device(), ", got ", gamma.scalar_type(), " on ",
              gamma.device(), " and ", beta.scalar_type(), " on ",
              beta.device());
  at::Tensor bc = check_bias(name, bias, x);
  const int64_t nmask = mask_units(x, shared_dim);
  auto dmask = at::empty({nmask}, x.options().dtype(at::kByte));
  if (x.numel() == 0) {
    auto fopt = x.options().dtype(at::kFloat);
    return {at::empty_like(x), at::empty_like(x), dmask, at::empty({0}, fopt),
            at::empty({0}, fopt)};
  }
  // the generator draw of the unshared entry, sized by the mask units
  return launch_ln_fwd(name, x, res, bc, gamma, beta, dmask,
                       row_map(x, shared_dim), true, eps,
                       (float)(1.0 / (1.0 - p)), keep16_threshold(p),
                       reserve_dropout_key(nmask));
}
