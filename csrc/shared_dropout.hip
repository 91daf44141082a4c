// Shared-axis (row-/column-wise) dropout for the fused residual joins on
// gfx950: out = residual + keep * (x [+ bias]) / (1 - p), where the keep
// decision ignores one spatial axis of a contiguous (B, R, T, C) tensor
// (AlphaFold 2 DropoutRowwise / DropoutColumnwise).
//
//   shared_dim = 1: keep(b, r, t, c) depends on (b, t, c) only
//   shared_dim = 2: keep(b, r, t, c) depends on (b, r, c) only
//
// Both cases are one index map over the 8-element units (or, in the LN
// kernel, over rows): view the index space as (outer, shared, inner) and
// drop the shared coordinate,
//
//   m = (i / (shared * inner)) * inner + i % inner,   first = shared coord == 0
//
// with inner = T*C/8 (shared_dim 1) or C/8 (shared_dim 2) for units and
// inner = T or 1 for rows. m is the unit's flat index in the small bitfield
// mask, (B, T, C/8) or (B, R, C/8) bytes, and the Philox subsequence: every
// thread recomputes keep16x8(key, m, 0, ...) for its unit, and only the
// threads with first == true store the byte. One launch, no extra pass, no
// activation-sized mask. Backward reads the byte through the same map and
// never touches Philox.
//
// The unshared kernels in dropout_add.hip / dropout_add_ln.hip are not
// touched: their keying, offset consumption and results stay as they are.
#include "common.h"
#include "fold.h"

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAGeneratorImpl.h>

#include <optional>
#include <vector>

namespace {

// (outer, shared, inner) index map. `small` is a kernel argument (uniform):
// when the whole index space fits 31 bits the two divisions are 32-bit.
struct SharedMap {
  int64_t inner;
  int64_t shared;
  bool small;
};

__device__ __forceinline__ int64_t shared_index(const SharedMap& sm, int64_t i,
                                                bool& first) {
  if (sm.small) {
    const uint32_t inner = (uint32_t)sm.inner, shared = (uint32_t)sm.shared;
    const uint32_t q = (uint32_t)i / inner;
    const uint32_t in = (uint32_t)i - q * inner;
    const uint32_t o = q / shared;
    first = q - o * shared == 0;
    return (int64_t)(o * inner + in);
  }
  const int64_t q = i / sm.inner;
  const int64_t in = i - q * sm.inner;
  const int64_t o = q / sm.shared;
  first = q - o * sm.shared == 0;
  return o * sm.inner + in;
}

template <typename T, bool HAS_BIAS>
__global__ void shared_dropout_add_fwd_kernel(
    T* __restrict__ out, uint8_t* __restrict__ dmask, const T* __restrict__ x,
    const T* __restrict__ res, const T* __restrict__ bias, int C, int64_t n8,
    SharedMap sm, float pinv, uint32_t pthresh, uint64_t rngkey) {
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
    bool first;
    const int64_t m = shared_index(sm, i, first);
    bool keep[8];
    keep16x8(rngkey, (uint64_t)m, 0, pthresh, keep);
    uint8_t bits = 0;
    {
      // product and sum each rounded once, for every element alike (the
      // compiler otherwise fuses some of the eight into an fma)
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bits |= (uint8_t)(keep[j] ? 1u : 0u) << j;
        fx[j] = fr[j] + (keep[j] ? fx[j] * pinv : 0.f);
      }
    }
    if (first) dmask[m] = bits;
    store8(out + i * 8, fx);
  }
}

// dropout_add_ln_fwd_kernel (dropout_add_ln.hip) with the keep decision
// taken per mask row: one index split per row, the lanes add their unit.
template <typename T, int NV, bool HAS_BIAS>
__global__ void shared_dropout_add_ln_fwd_kernel(
    T* __restrict__ normed, T* __restrict__ summed,
    uint8_t* __restrict__ dmask, float* __restrict__ mean,
    float* __restrict__ invvar, const T* __restrict__ x,
    const T* __restrict__ res, const T* __restrict__ bias,
    const T* __restrict__ gamma, const T* __restrict__ beta, int64_t n1,
    int n2, SharedMap sm, float eps, float pinv, uint32_t pthresh,
    uint64_t rngkey) {
  const int lane = threadIdx.x;
  const int wid = threadIdx.y;
  const int row8 = n2 / 8;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.y + wid; row < n1;
       row += (int64_t)gridDim.x * blockDim.y) {
    const int64_t rbase = row * (int64_t)n2;
    bool first;
    const int64_t mbase = shared_index(sm, row, first) * (int64_t)row8;
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
        const int64_t m = mbase + lane + i * 64;
        bool keep[8];
        keep16x8(rngkey, (uint64_t)m, 0, pthresh, keep);
        uint8_t bits = 0;
        {
          // as in shared_dropout_add_fwd_kernel: no fma into the sum below
#pragma clang fp contract(off)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            bits |= (uint8_t)(keep[j] ? 1u : 0u) << j;
            fx[j] = keep[j] ? fx[j] * pinv : 0.f;
          }
        }
        if (first) dmask[m] = bits;
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

template <typename T, bool BGRAD>
__global__ void shared_dropout_add_bwd_kernel(
    T* __restrict__ dx, const T* __restrict__ g,
    const uint8_t* __restrict__ dmask, float* __restrict__ partials, int C,
    int64_t n8, SharedMap sm, float pinv) {
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
    bool first;
    const uint8_t bits = dmask[shared_index(sm, i, first)];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (bits >> j) & 1 ? f[j] * pinv : 0.f;
    store8(dx + i * 8, f);
    if constexpr (BGRAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
  if constexpr (BGRAD) {
    colsum_block_fold(acc, c0, C, s_col, partials + (int64_t)blockIdx.x * C);
  }
}

#define DISPATCH_FTYPES(st, NAME, ...)                               \
  switch (st) {                                                      \
    case at::ScalarType::Float: {                                    \
      using scalar_t = float;                                        \
      __VA_ARGS__;                                                   \
      break;                                                         \
    }                                                                \
    case at::ScalarType::Half: {                                     \
      using scalar_t = __half;                                       \
      __VA_ARGS__;                                                   \
      break;                                                         \
    }                                                                \
    case at::ScalarType::BFloat16: {                                 \
      using scalar_t = __hip_bfloat16;                               \
      __VA_ARGS__;                                                   \
      break;                                                         \
    }                                                                \
    default:                                                         \
      TORCH_CHECK(false, NAME, ": unsupported dtype ", st);          \
  }

// checks common to the three entries; t is x (forward) or grad (backward)
void check_operand(const char* name, const at::Tensor& t, int64_t shared_dim) {
  TORCH_CHECK(t.is_cuda(), name, ": tensor must be on the GPU, got device ",
              t.device());
  TORCH_CHECK(t.dim() == 4, name, ": expected a 4-D (B, R, T, C) tensor, got ",
              t.dim(), "-D with sizes ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), name,
              ": tensor must be contiguous, got sizes ", t.sizes(),
              " strides ", t.strides());
  TORCH_CHECK(shared_dim == 1 || shared_dim == 2, name,
              ": shared_dim must be 1 or 2, got ", shared_dim);
  TORCH_CHECK(t.size(3) > 0 && t.size(3) % 8 == 0, name,
              ": channel width must be a positive multiple of 8, got ",
              t.size(3));
}

void check_pair(const char* name, const at::Tensor& x, const at::Tensor& res) {
  TORCH_CHECK(res.device() == x.device(), name,
              ": residual must be on the device of x, got ", res.device(),
              " vs ", x.device());
  TORCH_CHECK(res.sizes() == x.sizes(), name, ": residual sizes ", res.sizes(),
              " do not match x sizes ", x.sizes());
  TORCH_CHECK(res.scalar_type() == x.scalar_type(), name, ": residual dtype ",
              res.scalar_type(), " does not match x dtype ", x.scalar_type());
  TORCH_CHECK(res.is_contiguous(), name,
              ": residual must be contiguous, got strides ", res.strides());
}

void check_p(const char* name, double p) {
  TORCH_CHECK(p > 0.0 && p < 1.0, name,
              ": p must be in (0, 1) (the unshared entry serves p = 0), got ",
              p);
}

at::Tensor check_bias(const char* name, const std::optional<at::Tensor>& bias,
                      const at::Tensor& x) {
  at::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous();
    TORCH_CHECK(bc.numel() == x.size(3), name, ": bias has ", bc.numel(),
                " elements, the channel width is ", x.size(3));
    TORCH_CHECK(bc.scalar_type() == x.scalar_type() &&
                    bc.device() == x.device(),
                name, ": bias dtype/device ", bc.scalar_type(), " ",
                bc.device(), " does not match x ", x.scalar_type(), " ",
                x.device());
  }
  return bc;
}

// bytes of the small mask: B*T*C/8 (shared_dim 1) or B*R*C/8 (shared_dim 2)
int64_t mask_units(const at::Tensor& t, int64_t shared_dim) {
  return t.size(0) * t.size(shared_dim == 1 ? 2 : 1) * (t.size(3) / 8);
}

SharedMap unit_map(const at::Tensor& t, int64_t shared_dim) {
  const int64_t c8 = t.size(3) / 8;
  SharedMap sm;
  sm.inner = shared_dim == 1 ? t.size(2) * c8 : c8;
  sm.shared = t.size(shared_dim);
  sm.small = t.numel() / 8 <= 0x7fffffffLL;
  return sm;
}

SharedMap row_map(const at::Tensor& t, int64_t shared_dim) {
  SharedMap sm;
  sm.inner = shared_dim == 1 ? t.size(2) : 1;
  sm.shared = t.size(shared_dim);
  sm.small = t.numel() / t.size(3) <= 0x7fffffffLL;
  return sm;
}

// the generator draw of the unshared kernels, sized by the mask units
uint64_t reserve_key(int64_t nmask) {
  auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      std::nullopt, at::cuda::detail::getDefaultCUDAGenerator());
  at::PhiloxCudaState state;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    state = gen->philox_cuda_state(4 + nmask / (2048LL * 256) * 2);
  }
  return state.seed_.val + state.offset_.val * 0x9E3779B97F4A7C15ull;
}

}  // namespace

// returns {out, dmask}
std::vector<at::Tensor> shared_dropout_add_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias, double p,
    int64_t shared_dim) {
  const char* name = "shared_dropout_add_forward";
  check_operand(name, x, shared_dim);
  check_pair(name, x, res);
  check_p(name, p);
  at::Tensor bc = check_bias(name, bias, x);
  const bool has_bias = bias.has_value();
  const int C = (int)x.size(3);
  const int64_t n8 = x.numel() / 8;
  auto out = at::empty_like(x);
  const int64_t nmask = mask_units(x, shared_dim);
  auto dmask = at::empty({nmask}, x.options().dtype(at::kByte));
  if (n8 == 0) return {out, dmask};
  const SharedMap sm = unit_map(x, shared_dim);
  const float pinv = (float)(1.0 / (1.0 - p));
  const uint32_t pthresh = keep16_threshold(p);
  const uint64_t rngkey = reserve_key(nmask);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = unicore_grid((n8 + 255) / 256);
  DISPATCH_FTYPES(x.scalar_type(), name, {
    auto launch = [&](auto bias_tag) {
      constexpr bool HB = decltype(bias_tag)::value;
      shared_dropout_add_fwd_kernel<scalar_t, HB><<<grid, 256, 0, stream>>>(
          reinterpret_cast<scalar_t*>(out.data_ptr()),
          dmask.data_ptr<uint8_t>(),
          reinterpret_cast<const scalar_t*>(x.data_ptr()),
          reinterpret_cast<const scalar_t*>(res.data_ptr()),
          HB ? reinterpret_cast<const scalar_t*>(bc.data_ptr()) : nullptr, C,
          n8, sm, pinv, pthresh, rngkey);
    };
    if (has_bias) launch(std::true_type{});
    else launch(std::false_type{});
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {out, dmask};
}

// returns {normed, summed, dmask, mean, invvar}
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
  const bool has_bias = bias.has_value();
  const int64_t n1 = x.numel() / n2;

  auto normed = at::empty_like(x);
  auto summed = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({n1}, fopt);
  auto invvar = at::empty({n1}, fopt);
  const int64_t nmask = mask_units(x, shared_dim);
  auto dmask = at::empty({nmask}, x.options().dtype(at::kByte));
  if (n1 == 0) return {normed, summed, dmask, mean, invvar};
  const SharedMap sm = row_map(x, shared_dim);
  const float pinv = (float)(1.0 / (1.0 - p));
  const uint32_t pthresh = keep16_threshold(p);
  const uint64_t rngkey = reserve_key(nmask);

  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 block(64, 4);
  const dim3 grid(unicore_grid((n1 + 3) / 4));
  DISPATCH_FTYPES(x.scalar_type(), name, {
    auto launch = [&](auto nv_tag, auto bias_tag) {
      constexpr int NV = decltype(nv_tag)::value;
      constexpr bool HB = decltype(bias_tag)::value;
      shared_dropout_add_ln_fwd_kernel<scalar_t, NV, HB>
          <<<grid, block, 0, stream>>>(
              reinterpret_cast<scalar_t*>(normed.data_ptr()),
              reinterpret_cast<scalar_t*>(summed.data_ptr()),
              dmask.data_ptr<uint8_t>(), mean.data_ptr<float>(),
              invvar.data_ptr<float>(),
              reinterpret_cast<const scalar_t*>(x.data_ptr()),
              reinterpret_cast<const scalar_t*>(res.data_ptr()),
              HB ? reinterpret_cast<const scalar_t*>(bc.data_ptr()) : nullptr,
              reinterpret_cast<const scalar_t*>(gamma.data_ptr()),
              reinterpret_cast<const scalar_t*>(beta.data_ptr()), n1, n2, sm,
              (float)eps, pinv, pthresh, rngkey);
    };
    auto pick = [&](auto nv_tag) {
      if (has_bias) launch(nv_tag, std::true_type{});
      else launch(nv_tag, std::false_type{});
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
  const int64_t n8 = grad.numel() / 8;
  const float pinv = (float)(1.0 / (1.0 - p));
  auto dx = at::empty_like(grad);
  auto dbias = at::zeros({bgrad ? (int64_t)C : 0},
                         grad.options().dtype(at::kFloat));
  if (n8 == 0) return {dx, dbias};
  const SharedMap sm = unit_map(grad, shared_dim);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = bgrad ? colsum_grid(n8, C) : unicore_grid((n8 + 255) / 256);
  at::Tensor partials;
  if (bgrad) partials = at::empty({grid, (int64_t)C}, dbias.options());
  const size_t lds = bgrad ? (size_t)C * sizeof(float) : 0;
  DISPATCH_FTYPES(grad.scalar_type(), name, {
    auto launch = [&](auto bg_tag) {
      constexpr bool BG = decltype(bg_tag)::value;
      shared_dropout_add_bwd_kernel<scalar_t, BG><<<grid, 256, lds, stream>>>(
          reinterpret_cast<scalar_t*>(dx.data_ptr()),
          reinterpret_cast<const scalar_t*>(grad.data_ptr()),
          dmask.data_ptr<uint8_t>(),
          BG ? partials.data_ptr<float>() : nullptr, C, n8, sm, pinv);
    };
    if (bgrad) launch(std::true_type{});
    else launch(std::false_type{});
  });
  if (bgrad) {
    unicore_fold_columns(partials.data_ptr<float>(), dbias.data_ptr<float>(),
                         grid, C, partials.options(), stream);
  }
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {dx, dbias};
}
