// Uni-Mol's norm regularisers (x_norm, delta_pair_repr_norm) for gfx950.
//
//   err(ss, C)  = relu(|sqrt(ss + 1e-10) - sqrt(C)| - 1)
//   coef(ss, C) = d err / d ss * 2 = sign(n - sqrt(C)) [|n - sqrt(C)| > 1] / n
//
// so that d err / d v = coef * v for every element v of the reduced vector.
// A padded position is removed by a select: err = coef = 0 whatever the
// inputs hold there, and its gradient is a stored 0, never 0 * value.
//
// pair_norm_fwd  (B,H,L,L) x 2 -> coef (B,L,L) fp32 + per-unit error sums.
//   256 threads own 64 consecutive 8-position units of the flattened
//   (b, i, j/8) space; lane l of every wave owns unit l and wave w sums the
//   heads [w H/4, (w+1) H/4). One wave instruction reads 1 KB of contiguous
//   memory per tensor; the head loop keeps 8 16 B loads per tensor in
//   flight. The four partial sums meet in 8 KB of LDS, summed in wave order
//   by wave 0, which writes coef (two 16 B stores) and the unit's error.
// pair_norm_bwd  streaming: a thread owns one 8-position unit of one
//   (b, h, i) row, reads its 8 coefs (shared by the H heads) and, unless all
//   are 0, pair and bias; d_pair = gscale[b] * coef * delta rounded once,
//   d_bias = -d_pair written in the same pass.
// row_norm_fwd / _bwd  (N, E) channels last, one wave per row.
//
// No atomics anywhere: every output element has one owner and one
// summation order.
#include "pair_norm.h"

#include "common.h"

#include <ATen/cuda/CUDAContext.h>

namespace {

constexpr float kNormEps = 1e-10f;
constexpr float kNormTol = 1.0f;

// sum of squares -> (err, coef). The one copy of the formula: the pair and
// the row kernels both call it. !(a <= tol) keeps a NaN norm visible at a
// valid position, as the eager definition does.
__device__ __forceinline__ void norm_err_coef(float ss, float root_c,
                                              bool valid, float& err,
                                              float& coef) {
  const float n = sqrtf(ss + kNormEps);
  const float d = n - root_c;
  const float a = fabsf(d);
  const bool on = valid && !(a <= kNormTol);
  err = on ? a - kNormTol : 0.f;
  coef = on ? copysignf(1.f, d) / n : 0.f;
}

// 8 elements as they come from memory: the head loop issues its loads into
// these and converts afterwards, so the loads of one trip are all in flight
template <typename T>
struct Raw8 {
  uint4 v;
};
template <>
struct Raw8<float> {
  float4 a, b;
};

template <typename T>
__device__ __forceinline__ Raw8<T> load_raw8(const T* p) {
  Raw8<T> r;
  if constexpr (sizeof(T) == 2) {
    r.v = *reinterpret_cast<const uint4*>(p);
  } else {
    r.a = reinterpret_cast<const float4*>(p)[0];
    r.b = reinterpret_cast<const float4*>(p)[1];
  }
  return r;
}

template <typename T>
__device__ __forceinline__ void unpack8(const Raw8<T>& r, float (&f)[8]) {
  if constexpr (sizeof(T) == 2) {
    union {
      uint4 u;
      T t[8];
    } U;
    U.u = r.v;
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = Cvt<T>::to_f(U.t[k]);
  } else {
    f[0] = r.a.x; f[1] = r.a.y; f[2] = r.a.z; f[3] = r.a.w;
    f[4] = r.b.x; f[5] = r.b.y; f[6] = r.b.z; f[7] = r.b.w;
  }
}

template <typename T>
__device__ __forceinline__ void add_sq8(const Raw8<T>& rp, const Raw8<T>& rb,
                                        float (&ss)[8]) {
  float p[8], q[8];
  unpack8(rp, p);
  unpack8(rb, q);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float d = p[k] - q[k];
    ss[k] = fmaf(d, d, ss[k]);
  }
}

// ---------------------------------------------------------------------------
// pair forward
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pair_norm_fwd_kernel(
    const T* __restrict__ pair, const T* __restrict__ bias,
    const uint8_t* __restrict__ pad, float* __restrict__ coef,
    float* __restrict__ uerr, uint32_t n_units, int n_blocks, int H, int L,
    float root_h) {
  // [wave][position][lane]: lanes on consecutive banks
  __shared__ float s_ss[4][8][64];
  // heads per trip: 8 loads of 16 B per tensor
  constexpr int UNR = sizeof(T) == 2 ? 8 : 4;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const uint32_t l8 = (uint32_t)L / 8;
  const uint32_t ll8 = (uint32_t)L * l8;  // units per sample
  const int64_t LL = (int64_t)L * L;
  const int hw = H / 4;

  for (int blk = (int)blockIdx.x; blk < n_blocks; blk += (int)gridDim.x) {
    const uint32_t u = (uint32_t)blk * 64u + (uint32_t)lane;
    const bool live = u < n_units;
    const uint32_t b = live ? u / ll8 : 0u;
    const uint32_t r = live ? u - b * ll8 : 0u;  // (i, j/8) within the sample
    float ss[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      const int64_t base =
          ((int64_t)b * H + (int64_t)wave * hw) * LL + (int64_t)r * 8;
      const T* pp = pair + base;
      const T* pb = bias + base;
      int h = 0;
      for (; h + UNR <= hw; h += UNR) {
        Raw8<T> rp[UNR], rb[UNR];
#pragma unroll
        for (int t = 0; t < UNR; ++t) {
          rp[t] = load_raw8(pp + (int64_t)(h + t) * LL);
          rb[t] = load_raw8(pb + (int64_t)(h + t) * LL);
        }
#pragma unroll
        for (int t = 0; t < UNR; ++t) add_sq8(rp[t], rb[t], ss);
      }
      for (; h < hw; ++h)
        add_sq8(load_raw8(pp + (int64_t)h * LL), load_raw8(pb + (int64_t)h * LL),
                ss);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_ss[wave][k][lane] = ss[k];
    __syncthreads();
    if (wave == 0 && live) {
      const uint32_t i = r / l8, j8 = r - i * l8;
      bool pad_i = false;
      uint64_t pad_j = 0;
      if (pad != nullptr) {
        const uint8_t* prow = pad + (int64_t)b * L;
        pad_i = prow[i] != 0;
        pad_j = *reinterpret_cast<const uint64_t*>(prow + j8 * 8);
      }
      float c[8], esum = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float tot = ((s_ss[0][k][lane] + s_ss[1][k][lane]) +
                           s_ss[2][k][lane]) + s_ss[3][k][lane];
        const bool valid = !pad_i && ((pad_j >> (8 * k)) & 0xffull) == 0;
        float e;
        norm_err_coef(tot, root_h, valid, e, c[k]);
        esum += e;
      }
      store8<float>(coef + (int64_t)u * 8, c);
      uerr[u] = esum;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// pair backward
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pair_norm_bwd_kernel(
    const T* __restrict__ pair, const T* __restrict__ bias,
    const float* __restrict__ coef, const float* __restrict__ gscale,
    T* __restrict__ d_pair, T* __restrict__ d_bias, uint32_t n_units,
    uint32_t hll8 /* units per sample, all heads */,
    uint32_t ll8 /* units per (b, h) plane */) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint64_t v64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; v64 < n_units;
       v64 += stride) {
    const uint32_t v = (uint32_t)v64;
    const uint32_t b = v / hll8;
    const uint32_t r = (v - b * hll8) % ll8;
    float cf[8];
    load8<float>(coef + ((int64_t)b * ll8 + r) * 8, cf);
    const int64_t off = (int64_t)v * 8;
    float g[8], ng[8];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) any = any || cf[k] != 0.f;
    if (!any) {
      // inside the tolerance band or padded: nothing to read
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        g[k] = 0.f;
        ng[k] = -0.f;
      }
    } else {
      const float gs = gscale[b];
      float p[8], q[8];
      load8(pair + off, p);
      load8(bias + off, q);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        // select, not multiply: a masked position may hold inf or NaN
        g[k] = cf[k] != 0.f ? (gs * cf[k]) * (p[k] - q[k]) : 0.f;
        ng[k] = -g[k];
      }
    }
    store8(d_pair + off, g);
    store8(d_bias + off, ng);
  }
}

// ---------------------------------------------------------------------------
// rows: (N, E), one wave per row
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void row_norm_fwd_kernel(
    const T* __restrict__ x, const uint8_t* __restrict__ pad,
    float* __restrict__ coef, float* __restrict__ err, int64_t N, int E,
    float root_e) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N;
       row += (int64_t)gridDim.x * 4) {
    const bool valid = pad == nullptr || pad[row] == 0;
    float ss = 0.f;
    if (valid) {  // wave-uniform
      const T* xr = x + row * E;
      for (int c = lane * 8; c < E; c += 512) {
        float f[8];
        load8(xr + c, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss = fmaf(f[k], f[k], ss);
      }
    }
    ss = wave_sum(ss);
    float e, cf;
    norm_err_coef(ss, root_e, valid, e, cf);
    if (lane == 0) {
      err[row] = e;
      coef[row] = cf;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void row_norm_bwd_kernel(
    const T* __restrict__ x, const float* __restrict__ coef,
    const float* __restrict__ g_row, T* __restrict__ dx, int64_t N, int E) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N;
       row += (int64_t)gridDim.x * 4) {
    const float cf = coef[row];
    const T* xr = x + row * E;
    T* dr = dx + row * E;
    float f[8];
    if (cf == 0.f) {  // wave-uniform; inside the band or padded
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = 0.f;
      for (int c = lane * 8; c < E; c += 512) store8(dr + c, f);
      continue;
    }
    const float s = g_row[row] * cf;
    for (int c = lane * 8; c < E; c += 512) {
      load8(xr + c, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] *= s;
      store8(dr + c, f);
    }
  }
}

// the regularisers serve bf16 and fp32 only
#define DISPATCH_NORM_TYPES(st, NAME, ...)                       \
  switch (st) {                                                  \
    case at::ScalarType::Float: {                                \
      using scalar_t = float;                                    \
      __VA_ARGS__;                                               \
      break;                                                     \
    }                                                            \
    case at::ScalarType::BFloat16: {                             \
      using scalar_t = __hip_bfloat16;                           \
      __VA_ARGS__;                                               \
      break;                                                     \
    }                                                            \
    default:                                                     \
      TORCH_CHECK(false, NAME, ": unsupported dtype ", st);      \
  }

}  // namespace

void pair_norm_forward_launch(at::Tensor& coef, at::Tensor& uerr,
                              const at::Tensor& pair, const at::Tensor& bias,
                              const uint8_t* pad) {
  const int64_t B = pair.size(0), H = pair.size(1), L = pair.size(3);
  const int64_t n_units = B * L * (L / 8);
  const int64_t n_blocks = (n_units + 63) / 64;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_NORM_TYPES(pair.scalar_type(), "pair_norm_forward", {
    pair_norm_fwd_kernel<scalar_t>
        <<<unicore_grid(n_blocks), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(pair.data_ptr()),
            reinterpret_cast<const scalar_t*>(bias.data_ptr()), pad,
            coef.data_ptr<float>(), uerr.data_ptr<float>(), (uint32_t)n_units,
            (int)n_blocks, (int)H, (int)L, sqrtf((float)H));
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair_norm_backward_launch(at::Tensor& d_pair, at::Tensor& d_bias,
                               const at::Tensor& gscale, const at::Tensor& coef,
                               const at::Tensor& pair, const at::Tensor& bias) {
  const int64_t B = pair.size(0), H = pair.size(1), L = pair.size(3);
  const int64_t ll8 = L * (L / 8);
  const int64_t n_units = B * H * ll8;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_NORM_TYPES(pair.scalar_type(), "pair_norm_backward", {
    pair_norm_bwd_kernel<scalar_t>
        <<<unicore_grid((n_units + 255) / 256), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(pair.data_ptr()),
            reinterpret_cast<const scalar_t*>(bias.data_ptr()),
            coef.data_ptr<float>(), gscale.data_ptr<float>(),
            reinterpret_cast<scalar_t*>(d_pair.data_ptr()),
            reinterpret_cast<scalar_t*>(d_bias.data_ptr()), (uint32_t)n_units,
            (uint32_t)(H * ll8), (uint32_t)ll8);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void row_norm_forward_launch(at::Tensor& coef, at::Tensor& err,
                             const at::Tensor& x, const uint8_t* pad) {
  const int64_t N = x.size(0), E = x.size(1);
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_NORM_TYPES(x.scalar_type(), "row_norm_forward", {
    row_norm_fwd_kernel<scalar_t>
        <<<unicore_grid((N + 3) / 4), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(x.data_ptr()), pad,
            coef.data_ptr<float>(), err.data_ptr<float>(), N, (int)E,
            sqrtf((float)E));
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void row_norm_backward_launch(at::Tensor& dx, const at::Tensor& g_row,
                              const at::Tensor& coef, const at::Tensor& x) {
  const int64_t N = x.size(0), E = x.size(1);
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_NORM_TYPES(x.scalar_type(), "row_norm_backward", {
    row_norm_bwd_kernel<scalar_t>
        <<<unicore_grid((N + 3) / 4), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(x.data_ptr()),
            coef.data_ptr<float>(), g_row.data_ptr<float>(),
            reinterpret_cast<scalar_t*>(dx.data_ptr()), N, (int)E);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}
