// Host-side helpers shared by the kernel entry points: the floating dtype
// switch and the generator reservation of the dropout kernels.
// Needs the torch headers, so it is kept out of common.h.
#pragma once

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAGeneratorImpl.h>

#include <cstdint>
#include <mutex>

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

// Advances the default generator's Philox offset by `increment` and returns
// the kernel's key: seed and the offset before the advance, folded into the
// one 64-bit value keep16x8 is keyed by.
static inline uint64_t reserve_philox_key(uint64_t increment) {
  auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      std::nullopt, at::cuda::detail::getDefaultCUDAGenerator());
  at::PhiloxCudaState state;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    state = gen->philox_cuda_state(increment);
  }
  return state.seed_.val + state.offset_.val * 0x9E3779B97F4A7C15ull;
}

// The reservation of a dropout kernel that draws once per 8-element unit,
// n units in all.
static inline uint64_t reserve_dropout_key(int64_t n) {
  return reserve_philox_key(4 + n / (2048LL * 256) * 2);
}
