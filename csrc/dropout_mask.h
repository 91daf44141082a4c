// Mask maps of the fused residual joins (dropout_add.hip, dropout_add_ln.hip)
// and the host helpers of their shared-axis entries.
//
// A join kernel is templated on a map from its index space (8-element units,
// or rows in the LN kernel) to the index m that is both the Philox
// subsequence and the byte of the bitfield mask. Every thread recomputes
// keep16x8(key, m, 0, ...) for its unit; the threads the map calls `first`
// store the byte; backward reads the byte through the same map.
//
//   FlatMap    m = i: one decision per element, a mask of numel/8 bytes.
//   SharedMap  the keep decision ignores one spatial axis of a contiguous
//              (B, R, T, C) tensor (AlphaFold 2 DropoutRowwise /
//              DropoutColumnwise):
//                shared_dim = 1: keep(b, r, t, c) depends on (b, t, c) only
//                shared_dim = 2: keep(b, r, t, c) depends on (b, r, c) only
//              View the index space as (outer, shared, inner) and drop the
//              shared coordinate,
//                m = (i / (shared * inner)) * inner + i % inner,
//                first = shared coord == 0
//              with inner = T*C/8 (shared_dim 1) or C/8 (shared_dim 2) for
//              units and inner = T or 1 for rows. The mask is the small
//              (B, T, C/8) or (B, R, C/8) bytes. With a shared extent of 1
//              this is the flat map.
//
// kExact is the map's rounding policy for out = res + keep * x * pinv. The
// shared entries promise the fp32 result res + where(keep, x * pinv, 0)
// exactly, so their product is rounded on its own; the flat kernels leave it
// open to contraction into the add, as they always have.
#pragma once

#include <torch/extension.h>

#include <optional>

#include "common.h"

struct FlatMap {
  static constexpr bool kExact = false;
};

// `small` is a kernel argument (uniform): when the whole index space fits 31
// bits the two divisions are 32-bit.
struct SharedMap {
  static constexpr bool kExact = true;
  int64_t inner;
  int64_t shared;
  bool small;
};

__device__ __forceinline__ int64_t mask_index(const FlatMap&, int64_t i,
                                              bool& first) {
  first = true;
  return i;
}

__device__ __forceinline__ int64_t mask_index(const SharedMap& sm, int64_t i,
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

// keep ? x * pinv : 0. EXACT: the product is rounded once, for every element
// alike (the compiler otherwise fuses some of them into an fma with the add
// that follows).
template <bool EXACT>
__device__ __forceinline__ float drop_scale(bool keep, float x, float pinv) {
  if constexpr (EXACT) {
#pragma clang fp contract(off)
    return keep ? x * pinv : 0.f;
  } else {
    return keep ? x * pinv : 0.f;
  }
}

// ---------------------------------------------------------------------------
// host side of the shared-axis entries
// ---------------------------------------------------------------------------

// checks common to the three entries; t is x (forward) or grad (backward)
static inline void check_operand(const char* name, const at::Tensor& t,
                                 int64_t shared_dim) {
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

static inline void check_pair(const char* name, const at::Tensor& x,
                              const at::Tensor& res) {
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

static inline void check_p(const char* name, double p) {
  TORCH_CHECK(p > 0.0 && p < 1.0, name,
              ": p must be in (0, 1) (the unshared entry serves p = 0), got ",
              p);
}

static inline at::Tensor check_bias(const char* name,
                                    const std::optional<at::Tensor>& bias,
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
static inline int64_t mask_units(const at::Tensor& t, int64_t shared_dim) {
  return t.size(0) * t.size(shared_dim == 1 ? 2 : 1) * (t.size(3) / 8);
}

static inline SharedMap unit_map(const at::Tensor& t, int64_t shared_dim) {
  const int64_t c8 = t.size(3) / 8;
  SharedMap sm;
  sm.inner = shared_dim == 1 ? t.size(2) * c8 : c8;
  sm.shared = t.size(shared_dim);
  sm.small = t.numel() / 8 <= 0x7fffffffLL;
  return sm;
}

static inline SharedMap row_map(const at::Tensor& t, int64_t shared_dim) {
  SharedMap sm;
  sm.inner = shared_dim == 1 ? t.size(2) : 1;
  sm.shared = t.size(shared_dim);
  sm.small = t.numel() / t.size(3) <= 0x7fffffffLL;
  return sm;
}
