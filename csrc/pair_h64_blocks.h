// Device blocks the fp32-MFMA pair-track heads at H = 64 share
// (pair_coord_h64.hip, pair_dist_h64.hip): the step geometry, the matrix
// instruction, the wave fence, 16 B chunk (un)packing, the row a wave owns,
// the lane -> (plane, chunk) map and the W1 fragments of hid^T = W1 x.
//
// Fragment map of v_mfma_f32_16x16x4_f32 (mfma_probe.hip checks it), lane l,
// g = l >> 4, r = l & 15:
//   A (16x4):  A[m = r][k = g]         B (4x16): B[k = g][n = r]
//   C (16x16): C[m = g*4 + v][n = r],  v = 0..3
#pragma once

#include "common.h"

#include <hip/hip_runtime.h>

namespace pair_h64 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH = 64;
constexpr int kWaves = 4;           // per block, one row each
constexpr int kDTile = kH * 16;     // floats of an input tile, pitch 16
constexpr int kOTile = kH * 20;     // floats of a dpair tile, pitch 20

// built without the packed fp32 VALU forms, as pair_attn.hip
#if defined(__HIP_DEVICE_COMPILE__)
#define PAIR_H64_KERNEL \
  __attribute__((target("no-packed-fp32-ops"))) __global__ void __launch_bounds__(256)
#else
#define PAIR_H64_KERNEL __global__ void __launch_bounds__(256)
#endif

template <typename T>
struct Step {
  static constexpr int E = 16 / (int)sizeof(T);       // elements of a chunk
  static constexpr int TS = sizeof(T) == 2 ? 2 : 1;   // 16-j tiles of a step
  static constexpr int JS = 16 * TS;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// orders this wave's LDS writes before its later LDS reads (and the reverse)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ void unpack(const uint4& u, float (&f)[Step<T>::E]) {
  if constexpr (sizeof(T) == 2) {
    union {
      uint4 u;
      T t[8];
    } U;
    U.u = u;
#pragma unroll
    for (int t = 0; t < 8; ++t) f[t] = Cvt<T>::to_f(U.t[t]);
  } else {
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y);
    f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
  }
}

template <typename T>
__device__ __forceinline__ uint4 pack(const float (&f)[Step<T>::E]) {
  if constexpr (sizeof(T) == 2) {
    union {
      uint4 u;
      T t[8];
    } U;
#pragma unroll
    for (int t = 0; t < 8; ++t) U.t[t] = Cvt<T>::from_f(f[t]);
    return U.u;
  } else {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                      __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
}

// The row a wave works on. Everything here is wave-uniform.
struct Row {
  int64_t row;   // b * L + i
  int64_t b;
  int64_t base;  // offset of pair[b, 0, i, 0]
  bool live;     // i is a real atom
};

__device__ __forceinline__ Row make_row(int64_t row, int L,
                                        const uint8_t* __restrict__ pad) {
  Row w;
  w.row = row;
  w.b = row / L;
  w.base = (w.b * kH * L + (row - w.b * L)) * (int64_t)L;
  w.live = pad == nullptr || !pad[row];
  return w;
}

// first j of this lane's chunk in step s; chunks lie wholly inside or outside
// the row because L % 8 == 0
template <typename T>
__device__ __forceinline__ int chunk_j(int s, int lane) {
  return s * Step<T>::JS + (lane & 3) * Step<T>::E;
}

// W1 (o, h) row-major as the fragments of hid^T = W1 x:
// wf[ot][ks] = W1[ot*16 + r][ks*4 + g]
__device__ __forceinline__ void load_w1_frags(const float* __restrict__ W1,
                                              int lane, float (&wf)[4][16]) {
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
      wf[ot][ks] = W1[(ot * 16 + r) * kH + ks * 4 + g];
}

// acc[ot][v] = hid[o = ot*16 + g*4 + v][j = r] of one tile
__device__ __forceinline__ void hidden_oj(const float* tile,
                                          const float (&wf)[4][16],
                                          const float (&b1v)[4][4], int lane,
                                          f32x4 (&acc)[4]) {
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[ot][v] = b1v[ot][v];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const float bv = tile[ks * 64 + lane];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) acc[ot] = mfma4(wf[ot][ks], bv, acc[ot]);
  }
}

// values of a length-64 vector on the C-layout rows: x[ot][v] = p[ot*16+g*4+v]
__device__ __forceinline__ void load_c_rows(const float* __restrict__ p,
                                            int lane, float (&x)[4][4]) {
  const int g = lane >> 4;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int v = 0; v < 4; ++v) x[ot][v] = p[ot * 16 + g * 4 + v];
}

// blocks of kWaves rows; the cap keeps a few blocks per CU resident
static inline int h64_grid(int64_t n_rows, int cap) {
  return unicore_grid((n_rows + kWaves - 1) / kWaves, cap);
}

}  // namespace pair_h64
