// Uni-Mol's edge-typed gaussian pair embedding at K = 128 gaussians, H = 64
// heads, bf16, for gfx950, every product on v_mfma_f32_16x16x32_bf16:
//
//   d_ij  = |c_i - c_j| (0 on the diagonal),  x_ij = a_ij d_ij + b_ij
//   g_ijk = exp(-0.5 ((x_ij - m_k) / s_k)^2) / (sqrt(2 * 3.14159) s_k),
//           s_k = |stds_k| + 1e-5                       fp32 -> bf16 operand
//   pre   = W1 g + b1 (fp32),  h = gelu(pre) -> bf16 operand
//   out[b, :, i, j] = W2 h + b2 -> bf16 at the store; fill where j is padded
//
// a and b are the per-edge-type affine terms the module gathers, (B, L, L)
// fp32. Nothing of B*L*L*128 elements exists in memory: the backward kernels
// recompute g, pre and h from coords, a and b.
//
// Geometry (all three kernels). A block is four waves, a wave owns one (b, i)
// row and walks it in tiles of 16 j; lane l = (g = l >> 4, r = l & 15) works
// on pair j0 + r. Fragment map of the instruction (mfma_probe.hip):
//   A (16x32): A[m = r][k = g*8 + e]    B (32x16): B[k = g*8 + e][n = r]
//   C (16x16): C[m = g*4 + v][n = r]
// The weights are on M, the pairs on N: pre^T = W1 g^T. A lane computes its
// pair's 32 features straight into the B operand, and a C tile [unit g*4+v]
// [pair r], once through the GELU, is again a B operand without leaving the
// registers, because the order of an MFMA's k is free as long as both operands
// agree: B slot (step ks, g, e) stands for unit
//   perm(ks, g, e) = (2 ks + (e >> 2)) * 16 + g*4 + (e & 3),
// which is C tile 2 ks + (e >> 2), register e & 3, and every weight fragment
// that multiplies such an operand is laid out in LDS with that k order. The
// features use the same order (k = kt*16 + g*4 + v), so in the backward dg,
// which arrives as C tiles, meets its own features in the same registers.
// Weight fragments are 16 B per lane, stored [fragment][lane]: one
// conflict-free ds_read_b128 each.
//
//   forward  pre^T (32 MFMAs), GELU, out^T = W2 h^T (16), + b2, select fill,
//            -> a wave-private bf16 tile [head][16 j] -> 16 B stores along j.
//            The next tile's a, b, pad and c_j are loaded before the products.
//   dx       d_out tile: 16 B loads along j, masked by a select, transposed
//            through a wave-private tile [j][head] into B operands;
//            dh^T = W2^T d_out^T (16), dpre = dh gelu'(pre) (fp32) -> bf16,
//            dg^T = W1^T dpre^T (32); per pair dx = sum_k dg_k g_k (-(x - m_k)
//            / s_k^2) in-lane over 32 k then two shuffles; d_a = dx d, d_b =
//            dx leave as 16 B fp32 stores; d_means and d_stds accumulate in
//            registers, are summed over the 16 lanes of a group and the waves
//            in order at the end, one partials row per block.
//   wgrad    pairs on the contraction: every wave recomputes g, h, dpre of its
//            own tile (the code of dx) and puts them, as bf16, into block
//            tiles [unit][64 pairs] next to the masked d_out [head][64 pairs].
//            Then wave w owns rows 32 w .. of dW1 = dpre^T g (16 C tiles) and
//            rows 16 w .. of dW2 = d_out^T h (8 C tiles); db1 and db2 are the
//            same A fragments against a B of ones. 96 + 12 accumulator
//            registers, no cross-wave sum: a block's partials row is written
//            by the owners.
// Partials are folded by unicore_fold_columns: no atomics anywhere.
#include "pair_gauss_h64.h"

#include "common.h"
#include "fold.h"
#include "pair_coord_h64.h"  // gelu_exact, gelu_exact_grad

#include <ATen/cuda/CUDAContext.h>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int kK = 128;     // gaussians = hidden units
constexpr int kH = 64;      // heads
constexpr int kWaves = 4;   // per block, one row each
constexpr int kOP = 24;     // pitch of the forward's [head][16 j] tile, bf16
constexpr int kTP = 72;     // pitch of the [j][head] and [unit][64 pairs] tiles
// dW1 | db1 | dW2 | db2
constexpr int kWCols = kK * kK + kK + kH * kK + kH;
constexpr int kSCols = 2 * kK;  // d_means | d_stds
constexpr float kLog2e = 1.4426950408889634f;

// per-k constants in LDS
constexpr int cM = 0, cIs2 = kK, cNrm = 2 * kK, cIsg = 3 * kK, cB1 = 4 * kK,
              cB2 = 5 * kK, kConsts = 5 * kK + kH;

union Frag {
  uint4 u;
  bf16x8 v;
};

__device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c) {
  Frag A, B;
  A.u = a;
  B.u = b;
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.v, B.v, c, 0, 0, 0);
}

// orders this wave's LDS writes before its later LDS reads (and the reverse)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int perm(int ks, int g, int e) {
  return (2 * ks + (e >> 2)) * 16 + g * 4 + (e & 3);
}

__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return (uint32_t)f32_to_bf16_bits(lo) | ((uint32_t)f32_to_bf16_bits(hi) << 16);
}

// C tiles [unit kt*16 + g*4 + v][pair r] -> the four B operands in perm order
__device__ __forceinline__ void pack_perm(const float (&f)[8][4],
                                          uint4 (&o)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    o[ks] = make_uint4(pack2(f[2 * ks][0], f[2 * ks][1]),
                       pack2(f[2 * ks][2], f[2 * ks][3]),
                       pack2(f[2 * ks + 1][0], f[2 * ks + 1][1]),
                       pack2(f[2 * ks + 1][2], f[2 * ks + 1][3]));
}

enum WKind {
  kW1A,   // (ot, ks): W1[ot*16 + r][perm(ks, g, e)]       pre^T = W1 g^T
  kW2A,   // (ht, ks): W2[ht*16 + r][perm(ks, g, e)]       out^T = W2 h^T
  kW2T,   // (ot, ks): W2[ks*32 + g*8 + e][ot*16 + r]      dh^T = W2^T d_out^T
  kW1T,   // (kt, ks): W1[perm(ks, g, e)][kt*16 + r]       dg^T = W1^T dpre^T
};

// weight fragments -> LDS, [fragment][lane]; W row-major with 128 columns
template <WKind KIND>
__device__ __forceinline__ void fill_frags(uint4* dst,
                                           const uint16_t* __restrict__ W) {
  constexpr int KS = KIND == kW2T ? 2 : 4;               // k steps
  constexpr int NF = (KIND == kW2A ? 4 : 8) * KS;        // fragments
  for (int idx = (int)threadIdx.x; idx < NF * 64; idx += 256) {
    const int f = idx >> 6, ln = idx & 63, g = ln >> 4, r = ln & 15;
    const int mt = f / KS, ks = f % KS;
    uint32_t w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int at;
      if constexpr (KIND == kW1A || KIND == kW2A)
        at = (mt * 16 + r) * kK + perm(ks, g, e);
      else if constexpr (KIND == kW2T)
        at = (ks * 32 + g * 8 + e) * kK + mt * 16 + r;
      else
        at = perm(ks, g, e) * kK + mt * 16 + r;
      w[e] = W[at];
    }
    dst[idx] = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16),
                          w[4] | (w[5] << 16), w[6] | (w[7] << 16));
  }
}

__device__ __forceinline__ void fill_consts(float* s_c,
                                            const float* __restrict__ means,
                                            const float* __restrict__ stds,
                                            const uint16_t* __restrict__ b1,
                                            const uint16_t* __restrict__ b2) {
  const int k = (int)threadIdx.x;
  if (k < kK) {
    const float sd = stds[k];
    const float s = fabsf(sd) + 1e-5f;
    s_c[cM + k] = means[k];
    s_c[cIs2 + k] = 1.f / (s * s);
    s_c[cNrm + k] = 1.f / (sqrtf(2.f * 3.14159f) * s);
    s_c[cIsg + k] = (sd > 0.f ? 1.f : (sd < 0.f ? -1.f : 0.f)) / s;
    s_c[cB1 + k] = bf16_bits_to_f32(b1[k]);
    if (k < kH) s_c[cB2 + k] = b2 != nullptr ? bf16_bits_to_f32(b2[k]) : 0.f;
  }
}

// what a lane needs of its pair (row, j)
struct PairIn {
  float a, b, cx, cy, cz;
  bool dead;  // j is padded or past the row end
};

// padb: the pad bytes of the row's sample, or null
__device__ __forceinline__ PairIn load_pair(const float* __restrict__ coords,
                                            const float* __restrict__ a,
                                            const float* __restrict__ b,
                                            const uint8_t* __restrict__ padb,
                                            int64_t row, int64_t bL, int L,
                                            int j) {
  const int jc = j < L ? j : 0;
  PairIn p;
  p.a = a[row * L + jc];
  p.b = b[row * L + jc];
  const float* c = coords + (bL + jc) * 3;
  p.cx = c[0];
  p.cy = c[1];
  p.cz = c[2];
  p.dead = j >= L || (padb != nullptr && padb[jc] != 0);
  return p;
}

// d = |c_i - c_j|, exactly 0 on the diagonal; returns x = a d + b
__device__ __forceinline__ float pair_x(const PairIn& p, float ix, float iy,
                                        float iz, bool diag, float& d) {
  const float dx = ix - p.cx, dy = iy - p.cy, dz = iz - p.cz;
  const float ssq = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                              __fmul_rn(dz, dz));
  d = diag ? 0.f : sqrtf(ssq);
  return __fadd_rn(__fmul_rn(p.a, d), p.b);
}

// gf[kt][v] = g at k = kt*16 + g*4 + v
__device__ __forceinline__ void features(const float* s_c, float x, int g,
                                         float (&gf)[8][4]) {
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const int k0 = kt * 16 + g * 4;
    const float4 m = *reinterpret_cast<const float4*>(s_c + cM + k0);
    const float4 q = *reinterpret_cast<const float4*>(s_c + cIs2 + k0);
    const float4 n = *reinterpret_cast<const float4*>(s_c + cNrm + k0);
    const float mv[4] = {m.x, m.y, m.z, m.w}, qv[4] = {q.x, q.y, q.z, q.w},
                nv[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float t = x - mv[v];
      gf[kt][v] =
          __builtin_amdgcn_exp2f(-0.5f * kLog2e * qv[v] * t * t) * nv[v];
    }
  }
}

// acc[ot][v] = pre[unit ot*16 + g*4 + v][pair r]
__device__ __forceinline__ void pre_tile(const uint4* s_w1, const float* s_c,
                                         const uint4 (&gb)[4], int lane,
                                         f32x4 (&acc)[8]) {
  const int g = lane >> 4;
#pragma unroll
  for (int ot = 0; ot < 8; ++ot) {
    const float4 bv =
        *reinterpret_cast<const float4*>(s_c + cB1 + ot * 16 + g * 4);
    acc[ot] = f32x4{bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      acc[ot] = mfma(s_w1[(ot * 4 + ks) * 64 + lane], gb[ks], acc[ot]);
  }
}

__global__ void __launch_bounds__(256) pair_gauss_h64_fwd_kernel(
    const float* __restrict__ coords, const float* __restrict__ a,
    const float* __restrict__ b, const uint8_t* __restrict__ pad,
    const float* __restrict__ means, const float* __restrict__ stds,
    const uint16_t* __restrict__ W1, const uint16_t* __restrict__ b1,
    const uint16_t* __restrict__ W2, const uint16_t* __restrict__ b2,
    uint16_t* __restrict__ out, int64_t n_rows, int L, uint32_t fill) {
  __shared__ __align__(16) uint4 s_w1[32 * 64];
  __shared__ __align__(16) uint4 s_w2[16 * 64];
  __shared__ __align__(16) float s_c[kConsts];
  __shared__ __align__(16) uint16_t s_o[kWaves][kH * kOP];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  fill_frags<kW1A>(s_w1, W1);
  fill_frags<kW2A>(s_w2, W2);
  fill_consts(s_c, means, stds, b1, b2);
  __syncthreads();
  uint16_t* so = s_o[wave];
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + 15) / 16;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += (int64_t)gridDim.x * kWaves) {
    const int64_t bb = row / L;
    const int i = (int)(row - bb * L);
    const int64_t obase = (bb * kH * L + i) * (int64_t)L;
    const uint8_t* padb = pad != nullptr ? pad + bb * L : nullptr;
    const float* ci = coords + row * 3;
    const float ix = ci[0], iy = ci[1], iz = ci[2];
    PairIn nx = load_pair(coords, a, b, padb, row, bb * L, L, r);
    for (int s = 0; s < steps; ++s) {
      const int j0 = s * 16;
      const PairIn cur = nx;
      if (s + 1 < steps)
        nx = load_pair(coords, a, b, padb, row, bb * L, L, j0 + 16 + r);
      float d;
      const float x = pair_x(cur, ix, iy, iz, j0 + r == i, d);
      uint4 gb[4];
      {
        float gf[8][4];
        features(s_c, x, g, gf);
        pack_perm(gf, gb);
      }
      f32x4 acc[8];
      pre_tile(s_w1, s_c, gb, lane, acc);
      uint4 hb[4];
      {
        float hv[8][4];
#pragma unroll
        for (int ot = 0; ot < 8; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) hv[ot][v] = gelu_exact(acc[ot][v]);
        pack_perm(hv, hb);
      }
      wave_sync();  // the previous tile's reads of so are done
#pragma unroll
      for (int ht = 0; ht < 4; ++ht) {
        const float4 bv =
            *reinterpret_cast<const float4*>(s_c + cB2 + ht * 16 + g * 4);
        f32x4 o = f32x4{bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          o = mfma(s_w2[(ht * 4 + ks) * 64 + lane], hb[ks], o);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const uint32_t bits = f32_to_bf16_bits(o[v]);
          so[(ht * 16 + g * 4 + v) * kOP + r] =
              (uint16_t)(cur.dead ? fill : bits);
        }
      }
      wave_sync();
      // 128 chunks of 8 j: head c >> 1, half c & 1
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = lane + 64 * q, h = c >> 1, jj = j0 + (c & 1) * 8;
        if (jj < L)
          *reinterpret_cast<uint4*>(out + obase + (int64_t)h * LL + jj) =
              *reinterpret_cast<const uint4*>(so + h * kOP + (c & 1) * 8);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// What a wave recomputes of its tile, everything at [unit ot*16 + g*4 + v]
// [pair r]: the features, h = gelu(pre) and dpre. x and d of the pair too.
struct Tile {
  float gf[8][4], hv[8][4], dp[8][4];
  float x, d;
};

// The wave's d_out tile: two 16 B chunks per lane (head c >> 1, half c & 1),
// 0 where the key is padded, past the row end or the row is dead; returned in
// ch for the caller and written transposed to sdo[j][head].
__device__ __forceinline__ void stage_dout(const uint16_t* __restrict__ grad,
                                           const uint8_t* __restrict__ padb,
                                           int64_t obase, int64_t LL, int L,
                                           int j0, bool live, int lane,
                                           uint16_t* sdo, uint4 (&ch)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = lane + 64 * q, h = c >> 1, half = c & 1;
    const int jj = j0 + half * 8;
    const bool ok = live && jj < L;
    const int jc = jj < L ? jj : 0;
    const uint4 u =
        *reinterpret_cast<const uint4*>(grad + obase + (int64_t)h * LL + jc);
    uint2 pw = make_uint2(0u, 0u);
    if (padb != nullptr) pw = *reinterpret_cast<const uint2*>(padb + jc);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w}, pwv[2] = {pw.x, pw.y};
    uint32_t e[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const bool keep = ok && ((pwv[t >> 2] >> (8 * (t & 3))) & 0xffu) == 0;
      e[t] = keep ? (w[t >> 1] >> (16 * (t & 1))) & 0xffffu : 0u;
      sdo[(half * 8 + t) * kTP + h] = (uint16_t)e[t];
    }
    ch[q] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16),
                       e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
}

// sdo must hold the wave's masked d_out tile [j][head] (stage_dout, then a
// wave_sync)
__device__ __forceinline__ void recompute_tile(const uint4* s_w1,
                                               const uint4* s_w2t,
                                               const float* s_c,
                                               const uint16_t* sdo,
                                               const PairIn& p, float ix,
                                               float iy, float iz, bool diag,
                                               int lane, Tile& t) {
  const int g = lane >> 4, r = lane & 15;
  t.x = pair_x(p, ix, iy, iz, diag, t.d);
  features(s_c, t.x, g, t.gf);
  uint4 gb[4];
  pack_perm(t.gf, gb);
  f32x4 pre[8];
  pre_tile(s_w1, s_c, gb, lane, pre);
  uint4 dob[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    dob[ks] =
        *reinterpret_cast<const uint4*>(sdo + r * kTP + ks * 32 + g * 8);
#pragma unroll
  for (int ot = 0; ot < 8; ++ot) {
    f32x4 dh = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      dh = mfma(s_w2t[(ot * 2 + ks) * 64 + lane], dob[ks], dh);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float dy;
      gelu_exact_grad(pre[ot][v], t.hv[ot][v], dy);
      t.dp[ot][v] = dh[v] * dy;
    }
  }
}

// sum over the 16 lanes of a g group
__device__ __forceinline__ float sum_r(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(256) pair_gauss_h64_dx_kernel(
    const uint16_t* __restrict__ grad, const float* __restrict__ coords,
    const float* __restrict__ a, const float* __restrict__ b,
    const uint8_t* __restrict__ pad, const float* __restrict__ means,
    const float* __restrict__ stds, const uint16_t* __restrict__ W1,
    const uint16_t* __restrict__ b1, const uint16_t* __restrict__ W2,
    float* __restrict__ d_a, float* __restrict__ d_b,
    float* __restrict__ partials, int64_t n_rows, int L) {
  __shared__ __align__(16) uint4 s_w1[32 * 64];
  __shared__ __align__(16) uint4 s_w1t[32 * 64];
  __shared__ __align__(16) uint4 s_w2t[16 * 64];
  __shared__ __align__(16) float s_c[kConsts];
  __shared__ __align__(16) uint16_t s_do[kWaves][16 * kTP];
  __shared__ __align__(16) float s_dx[kWaves][2][16];
  __shared__ float s_red[kSCols];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  fill_frags<kW1A>(s_w1, W1);
  fill_frags<kW1T>(s_w1t, W1);
  fill_frags<kW2T>(s_w2t, W2);
  fill_consts(s_c, means, stds, b1, nullptr);
  __syncthreads();
  uint16_t* sdo = s_do[wave];
  float dm[8][4], dsd[8][4];
#pragma unroll
  for (int kt = 0; kt < 8; ++kt)
#pragma unroll
    for (int v = 0; v < 4; ++v) dm[kt][v] = dsd[kt][v] = 0.f;
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + 15) / 16;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += (int64_t)gridDim.x * kWaves) {
    const int64_t bb = row / L;
    const int i = (int)(row - bb * L);
    const int64_t obase = (bb * kH * L + i) * (int64_t)L;
    const uint8_t* padb = pad != nullptr ? pad + bb * L : nullptr;
    const float* ci = coords + row * 3;
    const float ix = ci[0], iy = ci[1], iz = ci[2];
    for (int s = 0; s < steps; ++s) {
      const int j0 = s * 16;
      const PairIn p = load_pair(coords, a, b, padb, row, bb * L, L, j0 + r);
      uint4 ch[2];
      wave_sync();  // the previous tile's reads of sdo and s_dx are done
      stage_dout(grad, padb, obase, LL, L, j0, true, lane, sdo, ch);
      wave_sync();
      Tile t;
      recompute_tile(s_w1, s_w2t, s_c, sdo, p, ix, iy, iz, j0 + r == i, lane,
                     t);
      uint4 dpb[4];
      pack_perm(t.dp, dpb);
      float dxs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        f32x4 dg = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          dg = mfma(s_w1t[(kt * 4 + ks) * 64 + lane], dpb[ks], dg);
        const int k0 = kt * 16 + g * 4;
        const float4 m = *reinterpret_cast<const float4*>(s_c + cM + k0);
        const float4 q = *reinterpret_cast<const float4*>(s_c + cIs2 + k0);
        const float4 n = *reinterpret_cast<const float4*>(s_c + cIsg + k0);
        const float mv[4] = {m.x, m.y, m.z, m.w}, qv[4] = {q.x, q.y, q.z, q.w},
                    sv[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float tt = t.x - mv[v];
          const float w = dg[v] * t.gf[kt][v];
          const float u = w * tt * qv[v];
          dxs -= u;
          dm[kt][v] += u;
          dsd[kt][v] += w * (tt * tt * qv[v] - 1.f) * sv[v];
        }
      }
      dxs += __shfl_xor(dxs, 16, 64);
      dxs += __shfl_xor(dxs, 32, 64);
      if (g == 0) s_dx[wave][0][r] = dxs * t.d;
      if (g == 1) s_dx[wave][1][r] = dxs;
      wave_sync();
      if (lane < 8) {
        const int which = lane >> 2, jj = j0 + (lane & 3) * 4;
        if (jj < L)
          *reinterpret_cast<float4*>((which ? d_b : d_a) + row * L + jj) =
              *reinterpret_cast<const float4*>(&s_dx[wave][which][(lane & 3) * 4]);
      }
    }
  }
  // the 16 pairs of a group, then the waves in order
#pragma unroll
  for (int kt = 0; kt < 8; ++kt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      dm[kt][v] = sum_r(dm[kt][v]);
      dsd[kt][v] = sum_r(dsd[kt][v]);
    }
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv && r == 0) {
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* p1 = s_red + kt * 16 + g * 4 + v;
          float* p2 = p1 + kK;
          *p1 = wv == 0 ? dm[kt][v] : *p1 + dm[kt][v];
          *p2 = wv == 0 ? dsd[kt][v] : *p2 + dsd[kt][v];
        }
    }
    __syncthreads();
  }
  partials[(int64_t)blockIdx.x * kSCols + threadIdx.x] = s_red[threadIdx.x];
}

__global__ void __launch_bounds__(256) pair_gauss_h64_wgrad_kernel(
    const uint16_t* __restrict__ grad, const float* __restrict__ coords,
    const float* __restrict__ a, const float* __restrict__ b,
    const uint8_t* __restrict__ pad, const float* __restrict__ means,
    const float* __restrict__ stds, const uint16_t* __restrict__ W1,
    const uint16_t* __restrict__ b1, const uint16_t* __restrict__ W2,
    float* __restrict__ partials, int64_t n_rows, int L) {
  __shared__ __align__(16) uint4 s_w1[32 * 64];
  __shared__ __align__(16) uint4 s_w2t[16 * 64];
  __shared__ __align__(16) float s_c[kConsts];
  __shared__ __align__(16) uint16_t s_do[kWaves][16 * kTP];
  // the block's 64 pairs (wave w: 16 w ..), bf16
  __shared__ __align__(16) uint16_t s_g[kK * kTP];
  __shared__ __align__(16) uint16_t s_h[kK * kTP];
  __shared__ __align__(16) uint16_t s_dp[kK * kTP];
  __shared__ __align__(16) uint16_t s_dot[kH * kTP];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  fill_frags<kW1A>(s_w1, W1);
  fill_frags<kW2T>(s_w2t, W2);
  fill_consts(s_c, means, stds, b1, nullptr);
  __syncthreads();
  uint16_t* sdo = s_do[wave];
  // dW1[o = wave*32 + mt*16 + g*4 + v][k = nt*16 + r], db1 at the same o;
  // dW2[h = wave*16 + g*4 + v][o = nt*16 + r], db2 at the same h
  f32x4 dW1[2][8], dW2[8], db1a[2], db2a;
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    dW1[0][nt] = dW1[1][nt] = dW2[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  db1a[0] = db1a[1] = db2a = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint4 ones =
      make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + 15) / 16;
  // every wave of a block makes the same trips: the barriers are uniform
  for (int64_t row4 = (int64_t)blockIdx.x * kWaves; row4 < n_rows;
       row4 += (int64_t)gridDim.x * kWaves) {
    const bool live = row4 + wave < n_rows;
    const int64_t row = live ? row4 + wave : n_rows - 1;
    const int64_t bb = row / L;
    const int i = (int)(row - bb * L);
    const int64_t obase = (bb * kH * L + i) * (int64_t)L;
    const uint8_t* padb = pad != nullptr ? pad + bb * L : nullptr;
    const float* ci = coords + row * 3;
    const float ix = ci[0], iy = ci[1], iz = ci[2];
    for (int s = 0; s < steps; ++s) {
      const int j0 = s * 16;
      const PairIn p = load_pair(coords, a, b, padb, row, bb * L, L, j0 + r);
      uint4 ch[2];
      wave_sync();
      stage_dout(grad, padb, obase, LL, L, j0, live, lane, sdo, ch);
      wave_sync();
      Tile t;
      recompute_tile(s_w1, s_w2t, s_c, sdo, p, ix, iy, iz, j0 + r == i, lane,
                     t);
      __syncthreads();  // the previous step's products have read the tiles
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = lane + 64 * q;
        *reinterpret_cast<uint4*>(s_dot + (c >> 1) * kTP + wave * 16 +
                                  (c & 1) * 8) = ch[q];
      }
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int at = (kt * 16 + g * 4 + v) * kTP + wave * 16 + r;
          s_g[at] = f32_to_bf16_bits(t.gf[kt][v]);
          s_h[at] = f32_to_bf16_bits(t.hv[kt][v]);
          s_dp[at] = f32_to_bf16_bits(t.dp[kt][v]);
        }
      __syncthreads();
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {  // 32 pairs each
        const int po = kp * 32 + g * 8;
        const uint4 a0 = *reinterpret_cast<const uint4*>(
            s_dp + (wave * 32 + r) * kTP + po);
        const uint4 a1 = *reinterpret_cast<const uint4*>(
            s_dp + (wave * 32 + 16 + r) * kTP + po);
        const uint4 a2 = *reinterpret_cast<const uint4*>(
            s_dot + (wave * 16 + r) * kTP + po);
        db1a[0] = mfma(a0, ones, db1a[0]);
        db1a[1] = mfma(a1, ones, db1a[1]);
        db2a = mfma(a2, ones, db2a);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
          const uint4 bg = *reinterpret_cast<const uint4*>(
              s_g + (nt * 16 + r) * kTP + po);
          const uint4 bh = *reinterpret_cast<const uint4*>(
              s_h + (nt * 16 + r) * kTP + po);
          dW1[0][nt] = mfma(a0, bg, dW1[0][nt]);
          dW1[1][nt] = mfma(a1, bg, dW1[1][nt]);
          dW2[nt] = mfma(a2, bh, dW2[nt]);
        }
      }
    }
  }
  float* prow = partials + (int64_t)blockIdx.x * kWCols;
  float* pW2 = prow + kK * kK + kK;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int o = wave * 32 + mt * 16 + g * 4 + v;
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        prow[o * kK + nt * 16 + r] = dW1[mt][nt][v];
      if (r == 0) prow[kK * kK + o] = db1a[mt][v];
    }
    const int h = wave * 16 + g * 4 + v;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) pW2[h * kK + nt * 16 + r] = dW2[nt][v];
    if (r == 0) pW2[kH * kK + h] = db2a[v];
  }
}

inline int rows_grid(int64_t n_rows, int cap) {
  return unicore_grid((n_rows + kWaves - 1) / kWaves, cap);
}

inline const uint16_t* bits(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}

}  // namespace

int64_t pair_gauss_h64_wgrad_cols() { return kWCols; }

void pair_gauss_h64_forward_launch(at::Tensor& out, const at::Tensor& coords,
                                   const at::Tensor& a, const at::Tensor& b,
                                   const uint8_t* pad, const at::Tensor& means,
                                   const at::Tensor& stds, const at::Tensor& W1,
                                   const at::Tensor& b1, const at::Tensor& W2,
                                   const at::Tensor& b2, float fill) {
  const int64_t L = coords.size(1), n_rows = coords.size(0) * L;
  // fill in bf16, as masked_fill writes it
  const uint32_t fb = at::BFloat16(fill).x;
  auto stream = at::cuda::getCurrentCUDAStream();
  // two blocks per CU by LDS
  pair_gauss_h64_fwd_kernel<<<rows_grid(n_rows, 512), 256, 0, stream>>>(
      coords.data_ptr<float>(), a.data_ptr<float>(), b.data_ptr<float>(), pad,
      means.data_ptr<float>(), stds.data_ptr<float>(), bits(W1), bits(b1),
      bits(W2), bits(b2), reinterpret_cast<uint16_t*>(out.data_ptr()), n_rows,
      (int)L, fb);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair_gauss_h64_backward_launch(at::Tensor& d_a, at::Tensor& d_b,
                                    at::Tensor& stat_fold, at::Tensor& w_fold,
                                    const at::Tensor& grad,
                                    const at::Tensor& coords,
                                    const at::Tensor& a, const at::Tensor& b,
                                    const uint8_t* pad, const at::Tensor& means,
                                    const at::Tensor& stds, const at::Tensor& W1,
                                    const at::Tensor& b1, const at::Tensor& W2) {
  const int64_t L = coords.size(1), n_rows = coords.size(0) * L;
  // one block per CU by LDS; a wgrad partials row is 97 KB, 25 MB in all
  const int P = rows_grid(n_rows, 256);
  auto fopt = d_a.options();
  auto sp = at::empty({(int64_t)P, (int64_t)kSCols}, fopt);
  auto wp = at::empty({(int64_t)P, (int64_t)kWCols}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  pair_gauss_h64_dx_kernel<<<P, 256, 0, stream>>>(
      bits(grad), coords.data_ptr<float>(), a.data_ptr<float>(),
      b.data_ptr<float>(), pad, means.data_ptr<float>(),
      stds.data_ptr<float>(), bits(W1), bits(b1), bits(W2),
      d_a.data_ptr<float>(), d_b.data_ptr<float>(), sp.data_ptr<float>(),
      n_rows, (int)L);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  pair_gauss_h64_wgrad_kernel<<<P, 256, 0, stream>>>(
      bits(grad), coords.data_ptr<float>(), a.data_ptr<float>(),
      b.data_ptr<float>(), pad, means.data_ptr<float>(),
      stds.data_ptr<float>(), bits(W1), bits(b1), bits(W2),
      wp.data_ptr<float>(), n_rows, (int)L);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  unicore_fold_columns(sp.data_ptr<float>(), stat_fold.data_ptr<float>(), P,
                       kSCols, fopt, stream);
  unicore_fold_columns(wp.data_ptr<float>(), w_fold.data_ptr<float>(), P,
                       kWCols, fopt, stream);
}
