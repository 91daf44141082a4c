// Pair distance head at H = 64 (Uni-Mol's DistanceHead) for gfx950, fp32 on
// v_mfma_f32_16x16x4_f32:
//
//   x_ij[h] = pair[b,h,i,j], 0 where i or j is padded
//   g_ij    = gelu(W1 x_ij + b1)                     (64 -> 64, exact erf)
//   f_ij    = w2 . LayerNorm(g_ij; gamma, beta, eps) + b2
//   dist_ij = 0.5 * (f_ij + f_ji), 0 where i or j is padded
//
// The geometry is pair_coord_h64.hip's (pair_h64_blocks.h holds what the two
// share): a wave owns one (b, i) row and walks it in steps of 32 j (2-byte
// dtypes) or 16 j (fp32), four 16 B loads per lane and step, lane -> (plane =
// q*16 + l/4, chunk = l%4), values zeroed by a select at pads and past L,
// staged in a wave-private LDS tile [h][16 j], fragments read as one
// contiguous 256 B line, a wave fence instead of a block barrier, the next
// step's loads issued before this step's products.  Only pair is read, so the
// prefetch is 16 registers, not 32.
//
//   forward  hid^T[o,j] with W1 as A fragments, GELU on the C registers. A
//            lane then holds 16 of the 64 hidden units of its j, so the
//            LayerNorm sums are in-lane over 16 plus two shuffles (16, 32).
//            Two passes over the registers: mean, then squared deviations.
//            gamma and w2 fold into c[o] = gamma[o] w2[o], k0 = beta . w2 +
//            b2:  f = rstd * sum_o c[o] (g[o] - mean) + k0, one 64 B line of
//            the fp32 (B, L, L) buffer F per tile.
//   sym      out = 0.5 (F + F^T), masked: 32 x 32 tiles, the transposed one
//            through LDS at pitch 33 so both reads are whole lines.  f_ji
//            belongs to another wave's row, hence a kernel of its own. The
//            backward starts with the same kernel: dF = 0.5 (dOut + dOut^T).
//   dpair    recomputes hid, GELU and the statistics; with xhat = (g - mean)
//            rstd, df/dg[o] = rstd (c[o] - mean(c) - xhat[o] mean(c xhat));
//            dhid = dF df/dg gelu'(hid) stays in the C registers as the B
//            operand of dx = W1^T dhid (W1^T fragments in LDS, permuted o
//            order), dx leaves through the tile at pitch 20 with 16 B stores.
//   wgrad    pairs on M, so dhid[p,o] in C layout is the A operand of dW1. A
//            pair's 64 units then sit in 16 lanes x 4 registers: statistics
//            are four shuffles (1, 2, 4, 8) per pair. Register sums per unit:
//            db1 and S[o] = sum_p dF_p xhat[p,o]; db2 = sum_p dF_p. The other
//            three gradients are exact functions of those and are formed when
//            the block writes its partials row:
//              dgamma = w2 S, dbeta = w2 db2, dw2 = gamma S + beta db2.
//            Waves summed in order through LDS, one fp32 partials row per
//            block, unicore_fold_columns: no atomics.
#include "pair_dist_h64.h"

#include "dispatch.h"
#include "fold.h"
#include "pair_coord_h64.h"  // gelu_exact, gelu_exact_grad
#include "pair_h64_blocks.h"

#include <ATen/cuda/CUDAContext.h>

namespace {

using namespace pair_h64;

// dW1 (o-major) | db1 | dgamma | dbeta | dw2 | db2
constexpr int kCols = kH * kH + 4 * kH + 1;
constexpr float kInvH = 1.f / kH;

// raw 16 B chunks of step s: plane q*16 + lane/4, chunk lane%4. A chunk past
// the row end reads the row's first chunk instead (valid memory, never used).
template <typename T>
__device__ __forceinline__ void load_step(const T* __restrict__ pair,
                                          const Row& w, int64_t LL, int L,
                                          int s, int lane, uint4 (&ra)[4]) {
  int j0 = chunk_j<T>(s, lane);
  if (j0 >= L) j0 = 0;
  const int64_t off = w.base + (int64_t)(lane >> 2) * LL + j0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    ra[q] = *reinterpret_cast<const uint4*>(pair + off + (int64_t)q * 16 * LL);
}

// x in fp32 -> the wave's tiles, [tile][h][16 j]; 0 where j is padded or past
// the row end. tile_floats is the distance between tiles.
template <typename T>
__device__ __forceinline__ void stage_x(float* sd, int tile_floats,
                                        const uint4 (&ra)[4],
                                        const uint8_t* __restrict__ padb,
                                        int L, int s, int lane) {
  constexpr int E = Step<T>::E;
  const int jo = (lane & 3) * E;
  const int j0 = chunk_j<T>(s, lane);
  const int jc = j0 < L ? j0 : 0;
  bool ok[E];
#pragma unroll
  for (int t = 0; t < E; ++t)
    ok[t] = j0 < L && (padb == nullptr || !padb[jc + t]);
  float* dst = sd + (jo >> 4) * tile_floats + (lane >> 2) * 16 + (jo & 15);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float fa[E];
    unpack<T>(ra[q], fa);
#pragma unroll
    for (int t4 = 0; t4 < E; t4 += 4) {
      float4 d;
      d.x = ok[t4 + 0] ? fa[t4 + 0] : 0.f;
      d.y = ok[t4 + 1] ? fa[t4 + 1] : 0.f;
      d.z = ok[t4 + 2] ? fa[t4 + 2] : 0.f;
      d.w = ok[t4 + 3] ? fa[t4 + 3] : 0.f;
      *reinterpret_cast<float4*>(dst + q * 16 * 16 + t4) = d;
    }
  }
}

// sum over the four g groups: the 64 hidden units of a pair in the [o, j]
// layout
__device__ __forceinline__ float sum_g(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// sum over the 16 lanes of a g group: the 64 units of a pair in [p, o]
__device__ __forceinline__ float sum_r(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// y[ot][v] = g[o = ot*16 + g*4 + v] of this lane's pair: y -= mean, returns
// rstd. Two passes over the registers.
__device__ __forceinline__ float center_oj(float (&y)[4][4], float eps) {
  float s = 0.f;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int v = 0; v < 4; ++v) s += y[ot][v];
  const float mean = sum_g(s) * kInvH;
  float q = 0.f;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      y[ot][v] -= mean;
      q += y[ot][v] * y[ot][v];
    }
  return rsqrtf(sum_g(q) * kInvH + eps);
}

// cv = gamma * w2 on the C-layout rows; returns sum_o of a * w2 over all 64
// units (a = beta gives k0 - b2, a = gamma gives 64 mean(c))
__device__ __forceinline__ float fold_units(const float* __restrict__ gamma,
                                            const float* __restrict__ a,
                                            const float* __restrict__ w2,
                                            int lane, float (&cv)[4][4]) {
  float gm[4][4], av[4][4], wv[4][4];
  load_c_rows(gamma, lane, gm);
  load_c_rows(a, lane, av);
  load_c_rows(w2, lane, wv);
  float s = 0.f;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      cv[ot][v] = gm[ot][v] * wv[ot][v];
      s += av[ot][v] * wv[ot][v];
    }
  return sum_g(s);
}

template <typename T>
PAIR_H64_KERNEL pair_dist_h64_fwd_kernel(
    const T* __restrict__ pair, const uint8_t* __restrict__ pad,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ w2, const float* __restrict__ b2,
    float* __restrict__ F, int64_t n_rows, int L, float eps) {
  using S = Step<T>;
  __shared__ __align__(16) float s_x[kWaves][S::TS * kDTile];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  float* sx = s_x[wave];
  float wf[4][16], b1v[4][4], cv[4][4];
  load_w1_frags(W1, lane, wf);
  load_c_rows(b1, lane, b1v);
  const float k0 = fold_units(gamma, beta, w2, lane, cv) + b2[0];
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + S::JS - 1) / S::JS;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += nwaves) {
    const Row w = make_row(row, L, pad);
    if (!w.live) continue;  // F at a padded i is selected away, never used
    const uint8_t* padb = pad != nullptr ? pad + w.b * L : nullptr;
    uint4 ra[4];
    load_step<T>(pair, w, LL, L, 0, lane, ra);
    for (int s = 0; s < steps; ++s) {
      wave_sync();
      stage_x<T>(sx, kDTile, ra, padb, L, s, lane);
      wave_sync();
      if (s + 1 < steps) load_step<T>(pair, w, LL, L, s + 1, lane, ra);
#pragma unroll 1
      for (int t = 0; t < S::TS; ++t) {
        const int j = s * S::JS + t * 16 + r;
        f32x4 hid[4];
        hidden_oj(sx + t * kDTile, wf, b1v, lane, hid);
        float y[4][4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) y[ot][v] = gelu_exact(hid[ot][v]);
        const float rstd = center_oj(y, eps);
        float a = 0.f;
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) a += cv[ot][v] * y[ot][v];
        const float f = rstd * sum_g(a) + k0;
        if (g == 0 && j < L) F[row * L + j] = f;
      }
    }
  }
}

// out[b,i,j] = 0.5 (in[b,i,j] + in[b,j,i]), 0 where i or j is padded. Block
// = one 32 x 32 output tile, thread (tx, ty) of 32 x 8, four rows each.
__global__ void __launch_bounds__(256) pair_dist_sym_kernel(
    const float* __restrict__ in, const uint8_t* __restrict__ pad,
    float* __restrict__ out, int L, int nt) {
  __shared__ float s_t[32][33];
  const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
  const int64_t blk = blockIdx.x;
  const int tj = (int)(blk % nt), ti = (int)((blk / nt) % nt);
  const int64_t b = blk / ((int64_t)nt * nt);
  const int64_t base = b * L * (int64_t)L;
  const int i0 = ti * 32, j0 = tj * 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = ty + 8 * k;
    const int jj = j0 + rr, ii = i0 + tx;
    s_t[rr][tx] = (jj < L && ii < L) ? in[base + (int64_t)jj * L + ii] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = ty + 8 * k;
    const int i = i0 + rr, j = j0 + tx;
    if (i < L && j < L) {
      const bool ok =
          pad == nullptr || !(pad[b * L + i] || pad[b * L + j]);
      const int64_t at = base + (int64_t)i * L + j;
      const float v = 0.5f * (in[at] + s_t[tx][rr]);
      out[at] = ok ? v : 0.f;
    }
  }
}

template <typename T>
PAIR_H64_KERNEL pair_dist_h64_dpair_kernel(
    const T* __restrict__ pair, const float* __restrict__ dF,
    const uint8_t* __restrict__ pad, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ gamma,
    const float* __restrict__ w2, T* __restrict__ dpair, int64_t n_rows, int L,
    float eps) {
  using S = Step<T>;
  // W1^T as the A fragments of dx = W1^T dhid, K steps in the order the C
  // registers of dhid come: s_wt[(ht*16 + ot*4 + v)*64 + lane] =
  // W1[ot*16 + g*4 + v][ht*16 + r]
  __shared__ __align__(16) float s_wt[kH * kH];
  __shared__ __align__(16) float s_x[kWaves][S::TS * kOTile];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  for (int idx = (int)threadIdx.x; idx < kH * kH; idx += 256) {
    const int ln = idx & 63, f = idx >> 6;
    const int ht = f >> 4, kk = f & 15;
    s_wt[idx] = W1[((kk >> 2) * 16 + (ln >> 4) * 4 + (kk & 3)) * kH + ht * 16 +
                   (ln & 15)];
  }
  __syncthreads();
  float* sx = s_x[wave];
  float wf[4][16], b1v[4][4], cv[4][4];
  load_w1_frags(W1, lane, wf);
  load_c_rows(b1, lane, b1v);
  const float mc = fold_units(gamma, gamma, w2, lane, cv) * kInvH;  // mean(c)
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + S::JS - 1) / S::JS;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += nwaves) {
    const Row w = make_row(row, L, pad);
    if (!w.live) {  // a padded i: the row of exact zeros
      for (int s = 0; s < steps; ++s) {
        const int j0 = chunk_j<T>(s, lane);
        if (j0 < L) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *reinterpret_cast<uint4*>(dpair + w.base +
                                      (int64_t)(q * 16 + (lane >> 2)) * LL +
                                      j0) = make_uint4(0, 0, 0, 0);
        }
      }
      continue;
    }
    const uint8_t* padb = pad != nullptr ? pad + w.b * L : nullptr;
    uint4 ra[4];
    load_step<T>(pair, w, LL, L, 0, lane, ra);
    for (int s = 0; s < steps; ++s) {
      wave_sync();
      stage_x<T>(sx, kOTile, ra, padb, L, s, lane);
      wave_sync();
      if (s + 1 < steps) load_step<T>(pair, w, LL, L, s + 1, lane, ra);
#pragma unroll 1
      for (int t = 0; t < S::TS; ++t) {
        float* tile = sx + t * kOTile;
        const int j = s * S::JS + t * 16 + r;
        const int jc = j < L ? j : 0;
        const bool okj = j < L && (padb == nullptr || !padb[jc]);
        const float dfj = okj ? dF[row * L + jc] : 0.f;
        f32x4 hid[4];
        hidden_oj(tile, wf, b1v, lane, hid);
        float y[4][4], dy[4][4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            gelu_exact_grad(hid[ot][v], y[ot][v], dy[ot][v]);
        const float rstd = center_oj(y, eps);
        float a = 0.f;
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            y[ot][v] *= rstd;  // xhat
            a += cv[ot][v] * y[ot][v];
          }
        const float m2 = sum_g(a) * kInvH;  // mean(c xhat)
        const float sc = dfj * rstd;
        f32x4 dd[4];
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) dd[ht] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float dh =
                sc * (cv[ot][v] - mc - y[ot][v] * m2) * dy[ot][v];
#pragma unroll
            for (int ht = 0; ht < 4; ++ht)
              dd[ht] = mfma4(s_wt[(ht * 16 + ot * 4 + v) * 64 + lane], dh,
                             dd[ht]);
          }
        // every lane's reads of this x tile fed the products above
        wave_sync();
#pragma unroll
        for (int ht = 0; ht < 4; ++ht)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            tile[(ht * 16 + g * 4 + v) * 20 + r] = okj ? dd[ht][v] : 0.f;
      }
      wave_sync();
      const int j0 = chunk_j<T>(s, lane);
      if (j0 < L) {
        const int jo = (lane & 3) * S::E;
        const float* src =
            sx + (jo >> 4) * kOTile + (lane >> 2) * 20 + (jo & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float f[S::E];
#pragma unroll
          for (int t4 = 0; t4 < S::E; t4 += 4) {
            const float4 x =
                *reinterpret_cast<const float4*>(src + q * 16 * 20 + t4);
            f[t4] = x.x; f[t4 + 1] = x.y; f[t4 + 2] = x.z; f[t4 + 3] = x.w;
          }
          *reinterpret_cast<uint4*>(dpair + w.base +
                                    (int64_t)(q * 16 + (lane >> 2)) * LL + j0) =
              pack<T>(f);
        }
      }
    }
  }
}

// two waves per SIMD, as the coordinate head's wgrad kernel is held
template <typename T>
__attribute__((amdgpu_waves_per_eu(2, 2)))
PAIR_H64_KERNEL pair_dist_h64_wgrad_kernel(
    const T* __restrict__ pair, const float* __restrict__ dF,
    const uint8_t* __restrict__ pad, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ w2,
    float* __restrict__ partials, int64_t n_rows, int L, float eps) {
  using S = Step<T>;
  // s_w[(ot*16 + ks)*64 + lane] = W1[ot*16 + r][ks*4 + g], then the wave
  // tiles, then b1 | c | mean(c) in unit order (read at o = ot*16 + r, the
  // fragment order of this layout). The block fold reuses the front.
  constexpr int kTiles = kH * kH + kWaves * S::TS * kDTile;
  constexpr int kSmem = kTiles + 2 * kH + 1;
  constexpr int kFold = kH * kH + 2 * kH + 1;  // dW1 | db1 | S | db2
  static_assert(kTiles >= kFold, "the fold must not reach the constants");
  __shared__ __align__(16) float smem[kSmem];
  float* s_w = smem;
  float* s_b1 = smem + kTiles;
  float* s_c = s_b1 + kH;
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  float* sx = smem + kH * kH + wave * S::TS * kDTile;
  for (int idx = (int)threadIdx.x; idx < kH * kH; idx += 256) {
    const int ln = idx & 63, f = idx >> 6;
    s_w[idx] = W1[((f >> 4) * 16 + (ln & 15)) * kH + (f & 15) * 4 + (ln >> 4)];
  }
  if (threadIdx.x < kH) {
    const float c = gamma[threadIdx.x] * w2[threadIdx.x];
    s_b1[threadIdx.x] = b1[threadIdx.x];
    s_c[threadIdx.x] = c;
    const float m = wave_sum(c) * kInvH;  // threads 0..63 are wave 0
    if (threadIdx.x == 0) s_c[kH] = m;
  }
  __syncthreads();
  const float mc = s_c[kH];
  // dW[ot][ht][v] = dW1[o = ot*16 + g*4 + v][h = ht*16 + r]
  f32x4 dW[4][4];
  float db1a[4], sa[4], db2a = 0.f;  // at o = ot*16 + r
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    db1a[ot] = sa[ot] = 0.f;
#pragma unroll
    for (int ht = 0; ht < 4; ++ht) dW[ot][ht] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + S::JS - 1) / S::JS;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += nwaves) {
    const Row w = make_row(row, L, pad);
    if (!w.live) continue;
    const uint8_t* padb = pad != nullptr ? pad + w.b * L : nullptr;
    for (int s = 0; s < steps; ++s) {
      // no prefetch here, as in the coordinate head: registers
      uint4 ra[4];
      load_step<T>(pair, w, LL, L, s, lane, ra);
      wave_sync();
      stage_x<T>(sx, kDTile, ra, padb, L, s, lane);
      wave_sync();
#pragma unroll 1
      for (int t = 0; t < S::TS; ++t) {
        const float* tile = sx + t * kDTile;
        // this lane's four pairs: j = jg + v (a group of 4 lies wholly inside
        // or outside the row)
        const int jg = s * S::JS + t * 16 + g * 4;
        const int jc = jg < L ? jg : 0;
        const float4 dq =
            *reinterpret_cast<const float4*>(dF + row * L + jc);
        const float dq4[4] = {dq.x, dq.y, dq.z, dq.w};
        // the pad bytes of the four pairs as one aligned word (the host keeps
        // pad 4 B-aligned, L % 8 == 0, jc % 4 == 0): straight-line selects
        uint32_t pw = 0;
        if (padb != nullptr) pw = *reinterpret_cast<const uint32_t*>(padb + jc);
        if (jg >= L) pw = 0xffffffffu;
        float dfv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v)
          dfv[v] = ((pw >> (8 * v)) & 0xffu) == 0 ? dq4[v] : 0.f;
        if (r == 0) db2a += (dfv[0] + dfv[1]) + (dfv[2] + dfv[3]);
        // hid[ot][v] = hid[p = g*4 + v][o = ot*16 + r]
        f32x4 hid[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) {
          const float bv = s_b1[ot * 16 + r];
          hid[ot] = f32x4{bv, bv, bv, bv};
        }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const float av = tile[ks * 64 + lane];
#pragma unroll
          for (int ot = 0; ot < 4; ++ot)
            hid[ot] = mfma4(av, s_w[(ot * 16 + ks) * 64 + lane], hid[ot]);
        }
        float cr[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) cr[ot] = s_c[ot * 16 + r];
        f32x4 dh[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float y[4], dy[4];
#pragma unroll
          for (int ot = 0; ot < 4; ++ot)
            gelu_exact_grad(hid[ot][v], y[ot], dy[ot]);
          const float mean =
              sum_r((y[0] + y[1]) + (y[2] + y[3])) * kInvH;
          float q = 0.f;
#pragma unroll
          for (int ot = 0; ot < 4; ++ot) {
            y[ot] -= mean;
            q += y[ot] * y[ot];
          }
          const float rstd = rsqrtf(sum_r(q) * kInvH + eps);
          float a = 0.f;
#pragma unroll
          for (int ot = 0; ot < 4; ++ot) {
            y[ot] *= rstd;  // xhat
            a += cr[ot] * y[ot];
          }
          const float m2 = sum_r(a) * kInvH;
          const float sc = dfv[v] * rstd;
#pragma unroll
          for (int ot = 0; ot < 4; ++ot) {
            const float d = sc * (cr[ot] - mc - y[ot] * m2) * dy[ot];
            dh[ot][v] = d;
            db1a[ot] += d;
            sa[ot] += dfv[v] * y[ot];
          }
        }
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) {
          const float4 bq = *reinterpret_cast<const float4*>(
              tile + (ht * 16 + r) * 16 + g * 4);
          const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int ot = 0; ot < 4; ++ot)
              dW[ot][ht] = mfma4(dh[ot][v], bv[v], dW[ot][ht]);
        }
      }
    }
  }

  // sums over the four g groups, then the waves in order through LDS
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    db1a[ot] = sum_g(db1a[ot]);
    sa[ot] = sum_g(sa[ot]);
  }
  db2a = wave_sum(db2a);
  float* s_fold = smem;
  __syncthreads();  // every wave is done with s_w and its tiles
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) {
#pragma unroll
        for (int ht = 0; ht < 4; ++ht)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float* p = s_fold + (ot * 16 + g * 4 + v) * kH + ht * 16 + r;
            *p = wv == 0 ? dW[ot][ht][v] : *p + dW[ot][ht][v];
          }
        if (g == 0) {
          float* p1 = s_fold + kH * kH + ot * 16 + r;
          float* p2 = p1 + kH;
          *p1 = wv == 0 ? db1a[ot] : *p1 + db1a[ot];
          *p2 = wv == 0 ? sa[ot] : *p2 + sa[ot];
        }
      }
      if (lane == 0) {
        float* p = s_fold + kFold - 1;
        *p = wv == 0 ? db2a : *p + db2a;
      }
    }
    __syncthreads();
  }
  float* prow = partials + (int64_t)blockIdx.x * kCols;
  for (int c = (int)threadIdx.x; c < kH * kH + kH; c += 256) prow[c] = s_fold[c];
  if (threadIdx.x < kH) {
    const int o = (int)threadIdx.x;
    const float so = s_fold[kH * kH + kH + o], db2 = s_fold[kFold - 1];
    float* pu = prow + kH * kH + kH + o;
    pu[0] = w2[o] * so;                            // dgamma
    pu[kH] = w2[o] * db2;                          // dbeta
    pu[2 * kH] = gamma[o] * so + beta[o] * db2;    // dw2
    if (o == 0) prow[kCols - 1] = db2;
  }
}

}  // namespace

int64_t pair_dist_h64_wgrad_cols() { return kCols; }

void pair_dist_h64_forward_launch(at::Tensor& F, const at::Tensor& pair,
                                  const uint8_t* pad, const at::Tensor& W1,
                                  const at::Tensor& b1, const at::Tensor& gamma,
                                  const at::Tensor& beta, const at::Tensor& w2,
                                  const at::Tensor& b2, float eps) {
  const int64_t L = pair.size(3), n_rows = pair.size(0) * L;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(pair.scalar_type(), "pair_dist_forward", {
    pair_dist_h64_fwd_kernel<scalar_t>
        <<<h64_grid(n_rows, 1024), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(pair.data_ptr()), pad,
            W1.data_ptr<float>(), b1.data_ptr<float>(),
            gamma.data_ptr<float>(), beta.data_ptr<float>(),
            w2.data_ptr<float>(), b2.data_ptr<float>(), F.data_ptr<float>(),
            n_rows, (int)L, eps);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair_dist_sym_launch(at::Tensor& out, const at::Tensor& in,
                          const uint8_t* pad) {
  const int64_t B = in.size(0), L = in.size(1);
  const int64_t nt = (L + 31) / 32;
  auto stream = at::cuda::getCurrentCUDAStream();
  pair_dist_sym_kernel<<<(unsigned)(B * nt * nt), 256, 0, stream>>>(
      in.data_ptr<float>(), pad, out.data_ptr<float>(), (int)L, (int)nt);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair_dist_h64_backward_launch(at::Tensor& dpair, at::Tensor& fold,
                                   const at::Tensor& dF, const at::Tensor& pair,
                                   const uint8_t* pad, const at::Tensor& W1,
                                   const at::Tensor& b1,
                                   const at::Tensor& gamma,
                                   const at::Tensor& beta, const at::Tensor& w2,
                                   float eps) {
  const int64_t L = pair.size(3), n_rows = pair.size(0) * L;
  // about two blocks per CU: each writes a kCols partials row
  const int P = h64_grid(n_rows, 512);
  auto partials = at::empty({(int64_t)P, (int64_t)kCols}, fold.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(pair.scalar_type(), "pair_dist_backward", {
    const scalar_t* p = reinterpret_cast<const scalar_t*>(pair.data_ptr());
    pair_dist_h64_dpair_kernel<scalar_t>
        <<<h64_grid(n_rows, 1024), 256, 0, stream>>>(
            p, dF.data_ptr<float>(), pad, W1.data_ptr<float>(),
            b1.data_ptr<float>(), gamma.data_ptr<float>(),
            w2.data_ptr<float>(),
            reinterpret_cast<scalar_t*>(dpair.data_ptr()), n_rows, (int)L, eps);
    pair_dist_h64_wgrad_kernel<scalar_t><<<P, 256, 0, stream>>>(
        p, dF.data_ptr<float>(), pad, W1.data_ptr<float>(),
        b1.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(),
        w2.data_ptr<float>(), partials.data_ptr<float>(), n_rows, (int)L, eps);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  unicore_fold_columns(partials.data_ptr<float>(), fold.data_ptr<float>(), P,
                       (int)kCols, fold.options(), stream);
}
