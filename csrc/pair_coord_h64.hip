// Equivariant coordinate head at H = 64 (Uni-Mol's 64 heads) for gfx950: the
// definition of pair_coord.hip with the 64 x 64 hidden layer on the fp32
// matrix instruction v_mfma_f32_16x16x4_f32.  All arithmetic is fp32.
//
// Fragment map of the instruction (mfma_probe.hip checks it), lane l,
// g = l >> 4, r = l & 15:
//   A (16x4):  A[m = r][k = g]         B (4x16): B[k = g][n = r]
//   C (16x16): C[m = g*4 + v][n = r],  v = 0..3
//
// Work split. A wave owns one (b, i) row and walks it in steps of JS = 32 j
// (2-byte dtypes) or 16 j (fp32), so a step reads 64 contiguous bytes of each
// of the 64 head planes of pair and pair0: four 16 B loads per lane and
// tensor, lane -> (plane = q*16 + l/4, chunk = l%4).  The next step's loads
// are issued before the current step's products.  d = pair - pair0 is formed
// in fp32, zeroed by a select where j is padded or past L, and staged in a
// wave-private LDS tile [h][16 j] per 16 j: the fragment of K step ks is
// tile[ks*64 + l], one contiguous 256 B read with no bank conflict.  Waves
// never share a tile, LDS operations of a wave complete in order, so a wave
// fence orders stage and use and no block barrier sits in any loop.
//
//   forward  hid^T[o,j] = b1[o] + sum_h W1[o,h] d[h,j]: W1 as A fragments in
//            64 VGPRs, 64 products per tile, GELU on the C registers,
//            w_j = sum_o W2[o] g[o,j] in-lane then over g by two shuffles;
//            lane group g < 3 accumulates component g of (x_j - x_i) w_j and a
//            16-lane shuffle tree ends the row: three 4 B stores.
//   dpair    the same hid^T; dhid[o,j] = dw_j W2[o] gelu'(hid) stays in the C
//            registers and is the B operand of dd[h,j] = sum_o W1[o,h]
//            dhid[o,j] as it stands: K step (ot, v) carries o = ot*16 + g*4 + v
//            on k = g, and the W1^T fragments (LDS, fragment order) are laid
//            out with that permutation. dd leaves through the tile (pitch 20:
//            the four g groups of a C-layout write land in four bank
//            quarters) and is stored with the load's 16 B chunk map.
//   wgrad    hid[p,o] with the pairs on M: the same two fragments, operands
//            swapped. dhid[p,o] is then already the A operand of dW1[o,h] =
//            sum_p dhid[p,o] d[h,p] (K step v carries p = g*4 + v on k = g),
//            and its B operand d[h = ht*16 + r][p = g*4 ..+4] is one 16 B LDS
//            read of the same tile, 1 KB contiguous per wave. Nothing is
//            transposed through LDS. dW1 is 64 accumulator VGPRs, W1 comes
//            from LDS; db1/dW2/db2 are register sums. The four waves of a
//            block are summed in order through LDS, a block writes one fp32
//            partials row, unicore_fold_columns folds them: no atomics.
// Two backward kernels, not one: dW1 (64) + W1 and W1^T fragments + two sets
// of accumulators + the prefetch do not fit 256 VGPRs, and all fragments in
// LDS would leave one wave per SIMD.
#include "pair_coord_h64.h"

#include "common.h"
#include "dispatch.h"
#include "fold.h"
#include "pair_h64_blocks.h"

#include <ATen/cuda/CUDAContext.h>

namespace {

// Step, mfma4, wave_sync, unpack / pack, Row, the chunk map and the W1
// fragments are pair_h64_blocks.h's, shared with pair_dist_h64.hip
using namespace pair_h64;

constexpr int kCols = kH * kH + 2 * kH + 1;

#define PC64_KERNEL PAIR_H64_KERNEL

// raw 16 B chunks of step s: plane q*16 + lane/4, chunk lane%4. A chunk past
// the row end reads the row's first chunk instead (valid memory, never used).
template <typename T>
__device__ __forceinline__ void load_step(const T* __restrict__ pair,
                                          const T* __restrict__ pair0,
                                          const Row& w, int64_t LL, int L,
                                          int s, int lane, uint4 (&ra)[4],
                                          uint4 (&rb)[4]) {
  int j0 = chunk_j<T>(s, lane);
  if (j0 >= L) j0 = 0;
  const int64_t off = w.base + (int64_t)(lane >> 2) * LL + j0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ra[q] = *reinterpret_cast<const uint4*>(pair + off + (int64_t)q * 16 * LL);
    rb[q] = *reinterpret_cast<const uint4*>(pair0 + off + (int64_t)q * 16 * LL);
  }
}

// d = pair - pair0 in fp32 -> the wave's tiles, [tile][h][16 j]; 0 where j is
// padded or past the row end. tile_floats is the distance between tiles.
template <typename T>
__device__ __forceinline__ void stage_d(float* sd, int tile_floats,
                                        const uint4 (&ra)[4],
                                        const uint4 (&rb)[4],
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
    float fa[E], fb[E];
    unpack<T>(ra[q], fa);
    unpack<T>(rb[q], fb);
#pragma unroll
    for (int t4 = 0; t4 < E; t4 += 4) {
      float4 d;
      d.x = ok[t4 + 0] ? fa[t4 + 0] - fb[t4 + 0] : 0.f;
      d.y = ok[t4 + 1] ? fa[t4 + 1] - fb[t4 + 1] : 0.f;
      d.z = ok[t4 + 2] ? fa[t4 + 2] - fb[t4 + 2] : 0.f;
      d.w = ok[t4 + 3] ? fa[t4 + 3] - fb[t4 + 3] : 0.f;
      *reinterpret_cast<float4*>(dst + q * 16 * 16 + t4) = d;
    }
  }
}

template <typename T>
PC64_KERNEL pair_coord_h64_fwd_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ inv_n,
    const uint8_t* __restrict__ pad, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, float* __restrict__ out, int64_t n_rows,
    int L) {
  using S = Step<T>;
  __shared__ __align__(16) float s_d[kWaves][S::TS * kDTile];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  float* sd = s_d[wave];
  float wf[4][16], b1v[4][4], w2v[4][4];
  load_w1_frags(W1, lane, wf);
  load_c_rows(b1, lane, b1v);
  load_c_rows(W2, lane, w2v);
  const float b2v = b2[0];
  const int64_t LL = (int64_t)L * L;
  const int steps = (L + S::JS - 1) / S::JS;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < n_rows;
       row += nwaves) {
    const Row w = make_row(row, L, pad);
    float acc = 0.f;  // component g of the row's sum, this lane's j
    if (w.live) {
      const uint8_t* padb = pad != nullptr ? pad + w.b * L : nullptr;
      const float xi = g < 3 ? coords[row * 3 + g] : 0.f;
      uint4 ra[4], rb[4];
      load_step<T>(pair, pair0, w, LL, L, 0, lane, ra, rb);
      for (int s = 0; s < steps; ++s) {
        wave_sync();
        stage_d<T>(sd, kDTile, ra, rb, padb, L, s, lane);
        wave_sync();
        if (s + 1 < steps) load_step<T>(pair, pair0, w, LL, L, s + 1, lane, ra, rb);
#pragma unroll 1
        for (int t = 0; t < S::TS; ++t) {
          const int j = s * S::JS + t * 16 + r;
          const int jc = j < L ? j : 0;
          const bool okj = j < L && (padb == nullptr || !padb[jc]);
          const float xj = g < 3 ? coords[(w.b * L + jc) * 3 + g] : 0.f;
          f32x4 hid[4];
          hidden_oj(sd + t * kDTile, wf, b1v, lane, hid);
          float wj = 0.f;
#pragma unroll
          for (int ot = 0; ot < 4; ++ot)
#pragma unroll
            for (int v = 0; v < 4; ++v)
              wj += w2v[ot][v] * gelu_exact(hid[ot][v]);
          wj += __shfl_xor(wj, 16, 64);
          wj += __shfl_xor(wj, 32, 64);
          wj += b2v;
          acc += (xj - xi) * (okj ? wj : 0.f);
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (r == 0 && g < 3) out[row * 3 + g] = w.live ? inv_n[w.b] * acc : 0.f;
  }
}

template <typename T>
PC64_KERNEL pair_coord_h64_dpair_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ grad,
    const float* __restrict__ inv_n, const uint8_t* __restrict__ pad,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, T* __restrict__ dpair, int64_t n_rows,
    int L) {
  using S = Step<T>;
  // W1^T as the A fragments of dd = W1^T dhid, K steps in the order the C
  // registers of dhid come: s_wt[(ht*16 + ot*4 + v)*64 + lane] =
  // W1[ot*16 + g*4 + v][ht*16 + r]
  __shared__ __align__(16) float s_wt[kH * kH];
  __shared__ __align__(16) float s_d[kWaves][S::TS * kOTile];
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
  float* sd = s_d[wave];
  float wf[4][16], b1v[4][4], w2v[4][4];
  load_w1_frags(W1, lane, wf);
  load_c_rows(b1, lane, b1v);
  load_c_rows(W2, lane, w2v);
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
    const float sc = inv_n[w.b];
    const float xi = coords[row * 3 + 0], yi = coords[row * 3 + 1],
                zi = coords[row * 3 + 2];
    const float gx = sc * grad[row * 3 + 0], gy = sc * grad[row * 3 + 1],
                gz = sc * grad[row * 3 + 2];
    uint4 ra[4], rb[4];
    load_step<T>(pair, pair0, w, LL, L, 0, lane, ra, rb);
    for (int s = 0; s < steps; ++s) {
      wave_sync();
      stage_d<T>(sd, kOTile, ra, rb, padb, L, s, lane);
      wave_sync();
      if (s + 1 < steps) load_step<T>(pair, pair0, w, LL, L, s + 1, lane, ra, rb);
#pragma unroll 1
      for (int t = 0; t < S::TS; ++t) {
        float* tile = sd + t * kOTile;
        const int j = s * S::JS + t * 16 + r;
        const int jc = j < L ? j : 0;
        const bool okj = j < L && (padb == nullptr || !padb[jc]);
        const float* cj = coords + (w.b * L + jc) * 3;
        const float dwj =
            okj ? gx * (cj[0] - xi) + gy * (cj[1] - yi) + gz * (cj[2] - zi)
                : 0.f;
        f32x4 hid[4];
        hidden_oj(tile, wf, b1v, lane, hid);
        f32x4 dd[4];
#pragma unroll
        for (int ht = 0; ht < 4; ++ht) dd[ht] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float y, dy;
            gelu_exact_grad(hid[ot][v], y, dy);
            const float dh = dwj * w2v[ot][v] * dy;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht)
              dd[ht] = mfma4(s_wt[(ht * 16 + ot * 4 + v) * 64 + lane], dh,
                             dd[ht]);
          }
        // every lane's reads of this d tile fed the products above
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
            sd + (jo >> 4) * kOTile + (lane >> 2) * 20 + (jo & 15);
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

// two waves per SIMD: left alone the scheduler spends 256 + 64 registers
template <typename T>
__attribute__((amdgpu_waves_per_eu(2, 2)))
PC64_KERNEL pair_coord_h64_wgrad_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ grad,
    const float* __restrict__ inv_n, const uint8_t* __restrict__ pad,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, float* __restrict__ partials, int64_t n_rows,
    int L) {
  using S = Step<T>;
  // s_w[(ot*16 + ks)*64 + lane] = W1[ot*16 + r][ks*4 + g], then the wave
  // tiles; the block fold reuses the front of it
  constexpr int kSmem = kH * kH + kWaves * S::TS * kDTile;
  static_assert(kSmem >= kCols, "the fold needs kCols floats");
  __shared__ __align__(16) float smem[kSmem];
  float* s_w = smem;
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  float* sd = smem + kH * kH + wave * S::TS * kDTile;
  for (int idx = (int)threadIdx.x; idx < kH * kH; idx += 256) {
    const int ln = idx & 63, f = idx >> 6;
    s_w[idx] = W1[((f >> 4) * 16 + (ln & 15)) * kH + (f & 15) * 4 + (ln >> 4)];
  }
  __syncthreads();
  float b1r[4], w2r[4];  // at o = ot*16 + r
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    b1r[ot] = b1[ot * 16 + r];
    w2r[ot] = W2[ot * 16 + r];
  }
  // dW[ot][ht][v] = dW1[o = ot*16 + g*4 + v][h = ht*16 + r]
  f32x4 dW[4][4];
  float db1a[4], dw2a[4], db2a = 0.f;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    db1a[ot] = dw2a[ot] = 0.f;
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
    const float sc = inv_n[w.b];
    const float xi = coords[row * 3 + 0], yi = coords[row * 3 + 1],
                zi = coords[row * 3 + 2];
    const float gx = sc * grad[row * 3 + 0], gy = sc * grad[row * 3 + 1],
                gz = sc * grad[row * 3 + 2];
    for (int s = 0; s < steps; ++s) {
      // no prefetch here: 32 more live registers spill under the two-wave cap
      uint4 ra[4], rb[4];
      load_step<T>(pair, pair0, w, LL, L, s, lane, ra, rb);
      wave_sync();
      stage_d<T>(sd, kDTile, ra, rb, padb, L, s, lane);
      wave_sync();
#pragma unroll 1
      for (int t = 0; t < S::TS; ++t) {
        const float* tile = sd + t * kDTile;
        // this lane's four pairs: j = jg + v (a group of 4 lies wholly inside
        // or outside the row)
        const int jg = s * S::JS + t * 16 + g * 4;
        const int jc = jg < L ? jg : 0;
        float dwv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const bool ok = jg < L && (padb == nullptr || !padb[jc + v]);
          const float* cj = coords + (w.b * L + jc + v) * 3;
          dwv[v] = ok ? gx * (cj[0] - xi) + gy * (cj[1] - yi) + gz * (cj[2] - zi)
                      : 0.f;
        }
        if (r == 0) db2a += (dwv[0] + dwv[1]) + (dwv[2] + dwv[3]);
        // hid[ot][v] = hid[p = g*4 + v][o = ot*16 + r]
        f32x4 hid[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
          hid[ot] = f32x4{b1r[ot], b1r[ot], b1r[ot], b1r[ot]};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const float av = tile[ks * 64 + lane];
#pragma unroll
          for (int ot = 0; ot < 4; ++ot)
            hid[ot] = mfma4(av, s_w[(ot * 16 + ks) * 64 + lane], hid[ot]);
        }
        f32x4 dh[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float y, dy;
            gelu_exact_grad(hid[ot][v], y, dy);
            dh[ot][v] = dwv[v] * w2r[ot] * dy;
            db1a[ot] += dh[ot][v];
            dw2a[ot] += dwv[v] * y;
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
    db1a[ot] += __shfl_xor(db1a[ot], 16, 64);
    db1a[ot] += __shfl_xor(db1a[ot], 32, 64);
    dw2a[ot] += __shfl_xor(dw2a[ot], 16, 64);
    dw2a[ot] += __shfl_xor(dw2a[ot], 32, 64);
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
          *p2 = wv == 0 ? dw2a[ot] : *p2 + dw2a[ot];
        }
      }
      if (lane == 0) {
        float* p = s_fold + kCols - 1;
        *p = wv == 0 ? db2a : *p + db2a;
      }
    }
    __syncthreads();
  }
  for (int c = (int)threadIdx.x; c < kCols; c += 256)
    partials[(int64_t)blockIdx.x * kCols + c] = s_fold[c];
}

}  // namespace

void pair_coord_h64_forward_launch(at::Tensor& out, const at::Tensor& pair,
                                   const at::Tensor& pair0,
                                   const at::Tensor& coords,
                                   const at::Tensor& inv_n, const uint8_t* pad,
                                   const at::Tensor& W1, const at::Tensor& b1,
                                   const at::Tensor& W2, const at::Tensor& b2) {
  const int64_t L = pair.size(3), n_rows = pair.size(0) * L;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(pair.scalar_type(), "pair_coord_forward", {
    pair_coord_h64_fwd_kernel<scalar_t>
        <<<h64_grid(n_rows, 1024), 256, 0, stream>>>(
            reinterpret_cast<const scalar_t*>(pair.data_ptr()),
            reinterpret_cast<const scalar_t*>(pair0.data_ptr()),
            coords.data_ptr<float>(), inv_n.data_ptr<float>(), pad,
            W1.data_ptr<float>(), b1.data_ptr<float>(), W2.data_ptr<float>(),
            b2.data_ptr<float>(), out.data_ptr<float>(), n_rows, (int)L);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair_coord_h64_backward_launch(at::Tensor& dpair, at::Tensor& fold,
                                    const at::Tensor& grad,
                                    const at::Tensor& pair,
                                    const at::Tensor& pair0,
                                    const at::Tensor& coords,
                                    const at::Tensor& inv_n, const uint8_t* pad,
                                    const at::Tensor& W1, const at::Tensor& b1,
                                    const at::Tensor& W2) {
  const int64_t L = pair.size(3), n_rows = pair.size(0) * L;
  // about two blocks per CU: each writes a kCols partials row
  const int P = h64_grid(n_rows, 512);
  auto partials = at::empty({(int64_t)P, (int64_t)kCols}, fold.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(pair.scalar_type(), "pair_coord_backward", {
    const scalar_t* p = reinterpret_cast<const scalar_t*>(pair.data_ptr());
    const scalar_t* p0 = reinterpret_cast<const scalar_t*>(pair0.data_ptr());
    pair_coord_h64_dpair_kernel<scalar_t>
        <<<h64_grid(n_rows, 1024), 256, 0, stream>>>(
            p, p0, coords.data_ptr<float>(), grad.data_ptr<float>(),
            inv_n.data_ptr<float>(), pad, W1.data_ptr<float>(),
            b1.data_ptr<float>(), W2.data_ptr<float>(),
            reinterpret_cast<scalar_t*>(dpair.data_ptr()), n_rows, (int)L);
    pair_coord_h64_wgrad_kernel<scalar_t><<<P, 256, 0, stream>>>(
        p, p0, coords.data_ptr<float>(), grad.data_ptr<float>(),
        inv_n.data_ptr<float>(), pad, W1.data_ptr<float>(),
        b1.data_ptr<float>(), W2.data_ptr<float>(),
        partials.data_ptr<float>(), n_rows, (int)L);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  unicore_fold_columns(partials.data_ptr<float>(), fold.data_ptr<float>(), P,
                       (int)kCols, fold.options(), stream);
}
