// Outer-product-mean contractions for gfx950 (CDNA4 MFMA), bf16, width 32.
//
//   opm_forward   : o[b,i,j,c,d] = scale * sum_s     a[b,s,i,c]     * b[b,s,j,d]
//   opm_backward_a: da[b,s,i,c]  = scale * sum_{j,d} d_o[b,i,j,c,d] * b[b,s,j,d]
//   opm_backward_b: db[b,s,j,d]  = scale * sum_{i,c} d_o[b,i,j,c,d] * a[b,s,i,c]
//
// a is (B, S, I, 32), b is (B, S, J, 32), o / d_o are (B, I, J, 32, 32), all
// contiguous.  bf16 in, fp32 accumulation, scale applied in fp32, one
// rounding to bf16 per output element.  Results are written in the stored
// layout: o.view(B, I, J, 1024) feeds the output projection with no copy,
// no operand or result is permuted and no fp32 tensor of activation size
// exists.  The library route is an fp32 GEMM that lands in (i, c, j, d)
// followed by a permute copy, a division pass and a cast pass.
//
// All kernels: 256 threads (4 wave64), v_mfma_f32_16x16x32_bf16 with the
// fragment maps verified by csrc/mfma_probe.hip (see csrc/triangle.hip):
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
// LDS operand images are arrays of 16 B slots, one slot = 8 consecutive k of
// one row, so a lane's fragment is one ds_read_b128.  A fragment read takes
// 16 consecutive slots (one 256 B bank row): conflict-free.  Slot indices are
// XORed with bits 3..5 of themselves (opm_sw), a permutation inside every
// aligned group of 8 slots, so the staging writes of neighbouring lanes
// (8 slots apart) spread over the banks while reads keep their 16 distinct
// slots.
//
// Forward.  GEMM with M = (i, c), N = (j, d), K = s; s is the outermost
// dimension of both operands, so both need a k-major transposition.  A block
// owns OT x OT = 4 x 4 (i, j) pairs (a 128 x 128 tile; each wave 64 x 64 =
// 64 accumulator VGPRs) and walks s in steps of 64.  Staging: a thread loads
// 8 consecutive s of 8 consecutive (row, channel) elements as eight 16 B
// loads, transposes the 8 x 8 block in registers and writes eight slots;
// threads 0..127 stage a, 128..255 stage b.  The next step's loads are
// issued before the MFMA phase.  The b fragment is passed as the MFMA A
// operand so that a lane's four accumulator rows are four consecutive d.
// Epilogue through LDS as [pair][c][32 d + 8 pad] bf16 (8 B writes), then
// 16 B stores; every (i, j) result is 2 KB contiguous in global memory.
//
// Backward (one template for both).  For a fixed p (i for da, j for db) the
// result (S, 32) is a GEMM with M = 32 (c or d), N = s, K = (q, 32) where q
// runs over the other pair index.  A block owns one p and 128 s (wave w the
// s range [32 w, 32 w + 32): 2 x 2 MFMA tiles) and walks q in steps of 16.
// The 32 x 32 (c, d) tiles of d_o go through LDS: as they are for da (k = d
// is contiguous), transposed in registers for db (k = c has stride 32).  The
// other operand (b[s, q, :] or a[s, q, :]) is k-contiguous in 64 B runs and
// each wave owns its s range, so its fragments are plain 16 B global loads.
// Epilogue through LDS as [s][32 + 8 pad], then 16 B stores.
//
// Out-of-range s, rows and q are zero-filled (loads use a clamped in-range
// address and the value is replaced by zero); out-of-range outputs are
// predicated at the store.  Every output element is accumulated inside one
// wave in a fixed order: no atomics, no split-K, bitwise reproducible.
// Every offset product is int64_t.
//
// Weighted entries (opm_forward_w / opm_backward_a_w / opm_backward_b_w): a
// contiguous fp32 w[b,i,j] takes the place of scale, for padded batches where
// the mean's normaliser differs per pair.  They are the WT = true
// instantiations of the same kernels; WT = false is the code as it was.
// Forward multiplies by w in the epilogue (fp32, one rounding).  In backward
// w varies along K, so each d_o tile is multiplied on its way into LDS and
// rounded to bf16 once more: a relative 2^-8 per product on top of the
// unweighted error.  Same fixed accumulation order, same reproducibility.
#include "common.h"

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int W = 32;                     // c = d = 32, the only width
constexpr int WW = W * W;                 // elements of one (i, j) result
constexpr int OT = 4;                     // forward: (i, j) pairs per block side
constexpr int FT = OT * W;                // forward tile edge (128)
constexpr int FKS = 64;                   // forward: s per step
constexpr int F_SLOTS = (FKS / 8) * FT;   // 16 B slots per forward operand image
constexpr int OPITCH = W + 8;             // epilogue row pitch in bf16 (80 B)
constexpr int F_SMEM = OT * OT * W * OPITCH * 2 / 16;  // uint4, 40 KB
constexpr int BQ = 16;                    // backward: q per step
constexpr int BS = 128;                   // backward: s per block
constexpr int B_SLOTS = BQ * 4 * W;       // 2048 slots, 32 KB

static_assert(2 * F_SLOTS <= F_SMEM, "forward operand images fit the epilogue buffer");
static_assert(BS * OPITCH * 2 <= B_SLOTS * 16, "backward epilogue fits the image");

__device__ __forceinline__ int opm_sw(int slot) { return slot ^ ((slot >> 3) & 7); }

__device__ __forceinline__ uint4 opm_ld(const uint16_t* p, bool ok) {
  // p is always in range; the select keeps the load unconditional
  uint4 v = *reinterpret_cast<const uint4*>(p);
  if (!ok) v = make_uint4(0u, 0u, 0u, 0u);
  return v;
}

__device__ __forceinline__ bf16x8 opm_frag(uint4 u) {
  union {
    uint4 u;
    bf16x8 v;
  } U;
  U.u = u;
  return U.v;
}

// r[j] = 8 elements (minor index e) of row j  ->  t[e] = rows 0..7 of element e
__device__ __forceinline__ void opm_transpose8(const uint4 (&r)[8], uint4 (&t)[8]) {
  uint32_t in[8][4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    in[j][0] = r[j].x;
    in[j][1] = r[j].y;
    in[j][2] = r[j].z;
    in[j][3] = r[j].w;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t e = in[2 * p][w], o = in[2 * p + 1][w];
      lo[p] = (e & 0xFFFFu) | (o << 16);
      hi[p] = (e >> 16) | (o & 0xFFFF0000u);
    }
    t[2 * w] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    t[2 * w + 1] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  }
}

__device__ __forceinline__ uint2 opm_pack4(const f32x4& v, float scale) {
  uint2 o;
  o.x = (uint32_t)f32_to_bf16_bits(v[0] * scale) |
        ((uint32_t)f32_to_bf16_bits(v[1] * scale) << 16);
  o.y = (uint32_t)f32_to_bf16_bits(v[2] * scale) |
        ((uint32_t)f32_to_bf16_bits(v[3] * scale) << 16);
  return o;
}

// 8 bf16 -> fp32, times w, rounded back to bf16 (weighted backward staging)
__device__ __forceinline__ uint4 opm_scale8(uint4 v, float w) {
  uint32_t in[4] = {v.x, v.y, v.z, v.w}, o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = (uint32_t)f32_to_bf16_bits(bf16_bits_to_f32((uint16_t)(in[k] & 0xFFFFu)) * w) |
           ((uint32_t)f32_to_bf16_bits(bf16_bits_to_f32((uint16_t)(in[k] >> 16)) * w) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// WT: the result is multiplied by Wt[b, i, j] (fp32, (B, I, J)) instead of
// by scale.  An accumulator fragment lies in one (i, j) pair, so that is one
// scalar per fragment.
template <bool WT>
__global__ __launch_bounds__(256) void opm_fwd_kernel(
    uint16_t* __restrict__ O, const uint16_t* __restrict__ A,
    const uint16_t* __restrict__ Bm, int S, int I, int J, int nit, int njt,
    float scale, const float* __restrict__ Wt) {
  __shared__ uint4 smem[F_SMEM];
  uint4* sA = smem;
  uint4* sB = smem + F_SLOTS;

  int bid = blockIdx.x;
  const int j0 = (bid % njt) * OT;
  bid /= njt;
  const int i0 = (bid % nit) * OT;
  const int64_t bt = bid / nit;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lr = lane & 15;
  const int lg = lane >> 4;

  // staging role: operand (wave-uniform), s group of 8, 8-element column group
  const bool st_b = tid >= 128;
  const int st_mg = tid & 15;
  const int st_g = (tid >> 4) & 7;
  const int R = st_b ? J : I;
  const int row = (st_b ? j0 : i0) + (st_mg >> 2);
  const bool row_ok = row < R;
  const int64_t s_stride = (int64_t)R * W;
  const uint16_t* src = (st_b ? Bm : A) + bt * S * s_stride +
                        (int64_t)min(row, R - 1) * W + (st_mg & 3) * 8;
  uint4* sdst = st_b ? sB : sA;

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int s = st_g * 8 + j;
    r[j] = opm_ld(src + (int64_t)min(s, S - 1) * s_stride, row_ok && s < S);
  }

  const int wr = wave >> 1, wc = wave & 1;
  for (int s0 = 0; s0 < S; s0 += FKS) {
    __syncthreads();  // previous step's fragment reads are done
    {
      uint4 t[8];
      opm_transpose8(r, t);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        sdst[opm_sw(st_g * FT + st_mg * 8 + e)] = t[e];
    }
    __syncthreads();
    if (s0 + FKS < S) {  // next step's loads fly across the MFMA phase
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int s = s0 + FKS + st_g * 8 + j;
        r[j] = opm_ld(src + (int64_t)min(s, S - 1) * s_stride, row_ok && s < S);
      }
    }
#pragma unroll
    for (int kk = 0; kk < FKS / 32; ++kk) {
      const int kbase = (kk * 4 + lg) * FT;
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        af[m] = opm_frag(sA[opm_sw(kbase + wr * 64 + m * 16 + lr)]);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        bfr[n] = opm_frag(sB[opm_sw(kbase + wc * 64 + n * 16 + lr)]);
      // b as the MFMA A operand: result rows are d, columns are c
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[n], af[m],
                                                              acc[m][n], 0, 0, 0);
    }
  }

  // epilogue: fragments -> LDS [pair][c][d + pad] -> 16 B stores along d
  __syncthreads();
  uint16_t* sO = reinterpret_cast<uint16_t*>(smem);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int pi = wr * 2 + (m >> 1), pj = wc * 2 + (n >> 1);
      const int c = (m & 1) * 16 + lr;
      const int d = (n & 1) * 16 + lg * 4;
      float sc = scale;
      if (WT)  // clamped: the pairs past I or J are dropped at the store
        sc = Wt[(bt * I + min(i0 + pi, I - 1)) * J + min(j0 + pj, J - 1)];
      *reinterpret_cast<uint2*>(sO + ((pi * OT + pj) * W + c) * OPITCH + d) =
          opm_pack4(acc[m][n], sc);
    }
  __syncthreads();
  uint16_t* po = O + bt * ((int64_t)I * J * WW);
#pragma unroll
  for (int t = 0; t < OT * OT * W * 4 / 256; ++t) {
    const int ch = tid + 256 * t;
    const int pair = ch >> 7;
    const int c = (ch >> 2) & 31;
    const int g = ch & 3;
    const int i = i0 + (pair >> 2), j = j0 + (pair & 3);
    if (i < I && j < J) {
      const uint4 v = *reinterpret_cast<const uint4*>(
          sO + (pair * W + c) * OPITCH + g * 8);
      *reinterpret_cast<uint4*>(po + ((int64_t)i * J + j) * WW + c * W + g * 8) = v;
    }
  }
}

// ---------------------------------------------------------------------------
// backward: out[b, s, p, m] = scale * sum_{q, k} T(p, q)[m, k] * X[b, s, q, k]
// T(p, q) is the (c, d) tile of d_o at tile_p * p + tile_q * q; TR = false
// takes it as [m = c][k = d] (da), TR = true as [m = d][k = c] (db).
// WT: the weight Wt[b, i, j] (fp32, (B, I, J), addressed with the tile
// strides / 1024) depends on (p, q), so it sits inside the K loop: every
// d_o tile is multiplied by its weight on the way into LDS (bf16 -> fp32,
// times w, one rounding back to bf16) and scale is 1.  The weight is loaded
// with the tile, from the same clamped q; no weighted copy of d_o exists.
// ---------------------------------------------------------------------------
template <bool TR, bool WT>
__global__ __launch_bounds__(256) void opm_bwd_kernel(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ dO,
    const uint16_t* __restrict__ X, int S, int P, int Q, int64_t tile_p,
    int64_t tile_q, int nsc, float scale, const float* __restrict__ Wt) {
  __shared__ uint4 smem[B_SLOTS];

  int bid = blockIdx.x;
  const int s0 = (bid % nsc) * BS;
  bid /= nsc;
  const int p = bid % P;
  const int64_t bt = bid / P;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lr = lane & 15;
  const int lg = lane >> 4;

  const uint16_t* tiles = dO + bt * ((int64_t)P * Q * WW) + (int64_t)p * tile_p;
  // TR staging role: (q in step, 8-row group of c, 8-column group of d)
  const int tq = tid >> 4, tcg = (tid >> 2) & 3, tdg = tid & 3;

  // weights of this p: one per q, at the tile strides in units of tiles
  const float* wrow = nullptr;
  int64_t w_q = 0;
  if (WT) {
    wrow = Wt + bt * ((int64_t)P * Q) + (int64_t)p * (tile_p / WW);
    w_q = tile_q / WW;
  }

  uint4 r[8];
  float wv[TR ? 1 : 8];  // WT: the weight of r[j]'s tile (one q for all if TR)
  auto load_tiles = [&](int q0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (TR) {
        const int q = q0 + tq;
        r[j] = opm_ld(tiles + (int64_t)min(q, Q - 1) * tile_q +
                          (tcg * 8 + j) * W + tdg * 8,
                      q < Q);
        if (WT && j == 0) wv[0] = wrow[(int64_t)min(q, Q - 1) * w_q];
      } else {
        const int ch = j * 256 + tid;  // 16 B chunk of the step's 16 tiles
        const int q = q0 + (ch >> 7);
        r[j] = opm_ld(tiles + (int64_t)min(q, Q - 1) * tile_q + (ch & 127) * 8,
                      q < Q);
        if (WT) wv[j] = wrow[(int64_t)min(q, Q - 1) * w_q];
      }
    }
  };

  // this wave's rows of X: s = s0 + 32 wave + 16 st + lr, k group lg
  const int sw0 = s0 + wave * 32;
  const bool wave_on = sw0 < S;
  const uint16_t* xp[2];
  bool x_ok[2];
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int s = sw0 + st * 16 + lr;
    x_ok[st] = s < S;
    xp[st] = X + (bt * S + min(s, S - 1)) * ((int64_t)Q * W) + lg * 8;
  }

  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_tiles(0);
  for (int q0 = 0; q0 < Q; q0 += BQ) {
    __syncthreads();  // previous step's fragment reads are done
    if (WT) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = opm_scale8(r[j], wv[TR ? 0 : j]);
    }
    if (TR) {
      uint4 t[8];
      opm_transpose8(r, t);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        smem[opm_sw((tq * 4 + tcg) * W + tdg * 8 + e)] = t[e];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = j * 256 + tid;
        const int c = (ch >> 2) & 31, dg = ch & 3;
        smem[opm_sw(((ch >> 7) * 4 + dg) * W + c)] = r[j];
      }
    }
    __syncthreads();
    if (q0 + BQ < Q) load_tiles(q0 + BQ);
    if (wave_on) {
#pragma unroll
      for (int ql = 0; ql < BQ; ++ql) {
        const int q = q0 + ql;
        const int64_t xo = (int64_t)min(q, Q - 1) * W;
        const bf16x8 x0 = opm_frag(opm_ld(xp[0] + xo, x_ok[0] && q < Q));
        const bf16x8 x1 = opm_frag(opm_ld(xp[1] + xo, x_ok[1] && q < Q));
        const int base = (ql * 4 + lg) * W;
        const bf16x8 t0 = opm_frag(smem[opm_sw(base + lr)]);
        const bf16x8 t1 = opm_frag(smem[opm_sw(base + 16 + lr)]);
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t0, x0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t0, x1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t1, x0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t1, x1, acc[1][1], 0, 0, 0);
      }
    }
  }

  // epilogue: rows are m, columns are s -> LDS [s][m + pad] -> 16 B stores
  __syncthreads();
  uint16_t* sO = reinterpret_cast<uint16_t*>(smem);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int st = 0; st < 2; ++st)
      *reinterpret_cast<uint2*>(sO + (wave * 32 + st * 16 + lr) * OPITCH +
                                mt * 16 + lg * 4) = opm_pack4(acc[mt][st], scale);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < BS * 4 / 256; ++t) {
    const int ch = tid + 256 * t;
    const int sl = ch >> 2, g = ch & 3;
    if (s0 + sl < S) {
      const uint4 v = *reinterpret_cast<const uint4*>(sO + sl * OPITCH + g * 8);
      *reinterpret_cast<uint4*>(out + ((bt * S + s0 + sl) * (int64_t)P + p) * W +
                                g * 8) = v;
    }
  }
}

void opm_check_operand(const at::Tensor& t, const char* fn, const char* name,
                       int rank) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be a CUDA tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be bf16 (got ", t.scalar_type(), ")");
  TORCH_CHECK(t.dim() == rank, fn, ": ", name, " must be ", rank, "-D (got ",
              t.dim(), "-D)");
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
  for (int d = 0; d < rank; ++d)
    TORCH_CHECK(t.size(d) >= 1 && t.size(d) < ((int64_t)1 << 30), fn, ": ", name,
                " size(", d, ") = ", t.size(d), " out of range");
  for (int d = 3; d < rank; ++d)
    TORCH_CHECK(t.size(d) == W, fn, ": ", name, " size(", d, ") = ", t.size(d),
                ", only width ", W, " is supported");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, ": ", name,
              " data pointer is not 16-byte aligned");
}

// the weight of the *_w entries: fp32 (B, I, J), contiguous, next to ref
void opm_check_weight(const at::Tensor& w, const at::Tensor& ref, int64_t B,
                      int64_t I, int64_t J, const char* fn) {
  TORCH_CHECK(w.is_cuda() && w.device() == ref.device(), fn,
              ": w must be a CUDA tensor on the operands' device");
  TORCH_CHECK(w.scalar_type() == at::kFloat, fn, ": w must be fp32 (got ",
              w.scalar_type(), ")");
  TORCH_CHECK(w.dim() == 3 && w.size(0) == B && w.size(1) == I && w.size(2) == J,
              fn, ": w ", w.sizes(), " must be (B, I, J) = (", B, ", ", I, ", ",
              J, ")");
  TORCH_CHECK(w.is_contiguous(), fn, ": w must be contiguous");
}

// every factor is below 2^30 (opm_check_operand), so no product overflows
unsigned opm_grid(int64_t n0, int64_t n1, int64_t n2, const char* fn) {
  const int64_t lim = (int64_t)1 << 31;
  TORCH_CHECK(n0 * n1 < lim && n0 * n1 * n2 < lim, fn, ": grid too large");
  return (unsigned)(n0 * n1 * n2);
}

const uint16_t* cptr(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}

// shared body of the two gradients: x is b (for da) or a (for db)
at::Tensor opm_backward(const at::Tensor& d_o, const at::Tensor& x, double scale,
                        bool for_a, const char* fn, const at::Tensor* w = nullptr) {
  opm_check_operand(d_o, fn, "d_o", 5);
  opm_check_operand(x, fn, for_a ? "b" : "a", 4);
  TORCH_CHECK(d_o.device() == x.device(), fn, ": operands on different devices");
  const int64_t B = d_o.size(0), I = d_o.size(1), J = d_o.size(2);
  const int64_t S = x.size(1);
  const int64_t P = for_a ? I : J, Q = for_a ? J : I;
  TORCH_CHECK(x.size(0) == B && x.size(2) == Q, fn, ": d_o ", d_o.sizes(), " and ",
              for_a ? "b " : "a ", x.sizes(), " must agree in B and ",
              for_a ? "J" : "I");
  if (w) opm_check_weight(*w, d_o, B, I, J, fn);
  const int64_t nsc = (S + BS - 1) / BS;
  const unsigned grid = opm_grid(B, P, nsc, fn);

  c10::cuda::CUDAGuard guard(d_o.device());
  auto out = at::empty({B, S, P, W}, d_o.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  uint16_t* po = reinterpret_cast<uint16_t*>(out.data_ptr());
  if (w) {
    const float* pw = w->data_ptr<float>();
    if (for_a)
      opm_bwd_kernel<false, true><<<grid, 256, 0, stream>>>(
          po, cptr(d_o), cptr(x), (int)S, (int)P, (int)Q, J * WW, (int64_t)WW,
          (int)nsc, 1.0f, pw);
    else
      opm_bwd_kernel<true, true><<<grid, 256, 0, stream>>>(
          po, cptr(d_o), cptr(x), (int)S, (int)P, (int)Q, (int64_t)WW, J * WW,
          (int)nsc, 1.0f, pw);
  } else if (for_a)
    opm_bwd_kernel<false, false><<<grid, 256, 0, stream>>>(
        po, cptr(d_o), cptr(x), (int)S, (int)P, (int)Q, J * WW, (int64_t)WW,
        (int)nsc, (float)scale, nullptr);
  else
    opm_bwd_kernel<true, false><<<grid, 256, 0, stream>>>(
        po, cptr(d_o), cptr(x), (int)S, (int)P, (int)Q, (int64_t)WW, J * WW,
        (int)nsc, (float)scale, nullptr);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

}  // namespace

namespace {

at::Tensor opm_forward_impl(const at::Tensor& a, const at::Tensor& b, double scale,
                            const at::Tensor* w, const char* fn) {
  opm_check_operand(a, fn, "a", 4);
  opm_check_operand(b, fn, "b", 4);
  TORCH_CHECK(a.device() == b.device(), fn, ": a and b on different devices");
  const int64_t B = a.size(0), S = a.size(1), I = a.size(2), J = b.size(2);
  TORCH_CHECK(b.size(0) == B && b.size(1) == S, fn, ": a ", a.sizes(), " and b ",
              b.sizes(), " must agree in B and S");
  if (w) opm_check_weight(*w, a, B, I, J, fn);
  const int64_t nit = (I + OT - 1) / OT, njt = (J + OT - 1) / OT;
  const unsigned grid = opm_grid(B, nit, njt, fn);

  c10::cuda::CUDAGuard guard(a.device());
  auto o = at::empty({B, I, J, W, W}, a.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  uint16_t* po = reinterpret_cast<uint16_t*>(o.data_ptr());
  if (w)
    opm_fwd_kernel<true><<<grid, 256, 0, stream>>>(
        po, cptr(a), cptr(b), (int)S, (int)I, (int)J, (int)nit, (int)njt, 1.0f,
        w->data_ptr<float>());
  else
    opm_fwd_kernel<false><<<grid, 256, 0, stream>>>(
        po, cptr(a), cptr(b), (int)S, (int)I, (int)J, (int)nit, (int)njt,
        (float)scale, nullptr);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return o;
}

}  // namespace

at::Tensor opm_forward(at::Tensor a, at::Tensor b, double scale) {
  return opm_forward_impl(a, b, scale, nullptr, "opm_forward");
}

at::Tensor opm_backward_a(at::Tensor d_o, at::Tensor b, double scale) {
  return opm_backward(d_o, b, scale, true, "opm_backward_a");
}

at::Tensor opm_backward_b(at::Tensor d_o, at::Tensor a, double scale) {
  return opm_backward(d_o, a, scale, false, "opm_backward_b");
}

// the same three contractions with a per-pair weight w[b, i, j] in place of
// the scalar scale (the reciprocal mask normaliser of a padded batch)
at::Tensor opm_forward_w(at::Tensor a, at::Tensor b, at::Tensor w) {
  return opm_forward_impl(a, b, 1.0, &w, "opm_forward_w");
}

at::Tensor opm_backward_a_w(at::Tensor d_o, at::Tensor b, at::Tensor w) {
  return opm_backward(d_o, b, 1.0, true, "opm_backward_a_w", &w);
}

at::Tensor opm_backward_b_w(at::Tensor d_o, at::Tensor a, at::Tensor w) {
  return opm_backward(d_o, a, 1.0, false, "opm_backward_b_w", &w);
}
