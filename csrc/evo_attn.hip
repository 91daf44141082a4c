// Fused attention for the Evoformer's attention sites: bf16, head dim 32,
// 64 <= T <= 512, T % 64 == 0.
//
//   O = dropout(softmax(Q K^T + bias + mask)) V,   q, k, v: (N, T, 32)
//
// Head dim 32 is the K of v_mfma_f32_16x16x32_bf16, so a 16 x 16 score tile
// is ONE MFMA on fragments loaded straight from global Q / K rows, and so is
// dP = dO V^T.  A transposed operand of a whole attention batch (V^T, K^T,
// Q^T, dO^T: 32 x T bf16) is at most 32 KB, so every kernel stages what it
// needs once and runs its tile loop without a barrier.
//
// Fragment maps (csrc/mfma_probe.hip):
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
//
// Bias (nb, T, T) and mask (nb, 1, T) follow the broadcast contract of
// softmax_dropout and flash_attn.hip: source row of score row (n, q) is
//   ((n / od) % nb) * q_src + (q % q_src).
// Keep bits are the flash definition: field kv % 8 of
// philox(seed, n*T + q, kv / 8), recomputed in backward, never stored.
//
// Scores are clamped below at SCORE_FLOOR after bias and mask are added.  A
// key masked with the project's -1e9 lands on the floor; a row with every key
// masked is exactly uniform, and its LSE (floor + log T) keeps log T in fp32,
// which -1e9 + log T does not, so the backward recomputes P = 1/T for it.
//
// The bias gradient has a kernel of its own (evo_dbias_kernel): no dS tensor,
// no atomics.  docs/KERNELS.md, "Evoformer attention", has the geometry, the
// resource table and the measurements.
#include "common.h"
#include "dispatch.h"

#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int BM = 64;     // rows per block (q rows; kv rows in dkv)
constexpr int BN = 64;     // columns per tile of the loop
constexpr int HD = 32;     // head dim = K of the MFMA
constexpr int TMAX = 512;  // longest T: 32 x 512 bf16 = 32 KB per operand
constexpr float SCORE_FLOOR = -8192.f;

__device__ __forceinline__ bf16x8 load_frag(const uint16_t* p) {
  union {
    uint4 u;
    bf16x8 v;
  } U;
  U.u = *reinterpret_cast<const uint4*>(p);
  return U.v;
}

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float bf16_at(const uint16_t* p, int i) {
  return bf16_bits_to_f32(p[i]);
}

// reductions across the 16 lanes that share a C-tile row
__device__ __forceinline__ float rowgroup_max(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float rowgroup_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// wave 0..3 of the block, fragment k-group / C row group lg, fragment row
// (A) / column (B, C) lr
struct Lane {
  int wid, lg, lr;
};

__device__ __forceinline__ Lane lane_coords() {
  const int lane = threadIdx.x & 63;
  return {(int)threadIdx.x >> 6, lane >> 4, lane & 15};
}

struct Src {
  const uint16_t* ptr = nullptr;
  int64_t nb = 1;
  int q = 1;
  int64_t od = 1;

  __device__ __forceinline__ const uint16_t* row(int64_t n, int qrow,
                                                 int T) const {
    return ptr + (((n / od) % nb) * q + (qrow % q)) * (int64_t)T;
  }
};

// dropout scalars; pinv = 1 / (1 - p), pthresh = keep16_threshold(p)
struct Drop {
  float pinv = 1.f;
  uint32_t pthresh = 0;
  uint64_t seed = 0;
};

// the score the softmax sees
__device__ __forceinline__ float biased(float s, float bias_plus_mask) {
  return fmaxf(s + bias_plus_mask, SCORE_FLOOR);
}

// A transposed operand in LDS is [d][x], x XOR-swizzled in 8-element blocks
// keyed on d & 7 (the B-fragment reads of 16 d rows at one x range then hit
// distinct banks).  The writer and the reader both go through swz.
__device__ __forceinline__ int swz(int d, int x) { return x ^ ((d & 7) << 3); }

// Stage 64 rows of a (rows, 32) tensor, the first at src, transposed into
// dst[d][col0 + 0..63] (row pitch TMAX): thread tid moves row tid / 4,
// d = (tid % 4) * 8 + [0..8).
__device__ __forceinline__ void stage_transposed(uint16_t* dst, int col0,
                                                 const uint16_t* src) {
  const int x = col0 + ((int)threadIdx.x >> 2);
  const int d0 = ((int)threadIdx.x & 3) * 8;
  union {
    uint4 u;
    uint16_t h[8];
  } U;
  U.u = *reinterpret_cast<const uint4*>(src + ((int)threadIdx.x >> 2) * HD + d0);
#pragma unroll
  for (int j = 0; j < 8; ++j) dst[(d0 + j) * TMAX + swz(d0 + j, x)] = U.h[j];
}

// the whole (T, 32) operand of batch n, transposed; ends in a barrier
__device__ __forceinline__ void stage_all(uint16_t* dst, const uint16_t* base,
                                          int64_t n, int T) {
  for (int c = 0; c < T / 64; ++c)
    stage_transposed(dst, c * 64, base + (n * T + c * 64) * (int64_t)HD);
  __syncthreads();
}

// acc += A * X for one A fragment (16 x 32, k = x .. x+31) against the staged
// transpose X^T[d][x]: the 16 x 32 result is two C tiles
__device__ __forceinline__ void mma_staged(bf16x8 a, const uint16_t* t, int x,
                                           const Lane& ln, f32x4 (&acc)[2]) {
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int d = cb * 16 + ln.lr;
    acc[cb] = mfma(a, load_frag(t + d * TMAX + swz(d, x + ln.lg * 8)), acc[cb]);
  }
}

// the fragment of 16 rows, the first at global row `row`, of a (rows, 32)
// tensor: lane holds row lr, d = lg*8 + [0..8).  It is the A fragment of
// those rows and the B fragment of their transpose.
__device__ __forceinline__ bf16x8 row_frag(const uint16_t* base, int64_t row,
                                           const Lane& ln) {
  return load_frag(base + (row + ln.lr) * HD + ln.lg * 8);
}

// s[cb] = A * rows^T for the 64 rows starting at `row`: one MFMA per C tile
__device__ __forceinline__ void score_tile(bf16x8 a, const uint16_t* base,
                                           int64_t row, const Lane& ln,
                                           f32x4 (&s)[4]) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
    s[cb] = mfma(a, row_frag(base, row + cb * 16, ln), f32x4{0.f, 0.f, 0.f, 0.f});
}

// C layout -> A layout through a wave-private 16 x 64 LDS tile.  LDS
// operations of one wave complete in order and no other wave touches the
// tile, so no barrier is needed.
__device__ __forceinline__ void c_store(uint16_t (&t)[16][BN],
                                        const f32x4 (&c)[4], const Lane& ln) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      t[ln.lg * 4 + r][cb * 16 + ln.lr] = f32_to_bf16_bits(c[cb][r]);
}

__device__ __forceinline__ bf16x8 a_load(const uint16_t (&t)[16][BN], int ks2,
                                         const Lane& ln) {
  return load_frag(&t[ln.lr][ks2 * 32 + ln.lg * 8]);
}

// the wave's 16 x 32 C tiles to rows row .. row+15 of a (rows, 32) tensor
__device__ __forceinline__ void store_c_tile(uint16_t* dst, int64_t row,
                                             const f32x4 (&acc)[2],
                                             const Lane& ln) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
      dst[(row + ln.lg * 4 + r) * (int64_t)HD + cb * 16 + ln.lr] =
          f32_to_bf16_bits(acc[cb][r]);
}

// bias + mask of the wave's C tile rows q_first + [0..4), column kv
template <bool HAS_BIAS, bool HAS_MASK>
__device__ __forceinline__ void bias_mask4(const uint16_t* const (&bias_rows)[4],
                                           const uint16_t* mask_row, int kv,
                                           float (&bm)[4]) {
  const float mv = HAS_MASK ? bf16_at(mask_row, kv) : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    bm[r] = (HAS_BIAS ? bf16_at(bias_rows[r], kv) : 0.f) + mv;
}

// ===========================================================================
// forward: grid N * T/64, block = 64 q rows of one batch, wave = 16 of them
// ===========================================================================
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void evo_fwd_kernel(
    uint16_t* __restrict__ out, float* __restrict__ lse,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, Src bias, Src mask, int T, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = T / BM;
  const int64_t n = blockIdx.x / tiles;
  const int q0 = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int64_t row0 = n * T + q0;   // this wave's first q row

  __shared__ __attribute__((aligned(16))) uint16_t lds_p[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_vt[HD * TMAX];
  stage_all(lds_vt, vp, n, T);

  const bf16x8 aq = row_frag(qp, row0, ln);
  f32x4 o_acc[2] = {};
  float m_i[4], l_i[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_i[r] = -INFINITY;
    l_i[r] = 0.f;
  }
  const uint16_t* bias_rows[4];
  if (HAS_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bias_rows[r] = bias.row(n, q0 + ln.lg * 4 + r, T);
  }
  const uint16_t* mask_row = HAS_MASK ? mask.row(n, 0, T) : nullptr;

  for (int kv0 = 0; kv0 < T; kv0 += BN) {
    f32x4 s[4];
    score_tile(aq, kp, n * T + kv0, ln, s);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      float bm[4];
      bias_mask4<HAS_BIAS, HAS_MASK>(bias_rows, mask_row, kv0 + cb * 16 + ln.lr,
                                     bm);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[cb][r] = biased(s[cb][r], bm[r]);
    }
    // online softmax
    float alpha[4], psum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mx = rowgroup_max(
          fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])));
      const float mnew = fmaxf(m_i[r], mx);
      alpha[r] = __expf(m_i[r] - mnew);
      m_i[r] = mnew;
      psum[r] = 0.f;
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[cb][r] = __expf(s[cb][r] - m_i[r]);
        psum[r] += s[cb][r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      l_i[r] = l_i[r] * alpha[r] + rowgroup_sum(psum[r]);
      o_acc[0][r] *= alpha[r];
      o_acc[1][r] *= alpha[r];
    }
    // O += dropout(P) V
    c_store(lds_p[ln.wid], s, ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      bf16x8 ap = a_load(lds_p[ln.wid], ks2, ln);
      if constexpr (DROP) {
        bool keep[8];
        keep16x8(dr.seed, (uint64_t)(row0 + ln.lr), kv0 + ks2 * 32 + ln.lg * 8,
                 dr.pthresh, keep);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float pv = bf16_bits_to_f32((uint16_t)ap[j]);
          ap[j] = (short)f32_to_bf16_bits(keep[j] ? pv * dr.pinv : 0.f);
        }
      }
      mma_staged(ap, lds_vt, kv0 + ks2 * 32, ln, o_acc);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.0f / l_i[r];
    o_acc[0][r] *= inv;
    o_acc[1][r] *= inv;
    if (ln.lr == 0) lse[row0 + ln.lg * 4 + r] = m_i[r] + __logf(l_i[r]);
  }
  store_c_tile(out, row0, o_acc, ln);
}

// ===========================================================================
// backward
// ===========================================================================
//   P = exp(S - lse);  dP = dO V^T;  Di = rowsum(dO o O);
//   dS = P o (keep * pinv * dP - Di)
//   dQ = dS K;  dK = dS^T Q;  dV = (keep * pinv * P)^T dO
//   dbias = sum of dS over the batches that share a bias row block

// Di, fp32: 4 lanes per row of 32
__global__ void evo_dot_do_o_kernel(float* __restrict__ di,
                                    const uint16_t* __restrict__ dop,
                                    const uint16_t* __restrict__ op,
                                    int64_t n_rows) {
  const int el = threadIdx.x & 3;
  for (int64_t row = (int64_t)blockIdx.x * 64 + ((int)threadIdx.x >> 2);
       row < n_rows; row += (int64_t)gridDim.x * 64) {
    float a[8], b[8];
    load8(reinterpret_cast<const __hip_bfloat16*>(dop) + row * HD + el * 8, a);
    load8(reinterpret_cast<const __hip_bfloat16*>(op) + row * HD + el * 8, b);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a[j] * b[j];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (el == 0) di[row] = s;
  }
}

// dQ: grid N * T/64, wave = 16 q rows, K^T resident, kv loop in ascending
// order without barriers
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void evo_bwd_dq_kernel(
    uint16_t* __restrict__ dq, const uint16_t* __restrict__ dop,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const float* __restrict__ lse,
    const float* __restrict__ di, Src bias, Src mask, int T, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = T / BM;
  const int64_t n = blockIdx.x / tiles;
  const int q0 = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int64_t row0 = n * T + q0;

  // [wave][0] = P, [wave][1] = dP: C-layout write, A-layout read
  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][2][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_kt[HD * TMAX];
  stage_all(lds_kt, kp, n, T);

  const bf16x8 aq = row_frag(qp, row0, ln);
  const bf16x8 ado = row_frag(dop, row0, ln);
  float lse_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) lse_r[r] = lse[row0 + ln.lg * 4 + r];
  const float di_row = di[row0 + ln.lr];   // Di of this lane's A row
  const uint16_t* bias_rows[4];
  if (HAS_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bias_rows[r] = bias.row(n, q0 + ln.lg * 4 + r, T);
  }
  const uint16_t* mask_row = HAS_MASK ? mask.row(n, 0, T) : nullptr;

  f32x4 dq_acc[2] = {};
  for (int kv0 = 0; kv0 < T; kv0 += BN) {
    f32x4 s[4], dp[4];
    score_tile(aq, kp, n * T + kv0, ln, s);
    score_tile(ado, vp, n * T + kv0, ln, dp);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      float bm[4];
      bias_mask4<HAS_BIAS, HAS_MASK>(bias_rows, mask_row, kv0 + cb * 16 + ln.lr,
                                     bm);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[cb][r] = __expf(biased(s[cb][r], bm[r]) - lse_r[r]);
    }
    c_store(lds_t[ln.wid][0], s, ln);
    c_store(lds_t[ln.wid][1], dp, ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const bf16x8 pa = a_load(lds_t[ln.wid][0], ks2, ln);
      const bf16x8 dpa = a_load(lds_t[ln.wid][1], ks2, ln);
      bool keep[8];
      if constexpr (DROP)
        keep16x8(dr.seed, (uint64_t)(row0 + ln.lr), kv0 + ks2 * 32 + ln.lg * 8,
                 dr.pthresh, keep);
      bf16x8 dsa;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = bf16_bits_to_f32((uint16_t)pa[j]);
        float dpv = bf16_bits_to_f32((uint16_t)dpa[j]);
        if constexpr (DROP) dpv = keep[j] ? dpv * dr.pinv : 0.f;
        dsa[j] = (short)f32_to_bf16_bits(pv * (dpv - di_row));
      }
      mma_staged(dsa, lds_kt, kv0 + ks2 * 32, ln, dq_acc);
    }
  }
  store_c_tile(dq, row0, dq_acc, ln);
}

// dK, dV: grid N * T/64, wave = 16 kv rows, Q^T and dO^T resident, q loop in
// ascending order without barriers.  The score tile is transposed: lane
// holds kv rows kv_first + [0..4), q column q0 + cq*16 + lr.
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void evo_bwd_dkv_kernel(
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const float* __restrict__ lse, const float* __restrict__ di, Src bias,
    Src mask, int T, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = T / BM;
  const int64_t n = blockIdx.x / tiles;
  const int kv0w = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int kv_first = kv0w + ln.lg * 4;
  const int64_t row0 = n * T + kv0w;   // this wave's first kv row

  // P^T, then dS^T, through one buffer (wave-local order)
  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_qt[HD * TMAX];
  __shared__ __attribute__((aligned(16))) uint16_t lds_dot[HD * TMAX];
  for (int c = 0; c < T / 64; ++c) {
    stage_transposed(lds_qt, c * 64, qp + (n * T + c * 64) * (int64_t)HD);
    stage_transposed(lds_dot, c * 64, dop + (n * T + c * 64) * (int64_t)HD);
  }
  __syncthreads();

  const bf16x8 ak = row_frag(kp, row0, ln);
  const bf16x8 av = row_frag(vp, row0, ln);
  float maskv[4] = {0.f, 0.f, 0.f, 0.f};
  if (HAS_MASK) {
    const uint16_t* mask_row = mask.row(n, 0, T);
#pragma unroll
    for (int r = 0; r < 4; ++r) maskv[r] = bf16_at(mask_row, kv_first + r);
  }

  f32x4 dk_acc[2] = {}, dv_acc[2] = {};
  for (int q0 = 0; q0 < T; q0 += BM) {
    f32x4 st[4], dpt[4];
    score_tile(ak, qp, n * T + q0, ln, st);
    score_tile(av, dop, n * T + q0, ln, dpt);
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
      const int qcol = q0 + cq * 16 + ln.lr;
      const float lse_c = lse[n * T + qcol];
      const float di_c = di[n * T + qcol];
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (HAS_BIAS) {
        // the lane's 4 kv columns of bias row qcol: one 8 B load
        union {
          uint2 u;
          uint16_t h[4];
        } U;
        U.u = *reinterpret_cast<const uint2*>(bias.row(n, qcol, T) + kv_first);
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = bf16_bits_to_f32(U.h[r]);
      }
      bool keep[4] = {true, true, true, true};
      if constexpr (DROP) {
        // the lane's 4 kv rows lie in one 8-block of the keep definition
        bool k8[8];
        const int blk = kv_first & ~7;
        keep16x8(dr.seed, (uint64_t)(n * T + qcol), blk, dr.pthresh, k8);
#pragma unroll
        for (int r = 0; r < 4; ++r) keep[r] = k8[(kv_first - blk) + r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv =
            __expf(biased(st[cq][r], bv[r] + maskv[r]) - lse_c);
        float dpv = dpt[cq][r];
        if constexpr (DROP) dpv = keep[r] ? dpv * dr.pinv : 0.f;
        st[cq][r] = DROP ? (keep[r] ? pv * dr.pinv : 0.f) : pv;  // for dV
        dpt[cq][r] = pv * (dpv - di_c);                          // dS^T
      }
    }
    c_store(lds_t[ln.wid], st, ln);
    bf16x8 pta[2];
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) pta[ks2] = a_load(lds_t[ln.wid], ks2, ln);
    c_store(lds_t[ln.wid], dpt, ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const bf16x8 dsta = a_load(lds_t[ln.wid], ks2, ln);
      mma_staged(pta[ks2], lds_dot, q0 + ks2 * 32, ln, dv_acc);
      mma_staged(dsta, lds_qt, q0 + ks2 * 32, ln, dk_acc);
    }
  }
  store_c_tile(dk, row0, dk_acc, ln);
  store_c_tile(dv, row0, dv_acc, ln);
}

// dbias (nb, T, T) fp32.  A block owns 64 q rows x 32 kv columns of ONE bias
// batch b, a wave 16 q rows of them, and walks the `count` attention batches
// that read that bias block,
//   n_i = ((i / od) * nb + b) * od + i % od,   i = 0 .. count-1,
// in ascending order.  For each it recomputes S and dP (two MFMAs each), P
// from the LSE and dS, and adds dS to 8 fp32 registers per lane: every
// output element has one owner and one summation order, so the result is
// bitwise reproducible with no dS tensor and no atomics.  The next batch's
// fragments are loaded before the current one is consumed.
//
// Keep bits: the wave's 16 x 32 tile needs 16 rows x 4 eight-blocks = 64
// Philox draws, one per lane; each lane packs its 8 bits into a byte of a
// wave-private LDS table that the C-layout owners then read.
struct DbiasIn {
  bf16x8 aq, ado, bk[2], bv[2];
  float lse_r[4], di_r[4], mv[2];
};

template <bool HAS_MASK>
__device__ __forceinline__ void dbias_load(
    DbiasIn& in, int64_t n, int q0, int kv0, const uint16_t* dop,
    const uint16_t* qp, const uint16_t* kp, const uint16_t* vp,
    const float* lse, const float* di, const Src& mask, int T, const Lane& ln) {
  const int64_t base = n * T;
  in.aq = row_frag(qp, base + q0, ln);
  in.ado = row_frag(dop, base + q0, ln);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    in.bk[cb] = row_frag(kp, base + kv0 + cb * 16, ln);
    in.bv[cb] = row_frag(vp, base + kv0 + cb * 16, ln);
    in.mv[cb] =
        HAS_MASK ? bf16_at(mask.row(n, 0, T), kv0 + cb * 16 + ln.lr) : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    in.lse_r[r] = lse[base + q0 + ln.lg * 4 + r];
    in.di_r[r] = di[base + q0 + ln.lg * 4 + r];
  }
}

template <bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void evo_dbias_kernel(
    float* __restrict__ dbias, const uint16_t* __restrict__ dop,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const float* __restrict__ lse,
    const float* __restrict__ di, Src bias, Src mask, int T, int64_t count,
    Drop dr) {
  const Lane ln = lane_coords();
  const int kvt = T / 32, qt = T / BM;
  const int kv0 = ((int)(blockIdx.x % kvt)) * 32;
  const int q0 = ((int)((blockIdx.x / kvt) % qt)) * BM + ln.wid * 16;
  const int64_t b = blockIdx.x / (kvt * qt);

  __shared__ uint8_t lds_keep[4][16][4];

  // the bias of the tile is the same for every batch that shares it
  float bias_v[2][4];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      bias_v[cb][r] =
          bf16_at(bias.ptr + (b * T + q0 + ln.lg * 4 + r) * (int64_t)T,
                  kv0 + cb * 16 + ln.lr);

  auto batch_of = [&](int64_t i) {
    return ((i / bias.od) * bias.nb + b) * bias.od + i % bias.od;
  };

  f32x4 acc[2] = {};
  DbiasIn nxt;
  dbias_load<HAS_MASK>(nxt, batch_of(0), q0, kv0, dop, qp, kp, vp, lse, di,
                       mask, T, ln);
  for (int64_t i = 0; i < count; ++i) {
    const DbiasIn cur = nxt;
    const int64_t n = batch_of(i);
    if (i + 1 < count)
      dbias_load<HAS_MASK>(nxt, batch_of(i + 1), q0, kv0, dop, qp, kp, vp, lse,
                           di, mask, T, ln);
    if constexpr (DROP) {
      bool keep[8];
      keep16x8(dr.seed, (uint64_t)(n * T + q0 + ln.lr), kv0 + ln.lg * 8,
               dr.pthresh, keep);
      uint32_t bits = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) bits |= (keep[j] ? 1u : 0u) << j;
      lds_keep[ln.wid][ln.lr][ln.lg] = (uint8_t)bits;
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      const f32x4 s = mfma(cur.aq, cur.bk[cb], zero);
      const f32x4 dp = mfma(cur.ado, cur.bv[cb], zero);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv =
            __expf(biased(s[r], bias_v[cb][r] + cur.mv[cb]) - cur.lse_r[r]);
        float dpv = dp[r];
        if constexpr (DROP) {
          const uint32_t bits =
              lds_keep[ln.wid][ln.lg * 4 + r][cb * 2 + (ln.lr >> 3)];
          dpv = ((bits >> (ln.lr & 7)) & 1u) ? dpv * dr.pinv : 0.f;
        }
        acc[cb][r] += pv * (dpv - cur.di_r[r]);
      }
    }
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dbias[(b * T + q0 + ln.lg * 4 + r) * (int64_t)T + kv0 + cb * 16 + ln.lr] =
          acc[cb][r];
}

// ---- host ------------------------------------------------------------------

constexpr int64_t GRID_MAX = 2147483647LL;

const char* shape_problem(int64_t N, int64_t T, int64_t D) {
  if (D != HD) return "head dim must be 32";
  if (T < 64 || T > TMAX || T % 64 != 0)
    return "T must be a multiple of 64 in [64, 512]";
  if (N < 1 || N * (T / BM) > GRID_MAX) return "N * T / 64 must fit the grid";
  return nullptr;
}

bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

Src describe(const char* fn, const std::optional<at::Tensor>& t,
             int64_t outer_div, int64_t N, int T, const char* what,
             bool is_mask) {
  Src d;
  if (!t.has_value() || !t->defined()) return d;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->dim() == 3 &&
                  t->size(2) == T && t->scalar_type() == at::kBFloat16,
              fn, ": ", what, " must be contiguous bf16 (nb, q, T=", T,
              ") on the GPU, got ", t->scalar_type(), " ", t->sizes());
  TORCH_CHECK(aligned16(*t), fn, ": ", what, " must be 16 B aligned");
  if (is_mask) {
    TORCH_CHECK(t->size(1) == 1, fn, ": mask must be (nb, 1, T), got q = ",
                t->size(1));
  } else {
    TORCH_CHECK(t->size(1) == 1 || t->size(1) == T, fn,
                ": bias must have q = 1 or q = T = ", T, ", got q = ",
                t->size(1));
  }
  TORCH_CHECK(outer_div >= 1, fn, ": ", what, " outer_div must be >= 1, got ",
              outer_div);
  TORCH_CHECK(N % (t->size(0) * outer_div) == 0, fn, ": N = ", N,
              " is not a multiple of ", what, " nb * outer_div = ", t->size(0),
              " * ", outer_div);
  d.ptr = reinterpret_cast<const uint16_t*>(t->data_ptr());
  d.nb = t->size(0);
  d.q = (int)t->size(1);
  d.od = outer_div;
  return d;
}

// every operand contiguous bf16 (N, T, 32) on the GPU, 16 B aligned
void check_operands(
    const char* fn,
    std::initializer_list<std::pair<const char*, const at::Tensor*>> operands) {
  const at::Tensor& q = *operands.begin()->second;
  TORCH_CHECK(q.dim() == 3, fn, ": q must be (N, T, 32), got ", q.sizes());
  const char* problem = shape_problem(q.size(0), q.size(1), q.size(2));
  TORCH_CHECK(problem == nullptr, fn, ": ", problem, ", got q ", q.sizes());
  for (const auto& [name, t] : operands) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous(), fn, ": ", name,
                " must be a contiguous GPU tensor, got strides ", t->strides());
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, fn, ": ", name,
                " must be bf16, got ", t->scalar_type());
    TORCH_CHECK(t->sizes() == q.sizes(), fn, ": ", name, " has shape ",
                t->sizes(), ", q has ", q.sizes());
    TORCH_CHECK(aligned16(*t), fn, ": ", name, " must be 16 B aligned");
  }
}

Drop make_drop(const char* fn, bool drop, double p, uint64_t seed) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, fn, ": p must be in [0, 1), got ", p);
  Drop d;
  if (drop) {
    d.pinv = (float)(1.0 / (1.0 - p));
    d.pthresh = keep16_threshold(p);
  }
  d.seed = seed;
  return d;
}

// f(flags...) with each flag as std::bool_constant
template <class F>
void dispatch_flags(F&& f) {
  f();
}
template <class F, class... Rest>
void dispatch_flags(F&& f, bool flag, Rest... rest) {
  if (flag)
    dispatch_flags([&](auto... fs) { f(std::true_type{}, fs...); }, rest...);
  else
    dispatch_flags([&](auto... fs) { f(std::false_type{}, fs...); }, rest...);
}

const uint16_t* bits(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bits_mut(at::Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}

}  // namespace

bool evo_attn_supported(int64_t N, int64_t T, int64_t D, bool is_bf16) {
  return is_bf16 && shape_problem(N, T, D) == nullptr;
}

// q, k, v: (N, T, 32) contiguous bf16, q pre-scaled -> (o, lse, seed)
std::vector<at::Tensor> evo_attn_forward(at::Tensor q, at::Tensor k,
                                         at::Tensor v,
                                         std::optional<at::Tensor> bias,
                                         int64_t bias_outer_div,
                                         std::optional<at::Tensor> mask,
                                         int64_t mask_outer_div,
                                         double dropout_p, bool is_training) {
  const char* fn = "evo_attn_forward";
  check_operands(fn, {{"q", &q}, {"k", &k}, {"v", &v}});
  const int64_t N = q.size(0);
  const int T = (int)q.size(1);
  const Src bd = describe(fn, bias, bias_outer_div, N, T, "bias", false);
  const Src md = describe(fn, mask, mask_outer_div, N, T, "mask", true);

  const bool drop = is_training && dropout_p > 0.0;
  // a row draws Philox counters 0 .. T/8 - 1 of its own subsequence; the
  // offset is folded into the key, which forward and backward both use
  Drop dr = make_drop(fn, drop, dropout_p, 0);
  const uint64_t seed = drop ? reserve_philox_key(T / 8 + 4) : 0;
  dr.seed = seed;

  auto o = at::empty_like(q);
  auto lse = at::empty({N, (int64_t)T}, q.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)(N * (T / BM)));
  dispatch_flags(
      [&](auto hb, auto hm, auto dt) {
        evo_fwd_kernel<decltype(hb)::value, decltype(hm)::value,
                       decltype(dt)::value><<<grid, 256, 0, stream>>>(
            bits_mut(o), lse.data_ptr<float>(), bits(q), bits(k), bits(v), bd,
            md, T, dr);
      },
      bd.ptr != nullptr, md.ptr != nullptr, drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  // the seed is host state: a CPU scalar costs the wrapper no sync
  return {o, lse,
          at::scalar_tensor((int64_t)seed, at::TensorOptions().dtype(at::kLong))};
}

std::vector<at::Tensor> evo_attn_backward(
    at::Tensor d_out, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
    at::Tensor lse, std::optional<at::Tensor> bias, int64_t bias_outer_div,
    bool want_dbias, std::optional<at::Tensor> mask, int64_t mask_outer_div,
    double dropout_p, bool dropped, int64_t seed_in) {
  const char* fn = "evo_attn_backward";
  check_operands(fn,
                 {{"q", &q}, {"k", &k}, {"v", &v}, {"o", &o}, {"d_out", &d_out}});
  const int64_t N = q.size(0);
  const int T = (int)q.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == N && lse.size(1) == T,
              fn, ": lse must be contiguous fp32 (", N, ", ", T, "), got ",
              lse.scalar_type(), " ", lse.sizes());
  const Src bd = describe(fn, bias, bias_outer_div, N, T, "bias", false);
  const Src md = describe(fn, mask, mask_outer_div, N, T, "mask", true);
  const bool drop = dropped && dropout_p > 0.0;
  const Drop dr = make_drop(fn, drop, dropout_p, (uint64_t)seed_in);
  const bool dbias_on = bd.ptr != nullptr && want_dbias;
  if (dbias_on) {
    TORCH_CHECK(bd.q == T, fn,
                ": the bias gradient needs a (nb, T, T) bias, got q = ", bd.q);
    TORCH_CHECK(bd.nb * (T / BM) * (T / 32) <= GRID_MAX, fn,
                ": bias nb = ", bd.nb, " does not fit the dbias grid");
  }

  auto stream = at::cuda::getCurrentCUDAStream();
  auto di = at::empty({N, (int64_t)T}, q.options().dtype(at::kFloat));
  const int64_t n_rows = N * T;
  evo_dot_do_o_kernel<<<unicore_grid((n_rows + 63) / 64), 256, 0, stream>>>(
      di.data_ptr<float>(), bits(d_out), bits(o), n_rows);

  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  const float* lse_p = lse.data_ptr<float>();
  const float* di_p = di.data_ptr<float>();
  const dim3 grid((unsigned)(N * (T / BM)));
  dispatch_flags(
      [&](auto hb, auto hm, auto dt) {
        constexpr bool HB = decltype(hb)::value;
        constexpr bool HM = decltype(hm)::value;
        constexpr bool DR = decltype(dt)::value;
        evo_bwd_dq_kernel<HB, HM, DR><<<grid, 256, 0, stream>>>(
            bits_mut(dq), bits(d_out), bits(q), bits(k), bits(v), lse_p, di_p,
            bd, md, T, dr);
        evo_bwd_dkv_kernel<HB, HM, DR><<<grid, 256, 0, stream>>>(
            bits_mut(dk), bits_mut(dv), bits(d_out), bits(q), bits(k), bits(v),
            lse_p, di_p, bd, md, T, dr);
      },
      bd.ptr != nullptr, md.ptr != nullptr, drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  if (!dbias_on) return {dq, dk, dv};

  auto dbias = at::empty({bd.nb, (int64_t)T, (int64_t)T},
                         q.options().dtype(at::kFloat));
  const int64_t count = N / bd.nb;   // batches per bias block
  const dim3 bgrid((unsigned)(bd.nb * (T / BM) * (T / 32)));
  dispatch_flags(
      [&](auto hm, auto dt) {
        evo_dbias_kernel<decltype(hm)::value, decltype(dt)::value>
            <<<bgrid, 256, 0, stream>>>(dbias.data_ptr<float>(), bits(d_out),
                                        bits(q), bits(k), bits(v), lse_p, di_p,
                                        bd, md, T, count, dr);
      },
      md.ptr != nullptr, drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {dq, dk, dv, dbias};
}
