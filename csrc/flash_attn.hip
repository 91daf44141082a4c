// Flash-style fused attention for gfx950 (CDNA4 MFMA), bf16, head_dim 64.
//
// Beyond-reference optimization: the reference materializes the O(L^2)
// score matrix (bmm -> fused softmax -> bmm, reference
// unicore/modules/multihead_attention.py:83-105); this kernel computes
// O = dropout(softmax(Q K^T + bias + mask)) V tile-by-tile with online
// softmax, never touching HBM with the score matrix.
//
// Geometry: one 256-thread block (4 wave64) per 64 query rows of one
// (batch*head); each wave owns 16 rows.  S tiles are built from
// v_mfma_f32_16x16x32_bf16 (fragment mappings verified by
// csrc/mfma_probe.hip / tests/test_kernels_gpu.py):
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
// P is redistributed C-layout -> A-layout through a per-wave LDS tile.
// Dropout keep bits are a pure function of (seed, bh*L+q, kv):
//   16-bit field kv%8 of philox(seed, bh*L+q, kv/8), kept when it is
//   >= p * 65536 (common.h keep16x8) — recomputable by the backward
// kernels with no stored mask.
//
// Per-row LSE (= m + log l) is saved for the backward recomputation.
//
// Every kernel below is assembled from the device blocks that follow; a
// block is the only place its step is written.  docs/KERNELS.md ("Flash
// attention") lists which kernel runs when and what each block owns.
#include "common.h"
#include "dispatch.h"

#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int BM = 64;   // query rows per block
constexpr int BN = 64;   // kv rows per tile
constexpr int HD = 64;   // head dim
// longest L whose whole V^T / K^T the resident kernels keep in LDS (64 KB)
constexpr int LRES = 512;

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
  return __bfloat162float(reinterpret_cast<const __hip_bfloat16*>(p)[i]);
}

// reduce a per-lane value across the 16 lanes that share a C-tile row
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

// ---- the shared blocks -----------------------------------------------------

// Where a lane sits: wave 0..3 of the block, fragment k-group / C row group
// lg, fragment row (A) / col (B, C) lr, and the first of the rows_per_wave
// rows (q rows in forward and dq, kv rows in dkv) that its wave owns.
struct Lane {
  int wid, lg, lr, row0;
};

__device__ __forceinline__ Lane lane_coords(int rows_per_wave) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  return {wid, lane >> 4, lane & 15,
          ((int)blockIdx.x * 4 + wid) * rows_per_wave};
}

// An additive bias or mask, contiguous bf16 (nb, q, L), broadcast over the
// (BH, L, L) scores by the contract shared with softmax_dropout:
//   source row of score row (bh, qrow) = ((bh / od) % nb) * q + (qrow % q)
struct Src {
  const uint16_t* ptr = nullptr;
  int64_t nb = 1;
  int q = 1;
  int64_t od = 1;

  __device__ __forceinline__ int64_t row_index(int64_t bh, int qrow) const {
    return ((bh / od) % nb) * q + (qrow % q);
  }
  __device__ __forceinline__ const uint16_t* row(int64_t bh, int qrow,
                                                 int L) const {
    return ptr + row_index(bh, qrow) * (int64_t)L;
  }
};

// dropout scalars; pinv = 1 / (1 - p), pthresh = keep16_threshold(p)
struct Drop {
  float pinv = 1.f;
  uint32_t pthresh = 0;
  uint64_t seed = 0;
};

// A transposed tile in LDS is [d][x] with x XOR-swizzled in 8-element blocks
// keyed on d & 7, so the B-fragment reads (16 d rows, one x range) are
// bank-conflict-free (guide T2 pattern).  Writer and readers go through swz.
__device__ __forceinline__ int swz(int d, int x) { return x ^ ((d & 7) << 3); }

// Stage 64 rows of a (rows, HD) tensor, the first at src, transposed into
// dst[d][col0 + 0..63] (row pitch `pitch`): thread handles row tid/4,
// d block (tid%4)*16.  The resident kernels call it once per tile of L, the
// tiled ones once per iteration (ping-pong: dst = buffer tile & 1).
__device__ __forceinline__ void stage_transposed(uint16_t* dst, int pitch,
                                                 int col0,
                                                 const uint16_t* src) {
  const int x = col0 + ((int)threadIdx.x >> 2);
  const int st_d0 = ((int)threadIdx.x & 3) * 16;
  const __hip_bfloat16* row = reinterpret_cast<const __hip_bfloat16*>(src) +
                              ((int)threadIdx.x >> 2) * HD + st_d0;
  float f0[8], f1[8];
  load8(row, f0);
  load8(row + 8, f1);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d0 = st_d0 + j;
    const int d1 = st_d0 + 8 + j;
    dst[d0 * pitch + swz(d0, x)] = f32_to_bf16_bits(f0[j]);
    dst[d1 * pitch + swz(d1, x)] = f32_to_bf16_bits(f1[j]);
  }
}

// acc[m] += A[m] * T for M A fragments (16 x 32, k = x .. x+31) against the
// staged transpose T[d][x]: each 16 B B-fragment read feeds M MFMAs.
template <int M>
__device__ __forceinline__ void mma_staged(const bf16x8 (&a)[M],
                                           const uint16_t* t, int pitch, int x,
                                           const Lane& ln,
                                           f32x4 (&acc)[M][4]) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int d = cb * 16 + ln.lr;
    const bf16x8 b = load_frag(t + d * pitch + swz(d, x + ln.lg * 8));
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m][cb] = mfma(a[m], b, acc[m][cb]);
  }
}

// A fragments of 16 rows (the first at global row `row`) of a (rows, HD)
// tensor: lane holds row lr, d = ks*32 + lg*8 + [0..8)
__device__ __forceinline__ void load_a(const uint16_t* base, int64_t row,
                                       const Lane& ln, bf16x8 (&a)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    a[ks] = load_frag(base + (row + ln.lr) * HD + ks * 32 + ln.lg * 8);
}

// One k-step of a score tile: the B fragment of global row cb*16 + lr of the
// 64 rows at `rows` (k = d = ks*32 + lg*8 + [0..8)) feeds the M MFMAs of M
// 16-row A tiles.
template <int M>
__device__ __forceinline__ void score_step(const bf16x8 (&a)[M][2],
                                           const uint16_t* rows, int cb, int ks,
                                           const Lane& ln, f32x4 (&acc)[M]) {
  const bf16x8 b = load_frag(rows + (cb * 16 + ln.lr) * (int64_t)HD + ks * 32 +
                             ln.lg * 8);
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = mfma(a[m][ks], b, acc[m]);
}

// s[m] = A[m] * rows^T: M 16-row A tiles against the same 64 global rows, as
// four 16 x 16 C tiles each.
template <int M>
__device__ __forceinline__ void score_tile(const bf16x8 (&a)[M][2],
                                           const uint16_t* rows,
                                           const Lane& ln, f32x4 (&s)[M][4]) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    f32x4 acc[M] = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) score_step<M>(a, rows, cb, ks, ln, acc);
#pragma unroll
    for (int m = 0; m < M; ++m) s[m][cb] = acc[m];
  }
}

// v + bias[kv] + mask[kv], added in that order.  The forward starts from
// v = 0 and adds the sum to the score; the backward starts from the score.
template <bool HAS_BIAS, bool HAS_MASK>
__device__ __forceinline__ float add_bias_mask(float v, const uint16_t* bias_row,
                                               const uint16_t* mask_row,
                                               int kv) {
  if (HAS_BIAS) v += bf16_at(bias_row, kv);
  if (HAS_MASK) v += bf16_at(mask_row, kv);
  return v;
}

__device__ __forceinline__ float p_from_lse(float s, float lse) {
  return __expf(s - lse);
}

// bias rows of the 4 C rows q_first + [0..4) of a wave's tile
template <bool HAS_BIAS>
__device__ __forceinline__ void bias_rows4(const Src& bias, int64_t bh,
                                           int q_first, int L,
                                           const uint16_t* (&rows)[4]) {
  if (HAS_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) rows[r] = bias.row(bh, q_first + r, L);
  }
}

// the mask is (nb, 1, L): one row per (bh / od) batch, shared by all q
template <bool HAS_MASK>
__device__ __forceinline__ const uint16_t* mask_row_of(const Src& mask,
                                                       int64_t bh, int L) {
  return HAS_MASK ? mask.row(bh, 0, L) : nullptr;
}

// P = exp(S + bias + mask - lse) on a 16 x 64 C-layout tile (dq kernels)
template <bool HAS_BIAS, bool HAS_MASK>
__device__ __forceinline__ void p_tile(f32x4 (&s)[4],
                                       const uint16_t* const (&bias_rows)[4],
                                       const uint16_t* mask_row,
                                       const float (&lse_r)[4], int kv0,
                                       const Lane& ln) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int kv = kv0 + cb * 16 + ln.lr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      s[cb][r] = p_from_lse(
          add_bias_mask<HAS_BIAS, HAS_MASK>(s[cb][r], bias_rows[r], mask_row, kv),
          lse_r[r]);
  }
}

// C layout -> A layout through a wave-private 16 x 64 LDS tile.  The
// compiler's lgkmcnt waits order write -> read within the wave, and no other
// wave touches the tile, so no barrier is needed.
__device__ __forceinline__ void c_store(uint16_t (&t)[16][BN],
                                        const f32x4 (&c)[4], const Lane& ln) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      t[ln.lg * 4 + r][cb * 16 + ln.lr] = f32_to_bf16_bits(c[cb][r]);
}

// A frag of the tile: row = lr, cols ks2*32 + lg*8 + [0..8)
__device__ __forceinline__ bf16x8 a_load(const uint16_t (&t)[16][BN], int ks2,
                                         const Lane& ln) {
  return load_frag(&t[ln.lr][ks2 * 32 + ln.lg * 8]);
}

// keep bits of P[row, kv0 .. kv0+7]; all true without dropout
template <bool DROP>
__device__ __forceinline__ void keep_bits8(uint64_t seed, uint64_t subseq,
                                           int kv0, uint32_t pthresh,
                                           bool (&keep)[8]) {
  if constexpr (!DROP) {
#pragma unroll
    for (int j = 0; j < 8; ++j) keep[j] = true;
    return;
  }
  keep16x8(seed, subseq, kv0, pthresh, keep);
}

// dropout on the A fragment P[row, kv .. kv+7] (row = bh*L + q)
template <bool DROP>
__device__ __forceinline__ void drop_frag(bf16x8& ap, const Drop& dr,
                                          int64_t row, int kv) {
  if constexpr (DROP) {
    bool keep[8];
    keep16x8(dr.seed, (uint64_t)row, kv, dr.pthresh, keep);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pv = bf16_bits_to_f32((uint16_t)(unsigned short)ap[j]);
      pv = keep[j] ? pv * dr.pinv : 0.f;
      ap[j] = (short)f32_to_bf16_bits(pv);
    }
  }
}

// dS = P o (keep * pinv * dP - Di) on the A fragments of row `row`, columns
// kv .. kv+7; dsf is the fp32 value before rounding (atomic dbias path)
template <bool DROP>
__device__ __forceinline__ void ds_frag(const bf16x8& pa, const bf16x8& dpa,
                                        float di_row, const Drop& dr,
                                        int64_t row, int kv, bf16x8& dsa,
                                        float (&dsf)[8]) {
  bool keep[8];
  if constexpr (DROP) keep16x8(dr.seed, (uint64_t)row, kv, dr.pthresh, keep);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float pv = bf16_bits_to_f32((uint16_t)(unsigned short)pa[j]);
    float dpv = bf16_bits_to_f32((uint16_t)(unsigned short)dpa[j]);
    if constexpr (DROP) dpv = keep[j] ? dpv * dr.pinv : 0.f;
    dsf[j] = pv * (dpv - di_row);
    dsa[j] = (short)f32_to_bf16_bits(dsf[j]);
  }
}

// materialize dS (BH*L, L) for the bias gradient when asked to: one 16 B store
__device__ __forceinline__ void store_ds(uint16_t* ds_out, int64_t row, int L,
                                         int kv, const bf16x8& dsa) {
  if (ds_out != nullptr) {
    union {
      bf16x8 v;
      uint4 u;
    } U;
    U.v = dsa;
    *reinterpret_cast<uint4*>(ds_out + row * (int64_t)L + kv) = U.u;
  }
}

// epilogue: the wave's 16 x 64 C tiles to rows row .. row+15 of (rows, HD)
__device__ __forceinline__ void store_c_tile(uint16_t* dst, int64_t row,
                                             const f32x4 (&acc)[4],
                                             const Lane& ln) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      dst[(row + ln.lg * 4 + r) * (int64_t)HD + cb * 16 + ln.lr] =
          f32_to_bf16_bits(acc[cb][r]);
}

// ===========================================================================
// forward
// ===========================================================================
//
// The forward of one block, grid (L/BM, B*H).
// RESIDENT (L <= LRES): the whole V^T is staged once and the kv loop runs
// barrier-free (same PMC-driven rationale as the K^T-resident dq variant).
// Otherwise V^T is staged per tile, between two barriers.
template <bool HAS_BIAS, bool HAS_MASK, bool DROP, bool RESIDENT>
__device__ __forceinline__ void flash_fwd_block(
    uint16_t* __restrict__ out, float* __restrict__ lse,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const Src& bias, const Src& mask, int L,
    const Drop& dr) {
  const Lane ln = lane_coords(16);
  const int64_t bh = blockIdx.y;
  const int64_t row0 = bh * L + ln.row0;   // this wave's first q row

  __shared__ __attribute__((aligned(16))) uint16_t lds_p[4][16][BN];
  constexpr int VT_COLS = RESIDENT ? LRES : BN;
  __shared__ __attribute__((aligned(16))) uint16_t lds_vt[HD][VT_COLS];

  if constexpr (RESIDENT) {
    for (int c = 0; c < L / BN; ++c)
      stage_transposed(&lds_vt[0][0], VT_COLS, c * BN,
                       vp + (bh * L + c * BN) * (int64_t)HD);
    __syncthreads();
  }

  bf16x8 aq[1][2];
  load_a(qp, row0, ln, aq[0]);

  f32x4 o_acc[1][4] = {};
  float m_i[4], l_i[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_i[r] = -INFINITY;
    l_i[r] = 0.f;
  }
  const uint16_t* bias_rows[4];
  bias_rows4<HAS_BIAS>(bias, bh, ln.row0 + ln.lg * 4, L, bias_rows);
  const uint16_t* mask_row = mask_row_of<HAS_MASK>(mask, bh, L);

  const int n_tiles = L / BN;
  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * BN;
    if constexpr (!RESIDENT) {
      stage_transposed(&lds_vt[0][0], VT_COLS, 0,
                       vp + (bh * L + kv0) * (int64_t)HD);
      __syncthreads();
    }
    // ---- S = Q K^T (per wave: 16 x 64 as 4 C tiles) + bias + mask ------
    f32x4 s[1][4];
    score_tile<1>(aq, kp + (bh * L + kv0) * (int64_t)HD, ln, s);
    if constexpr (HAS_BIAS || HAS_MASK) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s[0][cb][r] += add_bias_mask<HAS_BIAS, HAS_MASK>(
              0.f, bias_rows[r], mask_row, kv0 + cb * 16 + ln.lr);
    }
    // ---- online softmax ----------------------------------------------
    float mnew[4], alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = fmaxf(fmaxf(s[0][0][r], s[0][1][r]),
                       fmaxf(s[0][2][r], s[0][3][r]));
      mx = rowgroup_max(mx);
      mnew[r] = fmaxf(m_i[r], mx);
      alpha[r] = __expf(m_i[r] - mnew[r]);
      m_i[r] = mnew[r];
    }
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[0][cb][r] = p_from_lse(s[0][cb][r], mnew[r]);
        psum[r] += s[0][cb][r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      l_i[r] = l_i[r] * alpha[r] + rowgroup_sum(psum[r]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) o_acc[0][cb][r] *= alpha[r];
    }
    // ---- O += dropout(P) V -------------------------------------------
    c_store(lds_p[ln.wid], s[0], ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      bf16x8 ap[1] = {a_load(lds_p[ln.wid], ks2, ln)};
      drop_frag<DROP>(ap[0], dr, row0 + ln.lr, kv0 + ks2 * 32 + ln.lg * 8);
      mma_staged<1>(ap, &lds_vt[0][0], VT_COLS,
                    (RESIDENT ? kv0 : 0) + ks2 * 32, ln, o_acc);
    }
    if constexpr (!RESIDENT) __syncthreads();
  }

  // ---- epilogue: normalize, store O (bf16) and LSE (fp32) -------------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.0f / l_i[r];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) o_acc[0][cb][r] *= inv;
    if (ln.lr == 0) lse[row0 + ln.lg * 4 + r] = m_i[r] + __logf(l_i[r]);
  }
  store_c_tile(out, row0, o_acc[0], ln);
}

template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void flash_fwd_vres_kernel(
    uint16_t* __restrict__ out, float* __restrict__ lse,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, Src bias, Src mask, int L, Drop dr) {
  flash_fwd_block<HAS_BIAS, HAS_MASK, DROP, true>(out, lse, qp, kp, vp, bias,
                                                  mask, L, dr);
}

// The tiled forward takes bias, mask and dropout scalars as loose arguments.
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void flash_fwd_kernel(
    uint16_t* __restrict__ out, float* __restrict__ lse,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp,
    const uint16_t* __restrict__ bias, int64_t bias_nb, int bias_q, int64_t bias_od,
    const uint16_t* __restrict__ mask, int64_t mask_nb, int mask_q, int64_t mask_od,
    int L, float pinv, uint32_t pthresh, uint64_t seed) {
  flash_fwd_block<HAS_BIAS, HAS_MASK, DROP, false>(
      out, lse, qp, kp, vp, Src{bias, bias_nb, bias_q, bias_od},
      Src{mask, mask_nb, mask_q, mask_od}, L, Drop{pinv, pthresh, seed});
}

Src describe(const std::optional<at::Tensor>& t, int64_t outer_div, int L,
             const char* what) {
  Src d;
  if (t.has_value() && t->defined()) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->dim() == 3 &&
                    t->size(2) == L && t->scalar_type() == at::kBFloat16,
                "flash_attn: ", what, " must be contiguous bf16 (nb, q, L=", L,
                "), got ", t->scalar_type(), " ", t->sizes());
    d.ptr = reinterpret_cast<const uint16_t*>(t->data_ptr());
    d.nb = t->size(0);
    d.q = (int)t->size(1);
    d.od = outer_div > 0 ? outer_div : 1;
  }
  return d;
}

// The input contract of both entries: every operand contiguous bf16
// (BH, L, 64) on the GPU with L % 64 == 0, a mask that broadcasts over q.
// Returns L.
int check_inputs(const char* fn,
                 std::initializer_list<std::pair<const char*, const at::Tensor*>>
                     operands) {
  const at::Tensor& q = *operands.begin()->second;
  TORCH_CHECK(q.dim() == 3 && q.size(2) == HD, fn,
              ": q must be (BH, L, 64), got ", q.sizes());
  TORCH_CHECK(q.size(1) % BN == 0, fn, ": L must be a multiple of 64, got ",
              q.size(1));
  for (const auto& [name, t] : operands) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous(), fn, ": ", name,
                " must be a contiguous GPU tensor");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, fn, ": ", name,
                " must be bf16, got ", t->scalar_type());
    TORCH_CHECK(t->sizes() == q.sizes(), fn, ": ", name, " has shape ",
                t->sizes(), ", q has ", q.sizes());
  }
  return (int)q.size(1);
}

Drop make_drop(bool drop, double dropout_p, uint64_t seed) {
  Drop d;
  if (drop) {
    const double pc = std::min(dropout_p, 0.999999);
    d.pinv = (float)(1.0 / (1.0 - pc));
    d.pthresh = keep16_threshold(pc);
  }
  d.seed = seed;
  return d;
}

// f(has_bias, has_mask, drop) with the three flags as std::bool_constant
template <class F>
void dispatch_flags(bool has_bias, bool has_mask, bool drop, F&& f) {
  auto with_drop = [&](auto hb, auto hm) {
    if (drop)
      f(hb, hm, std::true_type{});
    else
      f(hb, hm, std::false_type{});
  };
  auto with_mask = [&](auto hb) {
    if (has_mask)
      with_drop(hb, std::true_type{});
    else
      with_drop(hb, std::false_type{});
  };
  if (has_bias)
    with_mask(std::true_type{});
  else
    with_mask(std::false_type{});
}

// kernel<<<grid, 256>>>(outs..., common...): `common` is the argument pack
// an entry builds once and every one of its kernels takes after its outputs
template <class Kernel, class Common, class... Outs>
void launch(Kernel* kernel, dim3 grid, hipStream_t stream, const Common& common,
            Outs... outs) {
  std::apply(
      [&](auto... in) { kernel<<<grid, 256, 0, stream>>>(outs..., in...); },
      common);
}

const uint16_t* bits(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bits_mut(at::Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}

}  // namespace

// q, k, v: (B*H, L, 64) contiguous bf16 (q pre-scaled).  Returns (o, lse).
std::vector<at::Tensor> flash_attn_forward(at::Tensor q, at::Tensor k, at::Tensor v,
                                           std::optional<at::Tensor> bias,
                                           int64_t bias_outer_div,
                                           std::optional<at::Tensor> mask,
                                           int64_t mask_outer_div,
                                           double dropout_p, bool is_training) {
  const int L =
      check_inputs("flash_attn", {{"q", &q}, {"k", &k}, {"v", &v}});
  const int64_t BH = q.size(0);
  const Src bd = describe(bias, bias_outer_div, L, "bias");
  const Src md = describe(mask, mask_outer_div, L, "mask");
  TORCH_CHECK(md.q == 1, "flash_attn: mask must broadcast over q, got q = ",
              md.q);

  const bool drop = is_training && dropout_p > 0.0;
  // A row's keep bits consume Philox counters 0 .. L/8 - 1 of its own
  // subsequence.  The generator is advanced by (L + 3) / 4 + 4, twice what a
  // row needs: the figure dates from a 4-per-draw keep definition and stays,
  // so that the ops after this one draw what they always drew.
  // The offset is folded into the seed and otherwise NOT used — keep bits
  // must be identical in forward and backward, and both derive them from
  // (seed, row, kv).  The generator advance still makes the NEXT op see
  // fresh randomness.
  const uint64_t seed = drop ? reserve_philox_key((L + 3) / 4 + 4) : 0;
  const Drop dr = make_drop(drop, dropout_p, seed);

  auto o = at::empty_like(q);
  auto lse_t = at::empty({BH, (int64_t)L}, q.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid(L / BM, BH);
  const auto common = std::make_tuple(bits(q), bits(k), bits(v), bd, md, L, dr);
  // the tiled kernel takes the same values as loose arguments
  const auto loose = std::make_tuple(bits(q), bits(k), bits(v), bd.ptr, bd.nb,
                                     bd.q, bd.od, md.ptr, md.nb, md.q, md.od, L,
                                     dr.pinv, dr.pthresh, dr.seed);

  dispatch_flags(bd.ptr, md.ptr, drop, [&](auto hb, auto hm, auto dt) {
    constexpr bool HB = decltype(hb)::value;
    constexpr bool HM = decltype(hm)::value;
    constexpr bool DR = decltype(dt)::value;
    if (L <= LRES)
      launch(flash_fwd_vres_kernel<HB, HM, DR>, grid, stream, common,
             bits_mut(o), lse_t.data_ptr<float>());
    else
      launch(flash_fwd_kernel<HB, HM, DR>, grid, stream, loose, bits_mut(o),
             lse_t.data_ptr<float>());
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  // seed is host-side state: keep it on CPU so `int(seed)` in the autograd
  // wrapper is free (a CUDA scalar here cost a D2H sync per forward and
  // broke hipGraph capture).
  return {o, lse_t,
          at::scalar_tensor((int64_t)seed,
                            at::TensorOptions().dtype(at::kLong))};
}

// ===========================================================================
// backward
// ===========================================================================
//
// Standard flash recomputation: P = exp(S - lse); dP = dO V^T;
// dS = P o (dropmask*pinv*dP - Di),  Di = rowsum(dO o O);
// dQ = dS K;  dK = dS^T Q;  dV = (dropmask*pinv*P)^T dO;
// dBias = sum over broadcast batches of dS (separate grouped pass).
// Dropout keep bits are recomputed from (seed, bh*L+q, kv) — no stored mask.

namespace {

// Di = rowsum(dO o O), fp32; one 8-lane group per row
__global__ void flash_dot_do_o_kernel(float* __restrict__ di,
                                      const uint16_t* __restrict__ dop,
                                      const uint16_t* __restrict__ op,
                                      int64_t n_rows) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int sub = lane >> 3;       // 8 rows per wave
  const int el = lane & 7;         // 8 elems x 8 bytes each
  for (int64_t row = ((int64_t)blockIdx.x * 4 + wid) * 8 + sub;
       row < n_rows; row += (int64_t)gridDim.x * 32) {
    float a[8], b[8];
    load8(reinterpret_cast<const __hip_bfloat16*>(dop) + row * HD + el * 8, a);
    load8(reinterpret_cast<const __hip_bfloat16*>(op) + row * HD + el * 8, b);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a[j] * b[j];
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off, 64);
    if (el == 0) di[row] = s;
  }
}

// The atomic dbias accumulator is an argument of the tiled dq kernel only:
// merely carrying the never-taken branch in a short-L kernel cost 8 VGPRs
// and an occupancy step (docs/KERNELS.md, "Flash dbias fusion").
struct NoDbiasAcc {};
template <bool RESIDENT>
using DbiasAcc = std::conditional_t<RESIDENT, NoDbiasAcc, float*>;

// dQ, 16 q rows per wave.
// RESIDENT (L <= LRES with L % 128 != 0; profiles call it dq_kres): the
// whole K^T is staged once (L*HD bf16 <= 64 KB LDS) so the kv loop runs with
// NO per-tile barriers — the per-tile barrier+staging serialization is what
// keeps the tiled variant at ~2%% MFMA utilization (PMC evidence in
// profiles/).  Otherwise (L > LRES) K^T is staged per tile, and dS can be
// accumulated into dbias_acc with atomics (run-time null check).
// The body keeps its statements written out, in the order they had before
// the shared blocks existed, and loose bias / mask / dropout arguments:
// assembled from score_tile, p_tile, c_store / a_load, ds_frag and
// mma_staged it took 148-156 VGPRs where this text takes 120-128 (a wave
// per SIMD less) and its backward ran 9.3% slower with mask + dropout at
// L 1024.  swz is the one block it shares: with Lane, Src::row, store_ds and
// store_c_tile as well, the RESIDENT instantiations 001 / 010 took 132 VGPRs
// against 128, again a wave less.
template <bool HAS_BIAS, bool HAS_MASK, bool DROP, bool RESIDENT>
__global__ __launch_bounds__(256) void flash_bwd_dq_kernel(
    uint16_t* __restrict__ dq, uint16_t* __restrict__ ds_out,
    DbiasAcc<RESIDENT> dbias_acc,
    const uint16_t* __restrict__ dop,
    const uint16_t* __restrict__ qp, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const float* __restrict__ lse,
    const float* __restrict__ di,
    const uint16_t* __restrict__ bias, int64_t bias_nb, int bias_q, int64_t bias_od,
    const uint16_t* __restrict__ mask, int64_t mask_nb, int mask_q, int64_t mask_od,
    int L, float pinv, uint32_t pthresh, uint64_t seed) {
  const int qt = blockIdx.x;
  const int64_t bh = blockIdx.y;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lg = lane >> 4;
  const int lr = lane & 15;
  const int q0 = qt * BM + wid * 16;
  const int64_t qbase = (bh * L + q0) * HD;

  // [wave][0]=P tile, [wave][1]=dS tile (C-layout write, A-layout read)
  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][2][16][BN];
  // K tile transposed [d][kv] (swizzled) for the dQ = dS K product
  __shared__ __attribute__((aligned(16))) uint16_t lds_kt[HD][RESIDENT ? LRES : BN];
  const int st_kv = (int)threadIdx.x >> 2;
  const int st_d0 = ((int)threadIdx.x & 3) * 16;

  if constexpr (RESIDENT) {
    // stage the WHOLE K^T once: thread covers kv rows tid/4 + 64*c
    {
      const int st_kv0 = (int)threadIdx.x >> 2;
      const int st_d0 = ((int)threadIdx.x & 3) * 16;
      for (int c = 0; c < L / 64; ++c) {
        const int kv = st_kv0 + c * 64;
        float f0[8], f1[8];
        load8(reinterpret_cast<const __hip_bfloat16*>(kp) +
                  (bh * L + kv) * (int64_t)HD + st_d0,
              f0);
        load8(reinterpret_cast<const __hip_bfloat16*>(kp) +
                  (bh * L + kv) * (int64_t)HD + st_d0 + 8,
              f1);
  #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d0 = st_d0 + j;
          const int d1 = st_d0 + 8 + j;
          lds_kt[d0][swz(d0, kv)] = f32_to_bf16_bits(f0[j]);
          lds_kt[d1][swz(d1, kv)] = f32_to_bf16_bits(f1[j]);
        }
      }
    }
    __syncthreads();
  }

  bf16x8 aq[2], ado[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    aq[ks] = load_frag(qp + qbase + (int64_t)lr * HD + ks * 32 + lg * 8);
    ado[ks] = load_frag(dop + qbase + (int64_t)lr * HD + ks * 32 + lg * 8);
  }
  float lse_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lse_r[r] = lse[bh * L + q0 + lg * 4 + r];
  }
  const float di_row = di[bh * L + q0 + lr];   // Di for this lane's A row
  const uint16_t* bias_rows[4];
  const uint16_t* mask_row = nullptr;
  if (HAS_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + lg * 4 + r;
      bias_rows[r] =
          bias + (((bh / bias_od) % bias_nb) * bias_q + (q % bias_q)) * (int64_t)L;
    }
  }
  if (HAS_MASK)
    mask_row = mask + (((bh / mask_od) % mask_nb) * mask_q) * (int64_t)L;

  f32x4 dq_acc[4] = {};
  const int n_tiles = L / BN;
  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * BN;
    if constexpr (!RESIDENT) {
      {
        float f0[8], f1[8];
        load8(reinterpret_cast<const __hip_bfloat16*>(kp) +
                  (bh * L + kv0 + st_kv) * (int64_t)HD + st_d0,
              f0);
        load8(reinterpret_cast<const __hip_bfloat16*>(kp) +
                  (bh * L + kv0 + st_kv) * (int64_t)HD + st_d0 + 8,
              f1);
  #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d0 = st_d0 + j;
          const int d1 = st_d0 + 8 + j;
          lds_kt[d0][swz(d0, st_kv)] = f32_to_bf16_bits(f0[j]);
          lds_kt[d1][swz(d1, st_kv)] = f32_to_bf16_bits(f1[j]);
        }
      }
      __syncthreads();
    }
    f32x4 s[4], dp[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      f32x4 acc = {}, accd = {};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 bk = load_frag(
            kp + (bh * L + kv0 + cb * 16 + lr) * (int64_t)HD + ks * 32 + lg * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ks], bk, acc, 0, 0, 0);
        const bf16x8 bvt = load_frag(
            vp + (bh * L + kv0 + cb * 16 + lr) * (int64_t)HD + ks * 32 + lg * 8);
        accd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado[ks], bvt, accd, 0, 0, 0);
      }
      s[cb] = acc;
      dp[cb] = accd;
    }
    // P = exp(S + bias + mask - lse)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int kv = kv0 + cb * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sv = s[cb][r];
        if (HAS_BIAS)
          sv += __bfloat162float(
              reinterpret_cast<const __hip_bfloat16*>(bias_rows[r])[kv]);
        if (HAS_MASK)
          sv += __bfloat162float(
              reinterpret_cast<const __hip_bfloat16*>(mask_row)[kv]);
        s[cb][r] = __expf(sv - lse_r[r]);
      }
    }
    // redistribute P and dP to A layout
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lds_t[wid][0][lg * 4 + r][cb * 16 + lr] = f32_to_bf16_bits(s[cb][r]);
        lds_t[wid][1][lg * 4 + r][cb * 16 + lr] = f32_to_bf16_bits(dp[cb][r]);
      }
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const bf16x8 pa = load_frag(&lds_t[wid][0][lr][ks2 * 32 + lg * 8]);
      const bf16x8 dpa = load_frag(&lds_t[wid][1][lr][ks2 * 32 + lg * 8]);
      bool keep[8];
      keep_bits8<DROP>(seed, (uint64_t)(bh * L + q0 + lr),
                       kv0 + ks2 * 32 + lg * 8, pthresh, keep);
      bf16x8 dsa;
      float dsf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = bf16_bits_to_f32((uint16_t)(unsigned short)pa[j]);
        float dpv = bf16_bits_to_f32((uint16_t)(unsigned short)dpa[j]);
        if (DROP) dpv = keep[j] ? dpv * pinv : 0.f;
        dsf[j] = pv * (dpv - di_row);
        dsa[j] = (short)f32_to_bf16_bits(dsf[j]);
      }
      if constexpr (!RESIDENT) if (HAS_BIAS && dbias_acc != nullptr) {
        // fused dbias accumulation: fp32 dS straight into the (nb, L, L)
        // buffer; contention equals the broadcast batch count
        const int64_t brow =
            ((bh / bias_od) % bias_nb) * (int64_t)bias_q + ((q0 + lr) % bias_q);
        float* bdst = dbias_acc + brow * (int64_t)L + kv0 + ks2 * 32 + lg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(bdst + j, dsf[j]);
      }
      if (ds_out != nullptr) {
        // materialize dS for the bias gradient (deterministic fallback;
        // the broadcast-batch sum happens as one torch reduction)
        union {
          bf16x8 v;
          uint4 u;
        } U;
        U.v = dsa;
        *reinterpret_cast<uint4*>(ds_out + (bh * L + q0 + lr) * (int64_t)L +
                                  kv0 + ks2 * 32 + lg * 8) = U.u;
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int d = cb * 16 + lr;
        const bf16x8 bkf =
            load_frag(&lds_kt[d][swz(d, (RESIDENT ? kv0 : 0) + ks2 * 32 + lg * 8)]);
        dq_acc[cb] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bkf, dq_acc[cb], 0, 0, 0);
      }
    }
    if constexpr (!RESIDENT) __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + lg * 4 + r;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      dq[(bh * L + q) * (int64_t)HD + cb * 16 + lr] =
          f32_to_bf16_bits(dq_acc[cb][r]);
  }
}

// 32-row-per-wave dq (L % 128 == 0, L <= LRES): each wave owns TWO 16-row
// M-tiles, so every K/V B-fragment load feeds two MFMAs and the per-tile
// scalar overheads (lse/di/bias addressing, philox) amortize.
// P/dS redistribute shares one LDS buffer sequentially (wave-local order).
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void flash_bwd_dq_k32_kernel(
    uint16_t* __restrict__ dq, uint16_t* __restrict__ ds_out,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const float* __restrict__ lse, const float* __restrict__ di, Src bias,
    Src mask, int L, Drop dr) {
  const Lane ln = lane_coords(32);   // 2 M-tiles
  const int64_t bh = blockIdx.y;

  // K^T is staged per kv-tile (8 KB) instead of full-L resident (64 KB):
  // the resident version capped the block at 80 KB LDS -> 2 blocks/CU ->
  // 2 waves/SIMD, and PMC showed 41% of wave cycles parked on waits —
  // occupancy, not staging traffic, was the binding constraint.
  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][2][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_kt[2][HD][BN];

  bf16x8 aq[2][2], ado[2][2];
  float lse_r[2][4], di_row[2];
  const uint16_t* bias_rows[2][4];
#pragma unroll
  for (int mtile = 0; mtile < 2; ++mtile) {
    const int64_t row = bh * L + ln.row0 + mtile * 16;
    load_a(qp, row, ln, aq[mtile]);
    load_a(dop, row, ln, ado[mtile]);
#pragma unroll
    for (int r = 0; r < 4; ++r) lse_r[mtile][r] = lse[row + ln.lg * 4 + r];
    bias_rows4<HAS_BIAS>(bias, bh, ln.row0 + mtile * 16 + ln.lg * 4, L,
                         bias_rows[mtile]);
    di_row[mtile] = di[row + ln.lr];
  }
  const uint16_t* mask_row = mask_row_of<HAS_MASK>(mask, bh, L);

  f32x4 dq_acc[2][4] = {};
  const int n_tiles = L / BN;
  // NOTE (measured): a T14 register prefetch of the next tile's K/V
  // fragments was tried here (issue after the bias loads, single register
  // set) — dq went 630 -> 832-1099 us. At 264+ VGPR / 1 wave/SIMD the
  // extra 96 registers hurt scheduling more than the ~500-cycle load
  // latency costs; the FIFO vm-queue also forces later short loads to
  // drain any outstanding prefetch. Reverted; kept as a record.
  // ping-pong K^T staging: stage tile t+1 into the other buffer while
  // computing tile t, one barrier per iteration
  stage_transposed(&lds_kt[0][0][0], BN, 0, kp + bh * L * (int64_t)HD);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * BN;
    if (t + 1 < n_tiles)
      stage_transposed(&lds_kt[(t + 1) & 1][0][0], BN, 0,
                       kp + (bh * L + kv0 + BN) * (int64_t)HD);
    f32x4 s[2][4], dp[2][4];
    __builtin_amdgcn_s_setprio(1);
    score_tile<2>(aq, kp + (bh * L + kv0) * (int64_t)HD, ln, s);
    score_tile<2>(ado, vp + (bh * L + kv0) * (int64_t)HD, ln, dp);
    __builtin_amdgcn_s_setprio(0);
    // redistribute P (both M-tiles), read A-fragments, then reuse for dP
    bf16x8 pa[2][2];
#pragma unroll
    for (int mtile = 0; mtile < 2; ++mtile) {
      p_tile<HAS_BIAS, HAS_MASK>(s[mtile], bias_rows[mtile], mask_row,
                                 lse_r[mtile], kv0, ln);
      c_store(lds_t[ln.wid][mtile], s[mtile], ln);
    }
#pragma unroll
    for (int mtile = 0; mtile < 2; ++mtile)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
        pa[mtile][ks2] = a_load(lds_t[ln.wid][mtile], ks2, ln);
#pragma unroll
    for (int mtile = 0; mtile < 2; ++mtile)
      c_store(lds_t[ln.wid][mtile], dp[mtile], ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int kv = kv0 + ks2 * 32 + ln.lg * 8;
      bf16x8 dsa[2];
#pragma unroll
      for (int mtile = 0; mtile < 2; ++mtile) {
        const int64_t row = bh * L + ln.row0 + mtile * 16 + ln.lr;
        float dsf[8];
        ds_frag<DROP>(pa[mtile][ks2], a_load(lds_t[ln.wid][mtile], ks2, ln),
                      di_row[mtile], dr, row, kv, dsa[mtile], dsf);
        store_ds(ds_out, row, L, kv, dsa[mtile]);
      }
      mma_staged<2>(dsa, &lds_kt[t & 1][0][0], BN, ks2 * 32, ln, dq_acc);
    }
    // publish tile t+1's staging; reads of buffer t&1 are also done, so
    // its restage at t+2 (after the next barrier) is safe
    __syncthreads();
  }
#pragma unroll
  for (int mtile = 0; mtile < 2; ++mtile)
    store_c_tile(dq, bh * L + ln.row0 + mtile * 16, dq_acc[mtile], ln);
}

// ---- dK / dV: one wave owns 16 kv rows and walks the q tiles ---------------

// additive mask of the 4 kv rows kv_first + [0..4) (constant over q)
template <bool HAS_MASK>
__device__ __forceinline__ void load_maskv(const Src& mask, int64_t bh,
                                           int kv_first, int L,
                                           float (&maskv)[4]) {
  const uint16_t* mask_row = mask_row_of<HAS_MASK>(mask, bh, L);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    maskv[r] = HAS_MASK ? bf16_at(mask_row, kv_first + r) : 0.f;
}

// On the transposed 16 kv x 64 q C tiles of q tile q0 (lane: kv rows
// kv_first + [0..4), q column q0 + cq*16 + lr):
//   P^T = exp(S^T + bias + mask - lse[q]);
//   st <- dropped P^T (dV's operand), dpt <- dS^T = P^T o (drop(dP^T) - Di[q])
template <bool HAS_BIAS, bool DROP>
__device__ __forceinline__ void pt_dst_tile(f32x4 (&st)[4], f32x4 (&dpt)[4],
                                            const float* lse, const float* di,
                                            const Src& bias,
                                            const float (&maskv)[4], int64_t bh,
                                            int q0, int kv_first, int L,
                                            const Drop& dr, const Lane& ln) {
#pragma unroll
  for (int cq = 0; cq < 4; ++cq) {
    const int qcol = q0 + cq * 16 + ln.lr;
    const float lse_c = lse[bh * L + qcol];
    const float di_c = di[bh * L + qcol];
    const uint16_t* brow = HAS_BIAS ? bias.row(bh, qcol, L) : nullptr;
    bool keep[4] = {true, true, true, true};
    if (DROP) {
      // this lane's 4 kv rows live in one 8-block of the keep definition
      bool k8[8];
      const int blk = kv_first & ~7;
      keep16x8(dr.seed, (uint64_t)(bh * L + qcol), blk, dr.pthresh, k8);
      const int off = kv_first - blk;
#pragma unroll
      for (int r = 0; r < 4; ++r) keep[r] = k8[off + r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float sv = add_bias_mask<HAS_BIAS, false>(st[cq][r], brow, nullptr,
                                                      kv_first + r) +
                       maskv[r];
      const float pv = p_from_lse(sv, lse_c);
      float dpv = dpt[cq][r];
      if (DROP) dpv = keep[r] ? dpv * dr.pinv : 0.f;
      st[cq][r] = DROP ? (keep[r] ? pv * dr.pinv : 0.f) : pv;
      dpt[cq][r] = pv * (dpv - di_c);
    }
  }
}

// dkv for L <= LRES.  Both transposed operands (Q^T, dO^T) are staged per
// q-tile (8 KB each), ping-pong, rather than keeping dO^T L-resident
// (64 KB): the resident version held the block at 80 KB LDS -> 2 blocks/CU,
// and PMC showed the kernel parked on waits — occupancy was the binding
// constraint.  The P^T/dS^T redistribute buffer is shared sequentially
// (wave-local ordering).
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256, 3) void flash_bwd_dkv_qres_kernel(
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const float* __restrict__ lse, const float* __restrict__ di, Src bias,
    Src mask, int L, Drop dr) {
  const Lane ln = lane_coords(16);
  const int64_t bh = blockIdx.y;
  const int64_t row0 = bh * L + ln.row0;   // this wave's first kv row

  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_dot[2][HD][BM];
  __shared__ __attribute__((aligned(16))) uint16_t lds_qt[2][HD][BM];

  bf16x8 ak[1][2], av[1][2];
  load_a(kp, row0, ln, ak[0]);
  load_a(vp, row0, ln, av[0]);
  float maskv[4];
  load_maskv<HAS_MASK>(mask, bh, ln.row0 + ln.lg * 4, L, maskv);

  f32x4 dk_acc[1][4] = {}, dv_acc[1][4] = {};
  const int n_tiles = L / BM;
  // (T14 prefetch tried and reverted here too: 845 -> 918 us at the
  // 3->2 blocks/CU occupancy cost; see the dq_k32 kernel's note.)
  // ping-pong staging of Q^T/dO^T: tile tq+1 stages into the other
  // buffer while tile tq computes, one barrier per iteration
  auto stage_q = [&](int tile) {
    const int64_t off = (bh * L + tile * BM) * (int64_t)HD;
    stage_transposed(&lds_qt[tile & 1][0][0], BM, 0, qp + off);
    stage_transposed(&lds_dot[tile & 1][0][0], BM, 0, dop + off);
  };
  stage_q(0);
  __syncthreads();
  for (int tq = 0; tq < n_tiles; ++tq) {
    const int q0 = tq * BM;
    if (tq + 1 < n_tiles) stage_q(tq + 1);
    f32x4 st[1][4], dpt[1][4];
    score_tile<1>(ak, qp + (bh * L + q0) * (int64_t)HD, ln, st);
    score_tile<1>(av, dop + (bh * L + q0) * (int64_t)HD, ln, dpt);
    pt_dst_tile<HAS_BIAS, DROP>(st[0], dpt[0], lse, di, bias, maskv, bh, q0,
                                ln.row0 + ln.lg * 4, L, dr, ln);
    // redistribute P^T first (shared buffer, wave-local ordering), read
    // both A-fragments into registers, then reuse the buffer for dS^T
    c_store(lds_t[ln.wid], st[0], ln);
    bf16x8 pta[2][1];
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) pta[ks2][0] = a_load(lds_t[ln.wid], ks2, ln);
    c_store(lds_t[ln.wid], dpt[0], ln);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const bf16x8 dsta[1] = {a_load(lds_t[ln.wid], ks2, ln)};
      mma_staged<1>(pta[ks2], &lds_dot[tq & 1][0][0], BM, ks2 * 32, ln, dv_acc);
      mma_staged<1>(dsta, &lds_qt[tq & 1][0][0], BM, ks2 * 32, ln, dk_acc);
    }
    __syncthreads();
  }
  store_c_tile(dk, row0, dk_acc[0], ln);
  store_c_tile(dv, row0, dv_acc[0], ln);
}

// dkv for L > LRES: Q^T and dO^T staged per q tile between two barriers.
// The tile loop keeps its statements written out and the kernel its loose
// arguments, as in flash_bwd_dq_kernel and for the same reason: built from
// score_tile, pt_dst_tile, c_store / a_load and mma_staged it took 192-196
// VGPRs without dropout where this text takes 148-152.  Lane, Src::row,
// load_maskv, swz and store_c_tile are shared.
template <bool HAS_BIAS, bool HAS_MASK, bool DROP>
__global__ __launch_bounds__(256) void flash_bwd_dkv_kernel(
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const float* __restrict__ lse, const float* __restrict__ di,
    const uint16_t* __restrict__ bias, int64_t bias_nb, int bias_q, int64_t bias_od,
    const uint16_t* __restrict__ mask, int64_t mask_nb, int mask_q, int64_t mask_od,
    int L, float pinv, uint32_t pthresh, uint64_t seed) {
  const Lane ln = lane_coords(16);
  const int64_t bh = blockIdx.y;
  const int wid = ln.wid, lg = ln.lg, lr = ln.lr;
  const int kv0w = ln.row0;   // this wave's first kv row
  const Src bias_src{bias, bias_nb, bias_q, bias_od};
  const Src mask_src{mask, mask_nb, mask_q, mask_od};
  const int64_t kvbase = (bh * L + kv0w) * HD;

  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][2][16][BN];
  // dO and Q tiles transposed [d][q] (swizzled) for the dV / dK products
  __shared__ __attribute__((aligned(16))) uint16_t lds_dot[HD][BM];
  __shared__ __attribute__((aligned(16))) uint16_t lds_qt[HD][BM];
  const int st_q = (int)threadIdx.x >> 2;
  const int st_d0 = ((int)threadIdx.x & 3) * 16;

  bf16x8 ak[2], av[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    ak[ks] = load_frag(kp + kvbase + (int64_t)lr * HD + ks * 32 + lg * 8);
    av[ks] = load_frag(vp + kvbase + (int64_t)lr * HD + ks * 32 + lg * 8);
  }
  float maskv[4];   // additive mask for this wave's kv rows (constant over q)
  load_maskv<HAS_MASK>(mask_src, bh, kv0w + lg * 4, L, maskv);

  f32x4 dk_acc[4] = {}, dv_acc[4] = {};
  const int n_tiles = L / BM;
  for (int tq = 0; tq < n_tiles; ++tq) {
    const int q0 = tq * BM;
    {
      float f0[8], f1[8];
      const int64_t row = (bh * L + q0 + st_q) * (int64_t)HD;
      load8(reinterpret_cast<const __hip_bfloat16*>(dop) + row + st_d0, f0);
      load8(reinterpret_cast<const __hip_bfloat16*>(dop) + row + st_d0 + 8, f1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d0 = st_d0 + j;
        const int d1 = st_d0 + 8 + j;
        lds_dot[d0][swz(d0, st_q)] = f32_to_bf16_bits(f0[j]);
        lds_dot[d1][swz(d1, st_q)] = f32_to_bf16_bits(f1[j]);
      }
      load8(reinterpret_cast<const __hip_bfloat16*>(qp) + row + st_d0, f0);
      load8(reinterpret_cast<const __hip_bfloat16*>(qp) + row + st_d0 + 8, f1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d0 = st_d0 + j;
        const int d1 = st_d0 + 8 + j;
        lds_qt[d0][swz(d0, st_q)] = f32_to_bf16_bits(f0[j]);
        lds_qt[d1][swz(d1, st_q)] = f32_to_bf16_bits(f1[j]);
      }
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
      const int qcol = q0 + cq * 16 + lr;
      f32x4 acc = {}, accd = {};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 bq =
            load_frag(qp + (bh * L + qcol) * (int64_t)HD + ks * 32 + lg * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak[ks], bq, acc, 0, 0, 0);
        const bf16x8 bdo =
            load_frag(dop + (bh * L + qcol) * (int64_t)HD + ks * 32 + lg * 8);
        accd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[ks], bdo, accd, 0, 0, 0);
      }
      st[cq] = acc;
      dpt[cq] = accd;
    }
    // P^T = exp(S^T + bias + mask - lse[q]); dS^T = P^T o (drop(dP^T) - Di[q])
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
      const int qcol = q0 + cq * 16 + lr;
      const float lse_c = lse[bh * L + qcol];
      const float di_c = di[bh * L + qcol];
      const uint16_t* brow = HAS_BIAS ? bias_src.row(bh, qcol, L) : nullptr;
      bool keep[4] = {true, true, true, true};
      if (DROP) {
        // this lane's kv rows kv0w + lg*4 + [0..4) live in one 8-block
        bool k8[8];
        const int blk = (kv0w + lg * 4) & ~7;
        keep16x8(seed, (uint64_t)(bh * L + qcol), blk, pthresh, k8);
        const int off = (kv0w + lg * 4) - blk;
#pragma unroll
        for (int r = 0; r < 4; ++r) keep[r] = k8[off + r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sv = st[cq][r];
        if (HAS_BIAS)
          sv += __bfloat162float(reinterpret_cast<const __hip_bfloat16*>(
              brow)[kv0w + lg * 4 + r]);
        sv += maskv[r];
        const float pv = __expf(sv - lse_c);
        float dpv = dpt[cq][r];
        if (DROP) dpv = keep[r] ? dpv * pinv : 0.f;
        st[cq][r] = DROP ? (keep[r] ? pv * pinv : 0.f) : pv;  // dropped P^T for dV
        dpt[cq][r] = pv * (dpv - di_c);                       // dS^T
      }
    }
    // redistribute P^T(dropped) and dS^T to A layout
#pragma unroll
    for (int cq = 0; cq < 4; ++cq)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lds_t[wid][0][lg * 4 + r][cq * 16 + lr] = f32_to_bf16_bits(st[cq][r]);
        lds_t[wid][1][lg * 4 + r][cq * 16 + lr] = f32_to_bf16_bits(dpt[cq][r]);
      }
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const bf16x8 pta = load_frag(&lds_t[wid][0][lr][ks2 * 32 + lg * 8]);
      const bf16x8 dsta = load_frag(&lds_t[wid][1][lr][ks2 * 32 + lg * 8]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int d = cb * 16 + lr;
        const int qx = swz(d, ks2 * 32 + lg * 8);
        const bf16x8 bdo = load_frag(&lds_dot[d][qx]);
        const bf16x8 bqf = load_frag(&lds_qt[d][qx]);
        dv_acc[cb] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(pta, bdo, dv_acc[cb], 0, 0, 0);
        dk_acc[cb] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsta, bqf, dk_acc[cb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  store_c_tile(dk, bh * L + kv0w, dk_acc, ln);
  store_c_tile(dv, bh * L + kv0w, dv_acc, ln);
}

}  // namespace

std::vector<at::Tensor> flash_attn_backward(
    at::Tensor d_out, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
    at::Tensor lse, std::optional<at::Tensor> bias, int64_t bias_outer_div,
    bool bias_needs_grad, std::optional<at::Tensor> mask, int64_t mask_outer_div,
    double dropout_p, bool dropped, int64_t seed_in) {
  const int L = check_inputs(
      "flash_attn_backward",
      {{"q", &q}, {"k", &k}, {"v", &v}, {"o", &o}, {"d_out", &d_out}});
  const int64_t BH = q.size(0);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == BH && lse.size(1) == L,
              "flash_attn_backward: lse must be contiguous fp32 (", BH, ", ", L,
              "), got ", lse.scalar_type(), " ", lse.sizes());
  const Src bd = describe(bias, bias_outer_div, L, "bias");
  const Src md = describe(mask, mask_outer_div, L, "mask");
  TORCH_CHECK(md.q == 1,
              "flash_attn_backward: mask must broadcast over q, got q = ", md.q);

  const bool drop = dropped && dropout_p > 0.0;
  const Drop dr = make_drop(drop, dropout_p, (uint64_t)seed_in);

  auto stream = at::cuda::getCurrentCUDAStream();
  auto di = at::empty({BH, (int64_t)L}, q.options().dtype(at::kFloat));
  const int64_t n_rows = BH * L;
  flash_dot_do_o_kernel<<<unicore_grid((n_rows + 31) / 32), 256, 0, stream>>>(
      di.data_ptr<float>(), bits(d_out), bits(o), n_rows);

  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  // bias gradient, two strategies:
  //  * short L: materialize dS (BH, L, L) and reduce it over the broadcast
  //    batches — deterministic, and faster than atomics when the broadcast
  //    factor is large (measured: fp32 atomicAdd contention at L=512/B=96
  //    serializes the dq kernel ~4x);
  //  * long L (>= 2048): accumulate dS straight into the (nb, L, L) fp32
  //    buffer with atomics inside the dq kernel — the dS materialization
  //    stops fitting (BH*L*L*2 bytes) while the broadcast factor (and so
  //    the atomic contention) is small. This is what makes a TRAINABLE
  //    pair bias affordable at Uni-Fold-scale sequence lengths.
  // torch.use_deterministic_algorithms() forces the materialized path.
  at::Tensor ds, dbias;
  if (bd.ptr && bias_needs_grad) {
    TORCH_CHECK(bd.q == L, "flash_attn: bias grad requires bias_q == L");
    const bool fuse = L >= 2048 &&
                      !at::globalContext().deterministicAlgorithms();
    if (fuse)
      dbias = at::zeros({bd.nb, (int64_t)bd.q, (int64_t)L},
                        q.options().dtype(at::kFloat));
    else
      ds = at::empty({BH, (int64_t)L, (int64_t)L}, q.options());
  }
  float* dbias_ptr = dbias.defined() ? dbias.data_ptr<float>() : nullptr;
  uint16_t* ds_ptr = ds.defined() ? bits_mut(ds) : nullptr;
  const dim3 grid(L / BM, BH);
  const auto common = std::make_tuple(
      bits(d_out), bits(q), bits(k), bits(v),
      static_cast<const float*>(lse.data_ptr<float>()),
      static_cast<const float*>(di.data_ptr<float>()), bd, md, L, dr);
  // the two tiled kernels take the same values as loose arguments
  const auto loose = std::make_tuple(
      bits(d_out), bits(q), bits(k), bits(v),
      static_cast<const float*>(lse.data_ptr<float>()),
      static_cast<const float*>(di.data_ptr<float>()), bd.ptr, bd.nb, bd.q,
      bd.od, md.ptr, md.nb, md.q, md.od, L, dr.pinv, dr.pthresh, dr.seed);

  dispatch_flags(bd.ptr, md.ptr, drop, [&](auto hb, auto hm, auto dt) {
    constexpr bool HB = decltype(hb)::value;
    constexpr bool HM = decltype(hm)::value;
    constexpr bool DR = decltype(dt)::value;
    if (L <= LRES && L % 128 == 0)
      launch(flash_bwd_dq_k32_kernel<HB, HM, DR>, dim3(L / 128, BH), stream,
             common, bits_mut(dq), ds_ptr);
    else if (L <= LRES)
      launch(flash_bwd_dq_kernel<HB, HM, DR, true>, grid, stream, loose,
             bits_mut(dq), ds_ptr, NoDbiasAcc{});
    else
      launch(flash_bwd_dq_kernel<HB, HM, DR, false>, grid, stream, loose,
             bits_mut(dq), ds_ptr, dbias_ptr);
    if (L <= LRES)
      launch(flash_bwd_dkv_qres_kernel<HB, HM, DR>, grid, stream, common,
             bits_mut(dk), bits_mut(dv));
    else
      launch(flash_bwd_dkv_kernel<HB, HM, DR>, grid, stream, loose,
             bits_mut(dk), bits_mut(dv));
  });

  C10_CUDA_KERNEL_LAUNCH_CHECK();
  if (dbias.defined()) return {dq, dk, dv, dbias};
  if (ds.defined()) {
    // deterministic fallback: reduce the materialized dS over the
    // broadcast axes here (BH rows decompose as (outer, nb, od))
    const int64_t outer = BH / (bd.nb * bd.od);
    auto db = ds.view({outer, bd.nb, bd.od, (int64_t)L, (int64_t)L})
                  .sum(at::IntArrayRef{0, 2}, /*keepdim=*/false, at::kFloat);
    return {dq, dk, dv, db};
  }
  return {dq, dk, dv};
}
