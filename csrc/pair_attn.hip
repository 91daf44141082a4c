// Pair-track attention for Uni-Mol's equivariant head: bf16, head dim 64,
// 64 <= L <= 512, L % 64 == 0.
//
//   logits = bf16(fp32(q k^T) + bias)      returned: the next pair state
//   P      = softmax(logits)               fp32, from the ROUNDED logits
//   o      = (keep * P / (1 - p)) v
//
// q, k, v: (B*H, L, 64), q pre-scaled; bias, logits, d_logits, dbias:
// (B, H, L, L), one row of L keys per (b, h, q).  Unlike flash_attn.hip and
// evo_attn.hip the score matrix is an OUTPUT here and the bias gradient is dS
// itself, so the four (B, H, L, L) tensors are the dominant traffic and the
// kernels are laid out around how they are read and written:
//
//   - forward and dq kernel touch them in the MFMA A layout (lane l -> row
//     l & 15, 8 consecutive keys at (l >> 4) * 8 of each 32-key half): one
//     16 B load or store per lane, a whole 128 B line per row and tile.
//     The fp32 C tile of the product (S, dP) crosses to that layout through
//     a wave-private fp32 LDS tile, so the bias is added in fp32, the sum is
//     rounded once, and softmax, dropout and dS run on A-layout registers
//     that feed the next MFMA with no second LDS trip.  A row's statistics
//     live in the 4 lanes that share l & 15 (two shuffles per reduction).
//   - the dkv kernel needs the tiles transposed.  Element [kv = 4g + r][q]
//     of a transposed C tile is x[q][4g .. 4g+3]: one 8 B load per lane, the
//     four waves of a block together covering the 128 B line of each row.
//     It reads logits and the dbias the dq kernel stored: no dP, no dS.
//
// Backward: P = exp(logits - lse) (no QK^T), dP = dO V^T,
//   dS = bf16(P * (keep / (1-p) * dP - Di) + d_logits) = dbias,
//   dq = dS k, dk = dS^T q, dv = (keep / (1-p) * P)^T dO:  four products.
//
// Keep bits are the flash definition: field kv % 8 of
// philox(seed, bh*L + q, kv / 8), recomputed in backward, never stored.
// Every output element has one owner and one summation order: no atomics.
//
// Padded keys carry finfo(bf16).min in the bias: fp32(s) + min rounds back to
// min, P there is exactly 0 and dS is d_logits alone.  A row whose keys are
// ALL at min is out of contract (docs/KERNELS.md, "Pair-track attention").
//
// Fragment maps (csrc/mfma_probe.hip), v_mfma_f32_16x16x32_bf16:
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
#include "common.h"
#include "dispatch.h"
#include "pair_attn_d8.h"

#include <optional>
#include <type_traits>
#include <vector>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int BM = 64;     // rows per block (q rows; kv rows in dkv)
constexpr int BN = 64;     // columns per tile of the loop
constexpr int HD = 64;     // head dim: two K steps of the MFMA
constexpr int LMAX = 512;  // 64 x 512 bf16 = 64 KB for a resident operand

// The kernels of this file are built without the packed fp32 VALU forms
// (v_pk_add / mul / fma_f32); the feature is a device one, the host pass of
// the compiler does not know it.
#if defined(__HIP_DEVICE_COMPILE__)
#define PAIR_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__
#else
#define PAIR_KERNEL __global__
#endif

union Frag {
  uint4 u;
  bf16x8 v;
  uint16_t h[8];
};

__device__ __forceinline__ bf16x8 load_frag(const uint16_t* p) {
  Frag f;
  f.u = *reinterpret_cast<const uint4*>(p);
  return f.v;
}

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// The runtime headers' __shfl, __shfl_xor and __syncthreads are plain inline
// functions built with the default features; a PAIR_KERNEL cannot inline
// them and would call them.  These are the same operations on the builtins.
__device__ __forceinline__ float lane_read(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float lane_xor(float v, int mask) {
  return lane_read(v, ((int)threadIdx.x & 63) ^ mask);
}

__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// reductions across the 4 lanes that hold one A-layout row (lane bits 4, 5)
__device__ __forceinline__ float arow_max(float v) {
  v = fmaxf(v, lane_xor(v, 16));
  return fmaxf(v, lane_xor(v, 32));
}

__device__ __forceinline__ float arow_sum(float v) {
  v += lane_xor(v, 16);
  return v + lane_xor(v, 32);
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

// dropout scalars; pinv = 1 / (1 - p), pthresh = keep16_threshold(p)
struct Drop {
  float pinv = 1.f;
  uint32_t pthresh = 0;
  uint64_t seed = 0;
};

// A transposed operand in LDS is [d][x], x XOR-swizzled in 8-element blocks
// keyed on d & 7 (the B-fragment reads of 16 d rows at one x range then hit
// distinct banks).  The writer and the reader both go through swz.
__device__ __forceinline__ int swz(int d, int x) { return x ^ ((d & 7) << 3); }

// Stage 64 rows of a (rows, 64) tensor, the first at src, transposed into
// dst[d][col0 + 0..63] (row pitch `pitch`): thread tid moves row tid / 4,
// d = (tid % 4) * 16 + [0..16).
__device__ __forceinline__ void stage_transposed(uint16_t* dst, int pitch,
                                                 int col0,
                                                 const uint16_t* src) {
  const int x = col0 + ((int)threadIdx.x >> 2);
  const int d0 = ((int)threadIdx.x & 3) * 16;
  Frag f[2];
  const uint16_t* row = src + ((int)threadIdx.x >> 2) * HD + d0;
  f[0].u = *reinterpret_cast<const uint4*>(row);
  f[1].u = *reinterpret_cast<const uint4*>(row + 8);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = d0 + i * 8 + j;
      dst[d * pitch + swz(d, x)] = f[i].h[j];
    }
}

// A fragments of 16 rows (the first at global row `row`) of a (rows, 64)
// tensor: lane holds row lr, d = ks*32 + lg*8 + [0..8)
__device__ __forceinline__ void load_a(const uint16_t* base, int64_t row,
                                       const Lane& ln, bf16x8 (&a)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    a[ks] = load_frag(base + (row + ln.lr) * HD + ks * 32 + ln.lg * 8);
}

// c[cb] = A * rows^T for the 64 (rows, 64) rows starting at `row`; the B
// fragments come straight from global rows
__device__ __forceinline__ void score_tile(const bf16x8 (&a)[2],
                                           const uint16_t* base, int64_t row,
                                           const Lane& ln, f32x4 (&c)[4]) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    c[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      c[cb] = mfma(a[ks],
                   load_frag(base + (row + cb * 16 + ln.lr) * HD + ks * 32 +
                             ln.lg * 8),
                   c[cb]);
  }
}

// acc += A * X for one A fragment (16 x 32, k = x .. x+31) against the staged
// transpose X^T[d][x]: the 16 x 64 result is four C tiles
__device__ __forceinline__ void mma_staged(bf16x8 a, const uint16_t* t,
                                           int pitch, int x, const Lane& ln,
                                           f32x4 (&acc)[4]) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int d = cb * 16 + ln.lr;
    acc[cb] = mfma(a, load_frag(t + d * pitch + swz(d, x + ln.lg * 8)), acc[cb]);
  }
}

// fp32 C tile -> A layout through a wave-private 16 x 64 fp32 LDS tile.  A
// row is 64 floats = the 64 banks; the column is XORed with 16 * (row / 4),
// so the four row groups of a C-layout write land in four bank quarters.
// LDS operations of one wave complete in order and no other wave touches the
// tile, so no block barrier is needed; wave_barrier pins the program order.
__device__ __forceinline__ int fswz(int row, int col) {
  return col ^ ((row >> 2 & 3) << 4);
}

__device__ __forceinline__ void c_to_a_f32(float (&t)[16][BN],
                                           const f32x4 (&c)[4], const Lane& ln,
                                           float (&a)[2][8]) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ln.lg * 4 + r;
      t[row][fswz(row, cb * 16 + ln.lr)] = c[cb][r];
    }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const float4* p = reinterpret_cast<const float4*>(
        &t[ln.lr][fswz(ln.lr, ks2 * 32 + ln.lg * 8)]);
    const float4 lo = p[0], hi = p[1];
    a[ks2][0] = lo.x; a[ks2][1] = lo.y; a[ks2][2] = lo.z; a[ks2][3] = lo.w;
    a[ks2][4] = hi.x; a[ks2][5] = hi.y; a[ks2][6] = hi.z; a[ks2][7] = hi.w;
  }
}

// bf16 C tile -> A layout through a wave-private 16 x 64 LDS tile (dkv)
__device__ __forceinline__ void c_to_a_bits(uint16_t (&t)[16][BN],
                                            const uint32_t (&c)[4][4],
                                            const Lane& ln, bf16x8 (&a)[2]) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      t[ln.lg * 4 + r][cb * 16 + ln.lr] = (uint16_t)c[cb][r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2)
    a[ks2] = load_frag(&t[ln.lr][ks2 * 32 + ln.lg * 8]);
}

// the wave's 16 x 64 C tiles to rows row .. row+15 of a (rows, 64) tensor
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
// forward: grid BH * L/64, block = 64 q rows of one (b, h), wave = 16 of them.
// LP >= L is the pitch of the resident V^T (128 / 256 / 512: 32 / 48 / 80 KB
// of LDS with the fp32 tiles).
// ===========================================================================
template <int LP, bool DROP>
PAIR_KERNEL __launch_bounds__(256) void pair_fwd_kernel(
    uint16_t* __restrict__ out, uint16_t* __restrict__ logits,
    float* __restrict__ lse, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const uint16_t* __restrict__ bias, int L, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = L / BM;
  const int64_t bh = blockIdx.x / tiles;
  const int q0 = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int64_t row0 = bh * L + q0;   // this wave's first q row

  __shared__ __attribute__((aligned(16))) float lds_s[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_vt[HD * LP];
  for (int c = 0; c < tiles; ++c)
    stage_transposed(lds_vt, LP, c * 64, vp + (bh * L + c * 64) * (int64_t)HD);
  block_barrier();

  bf16x8 aq[2];
  load_a(qp, row0, ln, aq);
  // the lane's A-layout row of the (B, H, L, L) tensors
  const int64_t big_row = (row0 + ln.lr) * (int64_t)L;
  f32x4 o_acc[4] = {};
  float m_i = -INFINITY, l_i = 0.f;   // of row lr, equal in its 4 lanes

  for (int kv0 = 0; kv0 < L; kv0 += BN) {
    f32x4 s[4];
    score_tile(aq, kp, bh * L + kv0, ln, s);
    float z[2][8];
    c_to_a_f32(lds_s[ln.wid], s, ln, z);
    float mx = -INFINITY;
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int64_t off = big_row + kv0 + ks2 * 32 + ln.lg * 8;
      Frag b, lg_out;
      b.u = *reinterpret_cast<const uint4*>(bias + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        lg_out.h[j] = f32_to_bf16_bits(z[ks2][j] + bf16_bits_to_f32(b.h[j]));
        z[ks2][j] = bf16_bits_to_f32(lg_out.h[j]);
        mx = fmaxf(mx, z[ks2][j]);
      }
      *reinterpret_cast<uint4*>(logits + off) = lg_out.u;
    }
    // online softmax on the rounded logits
    const float mnew = fmaxf(m_i, arow_max(mx));
    const float alpha = __expf(m_i - mnew);
    m_i = mnew;
    float psum = 0.f;
    bf16x8 ap[2];
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      bool keep[8];
      if constexpr (DROP)
        keep16x8(dr.seed, (uint64_t)(row0 + ln.lr), kv0 + ks2 * 32 + ln.lg * 8,
                 dr.pthresh, keep);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = __expf(z[ks2][j] - mnew);
        psum += pv;
        float pd = pv;
        if constexpr (DROP) pd = keep[j] ? pv * dr.pinv : 0.f;
        ap[ks2][j] = (short)f32_to_bf16_bits(pd);
      }
    }
    l_i = l_i * alpha + arow_sum(psum);
    // C row lg*4 + r of o_acc belongs to the lanes with lr = lg*4 + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a_r = lane_read(alpha, ln.lg * 4 + r);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) o_acc[cb][r] *= a_r;
    }
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2)
      mma_staged(ap[ks2], lds_vt, LP, kv0 + ks2 * 32, ln, o_acc);
  }

  const float inv = 1.0f / l_i;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv_r = lane_read(inv, ln.lg * 4 + r);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) o_acc[cb][r] *= inv_r;
  }
  if (ln.lg == 0) lse[row0 + ln.lr] = m_i + __logf(l_i);
  store_c_tile(out, row0, o_acc, ln);
}

// ===========================================================================
// backward
// ===========================================================================

// Di = rowsum(dO o O), fp32: 8 lanes per row of 64
PAIR_KERNEL void pair_dot_do_o_kernel(float* __restrict__ di,
                                     const uint16_t* __restrict__ dop,
                                     const uint16_t* __restrict__ op,
                                     int64_t n_rows) {
  const int el = threadIdx.x & 7;
  for (int64_t row = (int64_t)blockIdx.x * 32 + ((int)threadIdx.x >> 3);
       row < n_rows; row += (int64_t)gridDim.x * 32) {
    float a[8], b[8];
    load8(reinterpret_cast<const __hip_bfloat16*>(dop) + row * HD + el * 8, a);
    load8(reinterpret_cast<const __hip_bfloat16*>(op) + row * HD + el * 8, b);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a[j] * b[j];
    s += lane_xor(s, 1);
    s += lane_xor(s, 2);
    s += lane_xor(s, 4);
    if (el == 0) di[row] = s;
  }
}

// dS = dbias and dQ: grid BH * L/64, wave = 16 q rows, K^T resident, kv loop
// in ascending order without block barriers.  P, keep and dS are A-layout
// registers; dP reaches them through the fp32 tile.
template <int LP, bool DROP, bool HAS_DLOGITS>
PAIR_KERNEL __launch_bounds__(256) void pair_bwd_dq_kernel(
    uint16_t* __restrict__ dq, uint16_t* __restrict__ dbias,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const uint16_t* __restrict__ logits,
    const uint16_t* __restrict__ dlogits, const float* __restrict__ lse,
    const float* __restrict__ di, int L, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = L / BM;
  const int64_t bh = blockIdx.x / tiles;
  const int q0 = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int64_t row0 = bh * L + q0;

  __shared__ __attribute__((aligned(16))) float lds_dp[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_kt[HD * LP];
  for (int c = 0; c < tiles; ++c)
    stage_transposed(lds_kt, LP, c * 64, kp + (bh * L + c * 64) * (int64_t)HD);
  block_barrier();

  bf16x8 ado[2];
  load_a(dop, row0, ln, ado);
  const float lse_row = lse[row0 + ln.lr];
  const float di_row = di[row0 + ln.lr];
  const int64_t big_row = (row0 + ln.lr) * (int64_t)L;

  f32x4 dq_acc[4] = {};
  for (int kv0 = 0; kv0 < L; kv0 += BN) {
    f32x4 dp[4];
    score_tile(ado, vp, bh * L + kv0, ln, dp);
    float dpa[2][8];
    c_to_a_f32(lds_dp[ln.wid], dp, ln, dpa);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int kv = kv0 + ks2 * 32 + ln.lg * 8;
      Frag z, dl, ds;
      z.u = *reinterpret_cast<const uint4*>(logits + big_row + kv);
      if constexpr (HAS_DLOGITS)
        dl.u = *reinterpret_cast<const uint4*>(dlogits + big_row + kv);
      bool keep[8];
      if constexpr (DROP)
        keep16x8(dr.seed, (uint64_t)(row0 + ln.lr), kv, dr.pthresh, keep);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = __expf(bf16_bits_to_f32(z.h[j]) - lse_row);
        float dpv = dpa[ks2][j];
        if constexpr (DROP) dpv = keep[j] ? dpv * dr.pinv : 0.f;
        float dsv = pv * (dpv - di_row);
        if constexpr (HAS_DLOGITS) dsv += bf16_bits_to_f32(dl.h[j]);
        ds.h[j] = f32_to_bf16_bits(dsv);
      }
      *reinterpret_cast<uint4*>(dbias + big_row + kv) = ds.u;
      mma_staged(ds.v, lds_kt, LP, kv0 + ks2 * 32, ln, dq_acc);
    }
  }
  store_c_tile(dq, row0, dq_acc, ln);
}

// dK, dV: grid BH * L/64, wave = 16 kv rows; Q^T and dO^T of one q tile are
// staged ping-pong (tile t+1 while tile t computes, one barrier per
// iteration); the q loop runs in ascending order.  The tiles are transposed:
// lane holds kv rows kv_first + [0..4) of q column q0 + cq*16 + lr, which
// are 4 consecutive bf16 of row q of logits / dbias.
template <bool DROP>
PAIR_KERNEL __launch_bounds__(256) void pair_bwd_dkv_kernel(
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ logits, const uint16_t* __restrict__ dbias,
    const float* __restrict__ lse, int L, Drop dr) {
  const Lane ln = lane_coords();
  const int tiles = L / BM;
  const int64_t bh = blockIdx.x / tiles;
  const int kv0w = ((int)(blockIdx.x % tiles)) * BM + ln.wid * 16;
  const int kv_first = kv0w + ln.lg * 4;
  const int64_t row0 = bh * L + kv0w;   // this wave's first kv row

  // Pd^T, then dS^T, through one buffer (wave-local order)
  __shared__ __attribute__((aligned(16))) uint16_t lds_t[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_qt[2][HD * BM];
  __shared__ __attribute__((aligned(16))) uint16_t lds_dot[2][HD * BM];
  // Q^T and dO^T of q tile `tile` into buffer tile & 1
#define PAIR_STAGE_Q(tile)                                              \
  do {                                                                  \
    const int64_t off = (bh * L + (tile) * BM) * (int64_t)HD;           \
    stage_transposed(lds_qt[(tile) & 1], BM, 0, qp + off);              \
    stage_transposed(lds_dot[(tile) & 1], BM, 0, dop + off);            \
  } while (0)
  PAIR_STAGE_Q(0);
  block_barrier();

  f32x4 dk_acc[4] = {}, dv_acc[4] = {};
  for (int tq = 0; tq < tiles; ++tq) {
    const int q0 = tq * BM;
    if (tq + 1 < tiles) PAIR_STAGE_Q(tq + 1);
    uint32_t pt[4][4], dst[4][4];   // bf16 bits in the low half
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
      const int64_t qrow = bh * L + q0 + cq * 16 + ln.lr;
      const float lse_c = lse[qrow];
      const uint2 z = *reinterpret_cast<const uint2*>(logits + qrow * L + kv_first);
      const uint2 ds = *reinterpret_cast<const uint2*>(dbias + qrow * L + kv_first);
      const uint32_t zb[4] = {z.x & 0xFFFFu, z.x >> 16, z.y & 0xFFFFu, z.y >> 16};
      dst[cq][0] = ds.x & 0xFFFFu;
      dst[cq][1] = ds.x >> 16;
      dst[cq][2] = ds.y & 0xFFFFu;
      dst[cq][3] = ds.y >> 16;
      bool k8[8];
      const bool hi = (kv_first & 4) != 0;   // the lane's 4 keys: one half of
      if constexpr (DROP)                     // the 8-block of the keep bits
        keep16x8(dr.seed, (uint64_t)qrow, kv_first & ~7, dr.pthresh, k8);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = __expf(__builtin_bit_cast(float, zb[r] << 16) - lse_c);
        if constexpr (DROP) pv = (hi ? k8[4 + r] : k8[r]) ? pv * dr.pinv : 0.f;
        pt[cq][r] = f32_to_bf16_bits(pv);
      }
    }
    bf16x8 pta[2], dsta[2];
    c_to_a_bits(lds_t[ln.wid], pt, ln, pta);
    c_to_a_bits(lds_t[ln.wid], dst, ln, dsta);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      mma_staged(pta[ks2], lds_dot[tq & 1], BM, ks2 * 32, ln, dv_acc);
      mma_staged(dsta[ks2], lds_qt[tq & 1], BM, ks2 * 32, ln, dk_acc);
    }
    block_barrier();
  }
  store_c_tile(dk, row0, dk_acc, ln);
  store_c_tile(dv, row0, dv_acc, ln);
#undef PAIR_STAGE_Q
}

// ---- host ------------------------------------------------------------------

constexpr int64_t GRID_MAX = 2147483647LL;

// head dim 8 has the same contract and its own kernels (pair_attn_d8.hip)
constexpr int HD8 = 8;

const char* shape_problem(int64_t L, int64_t D) {
  if (D != HD && D != HD8) return "head dim must be 64 or 8";
  if (L < 64 || L > LMAX || L % 64 != 0)
    return "L must be a multiple of 64 in [64, 512]";
  return nullptr;
}

bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

void check_tensor(const char* fn, const char* name, const at::Tensor& t,
                  int64_t rank) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be on the GPU, got device ",
              t.device());
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == rank, fn, ": ", name, " must have rank ", rank,
              ", got sizes ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name,
              " must be contiguous, got sizes ", t.sizes(), " strides ",
              t.strides());
  TORCH_CHECK(aligned16(t), fn, ": ", name, " must be 16 B aligned, got ",
              t.data_ptr());
}

// q first: every operand is (BH, L, D) like it
void check_operands(
    const char* fn,
    std::initializer_list<std::pair<const char*, const at::Tensor*>> operands) {
  const at::Tensor& q = *operands.begin()->second;
  for (const auto& [name, t] : operands) {
    check_tensor(fn, name, *t, 3);
    TORCH_CHECK(t->sizes() == q.sizes(), fn, ": ", name, " has shape ",
                t->sizes(), ", q has ", q.sizes());
  }
  const char* problem = shape_problem(q.size(1), q.size(2));
  TORCH_CHECK(problem == nullptr, fn, ": ", problem, ", got q ", q.sizes());
  TORCH_CHECK(q.size(0) >= 1 && q.size(0) * (q.size(1) / BM) <= GRID_MAX, fn,
              ": B*H * L / 64 must fit the grid, got B*H = ", q.size(0));
}

// bias, logits, d_logits: (B, H, L, L) with B*H the batch of q
void check_pair(const char* fn, const char* name, const at::Tensor& t,
                const at::Tensor& q) {
  check_tensor(fn, name, t, 4);
  const int64_t L = q.size(1);
  TORCH_CHECK(t.size(2) == L && t.size(3) == L, fn, ": ", name,
              " must be (B, H, L = ", L, ", L), got ", t.sizes());
  TORCH_CHECK(t.size(0) * t.size(1) == q.size(0), fn, ": ", name, " has B*H = ",
              t.size(0), " * ", t.size(1), ", q has ", q.size(0));
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

// f(LP, flags...): LP the resident pitch as std::integral_constant, each flag
// as std::bool_constant
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
template <class F, class... Flags>
void dispatch_pitch(int L, F&& f, Flags... flags) {
  if (L <= 128)
    dispatch_flags(
        [&](auto... fs) { f(std::integral_constant<int, 128>{}, fs...); },
        flags...);
  else if (L <= 256)
    dispatch_flags(
        [&](auto... fs) { f(std::integral_constant<int, 256>{}, fs...); },
        flags...);
  else
    dispatch_flags(
        [&](auto... fs) { f(std::integral_constant<int, LMAX>{}, fs...); },
        flags...);
}

const uint16_t* bits(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bits_mut(at::Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}

}  // namespace

bool pair_attn_supported(int64_t L, int64_t D, bool is_bf16) {
  return is_bf16 && shape_problem(L, D) == nullptr;
}

// q, k, v: (B*H, L, D) contiguous bf16, D 64 or 8, q pre-scaled; bias
// (B, H, L, L) -> (o, logits, lse, seed)
std::vector<at::Tensor> pair_attn_forward(at::Tensor q, at::Tensor k,
                                          at::Tensor v, at::Tensor bias,
                                          double dropout_p, bool is_training) {
  const char* fn = "pair_attn_forward";
  check_operands(fn, {{"q", &q}, {"k", &k}, {"v", &v}});
  check_pair(fn, "bias", bias, q);
  const int64_t BH = q.size(0);
  const int L = (int)q.size(1);

  const bool drop = is_training && dropout_p > 0.0;
  Drop dr = make_drop(fn, drop, dropout_p, 0);
  // a row draws Philox counters 0 .. L/8 - 1 of its own subsequence; the
  // offset is folded into the key, which forward and backward both use
  const uint64_t seed = drop ? reserve_philox_key(L / 8 + 4) : 0;
  dr.seed = seed;

  auto o = at::empty_like(q);
  auto logits = at::empty_like(bias);
  auto lse = at::empty({BH, (int64_t)L}, q.options().dtype(at::kFloat));
  const at::Tensor seed_t =
      at::scalar_tensor((int64_t)seed, at::TensorOptions().dtype(at::kLong));
  if (q.size(2) == HD8) {
    pair8_forward_launch(o, logits, lse, q, k, v, bias,
                         Pair8Drop{drop, dr.pinv, dr.pthresh, dr.seed});
    return {o, logits, lse, seed_t};
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)(BH * (L / BM)));
  dispatch_pitch(
      L,
      [&](auto lp, auto dt) {
        pair_fwd_kernel<decltype(lp)::value, decltype(dt)::value>
            <<<grid, 256, 0, stream>>>(bits_mut(o), bits_mut(logits),
                                       lse.data_ptr<float>(), bits(q), bits(k),
                                       bits(v), bits(bias), L, dr);
      },
      drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  // the seed is host state: a CPU scalar costs the wrapper no sync
  return {o, logits, lse, seed_t};
}

// -> (dq, dk, dv, dbias); d_logits is the gradient arriving at the returned
// logits, or absent
std::vector<at::Tensor> pair_attn_backward(
    at::Tensor d_out, std::optional<at::Tensor> d_logits, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse, at::Tensor logits,
    double dropout_p, bool dropped, int64_t seed_in) {
  const char* fn = "pair_attn_backward";
  check_operands(fn,
                 {{"q", &q}, {"k", &k}, {"v", &v}, {"o", &o}, {"d_out", &d_out}});
  check_pair(fn, "logits", logits, q);
  const bool has_dl = d_logits.has_value() && d_logits->defined();
  if (has_dl) {
    check_pair(fn, "d_logits", *d_logits, q);
    TORCH_CHECK(d_logits->sizes() == logits.sizes(), fn, ": d_logits has shape ",
                d_logits->sizes(), ", logits has ", logits.sizes());
  }
  const int64_t BH = q.size(0);
  const int L = (int)q.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == BH && lse.size(1) == L,
              fn, ": lse must be contiguous fp32 (", BH, ", ", L, "), got ",
              lse.scalar_type(), " ", lse.sizes());
  const bool drop = dropped && dropout_p > 0.0;
  const Drop dr = make_drop(fn, drop, dropout_p, (uint64_t)seed_in);

  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto dbias = at::empty_like(logits);
  if (q.size(2) == HD8) {
    pair8_backward_launch(dq, dk, dv, dbias, d_out,
                          has_dl ? &*d_logits : nullptr, q, k, v, o, lse,
                          logits, Pair8Drop{drop, dr.pinv, dr.pthresh, dr.seed});
    return {dq, dk, dv, dbias};
  }

  auto stream = at::cuda::getCurrentCUDAStream();
  auto di = at::empty({BH, (int64_t)L}, q.options().dtype(at::kFloat));
  const int64_t n_rows = BH * L;
  pair_dot_do_o_kernel<<<unicore_grid((n_rows + 31) / 32), 256, 0, stream>>>(
      di.data_ptr<float>(), bits(d_out), bits(o), n_rows);

  const float* lse_p = lse.data_ptr<float>();
  const uint16_t* dl_p = has_dl ? bits(*d_logits) : nullptr;
  const dim3 grid((unsigned)(BH * (L / BM)));
  dispatch_pitch(
      L,
      [&](auto lp, auto dt, auto hd) {
        pair_bwd_dq_kernel<decltype(lp)::value, decltype(dt)::value,
                           decltype(hd)::value><<<grid, 256, 0, stream>>>(
            bits_mut(dq), bits_mut(dbias), bits(d_out), bits(k), bits(v),
            bits(logits), dl_p, lse_p, di.data_ptr<float>(), L, dr);
      },
      drop, has_dl);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  // after the dq kernel on the same stream: it reads the dbias stored there
  dispatch_flags(
      [&](auto dt) {
        pair_bwd_dkv_kernel<decltype(dt)::value><<<grid, 256, 0, stream>>>(
            bits_mut(dk), bits_mut(dv), bits(d_out), bits(q), bits(logits),
            bits(dbias), lse_p, L, dr);
      },
      drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {dq, dk, dv, dbias};
}
