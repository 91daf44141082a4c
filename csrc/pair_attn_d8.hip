// Pair-track attention at head dim 8 (Uni-Mol's 64-head shape): bf16,
// 64 <= L <= 512, L % 64 == 0.  Same mathematical contract as pair_attn.hip:
//
//   logits = bf16(fp32(q k^T) + bias)      returned: the next pair state
//   P      = softmax(logits)               fp32, from the ROUNDED logits
//   o      = (keep * P / (1 - p)) v
//   dS     = bf16(P * (keep / (1-p) * dP - Di) + d_logits) = dbias
//   dq = dS k, dk = dS^T q, dv = (keep / (1-p) * P)^T dO
//
// q, k, v: (B*H, L, 8): one row is 16 B, a whole head at L 512 is 8 KB.  The
// (B, H, L, L) tensors are 64 / D = 8 times heavier relative to the products
// than at head dim 64, so the kernels are laid out to touch each of them as
// few times as possible, always as 16 B per lane in the MFMA A layout (lane
// l -> row l & 15, 8 consecutive keys at (l >> 4) * 8 of a 32-key half):
//
//   forward   bias in, logits out                          2 passes
//   backward  logits, d_logits in, dbias out, ONE kernel   3 passes
//
// Products run on v_mfma_f32_16x16x32_bf16 with the operand zero-padded:
//   - q k^T and dP = dO v^T have K = head dim: lanes 0-15 (k-group 0) carry
//     a row's 16 B, lanes 16-63 carry zeros;
//   - P v, dS k, dS^T q and Pd^T dO have K = kv or q (full 32-deep steps)
//     and N = 8 padded to 16: B lanes with column >= 8 carry zeros, the
//     matching C columns are never stored.
//
// Backward, one block per (b, h): V, dO, K^T, Q^T, dO^T of the head are
// resident in LDS.  Outer loop over kv tiles of 64, inner loop over q tiles
// of 64.  A wave takes 16 q rows: dP crosses from the C to the A layout
// through the wave's fp32 LDS tile, dS is formed in fp32, rounded once,
// stored as dbias and multiplied into that q tile's dq accumulator (one C
// tile per q tile, L / 64 <= 8 of them live in registers across the whole
// loop).  The bf16 dS and dropped-P rows are WRITTEN TRANSPOSED ([kv][q],
// XOR-swizzled) into two block-shared 64 x 64 tiles; after a barrier each
// wave takes 16 kv rows and reads its A fragments of dS^T / Pd^T with 16 B
// reads for dk += dS^T q_tile, dv += Pd^T dO_tile.  dk / dv are complete
// when the inner loop ends; dq after the outer loop.
//
// Keep bits: field kv % 8 of philox(seed, bh*L + q, kv / 8), recomputed in
// backward.  One owner and one summation order per output element: no
// atomics.  Padded keys at finfo(bf16).min: P is exactly 0, dS is d_logits.
//
// Fragment maps (csrc/mfma_probe.hip), v_mfma_f32_16x16x32_bf16:
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
#include "pair_attn_d8.h"

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAException.h>

#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int BM = 64;     // q rows per tile
constexpr int BN = 64;     // kv columns per tile
constexpr int HD = 8;      // head dim: one 16 B row
constexpr int LMAX = 512;

// built without the packed fp32 VALU forms, as pair_attn.hip
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

// the builtins behind __shfl / __syncthreads: a PAIR_KERNEL cannot inline the
// runtime headers' versions (pair_attn.hip)
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

struct Lane {
  int wid, lg, lr;
};

__device__ __forceinline__ Lane lane_coords() {
  const int lane = threadIdx.x & 63;
  return {(int)threadIdx.x >> 6, lane >> 4, lane & 15};
}

struct Drop {
  float pinv;
  uint32_t pthresh;
  uint64_t seed;
};

// The zero padding of the operands.  The load itself is done by every lane
// (its address is valid for all of them), the select drops it.
// K = head dim: only k-group 0 carries data
__device__ __forceinline__ bf16x8 k_group0(const Lane& ln, bf16x8 f) {
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  return ln.lg == 0 ? f : zero;
}
// N = head dim: only columns 0..7 carry data
__device__ __forceinline__ bf16x8 cols_lt8(const Lane& ln, bf16x8 f) {
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  return ln.lr < HD ? f : zero;
}

// A transposed (L, 8) operand in LDS is [d][x], x XOR-swizzled in 8-element
// blocks keyed on d: the B-fragment read of the 8 d rows at one x range hits
// 8 distinct 16 B blocks.  Writer and reader both go through swz.
__device__ __forceinline__ int swz(int d, int x) { return x ^ ((d & 7) << 3); }

// B fragment of X (k = x .. x+31, col d) from the staged transpose X^T[d][x]
__device__ __forceinline__ bf16x8 load_b_t(const uint16_t* t, int pitch, int x,
                                           const Lane& ln) {
  const int d = ln.lr & 7;
  return cols_lt8(ln, load_frag(t + d * pitch + swz(d, x + ln.lg * 8)));
}

__device__ __forceinline__ void scatter_row(uint16_t* t, int pitch, int x,
                                            const Frag& f) {
#pragma unroll
  for (int d = 0; d < HD; ++d) t[d * pitch + swz(d, x)] = f.h[d];
}

// The block-shared dS^T / Pd^T tiles are [kv][q], written 2 B at a time from
// A-layout registers (lane: q = wid*16 + lr, kv = ks2*32 + lg*8 + j) and
// read as A fragments (lane: kv = wid*16 + lr, q = ks*32 + lg*8 + [0..8)).
// q is XORed in 8-blocks with kv & 7 (the 8 rows of a read pass hit distinct
// 16 B blocks) and in 16-blocks with kv >> 3 (the four lg groups of a write,
// 8 rows apart, land in four bank quarters).
__device__ __forceinline__ int tswz(int kv, int q) {
  return q ^ ((kv & 7) << 3) ^ ((kv >> 3 & 3) << 4);
}

// fp32 C tile -> A layout through a wave-private 16 x 64 fp32 LDS tile, as
// pair_attn.hip: LDS operations of one wave complete in order and no other
// wave touches the tile, so no block barrier is needed.
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

// columns 0..7 of the wave's C tile to rows row .. row+15 of a (rows, 8)
// tensor: 8 lanes cover a row's 16 B
__device__ __forceinline__ void store_c_tile(uint16_t* dst, int64_t row,
                                             const f32x4& acc, const Lane& ln) {
  if (ln.lr < HD) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dst[(row + ln.lg * 4 + r) * (int64_t)HD + ln.lr] =
          f32_to_bf16_bits(acc[r]);
  }
}

// ===========================================================================
// forward: grid BH * L/64, block = 64 q rows of one (b, h), wave = 16 of them.
// K and V^T of the head are resident (16 KB at the LMAX pitch); with the
// four fp32 crossing tiles the block holds 32 KB whatever L is, so there is
// no pitch template.
// ===========================================================================
template <bool DROP>
PAIR_KERNEL __launch_bounds__(256) void pair8_fwd_kernel(
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
  __shared__ __attribute__((aligned(16))) uint16_t lds_k[LMAX * HD];
  __shared__ __attribute__((aligned(16))) uint16_t lds_vt[HD * LMAX];
  for (int x = threadIdx.x; x < L; x += 256) {
    const int64_t src = (bh * L + x) * (int64_t)HD;
    *reinterpret_cast<uint4*>(&lds_k[x * HD]) =
        *reinterpret_cast<const uint4*>(kp + src);
    Frag f;
    f.u = *reinterpret_cast<const uint4*>(vp + src);
    scatter_row(lds_vt, LMAX, x, f);
  }
  block_barrier();

  const bf16x8 aq = k_group0(ln, load_frag(qp + (row0 + ln.lr) * (int64_t)HD));
  // the lane's A-layout row of the (B, H, L, L) tensors
  const int64_t big_row = (row0 + ln.lr) * (int64_t)L;
  f32x4 o_acc = {0.f, 0.f, 0.f, 0.f};
  float m_i = -INFINITY, l_i = 0.f;   // of row lr, equal in its 4 lanes

  for (int kv0 = 0; kv0 < L; kv0 += BN) {
    f32x4 s[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      s[cb] = mfma(aq,
                   k_group0(ln, load_frag(&lds_k[(kv0 + cb * 16 + ln.lr) * HD])),
                   f32x4{0.f, 0.f, 0.f, 0.f});
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
    for (int r = 0; r < 4; ++r)
      o_acc[r] *= lane_read(alpha, ln.lg * 4 + r);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2)
      o_acc = mfma(ap[ks2], load_b_t(lds_vt, LMAX, kv0 + ks2 * 32, ln), o_acc);
  }

  const float inv = 1.0f / l_i;
#pragma unroll
  for (int r = 0; r < 4; ++r) o_acc[r] *= lane_read(inv, ln.lg * 4 + r);
  if (ln.lg == 0) lse[row0 + ln.lr] = m_i + __logf(l_i);
  store_c_tile(out, row0, o_acc, ln);
}

// ===========================================================================
// backward
// ===========================================================================

// Di = rowsum(dO o O), fp32: a row is one 16 B load of each, one thread
PAIR_KERNEL void pair8_dot_do_o_kernel(float* __restrict__ di,
                                      const uint16_t* __restrict__ dop,
                                      const uint16_t* __restrict__ op,
                                      int64_t n_rows) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + (int)threadIdx.x; row < n_rows;
       row += (int64_t)gridDim.x * 256) {
    Frag a, b;
    a.u = *reinterpret_cast<const uint4*>(dop + row * HD);
    b.u = *reinterpret_cast<const uint4*>(op + row * HD);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s += bf16_bits_to_f32(a.h[j]) * bf16_bits_to_f32(b.h[j]);
    di[row] = s;
  }
}

// dS = dbias, dq, dk, dv in one pass: grid BH, one block per (b, h).  LP >= L
// is the pitch of the five resident operands (5 * 16 * LP bytes) and fixes
// the number of dq accumulators, LP / 64, whose indexing is fully unrolled.
template <int LP, bool DROP, bool HAS_DLOGITS>
PAIR_KERNEL __launch_bounds__(256) void pair8_bwd_kernel(
    uint16_t* __restrict__ dq, uint16_t* __restrict__ dk,
    uint16_t* __restrict__ dv, uint16_t* __restrict__ dbias,
    const uint16_t* __restrict__ dop, const uint16_t* __restrict__ qp,
    const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const uint16_t* __restrict__ logits, const uint16_t* __restrict__ dlogits,
    const float* __restrict__ lse, const float* __restrict__ di, int L,
    Drop dr) {
  const Lane ln = lane_coords();
  const int64_t head_row = (int64_t)blockIdx.x * L;   // first row of (b, h)

  __shared__ __attribute__((aligned(16))) float lds_dp[4][16][BN];
  __shared__ __attribute__((aligned(16))) uint16_t lds_ds[BN][BM];   // [kv][q]
  __shared__ __attribute__((aligned(16))) uint16_t lds_pd[BN][BM];
  __shared__ __attribute__((aligned(16))) uint16_t lds_v[LP * HD];
  __shared__ __attribute__((aligned(16))) uint16_t lds_do[LP * HD];
  __shared__ __attribute__((aligned(16))) uint16_t lds_kt[HD * LP];
  __shared__ __attribute__((aligned(16))) uint16_t lds_qt[HD * LP];
  __shared__ __attribute__((aligned(16))) uint16_t lds_dot[HD * LP];
  for (int x = threadIdx.x; x < L; x += 256) {
    const int64_t src = (head_row + x) * (int64_t)HD;
    Frag f;
    f.u = *reinterpret_cast<const uint4*>(vp + src);
    *reinterpret_cast<uint4*>(&lds_v[x * HD]) = f.u;
    f.u = *reinterpret_cast<const uint4*>(dop + src);
    *reinterpret_cast<uint4*>(&lds_do[x * HD]) = f.u;
    scatter_row(lds_dot, LP, x, f);
    f.u = *reinterpret_cast<const uint4*>(kp + src);
    scatter_row(lds_kt, LP, x, f);
    f.u = *reinterpret_cast<const uint4*>(qp + src);
    scatter_row(lds_qt, LP, x, f);
  }
  block_barrier();

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int qt = ln.wid * 16 + ln.lr;   // the lane's row of a tile, both roles
  f32x4 dq_acc[LP / BM];
#pragma unroll
  for (int tq = 0; tq < LP / BM; ++tq) dq_acc[tq] = zero4;

  for (int kv0 = 0; kv0 < L; kv0 += BN) {
    bf16x8 bv[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      bv[cb] = k_group0(ln, load_frag(&lds_v[(kv0 + cb * 16 + ln.lr) * HD]));
    f32x4 dk_acc = zero4, dv_acc = zero4;

#pragma unroll
    for (int tq = 0; tq < LP / BM; ++tq) {
      if (tq * BM < L) {   // uniform over the block: the barriers are safe
        // ---- wave = 16 q rows: dP, dS = dbias, dq ----
        // What is loaded through the q row (dO fragment, lse, Di, the row
        // offsets) is invariant in the kv loop; hoisted out of it for all
        // LP / 64 q tiles it costs up to 130 VGPRs.  The row is made opaque
        // here so that it is reloaded (LDS and cache hits) instead.
        int qt_v = qt;
        asm volatile("" : "+v"(qt_v));
        const int64_t qrow = head_row + tq * BM + qt_v;
        const bf16x8 ado =
            k_group0(ln, load_frag(&lds_do[(tq * BM + qt_v) * HD]));
        f32x4 dp[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) dp[cb] = mfma(ado, bv[cb], zero4);
        float dpa[2][8];
        c_to_a_f32(lds_dp[ln.wid], dp, ln, dpa);
        const float lse_row = lse[qrow];
        const float di_row = di[qrow];
        const int64_t big_row = qrow * (int64_t)L;
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          const int kvt = ks2 * 32 + ln.lg * 8;   // within the tile
          const int kv = kv0 + kvt;
          Frag z, dl, ds, pd;
          z.u = *reinterpret_cast<const uint4*>(logits + big_row + kv);
          if constexpr (HAS_DLOGITS)
            dl.u = *reinterpret_cast<const uint4*>(dlogits + big_row + kv);
          bool keep[8];
          if constexpr (DROP)
            keep16x8(dr.seed, (uint64_t)qrow, kv, dr.pthresh, keep);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float pv = __expf(bf16_bits_to_f32(z.h[j]) - lse_row);
            float pdv = pv, dpv = dpa[ks2][j];
            if constexpr (DROP) {
              pdv = keep[j] ? pv * dr.pinv : 0.f;
              dpv = keep[j] ? dpv * dr.pinv : 0.f;
            }
            float dsv = pv * (dpv - di_row);
            if constexpr (HAS_DLOGITS) dsv += bf16_bits_to_f32(dl.h[j]);
            ds.h[j] = f32_to_bf16_bits(dsv);
            pd.h[j] = f32_to_bf16_bits(pdv);
            lds_ds[kvt + j][tswz(kvt + j, qt_v)] = ds.h[j];
            lds_pd[kvt + j][tswz(kvt + j, qt_v)] = pd.h[j];
          }
          *reinterpret_cast<uint4*>(dbias + big_row + kv) = ds.u;
          dq_acc[tq] = mfma(ds.v, load_b_t(lds_kt, LP, kv0 + ks2 * 32, ln),
                            dq_acc[tq]);
        }
        block_barrier();
        // ---- wave = 16 kv rows: dk += dS^T q_tile, dv += Pd^T dO_tile ----
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int qc = ks * 32 + ln.lg * 8;
          const bf16x8 a_ds = load_frag(&lds_ds[qt][tswz(qt, qc)]);
          const bf16x8 a_pd = load_frag(&lds_pd[qt][tswz(qt, qc)]);
          dk_acc = mfma(a_ds, load_b_t(lds_qt, LP, tq * BM + ks * 32, ln), dk_acc);
          dv_acc = mfma(a_pd, load_b_t(lds_dot, LP, tq * BM + ks * 32, ln), dv_acc);
        }
        block_barrier();   // the tiles are rewritten by the next q tile
      }
    }
    store_c_tile(dk, head_row + kv0 + ln.wid * 16, dk_acc, ln);
    store_c_tile(dv, head_row + kv0 + ln.wid * 16, dv_acc, ln);
  }
#pragma unroll
  for (int tq = 0; tq < LP / BM; ++tq)
    if (tq * BM < L)
      store_c_tile(dq, head_row + tq * BM + ln.wid * 16, dq_acc[tq], ln);
}

// ---- host ------------------------------------------------------------------

const uint16_t* bits(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bits_mut(at::Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}

// f(flags...): each flag as std::bool_constant
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

}  // namespace

void pair8_forward_launch(at::Tensor& o, at::Tensor& logits, at::Tensor& lse,
                          const at::Tensor& q, const at::Tensor& k,
                          const at::Tensor& v, const at::Tensor& bias,
                          const Pair8Drop& pd) {
  TORCH_INTERNAL_ASSERT(q.size(2) == HD && q.size(1) % BM == 0 &&
                        q.size(1) >= BM && q.size(1) <= LMAX);
  const int64_t BH = q.size(0);
  const int L = (int)q.size(1);
  const Drop dr{pd.pinv, pd.pthresh, pd.seed};
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)(BH * (L / BM)));
  dispatch_flags(
      [&](auto dt) {
        pair8_fwd_kernel<decltype(dt)::value><<<grid, 256, 0, stream>>>(
            bits_mut(o), bits_mut(logits), lse.data_ptr<float>(), bits(q),
            bits(k), bits(v), bits(bias), L, dr);
      },
      pd.drop);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void pair8_backward_launch(at::Tensor& dq, at::Tensor& dk, at::Tensor& dv,
                           at::Tensor& dbias, const at::Tensor& d_out,
                           const at::Tensor* d_logits, const at::Tensor& q,
                           const at::Tensor& k, const at::Tensor& v,
                           const at::Tensor& o, const at::Tensor& lse,
                           const at::Tensor& logits, const Pair8Drop& pd) {
  TORCH_INTERNAL_ASSERT(q.size(2) == HD && q.size(1) % BM == 0 &&
                        q.size(1) >= BM && q.size(1) <= LMAX);
  const int64_t BH = q.size(0);
  const int L = (int)q.size(1);
  const Drop dr{pd.pinv, pd.pthresh, pd.seed};
  auto stream = at::cuda::getCurrentCUDAStream();
  auto di = at::empty({BH, (int64_t)L}, q.options().dtype(at::kFloat));
  const int64_t n_rows = BH * L;
  pair8_dot_do_o_kernel<<<unicore_grid((n_rows + 255) / 256), 256, 0, stream>>>(
      di.data_ptr<float>(), bits(d_out), bits(o), n_rows);
  C10_CUDA_KERNEL_LAUNCH_CHECK();

  const uint16_t* dl_p = d_logits ? bits(*d_logits) : nullptr;
  const dim3 grid((unsigned)BH);
  auto launch = [&](auto lp, auto dt, auto hd) {
    pair8_bwd_kernel<decltype(lp)::value, decltype(dt)::value,
                     decltype(hd)::value><<<grid, 256, 0, stream>>>(
        bits_mut(dq), bits_mut(dk), bits_mut(dv), bits_mut(dbias), bits(d_out),
        bits(q), bits(k), bits(v), bits(logits), dl_p, lse.data_ptr<float>(),
        di.data_ptr<float>(), L, dr);
  };
  if (L <= 128)
    dispatch_flags(
        [&](auto... fs) { launch(std::integral_constant<int, 128>{}, fs...); },
        pd.drop, d_logits != nullptr);
  else if (L <= 256)
    dispatch_flags(
        [&](auto... fs) { launch(std::integral_constant<int, 256>{}, fs...); },
        pd.drop, d_logits != nullptr);
  else
    dispatch_flags(
        [&](auto... fs) { launch(std::integral_constant<int, LMAX>{}, fs...); },
        pd.drop, d_logits != nullptr);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}
