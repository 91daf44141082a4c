// Channel-last triangle contraction for gfx950 (CDNA4 MFMA), bf16.
//
//   O[b, x, y, c] = sum_z A[b, x, z, c] * B[b, y, z, c]
//
// A is (Bt, X, Z, C) with element strides (sAb, sAx, sAz, 1), B is
// (Bt, Y, Z, C) with (sBb, sBy, sBz, 1), O is fresh contiguous
// (Bt, X, Y, C).  The two spatial strides are free, so transpose(1, 2)
// views are consumed in place: this one primitive is both Evoformer
// triangle-multiplication directions and all four of their gradient
// contractions (unicore_amd/modules/triangle.py holds the table).
// Every channel is an independent X x Z by Z x Y GEMM; the library route
// permute-copies to channel-first, runs Bt*C small batched GEMMs and
// permute-copies back.
//
// Geometry: 256 threads (4 wave64) per block; a block owns a 32 x 32 (x, y)
// output tile for a chunk of CC = 16 channels and walks z in steps of 32.
// Each wave owns 4 channels of the chunk: 2 x 2 tiles of
// v_mfma_f32_16x16x32_bf16 per channel (fragment maps verified by
// csrc/mfma_probe.hip):
//   A (16x32): lane l -> row l&15,  k (l>>4)*8+[0..8)
//   B (32x16): lane l -> col l&15,  k (l>>4)*8+[0..8)
//   C (16x16): lane l -> col l&15,  rows (l>>4)*4+[0..4)
// with the A rows = x, B cols = y, k = z.
//
// Staging: a thread loads 8 consecutive z of one (row, 8-channel group) as
// eight 16 B global loads along c, transposes the 8x8 block in registers
// and writes one 16 B LDS slot per channel.  LDS image per operand is
// [c 16][zgroup 4][row 32] slots of 16 B (8 consecutive z), so a lane's
// MFMA fragment is exactly one ds_read_b128.  The 16 lanes of every
// ds_read_b128 lane group carry 16 distinct rows (mod 16), hence 16
// distinct slots of the 256 B bank row: conflict-free without padding.
// Rows are XORed with 4 for the upper channel half so the two halves of a
// writing lane pair land on different banks.  The next z-step's global
// loads are issued before the MFMA phase and stay in flight across it.
//
// Out-of-range z and rows are zero-filled in LDS (exact); out-of-range
// (x, y) are predicated at the store.  Accumulation is fp32 in fixed z
// order inside one block: no atomics, no split-Z, one rounding to bf16
// per output element, bitwise reproducible.
//
// Epilogue: the C fragments (one y, four x per lane) go back through LDS
// as [x][y][c 16 + pad] bf16 (a wave packs its 4 channels into one 8 B
// write), then every thread stores 16 B along c.
#include "common.h"

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

constexpr int TT = 32;                    // x and y tile edge
constexpr int ZS = 32;                    // z per step (one MFMA k)
constexpr int CC = 16;                    // channels per block
constexpr int OPER_SLOTS = CC * 4 * TT;   // 16 B slots per operand image
constexpr int OROW = 24;                  // epilogue (x, y) pitch in bf16 (48 B)

// 8 consecutive z of one (row, 8-channel group); zero outside the tensor
__device__ __forceinline__ void tri_load(uint4 (&r)[8], const uint16_t* p,
                                         int64_t s_z, bool row_ok, int zb,
                                         int Z) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (row_ok && zb + j < Z)
      r[j] = *reinterpret_cast<const uint4*>(p + (int64_t)(zb + j) * s_z);
    else
      r[j] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// r[j] = 8 channels at z = j  ->  one slot per channel holding z = 0..7
__device__ __forceinline__ void tri_stage(uint4* s, const uint4 (&r)[8],
                                          int chalf, int g, int row) {
  uint32_t in[8][4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    in[j][0] = r[j].x;
    in[j][1] = r[j].y;
    in[j][2] = r[j].z;
    in[j][3] = r[j].w;
  }
  const int prow = row ^ (chalf << 2);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t e = in[2 * p][w], o = in[2 * p + 1][w];
      lo[p] = (e & 0xFFFFu) | (o << 16);
      hi[p] = (e >> 16) | (o & 0xFFFF0000u);
    }
    const int c = chalf * 8 + 2 * w;
    s[(c * 4 + g) * TT + prow] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    s[((c + 1) * 4 + g) * TT + prow] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  }
}

__device__ __forceinline__ bf16x8 tri_frag(const uint4* p) {
  union {
    uint4 u;
    bf16x8 v;
  } U;
  U.u = *p;
  return U.v;
}

__global__ __launch_bounds__(256) void tri_contract_kernel(
    uint16_t* __restrict__ O, const uint16_t* __restrict__ A,
    const uint16_t* __restrict__ B, int X, int Y, int Z, int C, int64_t sAb,
    int64_t sAx, int64_t sAz, int64_t sBb, int64_t sBy, int64_t sBz, int nxt,
    int nyt, int ncc) {
  __shared__ uint4 smem[2 * OPER_SLOTS];  // 64 KB: A image, B image
  uint4* sA = smem;
  uint4* sB = smem + OPER_SLOTS;

  // channel chunk fastest, then y tile, x tile, batch
  int bid = blockIdx.x;
  const int c0 = (bid % ncc) * CC;
  bid /= ncc;
  const int y0 = (bid % nyt) * TT;
  bid /= nyt;
  const int x0 = (bid % nxt) * TT;
  const int64_t bt = bid / nxt;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lr = lane & 15;
  const int lg = lane >> 4;

  // staging role: (8-channel half, tile row, z group)
  const int st_ch = tid & 1;
  const int st_row = (tid >> 1) & 31;
  const int st_g = tid >> 6;
  const bool a_ok = x0 + st_row < X;
  const bool b_ok = y0 + st_row < Y;
  const uint16_t* pa =
      A + bt * sAb + (int64_t)(x0 + st_row) * sAx + c0 + st_ch * 8;
  const uint16_t* pb =
      B + bt * sBb + (int64_t)(y0 + st_row) * sBy + c0 + st_ch * 8;

  f32x4 acc[4][2][2];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[ch][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[8], rb[8];
  tri_load(ra, pa, sAz, a_ok, st_g * 8, Z);
  tri_load(rb, pb, sBz, b_ok, st_g * 8, Z);

  for (int z0 = 0; z0 < Z; z0 += ZS) {
    __syncthreads();  // previous step's fragment reads are done
    tri_stage(sA, ra, st_ch, st_g, st_row);
    tri_stage(sB, rb, st_ch, st_g, st_row);
    __syncthreads();
    if (z0 + ZS < Z) {  // next step's loads fly across the MFMA phase
      tri_load(ra, pa, sAz, a_ok, z0 + ZS + st_g * 8, Z);
      tri_load(rb, pb, sBz, b_ok, z0 + ZS + st_g * 8, Z);
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const int c = wave * 4 + ch;
      const int sw = ((c >> 3) & 1) << 2;
      const int base = (c * 4 + lg) * TT;
      const bf16x8 a0 = tri_frag(sA + base + (lr ^ sw));
      const bf16x8 a1 = tri_frag(sA + base + ((16 + lr) ^ sw));
      const bf16x8 b0 = tri_frag(sB + base + (lr ^ sw));
      const bf16x8 b1 = tri_frag(sB + base + ((16 + lr) ^ sw));
      acc[ch][0][0] =
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[ch][0][0], 0, 0, 0);
      acc[ch][0][1] =
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[ch][0][1], 0, 0, 0);
      acc[ch][1][0] =
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[ch][1][0], 0, 0, 0);
      acc[ch][1][1] =
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[ch][1][1], 0, 0, 0);
    }
  }

  // epilogue: C fragments -> LDS [x][y][c] -> 16 B stores along c
  __syncthreads();
  uint16_t* sO = reinterpret_cast<uint16_t*>(smem);  // 32*32*48 B = 48 KB
#pragma unroll
  for (int tx = 0; tx < 2; ++tx)
#pragma unroll
    for (int ty = 0; ty < 2; ++ty)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = tx * 16 + lg * 4 + r;
        const int y = ty * 16 + lr;
        uint2 v;
        v.x = (uint32_t)f32_to_bf16_bits(acc[0][tx][ty][r]) |
              ((uint32_t)f32_to_bf16_bits(acc[1][tx][ty][r]) << 16);
        v.y = (uint32_t)f32_to_bf16_bits(acc[2][tx][ty][r]) |
              ((uint32_t)f32_to_bf16_bits(acc[3][tx][ty][r]) << 16);
        *reinterpret_cast<uint2*>(sO + (x * TT + y) * OROW + wave * 4) = v;
      }
  __syncthreads();
  uint16_t* po = O + bt * ((int64_t)X * Y * C) + c0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s = tid + 256 * i;
    const int ch8 = s & 1;
    const int y = (s >> 1) & 31;
    const int x = s >> 6;
    if (x0 + x < X && y0 + y < Y) {
      const uint4 v =
          *reinterpret_cast<const uint4*>(sO + (x * TT + y) * OROW + ch8 * 8);
      *reinterpret_cast<uint4*>(
          po + ((int64_t)(x0 + x) * Y + (y0 + y)) * C + ch8 * 8) = v;
    }
  }
}

void tri_check_operand(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "tri_contract: ", name, " must be a CUDA tensor");
  TORCH_CHECK(t.dim() == 4, "tri_contract: ", name, " must be 4-D (B, X, Z, C)");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "tri_contract: ", name,
              " must be bf16 (got ", t.scalar_type(), ")");
  TORCH_CHECK(t.stride(3) == 1, "tri_contract: ", name,
              " channel dim must be contiguous");
  for (int d = 0; d < 3; ++d)
    TORCH_CHECK(t.size(d) == 1 || (t.stride(d) >= 0 && t.stride(d) % 8 == 0),
                "tri_contract: ", name, " stride(", d, ") = ", t.stride(d),
                " is not a multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "tri_contract: ", name, " data pointer is not 16-byte aligned");
}

}  // namespace

at::Tensor tri_contract(at::Tensor a, at::Tensor b) {
  tri_check_operand(a, "a");
  tri_check_operand(b, "b");
  TORCH_CHECK(a.device() == b.device(), "tri_contract: a and b on different devices");
  const int64_t Bt = a.size(0), X = a.size(1), Z = a.size(2), C = a.size(3);
  const int64_t Y = b.size(1);
  TORCH_CHECK(b.size(0) == Bt && b.size(2) == Z && b.size(3) == C,
              "tri_contract: a ", a.sizes(), " and b ", b.sizes(),
              " must agree in batch, Z and C");
  TORCH_CHECK(Bt >= 1 && X >= 1 && Y >= 1 && Z >= 1, "tri_contract: empty dim");
  TORCH_CHECK(C > 0 && C % CC == 0, "tri_contract: C = ", C, " must be a positive multiple of ", CC);
  const int64_t lim = (int64_t)1 << 30;
  TORCH_CHECK(X < lim && Y < lim && Z < lim, "tri_contract: dim too large");
  const int64_t nxt = (X + TT - 1) / TT, nyt = (Y + TT - 1) / TT, ncc = C / CC;
  const int64_t blocks = Bt * nxt * nyt * ncc;
  TORCH_CHECK(blocks < ((int64_t)1 << 31), "tri_contract: grid too large");

  c10::cuda::CUDAGuard guard(a.device());
  auto o = at::empty({Bt, X, Y, C}, a.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  tri_contract_kernel<<<(unsigned)blocks, 256, 0, stream>>>(
      reinterpret_cast<uint16_t*>(o.data_ptr()),
      reinterpret_cast<const uint16_t*>(a.data_ptr()),
      reinterpret_cast<const uint16_t*>(b.data_ptr()), (int)X, (int)Y, (int)Z,
      (int)C, a.stride(0), a.stride(1), a.stride(2), b.stride(0), b.stride(1),
      b.stride(2), (int)nxt, (int)nyt, (int)ncc);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return o;
}
