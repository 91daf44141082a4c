// Layout moves for Evoformer triangle self-attention on gfx950.
//
// Triangle attention reads the stored pair tensor (B, I, J, C) row-wise
// (starting node) or column-wise (ending node) and needs head-major batches
// for the score / PV GEMMs, plus its (B, L, L, H) pair bias as (B, H, L, L).
// torch runs each of these as a strided permute copy with 2-byte scalars on
// one side; the bias (H = 4 or 8 innermost, 8 or 16 B per position) is the
// worst case.  The four entries here are pure copies: raw bits are moved,
// never converted, so results are exact and deterministic.
//
//   pair_arrange      (B, I, J, C) view      -> (B, H, R, T, D)
//   pair_merge        (B*H*R, T, D)          -> (B, I, J, C)
//   pair_bias_arrange (B, L, L, H)           -> (B, H, L, L)
//   pair_bias_arrange_bwd (B, H, L, L)       -> (B, L, L, H)
//
// with (i, j) = (r, t), or (t, r) when `transpose` is set: the ending node is
// the starting node on the transposed pair tensor, and the transposition is
// folded into these copies instead of ever being materialised.
//
// pair_arrange / pair_merge: one work item moves 16 B.  Items are ordered
// (b, r, t, c-unit) with the channel unit fastest on BOTH layouts, so
// consecutive lanes walk one whole C-row of the (B, I, J, C) side (256 B at
// C = 128 bf16) and then step to the next t.  In the transposed case the
// next t is stride(1) away, but every row is still read (or written) as one
// full contiguous segment; on the head-major side the lanes of one head
// cover D * sizeof(T) bytes per t and consecutive t are adjacent, so a
// 256-thread block moves runs of 16 * D * sizeof(T) bytes per head.
// Ordering by the head-major index instead would read D-sized fragments of
// every C-row in h-major order: each line of the input fetched H times by
// different waves.
//
// pair_bias_arrange (+ _bwd): a thread owns 8 spatial positions x H heads,
// transposes them in registers (the 2 x 2 half-word swap of tri_stage in
// triangle.hip for 2-byte dtypes, plain re-indexing for fp32) and moves
// 8-position rows of one head on the (B, H, L, L) side, 16 B for 2-byte
// dtypes.  The (B, L, L, H) side moves H * sizeof(T) per position: 16 B
// (H = 8) or 8 B (H = 4) for 2-byte dtypes.  No LDS.
//   transpose = false: the 8 positions are 8 consecutive y, one contiguous
//     8 * H * sizeof(T) run of the (B, L, L, H) side; items are ordered
//     (b, x, y-block), so a wave covers one contiguous span on both sides.
//   transpose = true: the 8 positions are 8 consecutive rows of the
//     (B, L, L, H) side at one column x.  A wave is an 8 x 8 tile: lane & 7
//     walks x, the contiguous spatial dimension of that side (8 lanes x
//     16 B = one 128 B line per row at H = 8 bf16), lane >> 3 walks the
//     y-block (8 lanes x 16 B = one 128 B line of the (B, H, L, L) side).
//     Both sides see full lines; a flat order would leave one side with
//     64 scattered 16 B pieces per instruction.
#include "common.h"
#include "dispatch.h"

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include <optional>
#include <type_traits>

namespace {

// strided (B, I, J, C) <-> head-major (B, H, R, T, D), in 16 B units.
// `sd` is the strided side with unit strides (sb, sr, st, 1), `hm` the
// contiguous head-major side; CU = H * DU units per C-row.
template <bool INVERSE>
__global__ void pair_move_kernel(uint4* __restrict__ dst,
                                 const uint4* __restrict__ src, int64_t n,
                                 int R, int T, int H, int DU, int64_t sb,
                                 int64_t sr, int64_t st) {
  const int CU = H * DU;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t tmp = i;
    const int cu = (int)(tmp % CU);
    tmp /= CU;
    const int t = (int)(tmp % T);
    tmp /= T;
    const int r = (int)(tmp % R);
    const int64_t b = tmp / R;
    const int h = cu / DU;
    const int du = cu - h * DU;
    const int64_t sd = b * sb + (int64_t)r * sr + (int64_t)t * st + cu;
    const int64_t hm = (((b * H + h) * (int64_t)R + r) * T + t) * DU + du;
    if constexpr (INVERSE)
      dst[sd] = src[hm];
    else
      dst[hm] = src[sd];
  }
}

// N 32-bit words (8, 16 or 32 B) at a byte offset that is a multiple of
// min(16, 4 N); the same width contract as loadN in common.h, on raw bits
template <int N>
__device__ __forceinline__ void load_words(const char* p, uint32_t (&w)[N]) {
  static_assert(N == 2 || N == 4 || N == 8, "load_words: N must be 2/4/8");
  if constexpr (N == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    w[0] = v.x; w[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
}

template <int N>
__device__ __forceinline__ void store_words(char* p, const uint32_t (&w)[N]) {
  static_assert(N == 2 || N == 4 || N == 8, "store_words: N must be 2/4/8");
  if constexpr (N == 2) {
    *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      reinterpret_cast<uint4*>(p)[q] =
          make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// in: NA rows of NB elements, out: NB rows of NA elements, EB bytes per
// element, both packed into 32-bit words.  For 2-byte elements this is the
// half-word swap of every 2 x 2 block (as tri_stage does it).
template <int EB, int NA, int NB>
__device__ __forceinline__ void reg_transpose(
    const uint32_t (&in)[NA][NB * EB / 4], uint32_t (&out)[NB][NA * EB / 4]) {
  if constexpr (EB == 4) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int c = 0; c < NB; ++c) out[c][a] = in[a][c];
  } else {
#pragma unroll
    for (int a = 0; a < NA / 2; ++a)
#pragma unroll
      for (int c = 0; c < NB / 2; ++c) {
        const uint32_t e = in[2 * a][c], o = in[2 * a + 1][c];
        out[2 * c][a] = (e & 0xFFFFu) | (o << 16);
        out[2 * c + 1][a] = (e >> 16) | (o & 0xFFFF0000u);
      }
  }
}

// pos = the (B, L, L, H) side, rows = the (B, H, L, L) side.
// !INVERSE: pos -> rows (pair_bias_arrange); INVERSE: rows -> pos.
template <int EB, int H, bool TRANSPOSE, bool INVERSE>
__global__ void pair_bias_kernel(char* __restrict__ dst,
                                 const char* __restrict__ src, int64_t n,
                                 int L) {
  constexpr int PW = H * EB / 4;  // words per position (H heads)
  constexpr int RW = 8 * EB / 4;  // words per head row of 8 positions
  const int NB = L / 8;           // y-blocks per row
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t b;
    int x, yb;
    if constexpr (!TRANSPOSE) {
      int64_t tmp = i;
      yb = (int)(tmp % NB);
      tmp /= NB;
      x = (int)(tmp % L);
      b = tmp / L;
    } else {
      // 64 consecutive items = one wave = 8 x by 8 y-blocks
      const int NBT = (NB + 7) / 8;
      const int lane = (int)(i & 63);
      int64_t tmp = i >> 6;
      yb = (int)(tmp % NBT) * 8 + (lane >> 3);
      tmp /= NBT;
      x = (int)(tmp % NB) * 8 + (lane & 7);
      b = tmp / NB;
      if (yb >= NB) continue;
    }
    // element offsets of this thread's 8 positions and of its H rows
    const int64_t pos0 = TRANSPOSE ? ((b * L + (int64_t)yb * 8) * L + x) * H
                                   : ((b * L + x) * (int64_t)L + yb * 8) * H;
    const int64_t pos_step = TRANSPOSE ? (int64_t)L * H : H;
    const int64_t row0 = ((b * H) * (int64_t)L + x) * L + yb * 8;
    const int64_t row_step = (int64_t)L * L;
    uint32_t pos[8][PW], rows[H][RW];
    if constexpr (!INVERSE) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        load_words<PW>(src + (pos0 + j * pos_step) * EB, pos[j]);
      reg_transpose<EB, 8, H>(pos, rows);
#pragma unroll
      for (int h = 0; h < H; ++h)
        store_words<RW>(dst + (row0 + h * row_step) * EB, rows[h]);
    } else {
#pragma unroll
      for (int h = 0; h < H; ++h)
        load_words<RW>(src + (row0 + h * row_step) * EB, rows[h]);
      reg_transpose<EB, H, 8>(rows, pos);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        store_words<PW>(dst + (pos0 + j * pos_step) * EB, pos[j]);
    }
  }
}

constexpr int64_t kDimLimit = (int64_t)1 << 30;

void check_aligned(const at::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              ": data pointer is not 16-byte aligned");
}

at::Tensor pair_bias_move(at::Tensor x, bool transpose, bool inverse,
                          const char* name) {
  TORCH_CHECK(x.is_cuda(), name, ": expected a CUDA tensor");
  TORCH_CHECK(x.dim() == 4, name, ": expected a 4-D tensor, got ", x.dim(), "-D");
  const int64_t B = x.size(0);
  const int64_t H = inverse ? x.size(1) : x.size(3);
  const int64_t L = x.size(2);
  TORCH_CHECK(H == 4 || H == 8, name, ": H = ", H, " is not supported (4 or 8)");
  TORCH_CHECK((inverse ? x.size(3) : x.size(1)) == L, name,
              ": the two spatial sizes must be equal, got ", x.sizes());
  TORCH_CHECK(L >= 8 && L % 8 == 0, name, ": L = ", L,
              " must be a positive multiple of 8");
  TORCH_CHECK(B >= 1 && L < kDimLimit, name, ": bad sizes ", x.sizes());
  TORCH_CHECK(x.is_contiguous(), name, ": input must be contiguous");
  check_aligned(x, name);

  c10::cuda::CUDAGuard guard(x.device());
  auto out = inverse ? at::empty({B, L, L, H}, x.options())
                     : at::empty({B, H, L, L}, x.options());
  const int64_t NB = L / 8;
  const int64_t n =
      transpose ? B * NB * ((NB + 7) / 8) * 64 : B * L * NB;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = unicore_grid((n + 255) / 256);
  DISPATCH_FTYPES(x.scalar_type(), name, {
    constexpr int EB = (int)sizeof(scalar_t);
    auto launch = [&](auto h_tag, auto tr_tag, auto inv_tag) {
      pair_bias_kernel<EB, decltype(h_tag)::value, decltype(tr_tag)::value,
                       decltype(inv_tag)::value><<<grid, 256, 0, stream>>>(
          reinterpret_cast<char*>(out.data_ptr()),
          reinterpret_cast<const char*>(x.data_ptr()), n, (int)L);
    };
    auto with_h = [&](auto h_tag) {
      if (transpose) {
        if (inverse) launch(h_tag, std::true_type{}, std::true_type{});
        else launch(h_tag, std::true_type{}, std::false_type{});
      } else {
        if (inverse) launch(h_tag, std::false_type{}, std::true_type{});
        else launch(h_tag, std::false_type{}, std::false_type{});
      }
    };
    if (H == 8) with_h(std::integral_constant<int, 8>{});
    else with_h(std::integral_constant<int, 4>{});
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

}  // namespace

at::Tensor pair_arrange(at::Tensor x, int64_t heads, bool transpose) {
  TORCH_CHECK(x.is_cuda(), "pair_arrange: expected a CUDA tensor");
  TORCH_CHECK(x.dim() == 4, "pair_arrange: expected a (B, I, J, C) view, got ",
              x.dim(), "-D");
  const int64_t B = x.size(0), I = x.size(1), J = x.size(2), C = x.size(3);
  TORCH_CHECK(heads >= 1 && C % heads == 0, "pair_arrange: C = ", C,
              " is not divisible by heads = ", heads);
  const int64_t D = C / heads;
  TORCH_CHECK(D > 0 && D % 8 == 0, "pair_arrange: head dim D = ", D,
              " must be a positive multiple of 8");
  TORCH_CHECK(B >= 1 && I >= 1 && J >= 1 && I < kDimLimit && J < kDimLimit &&
                  C < kDimLimit,
              "pair_arrange: bad sizes ", x.sizes());
  TORCH_CHECK(x.stride(3) == 1, "pair_arrange: channel dim must be contiguous "
              "(stride(3) = ", x.stride(3), ")");
  for (int d = 0; d < 3; ++d)
    TORCH_CHECK(x.size(d) == 1 || (x.stride(d) >= 0 && x.stride(d) % 8 == 0),
                "pair_arrange: stride(", d, ") = ", x.stride(d),
                " is not a non-negative multiple of 8");
  check_aligned(x, "pair_arrange");

  c10::cuda::CUDAGuard guard(x.device());
  const int64_t R = transpose ? J : I, T = transpose ? I : J;
  auto out = at::empty({B, heads, R, T, D}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(x.scalar_type(), "pair_arrange", {
    constexpr int64_t VEC = 16 / sizeof(scalar_t);  // elements per 16 B unit
    const int64_t n = B * I * J * (C / VEC);
    // a size-1 dim never contributes to an offset; its stride may be anything
    const int64_t s0 = B == 1 ? 0 : x.stride(0) / VEC;
    const int64_t s1 = I == 1 ? 0 : x.stride(1) / VEC;
    const int64_t s2 = J == 1 ? 0 : x.stride(2) / VEC;
    pair_move_kernel<false>
        <<<unicore_grid((n + 255) / 256), 256, 0, stream>>>(
            reinterpret_cast<uint4*>(out.data_ptr()),
            reinterpret_cast<const uint4*>(x.data_ptr()), n, (int)R, (int)T,
            (int)heads, (int)(D / VEC), s0, transpose ? s2 : s1,
            transpose ? s1 : s2);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

// `out`, if given, is a (B, I, J, C) view under the same layout rules as
// the input of pair_arrange (e.g. one third of a fused qkv gradient buffer)
at::Tensor pair_merge(at::Tensor o, int64_t B, int64_t I, int64_t J,
                      int64_t heads, bool transpose,
                      std::optional<at::Tensor> out_opt) {
  TORCH_CHECK(o.is_cuda(), "pair_merge: expected a CUDA tensor");
  TORCH_CHECK(o.dim() == 3, "pair_merge: expected (B*H*R, T, D), got ", o.dim(),
              "-D");
  TORCH_CHECK(B >= 1 && I >= 1 && J >= 1 && heads >= 1 && I < kDimLimit &&
                  J < kDimLimit,
              "pair_merge: bad B/I/J/heads");
  const int64_t R = transpose ? J : I, T = transpose ? I : J;
  const int64_t D = o.size(2);
  TORCH_CHECK(o.size(0) == B * heads * R && o.size(1) == T, "pair_merge: input ",
              o.sizes(), " does not match (B*H*R, T, D) = (", B * heads * R,
              ", ", T, ", D)");
  TORCH_CHECK(D > 0 && D % 8 == 0, "pair_merge: head dim D = ", D,
              " must be a positive multiple of 8");
  TORCH_CHECK(heads * D < kDimLimit, "pair_merge: C too large");
  TORCH_CHECK(o.is_contiguous(), "pair_merge: input must be contiguous");
  check_aligned(o, "pair_merge");

  c10::cuda::CUDAGuard guard(o.device());
  const int64_t C = heads * D;
  at::Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    TORCH_CHECK(out.is_cuda() && out.device() == o.device() &&
                    out.scalar_type() == o.scalar_type(),
                "pair_merge: out must match the input's device and dtype");
    TORCH_CHECK(out.dim() == 4 && out.size(0) == B && out.size(1) == I &&
                    out.size(2) == J && out.size(3) == C,
                "pair_merge: out ", out.sizes(), " is not (B, I, J, C)");
    TORCH_CHECK(out.stride(3) == 1, "pair_merge: out channel dim must be "
                "contiguous (stride(3) = ", out.stride(3), ")");
    // strictly positive: a stride of 0 would make the stores overlap
    for (int d = 0; d < 3; ++d)
      TORCH_CHECK(out.size(d) == 1 ||
                      (out.stride(d) > 0 && out.stride(d) % 8 == 0),
                  "pair_merge: out stride(", d, ") = ", out.stride(d),
                  " is not a positive multiple of 8");
    check_aligned(out, "pair_merge (out)");
  } else {
    out = at::empty({B, I, J, C}, o.options());
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(o.scalar_type(), "pair_merge", {
    constexpr int64_t VEC = 16 / sizeof(scalar_t);
    const int64_t CU = C / VEC;
    const int64_t n = B * I * J * CU;
    const int64_t s0 = B == 1 ? 0 : out.stride(0) / VEC;
    const int64_t s1 = I == 1 ? 0 : out.stride(1) / VEC;
    const int64_t s2 = J == 1 ? 0 : out.stride(2) / VEC;
    pair_move_kernel<true>
        <<<unicore_grid((n + 255) / 256), 256, 0, stream>>>(
            reinterpret_cast<uint4*>(out.data_ptr()),
            reinterpret_cast<const uint4*>(o.data_ptr()), n, (int)R, (int)T,
            (int)heads, (int)(D / VEC), s0, transpose ? s2 : s1,
            transpose ? s1 : s2);
  });
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

at::Tensor pair_bias_arrange(at::Tensor lin, bool transpose) {
  return pair_bias_move(lin, transpose, false, "pair_bias_arrange");
}

at::Tensor pair_bias_arrange_bwd(at::Tensor d_bias, bool transpose) {
  return pair_bias_move(d_bias, transpose, true, "pair_bias_arrange_bwd");
}
