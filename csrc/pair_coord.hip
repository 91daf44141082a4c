// Fused pair -> coordinate update for gfx950 (CDNA4): the SE(3)-equivariant
// coordinate head of the mol_pairbias model.
//
//   d_ij[h]  = pair[b,h,i,j] - pair0[b,h,i,j]            (fp32, after upcast)
//   w_ij     = W2 . gelu(W1 d_ij + b1) + b2              (exact erf GELU)
//   w_ij     = 0 where i or j is padded
//   update_i = inv_n[b] * sum_j (x_j - x_i) * w_ij
//
// It is the inverse of the fused gaussian pair bias (gaussian.hip): that one
// goes coords -> (B,H,L,L), this one (B,H,L,L) -> coords, and like it no
// (B,L,L,.) intermediate exists. The eager chain permutes the head-major
// pair tensor to channel-last, runs two Linears and a GELU over B*L*L rows,
// forms a (B,L,L,3) product and reduces it.
//
// Layout. pair is head-major, so the H values of one pair are H planes
// apart while each plane row pair[b,h,i,:] is contiguous in j. Lanes run
// along j: every load is coalesced and there is no permute. A group of G
// lanes (a power of two <= 64, the smallest that covers a row) owns one
// (b,i) row, so short rows still fill the wave; a lane holds the H values of
// NJ consecutive pairs in registers, produces the hidden units one at a
// time (MLP weights in LDS, every read a wave-wide broadcast shared by the
// NJ pairs) and accumulates three floats, which an xor-shuffle tree over
// the group reduces. NJ > 1 (16 B loads at H = 8, 8 B at H = 16 for the 2-byte
// dtypes) needs L % 8 == 0: otherwise row starts are not aligned and NJ = 1.
//
// Backward recomputes the hidden units and is deterministic (no atomics):
//   dpair kernel: same layout as forward, writes dpair head-major in the
//                 dtype of pair with one rounding, exact zeros at pads;
//   wgrad kernel: one thread per pair over the flat pair index, register
//                 accumulation of dW1/db1/dW2/db2, wave shuffle + LDS fold,
//                 per-block fp32 partials, then the two-stage column fold
//                 (fold.h). At H = 16 a block owns a 4-unit slice of the
//                 hidden layer, so dW1 stays at 64 registers per lane.
// Padded entries of pair/pair0 (finfo.min, or anything else) are never used:
// results at pads come from selects, not from multiplications by zero.
#include "common.h"
#include "dispatch.h"
#include "fold.h"

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <optional>
#include <vector>

namespace {

constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;

__device__ __forceinline__ float gelu_exact(float x) {
  return 0.5f * x * (1.f + erff(x * kRsqrt2));
}

// y = gelu(x), dy = gelu'(x)
__device__ __forceinline__ void gelu_exact_grad(float x, float& y, float& dy) {
  const float cdf = 0.5f * (1.f + erff(x * kRsqrt2));
  y = x * cdf;
  dy = cdf + x * kRsqrt2Pi * expf(-0.5f * x * x);
}

template <typename T, int NJ>
__device__ __forceinline__ void load_j(const T* p, float (&f)[NJ]) {
  if constexpr (NJ == 1)
    f[0] = Cvt<T>::to_f(p[0]);
  else
    loadN<T, NJ>(p, f);
}

template <typename T, int NJ>
__device__ __forceinline__ void store_j(T* p, const float (&f)[NJ]) {
  static_assert(NJ == 1 || NJ == 4 || NJ == 8, "store_j: NJ must be 1/4/8");
  if constexpr (NJ == 1) {
    p[0] = Cvt<T>::from_f(f[0]);
  } else if constexpr (NJ == 8) {
    store8(p, f);
  } else if constexpr (sizeof(T) == 2) {
    union {
      uint2 u;
      T t[4];
    } U;
#pragma unroll
    for (int t = 0; t < 4; ++t) U.t[t] = Cvt<T>::from_f(f[t]);
    *reinterpret_cast<uint2*>(p) = U.u;
  } else {
    float4 a;
    a.x = f[0]; a.y = f[1]; a.z = f[2]; a.w = f[3];
    *reinterpret_cast<float4*>(p) = a;
  }
}

// d[t][h] = pair - pair0 for the NJ pairs (b, i, j0 .. j0+NJ-1); plane0 is
// the offset of pair[b, 0, i, j0], planes are LL elements apart
template <typename T, int H, int NJ>
__device__ __forceinline__ void load_diff(const T* __restrict__ pair,
                                          const T* __restrict__ pair0,
                                          int64_t plane0, int64_t LL,
                                          float (&d)[NJ][H]) {
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float a[NJ], a0[NJ];
    load_j<T, NJ>(pair + plane0 + h * LL, a);
    load_j<T, NJ>(pair0 + plane0 + h * LL, a0);
#pragma unroll
    for (int t = 0; t < NJ; ++t) d[t][h] = a[t] - a0[t];
  }
}

// The MLP parameters in LDS: every read is a wave-wide broadcast.
template <int H>
struct MlpWeights {
  float W1[H * H];
  float b1[H];
  float W2[H];
  float b2;
};

template <int H>
__device__ __forceinline__ void stage_weights(
    MlpWeights<H>& sw, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2) {
  for (int c = (int)threadIdx.x; c < H * H; c += (int)blockDim.x)
    sw.W1[c] = W1[c];
  for (int c = (int)threadIdx.x; c < H; c += (int)blockDim.x) {
    sw.b1[c] = b1[c];
    sw.W2[c] = W2[c];
  }
  if (threadIdx.x == 0) sw.b2 = b2 != nullptr ? b2[0] : 0.f;
  __syncthreads();
}

// hk[t] = b1[k] + W1[k,:] . d[t][:], one weight read per NJ products
template <int H, int NJ>
__device__ __forceinline__ void hidden_unit(const MlpWeights<H>& sw, int k,
                                            const float (&d)[NJ][H],
                                            float (&hk)[NJ]) {
#pragma unroll
  for (int t = 0; t < NJ; ++t) hk[t] = sw.b1[k];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float wv = sw.W1[k * H + h];
#pragma unroll
    for (int t = 0; t < NJ; ++t) hk[t] += wv * d[t][h];
  }
}

// Lane geometry shared by the forward and the dpair kernel: G lanes per
// row, 64 / G rows per wave, waves grid-stride over groups of rows.
struct RowLanes {
  int gl;        // lane within the row's group
  int sub;       // row within the wave
  int rpw;       // rows per wave
  int64_t wave;  // global wave index
  int64_t nwaves;
};

__device__ __forceinline__ RowLanes row_lanes(int G) {
  RowLanes r;
  const int lane = (int)threadIdx.x % 64;
  r.gl = lane & (G - 1);
  r.sub = lane / G;
  r.rpw = 64 / G;
  r.wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  r.nwaves = (int64_t)gridDim.x * blockDim.x / 64;
  return r;
}

template <typename T, int H, int NJ>
__global__ void __launch_bounds__(256) pair_coord_fwd_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ inv_n,
    const uint8_t* __restrict__ pad,  // (B, L) | null
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2,
    float* __restrict__ out, int64_t n_rows, int L, int G) {
  __shared__ MlpWeights<H> sw;
  stage_weights<H>(sw, W1, b1, W2, b2);
  const RowLanes rl = row_lanes(G);
  const int64_t LL = (int64_t)L * L;
  const int units = L / NJ;
  const int64_t n_groups = (n_rows + rl.rpw - 1) / rl.rpw;
  // wave-uniform trip count: every lane reaches the shuffles
  for (int64_t wg = rl.wave; wg < n_groups; wg += rl.nwaves) {
    const int64_t row = wg * rl.rpw + rl.sub;
    const bool live = row < n_rows;
    float ax = 0.f, ay = 0.f, az = 0.f;
    int64_t b = 0;
    if (live) {
      b = row / L;
      const int i = (int)(row - b * L);
      if (pad == nullptr || !pad[row]) {
        const float xi = coords[row * 3 + 0], yi = coords[row * 3 + 1],
                    zi = coords[row * 3 + 2];
        for (int u = rl.gl; u < units; u += G) {
          const int j0 = u * NJ;
          float d[NJ][H];
          load_diff<T, H, NJ>(pair, pair0, (b * H * L + i) * (int64_t)L + j0,
                              LL, d);
          float w[NJ];
#pragma unroll
          for (int t = 0; t < NJ; ++t) w[t] = sw.b2;
          // k stays a loop: unrolled, the compiler hoists all H*H weights
          // into registers and spills
#pragma unroll(NJ == 1 ? 2 : 1)
          for (int k = 0; k < H; ++k) {
            float hk[NJ];
            hidden_unit<H, NJ>(sw, k, d, hk);
            const float w2 = sw.W2[k];
#pragma unroll
            for (int t = 0; t < NJ; ++t) w[t] += w2 * gelu_exact(hk[t]);
          }
#pragma unroll
          for (int t = 0; t < NJ; ++t) {
            const int64_t cj = b * L + j0 + t;
            const float wt = (pad != nullptr && pad[cj]) ? 0.f : w[t];
            ax += (coords[cj * 3 + 0] - xi) * wt;
            ay += (coords[cj * 3 + 1] - yi) * wt;
            az += (coords[cj * 3 + 2] - zi) * wt;
          }
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      if (off < G) {
        ax += __shfl_xor(ax, off, 64);
        ay += __shfl_xor(ay, off, 64);
        az += __shfl_xor(az, off, 64);
      }
    }
    if (live && rl.gl == 0) {
      const float s = inv_n[b];
      out[row * 3 + 0] = s * ax;
      out[row * 3 + 1] = s * ay;
      out[row * 3 + 2] = s * az;
    }
  }
}

template <typename T, int H, int NJ>
__global__ void __launch_bounds__(256) pair_coord_dpair_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ grad,  // (B,L,3)
    const float* __restrict__ inv_n, const uint8_t* __restrict__ pad,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, T* __restrict__ dpair, int64_t n_rows, int L,
    int G) {
  __shared__ MlpWeights<H> sw;
  stage_weights<H>(sw, W1, b1, W2, nullptr);
  const RowLanes rl = row_lanes(G);
  const int64_t LL = (int64_t)L * L;
  const int units = L / NJ;
  const int64_t n_groups = (n_rows + rl.rpw - 1) / rl.rpw;
  for (int64_t wg = rl.wave; wg < n_groups; wg += rl.nwaves) {
    const int64_t row = wg * rl.rpw + rl.sub;
    if (row >= n_rows) continue;
    const int64_t b = row / L;
    const int i = (int)(row - b * L);
    const bool row_pad = pad != nullptr && pad[row];
    const float s = inv_n[b];
    const float xi = coords[row * 3 + 0], yi = coords[row * 3 + 1],
                zi = coords[row * 3 + 2];
    const float gx = s * grad[row * 3 + 0], gy = s * grad[row * 3 + 1],
                gz = s * grad[row * 3 + 2];
    for (int u = rl.gl; u < units; u += G) {
      const int j0 = u * NJ;
      const int64_t plane0 = (b * H * L + i) * (int64_t)L + j0;
      float o[H][NJ];
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int t = 0; t < NJ; ++t) o[h][t] = 0.f;
      if (!row_pad) {
        float d[NJ][H];
        load_diff<T, H, NJ>(pair, pair0, plane0, LL, d);
        float dw[NJ];
        bool masked[NJ];
#pragma unroll
        for (int t = 0; t < NJ; ++t) {
          const int64_t cj = b * L + j0 + t;
          dw[t] = gx * (coords[cj * 3 + 0] - xi) +
                  gy * (coords[cj * 3 + 1] - yi) +
                  gz * (coords[cj * 3 + 2] - zi);
          masked[t] = pad != nullptr && pad[cj];
        }
#pragma unroll(NJ == 1 ? 2 : 1)
        for (int k = 0; k < H; ++k) {
          float hk[NJ], dh[NJ];
          hidden_unit<H, NJ>(sw, k, d, hk);
          const float w2 = sw.W2[k];
#pragma unroll
          for (int t = 0; t < NJ; ++t) {
            float y, dy;
            gelu_exact_grad(hk[t], y, dy);
            dh[t] = dw[t] * w2 * dy;
          }
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float wv = sw.W1[k * H + h];
#pragma unroll
            for (int t = 0; t < NJ; ++t) o[h][t] += wv * dh[t];
          }
        }
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int t = 0; t < NJ; ++t)
            if (masked[t]) o[h][t] = 0.f;
      }
#pragma unroll
      for (int h = 0; h < H; ++h)
        store_j<T, NJ>(dpair + plane0 + h * LL, o[h]);
    }
  }
}

// columns of a partials row: dW1 (k-major, H*H) | db1 (H) | dW2 (H) | db2
static inline int64_t wgrad_cols(int64_t H) { return H * H + 2 * H + 1; }

// Block blockIdx.x owns hidden units [s*KS, (s+1)*KS), s = blockIdx.x % TPP,
// and the pairs p*256 + tid (+ P*256 ...), p = blockIdx.x / TPP. It writes
// its own columns of partials row p; the TPP blocks of a row cover it.
template <typename T, int H, int KS>
__global__ void __launch_bounds__(256) pair_coord_wgrad_kernel(
    const T* __restrict__ pair, const T* __restrict__ pair0,
    const float* __restrict__ coords, const float* __restrict__ grad,
    const float* __restrict__ inv_n, const uint8_t* __restrict__ pad,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, float* __restrict__ partials,
    int64_t n_pairs, int L, int P) {
  constexpr int TPP = H / KS;
  constexpr int NACC = KS * H + 2 * KS + 1;
  constexpr int C = H * H + 2 * H + 1;
  __shared__ float s_red[4][NACC];
  __shared__ MlpWeights<H> sw;
  stage_weights<H>(sw, W1, b1, W2, nullptr);
  const int s = (int)blockIdx.x % TPP;
  const int p = (int)blockIdx.x / TPP;
  const int64_t LL = (int64_t)L * L;

  float aw1[KS][H], ab1[KS], aw2[KS], ab2 = 0.f;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    ab1[kk] = aw2[kk] = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) aw1[kk][h] = 0.f;
  }

  for (int64_t idx = (int64_t)p * 256 + threadIdx.x; idx < n_pairs;
       idx += (int64_t)P * 256) {
    const int64_t b = idx / LL;
    const int64_t rem = idx - b * LL;
    const int i = (int)(rem / L);
    const int j = (int)(rem - (int64_t)i * L);
    const int64_t ci = b * L + i, cj = b * L + j;
    if (pad != nullptr && (pad[ci] || pad[cj])) continue;
    float d[1][H];
    load_diff<T, H, 1>(pair, pair0, b * H * LL + rem, LL, d);
    const float dw =
        inv_n[b] *
        (grad[ci * 3 + 0] * (coords[cj * 3 + 0] - coords[ci * 3 + 0]) +
         grad[ci * 3 + 1] * (coords[cj * 3 + 1] - coords[ci * 3 + 1]) +
         grad[ci * 3 + 2] * (coords[cj * 3 + 2] - coords[ci * 3 + 2]));
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = s * KS + kk;
      float hk[1];
      hidden_unit<H, 1>(sw, k, d, hk);
      float y, dy;
      gelu_exact_grad(hk[0], y, dy);
      const float dh = dw * sw.W2[k] * dy;
#pragma unroll
      for (int h = 0; h < H; ++h) aw1[kk][h] += dh * d[0][h];
      ab1[kk] += dh;
      aw2[kk] += dw * y;
    }
    ab2 += dw;
  }

  // deterministic block fold: wave shuffle tree, then the waves in order
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float v = wave_sum(aw1[kk][h]);
      if (lane == 0) s_red[wave][kk * H + h] = v;
    }
    const float v1 = wave_sum(ab1[kk]);
    const float v2 = wave_sum(aw2[kk]);
    if (lane == 0) {
      s_red[wave][KS * H + kk] = v1;
      s_red[wave][KS * H + KS + kk] = v2;
    }
  }
  ab2 = wave_sum(ab2);
  if (lane == 0) s_red[wave][NACC - 1] = ab2;
  __syncthreads();
  for (int c = (int)threadIdx.x; c < NACC; c += 256) {
    const float v = (s_red[0][c] + s_red[1][c]) + (s_red[2][c] + s_red[3][c]);
    int col;
    if (c < KS * H)
      col = s * KS * H + c;
    else if (c < KS * H + KS)
      col = H * H + s * KS + (c - KS * H);
    else if (c < KS * H + 2 * KS)
      col = H * H + H + s * KS + (c - KS * H - KS);
    else
      col = (s == 0) ? H * H + 2 * H : -1;  // db2 is the same in every slice
    if (col >= 0) partials[(int64_t)p * C + col] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct PairCoordArgs {
  int64_t B, H, L;
  const uint8_t* pad;
  at::Tensor padc;
  bool vec;  // NJ > 1 allowed
};

static inline bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

static PairCoordArgs check_pair_coord(
    const char* name, const at::Tensor& pair, const at::Tensor& pair0,
    const at::Tensor& coords, const at::Tensor& inv_n,
    const std::optional<at::Tensor>& pad, const at::Tensor& W1,
    const at::Tensor& b1, const at::Tensor& W2, const at::Tensor& b2) {
  TORCH_CHECK(pair.is_cuda(), name, ": pair must be on the GPU, got device ",
              pair.device());
  TORCH_CHECK(pair.dim() == 4 && pair.size(2) == pair.size(3) &&
                  pair.size(3) >= 1,
              name, ": pair must be (B, H, L, L) with L >= 1, got sizes ",
              pair.sizes());
  TORCH_CHECK(pair.is_contiguous(), name,
              ": pair must be contiguous, got sizes ", pair.sizes(),
              " strides ", pair.strides());
  TORCH_CHECK(pair0.device() == pair.device(), name,
              ": pair0 must be on the device of pair, got ", pair0.device(),
              " vs ", pair.device());
  TORCH_CHECK(pair0.scalar_type() == pair.scalar_type(), name,
              ": pair0 dtype ", pair0.scalar_type(),
              " does not match pair dtype ", pair.scalar_type());
  TORCH_CHECK(pair0.sizes() == pair.sizes(), name, ": pair0 sizes ",
              pair0.sizes(), " do not match pair sizes ", pair.sizes());
  TORCH_CHECK(pair0.is_contiguous(), name,
              ": pair0 must be contiguous, got strides ", pair0.strides());
  PairCoordArgs a;
  a.B = pair.size(0);
  a.H = pair.size(1);
  a.L = pair.size(3);
  TORCH_CHECK(a.H == 8 || a.H == 16, name,
              ": the kernel serves H = 8 or 16 heads, got ", a.H);
  TORCH_CHECK(a.B * a.L <= 0x7fffffffLL, name, ": B * L = ", a.B * a.L,
              " does not fit 31 bits");
  TORCH_CHECK(coords.device() == pair.device() && coords.dim() == 3 &&
                  coords.size(0) == a.B && coords.size(1) == a.L &&
                  coords.size(2) == 3,
              name, ": coords must be (B, L, 3) = (", a.B, ", ", a.L,
              ", 3) on the device of pair, got sizes ", coords.sizes(), " on ",
              coords.device());
  TORCH_CHECK(coords.scalar_type() == at::kFloat && coords.is_contiguous(),
              name, ": coords must be contiguous fp32, got ",
              coords.scalar_type(), " strides ", coords.strides());
  TORCH_CHECK(inv_n.device() == pair.device() &&
                  inv_n.scalar_type() == at::kFloat && inv_n.dim() == 1 &&
                  inv_n.size(0) == a.B && inv_n.is_contiguous(),
              name, ": inv_n must be contiguous fp32 (B,) on the device of "
              "pair, got ", inv_n.scalar_type(), " sizes ", inv_n.sizes());
  a.pad = nullptr;
  if (pad.has_value()) {
    TORCH_CHECK(pad->device() == pair.device() &&
                    pad->scalar_type() == at::kBool && pad->dim() == 2 &&
                    pad->size(0) == a.B && pad->size(1) == a.L,
                name, ": padding_mask must be bool (B, L) on the device of "
                "pair, got ", pad->scalar_type(), " sizes ", pad->sizes());
    a.padc = pad->contiguous();
    a.pad = (const uint8_t*)a.padc.data_ptr<bool>();
  }
  auto check_w = [&](const char* wn, const at::Tensor& w, int64_t numel) {
    TORCH_CHECK(w.device() == pair.device() &&
                    w.scalar_type() == at::kFloat && w.numel() == numel &&
                    w.is_contiguous(),
                name, ": ", wn, " must be contiguous fp32 with ", numel,
                " elements on the device of pair, got ", w.scalar_type(),
                " sizes ", w.sizes());
  };
  check_w("fc1.weight", W1, a.H * a.H);
  check_w("fc1.bias", b1, a.H);
  check_w("fc2.weight", W2, a.H);
  check_w("fc2.bias", b2, 1);
  a.vec = a.L % 8 == 0 && aligned16(pair) && aligned16(pair0);
  return a;
}

// lanes per row: the smallest power of two that covers the row's units
static inline int lanes_per_row(int64_t units) {
  int G = 1;
  while (G < units && G < 64) G <<= 1;
  return G;
}

static inline int row_grid(int64_t n_rows, int G, int block) {
  const int64_t rpw = 64 / G;
  const int64_t groups = (n_rows + rpw - 1) / rpw;
  const int64_t wpb = block / 64;
  return unicore_grid((groups + wpb - 1) / wpb);
}

// H -> kH; the vector width NJ that keeps d[NJ][H] (+ the dpair output of
// the same size) at 64 registers each; the wgrad slice KS
#define DISPATCH_PAIR_COORD(H, VEC, ...)              \
  if ((H) == 8 && (VEC)) {                            \
    constexpr int kH = 8, kNJ = 8, kKS = 8;           \
    __VA_ARGS__;                                      \
  } else if ((H) == 8) {                              \
    constexpr int kH = 8, kNJ = 1, kKS = 8;           \
    __VA_ARGS__;                                      \
  } else if (VEC) {                                   \
    constexpr int kH = 16, kNJ = 4, kKS = 4;          \
    __VA_ARGS__;                                      \
  } else {                                            \
    constexpr int kH = 16, kNJ = 1, kKS = 4;          \
    __VA_ARGS__;                                      \
  }

}  // namespace

bool pair_coord_supported(int64_t H) { return H == 8 || H == 16; }

at::Tensor pair_coord_forward(at::Tensor pair, at::Tensor pair0,
                              at::Tensor coords, at::Tensor inv_n,
                              std::optional<at::Tensor> pad, at::Tensor W1,
                              at::Tensor b1, at::Tensor W2, at::Tensor b2) {
  const PairCoordArgs a = check_pair_coord("pair_coord_forward", pair, pair0,
                                           coords, inv_n, pad, W1, b1, W2, b2);
  auto out = at::empty({a.B, a.L, 3}, coords.options());
  const int64_t n_rows = a.B * a.L;
  if (n_rows == 0) return out;
  const int block = 256;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_FTYPES(pair.scalar_type(), "pair_coord_forward", {
    DISPATCH_PAIR_COORD(a.H, a.vec, {
      const int G = lanes_per_row(a.L / kNJ);
      pair_coord_fwd_kernel<scalar_t, kH, kNJ>
          <<<row_grid(n_rows, G, block), block, 0, stream>>>(
              reinterpret_cast<const scalar_t*>(pair.data_ptr()),
              reinterpret_cast<const scalar_t*>(pair0.data_ptr()),
              coords.data_ptr<float>(), inv_n.data_ptr<float>(), a.pad,
              W1.data_ptr<float>(), b1.data_ptr<float>(),
              W2.data_ptr<float>(), b2.data_ptr<float>(),
              out.data_ptr<float>(), n_rows, (int)a.L, G);
    });
  });
  return out;
}

// -> (dpair, dW1 (H,H), db1 (H), dW2 (H), db2 (1)); the weight gradients fp32
std::vector<at::Tensor> pair_coord_backward(
    at::Tensor grad, at::Tensor pair, at::Tensor pair0, at::Tensor coords,
    at::Tensor inv_n, std::optional<at::Tensor> pad, at::Tensor W1,
    at::Tensor b1, at::Tensor W2, at::Tensor b2) {
  const PairCoordArgs a = check_pair_coord("pair_coord_backward", pair, pair0,
                                           coords, inv_n, pad, W1, b1, W2, b2);
  TORCH_CHECK(grad.device() == pair.device() &&
                  grad.scalar_type() == at::kFloat &&
                  grad.sizes() == coords.sizes() && grad.is_contiguous(),
              "pair_coord_backward: grad must be contiguous fp32 (B, L, 3) on "
              "the device of pair, got ", grad.scalar_type(), " sizes ",
              grad.sizes(), " strides ", grad.strides());
  auto fopts = coords.options();
  auto dpair = at::empty_like(pair);
  const int64_t C = wgrad_cols(a.H);
  const int64_t n_rows = a.B * a.L;
  auto fold = n_rows > 0 ? at::empty({C}, fopts) : at::zeros({C}, fopts);
  if (n_rows > 0) {
    const bool vec = a.vec && aligned16(dpair);
    const int64_t n_pairs = n_rows * a.L;
    const int block = 256;
    const int P = unicore_grid((n_pairs + block - 1) / block, 1024);
    auto partials = at::empty({(int64_t)P, C}, fopts);
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FTYPES(pair.scalar_type(), "pair_coord_backward", {
      DISPATCH_PAIR_COORD(a.H, vec, {
        const int G = lanes_per_row(a.L / kNJ);
        pair_coord_dpair_kernel<scalar_t, kH, kNJ>
            <<<row_grid(n_rows, G, block), block, 0, stream>>>(
                reinterpret_cast<const scalar_t*>(pair.data_ptr()),
                reinterpret_cast<const scalar_t*>(pair0.data_ptr()),
                coords.data_ptr<float>(), grad.data_ptr<float>(),
                inv_n.data_ptr<float>(), a.pad, W1.data_ptr<float>(),
                b1.data_ptr<float>(), W2.data_ptr<float>(),
                reinterpret_cast<scalar_t*>(dpair.data_ptr()), n_rows,
                (int)a.L, G);
        pair_coord_wgrad_kernel<scalar_t, kH, kKS>
            <<<P * (kH / kKS), block, 0, stream>>>(
                reinterpret_cast<const scalar_t*>(pair.data_ptr()),
                reinterpret_cast<const scalar_t*>(pair0.data_ptr()),
                coords.data_ptr<float>(), grad.data_ptr<float>(),
                inv_n.data_ptr<float>(), a.pad, W1.data_ptr<float>(),
                b1.data_ptr<float>(), W2.data_ptr<float>(),
                partials.data_ptr<float>(), n_pairs, (int)a.L, P);
      });
    });
    unicore_fold_columns(partials.data_ptr<float>(), fold.data_ptr<float>(), P,
                         (int)C, fopts, stream);
  }
  const int64_t H = a.H;
  return {dpair, fold.narrow(0, 0, H * H).view({H, H}),
          fold.narrow(0, H * H, H), fold.narrow(0, H * H + H, H),
          fold.narrow(0, H * H + 2 * H, 1)};
}
