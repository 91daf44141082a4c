// pybind11 bindings for the unicore_amd gfx950 kernel extension.
// One module (`unicore_amd._kernels`) covers the same API surface as the
// reference's 8 separate CUDA extensions (reference setup.py:141-387).
#include <torch/extension.h>

#include "pair_dist_h64.h"
#include "pair_gauss_h64.h"
#include "pair_norm.h"

#include <optional>
#include <vector>

std::vector<at::Tensor> softmax_dropout_forward(bool is_training, at::Tensor input,
                                                std::optional<at::Tensor> mask,
                                                int64_t mask_outer_div,
                                                std::optional<at::Tensor> bias,
                                                int64_t bias_outer_div,
                                                double dropout_prob);
at::Tensor softmax_dropout_backward(at::Tensor grad_output,
                                    at::Tensor softmax_results,
                                    at::Tensor dropout_mask, double dropout_prob);
std::vector<at::Tensor> layernorm_forward(at::Tensor input, at::Tensor gamma,
                                          at::Tensor beta, double eps);
std::vector<at::Tensor> layernorm_backward(at::Tensor grad_out, at::Tensor input,
                                           at::Tensor mean, at::Tensor invvar,
                                           at::Tensor gamma);
std::vector<at::Tensor> rmsnorm_forward(at::Tensor input, at::Tensor gamma,
                                        double eps);
std::vector<at::Tensor> rmsnorm_backward(at::Tensor grad_out, at::Tensor input,
                                         at::Tensor invvar, at::Tensor gamma);
void fused_adam(at::Tensor p, at::Tensor m, at::Tensor v, at::Tensor g, double lr,
                double beta1, double beta2, double eps, double grad_scale,
                int64_t step, bool bias_correction, double weight_decay);
at::Tensor multi_tensor_l2norm(int64_t chunk_size, std::vector<at::Tensor> tensors);
void fp32_to_bf16_sr(at::Tensor src, at::Tensor dst);
std::vector<at::Tensor> qkv_split_forward(at::Tensor qkv,
                                          std::optional<at::Tensor> bias,
                                          int64_t num_heads, double scale);
std::vector<at::Tensor> qkv_split_backward(at::Tensor dq, at::Tensor dk,
                                           at::Tensor dv, int64_t B,
                                           int64_t num_heads, double scale,
                                           bool bias_grad);
at::Tensor gated_mul_forward(at::Tensor x, at::Tensor g,
                             std::optional<at::Tensor> bx,
                             std::optional<at::Tensor> bg);
std::vector<at::Tensor> gated_mul_backward(at::Tensor grad, at::Tensor x,
                                           at::Tensor g,
                                           std::optional<at::Tensor> bx,
                                           std::optional<at::Tensor> bg);
at::Tensor attn_merge(at::Tensor x, int64_t B, int64_t num_heads,
                      bool inverse);
at::Tensor msa_arrange(at::Tensor x, int64_t B, int64_t S, int64_t L,
                       int64_t H, bool col, bool inverse);
std::vector<at::Tensor> gelu_dropout_forward(at::Tensor x,
                                             std::optional<at::Tensor> bias,
                                             double p, bool is_training);
std::vector<at::Tensor> gelu_dropout_backward(at::Tensor grad, at::Tensor x,
                                              std::optional<at::Tensor> bias,
                                              at::Tensor dmask, double p);
at::Tensor mfma_gemm_16x16x32(at::Tensor A, at::Tensor B);
std::vector<at::Tensor> dropout_add_ln_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias,
    at::Tensor gamma, at::Tensor beta, double p, bool is_training, double eps);

std::vector<at::Tensor> dropout_add_forward(at::Tensor x, at::Tensor res,
                                            std::optional<at::Tensor> bias,
                                            double p, bool is_training);
std::vector<at::Tensor> dropout_add_backward(at::Tensor grad, at::Tensor dmask,
                                             double p, int64_t bias_dim);
at::Tensor embedding_backward(at::Tensor grad, at::Tensor indices,
                              int64_t num_embeddings, int64_t padding_idx);
std::vector<at::Tensor> cross_entropy_forward(at::Tensor logits, at::Tensor target,
                                              int64_t ignore_index);
at::Tensor cross_entropy_backward(at::Tensor logits, at::Tensor target,
                                  at::Tensor lse, at::Tensor grad_scale,
                                  int64_t ignore_index);
bool softmax_dropout_backward_bias_supported(int64_t n_batch, int64_t q,
                                             int64_t k, int64_t bb, int64_t bq,
                                             int64_t od);
std::vector<at::Tensor> softmax_dropout_backward_bias(
    at::Tensor grad_output, at::Tensor softmax_results, at::Tensor dropout_mask,
    double dropout_prob, int64_t bb, int64_t bq, int64_t od);
at::Tensor gaussian_basis_forward(at::Tensor coords, at::Tensor means,
                                  at::Tensor stds, at::ScalarType out_dtype);
std::vector<at::Tensor> gaussian_basis_backward(at::Tensor dg, at::Tensor coords,
                                                at::Tensor means, at::Tensor stds);
bool gaussian_basis_supported(int64_t K);
at::Tensor gaussian_pair_bias_forward(at::Tensor coords, at::Tensor means,
                                      at::Tensor stds, at::Tensor W,
                                      at::Tensor bvec,
                                      std::optional<at::Tensor> pad,
                                      double fill, at::ScalarType out_dtype);
std::vector<at::Tensor> gaussian_pair_bias_backward(
    at::Tensor dbias, at::Tensor coords, at::Tensor means, at::Tensor stds,
    at::Tensor W, std::optional<at::Tensor> pad);
bool gaussian_pair_bias_supported(int64_t K, int64_t H);
std::vector<at::Tensor> flash_attn_forward(at::Tensor q, at::Tensor k, at::Tensor v,
                                           std::optional<at::Tensor> bias,
                                           int64_t bias_outer_div,
                                           std::optional<at::Tensor> mask,
                                           int64_t mask_outer_div,
                                           double dropout_p, bool is_training);
std::vector<at::Tensor> flash_attn_backward(
    at::Tensor d_out, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
    at::Tensor lse, std::optional<at::Tensor> bias, int64_t bias_outer_div,
    bool bias_needs_grad, std::optional<at::Tensor> mask, int64_t mask_outer_div,
    double dropout_p, bool dropped, int64_t seed_in);
std::vector<at::Tensor> evo_attn_forward(at::Tensor q, at::Tensor k, at::Tensor v,
                                         std::optional<at::Tensor> bias,
                                         int64_t bias_outer_div,
                                         std::optional<at::Tensor> mask,
                                         int64_t mask_outer_div,
                                         double dropout_p, bool is_training);
std::vector<at::Tensor> evo_attn_backward(
    at::Tensor d_out, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
    at::Tensor lse, std::optional<at::Tensor> bias, int64_t bias_outer_div,
    bool want_dbias, std::optional<at::Tensor> mask, int64_t mask_outer_div,
    double dropout_p, bool dropped, int64_t seed_in);
bool evo_attn_supported(int64_t N, int64_t T, int64_t D, bool is_bf16);
std::vector<at::Tensor> pair_attn_forward(at::Tensor q, at::Tensor k,
                                          at::Tensor v, at::Tensor bias,
                                          double dropout_p, bool is_training);
std::vector<at::Tensor> pair_attn_backward(
    at::Tensor d_out, std::optional<at::Tensor> d_logits, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse, at::Tensor logits,
    double dropout_p, bool dropped, int64_t seed_in);
bool pair_attn_supported(int64_t L, int64_t D, bool is_bf16);
at::Tensor tri_contract(at::Tensor a, at::Tensor b);
at::Tensor opm_forward(at::Tensor a, at::Tensor b, double scale);
at::Tensor opm_backward_a(at::Tensor d_o, at::Tensor b, double scale);
at::Tensor opm_backward_b(at::Tensor d_o, at::Tensor a, double scale);
at::Tensor opm_forward_w(at::Tensor a, at::Tensor b, at::Tensor w);
at::Tensor opm_backward_a_w(at::Tensor d_o, at::Tensor b, at::Tensor w);
at::Tensor opm_backward_b_w(at::Tensor d_o, at::Tensor a, at::Tensor w);
at::Tensor gated_mul_masked_forward(at::Tensor x, at::Tensor g,
                                    std::optional<at::Tensor> bx,
                                    std::optional<at::Tensor> bg, at::Tensor m);
std::vector<at::Tensor> gated_mul_masked_backward(
    at::Tensor grad, at::Tensor x, at::Tensor g, std::optional<at::Tensor> bx,
    std::optional<at::Tensor> bg, at::Tensor m);
at::Tensor pair_arrange(at::Tensor x, int64_t heads, bool transpose);
at::Tensor pair_merge(at::Tensor o, int64_t B, int64_t I, int64_t J,
                      int64_t heads, bool transpose,
                      std::optional<at::Tensor> out);
at::Tensor pair_bias_arrange(at::Tensor lin, bool transpose);
at::Tensor pair_bias_arrange_bwd(at::Tensor d_bias, bool transpose);
std::vector<at::Tensor> shared_dropout_add_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias, double p,
    int64_t shared_dim);
std::vector<at::Tensor> shared_dropout_add_ln_forward(
    at::Tensor x, at::Tensor res, std::optional<at::Tensor> bias,
    at::Tensor gamma, at::Tensor beta, double p, int64_t shared_dim,
    double eps);
std::vector<at::Tensor> shared_dropout_add_backward(at::Tensor grad,
                                                    at::Tensor dmask, double p,
                                                    int64_t shared_dim,
                                                    int64_t bias_dim);
at::Tensor pair_coord_forward(at::Tensor pair, at::Tensor pair0,
                              at::Tensor coords, at::Tensor inv_n,
                              std::optional<at::Tensor> pad, at::Tensor W1,
                              at::Tensor b1, at::Tensor W2, at::Tensor b2);
std::vector<at::Tensor> pair_coord_backward(
    at::Tensor grad, at::Tensor pair, at::Tensor pair0, at::Tensor coords,
    at::Tensor inv_n, std::optional<at::Tensor> pad, at::Tensor W1,
    at::Tensor b1, at::Tensor W2, at::Tensor b2);
bool pair_coord_supported(int64_t H, int64_t L);
at::Tensor mfma_gemm_16x16x4_f32(at::Tensor A, at::Tensor B);

// ---------------------------------------------------------------------------
// Pair distance head (pair_dist_h64.hip): the entries and their host checks
// ---------------------------------------------------------------------------

bool pair_dist_supported(int64_t H, int64_t L) {
  return H == 64 && L >= 8 && L % 8 == 0;
}

namespace {

struct PairDistArgs {
  int64_t B, L;
  const uint8_t* pad;
  at::Tensor padc;
};

PairDistArgs check_pair_dist(const char* name, const at::Tensor& pair,
                             const std::optional<at::Tensor>& pad,
                             const at::Tensor& W1, const at::Tensor& b1,
                             const at::Tensor& gamma, const at::Tensor& beta,
                             const at::Tensor& w2, const at::Tensor& b2) {
  TORCH_CHECK(pair.is_cuda(), name, ": pair must be on the GPU, got device ",
              pair.device());
  TORCH_CHECK(pair.scalar_type() == at::kFloat ||
                  pair.scalar_type() == at::kHalf ||
                  pair.scalar_type() == at::kBFloat16,
              name, ": pair must be fp32, fp16 or bf16, got ",
              pair.scalar_type());
  TORCH_CHECK(pair.dim() == 4 && pair.size(2) == pair.size(3), name,
              ": pair must be (B, H, L, L), got sizes ", pair.sizes());
  PairDistArgs a;
  a.B = pair.size(0);
  a.L = pair.size(3);
  TORCH_CHECK(pair.size(1) == 64, name,
              ": the kernels serve H = 64 heads, got H = ", pair.size(1));
  TORCH_CHECK(a.L >= 8 && a.L % 8 == 0, name,
              ": needs L a multiple of 8 and >= 8, got L = ", a.L);
  TORCH_CHECK(pair.is_contiguous(), name,
              ": pair must be contiguous, got sizes ", pair.sizes(),
              " strides ", pair.strides());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pair.data_ptr()) % 16 == 0, name,
              ": pair must be 16 B-aligned, got address ", pair.data_ptr());
  TORCH_CHECK(a.B * a.L <= 0x7fffffffLL, name, ": B * L = ", a.B * a.L,
              " does not fit 31 bits");
  const int64_t tiles = (a.L + 31) / 32;
  TORCH_CHECK(a.B * tiles * tiles <= 0x7fffffffLL, name, ": a grid of ",
              a.B * tiles * tiles, " 32 x 32 tiles does not fit 31 bits");
  a.pad = nullptr;
  if (pad.has_value()) {
    TORCH_CHECK(pad->device() == pair.device() &&
                    pad->scalar_type() == at::kBool && pad->dim() == 2 &&
                    pad->size(0) == a.B && pad->size(1) == a.L,
                name, ": padding_mask must be bool (B, L) = (", a.B, ", ", a.L,
                ") on the device of pair, got ", pad->scalar_type(), " sizes ",
                pad->sizes(), " on ", pad->device());
    a.padc = pad->contiguous();
    // the wgrad kernel reads four pad bytes as one word
    if (reinterpret_cast<uintptr_t>(a.padc.data_ptr()) % 4 != 0)
      a.padc = a.padc.clone();
    a.pad = (const uint8_t*)a.padc.data_ptr<bool>();
  }
  auto check_w = [&](const char* wn, const at::Tensor& w,
                     at::IntArrayRef shape) {
    TORCH_CHECK(w.device() == pair.device(), name, ": ", wn,
                " must be on the device of pair, got ", w.device(), " vs ",
                pair.device());
    TORCH_CHECK(w.scalar_type() == at::kFloat, name, ": ", wn,
                " must be fp32, got ", w.scalar_type());
    TORCH_CHECK(w.sizes() == shape && w.is_contiguous(), name, ": ", wn,
                " must be contiguous ", shape, ", got sizes ", w.sizes(),
                " strides ", w.strides());
  };
  check_w("dense.weight", W1, {64, 64});
  check_w("dense.bias", b1, {64});
  check_w("layer_norm.weight", gamma, {64});
  check_w("layer_norm.bias", beta, {64});
  check_w("out_proj.weight", w2, {64});
  check_w("out_proj.bias", b2, {1});
  return a;
}

}  // namespace

// -> dist (B, L, L) fp32, symmetric, 0 where i or j is padded
at::Tensor pair_dist_forward(at::Tensor pair, std::optional<at::Tensor> pad,
                             at::Tensor W1, at::Tensor b1, at::Tensor gamma,
                             at::Tensor beta, at::Tensor w2, at::Tensor b2,
                             double eps) {
  const PairDistArgs a = check_pair_dist("pair_dist_forward", pair, pad, W1, b1,
                                         gamma, beta, w2, b2);
  auto out = at::empty({a.B, a.L, a.L}, W1.options());
  if (a.B == 0) return out;
  auto F = at::empty_like(out);
  pair_dist_h64_forward_launch(F, pair, a.pad, W1, b1, gamma, beta, w2, b2,
                               (float)eps);
  pair_dist_sym_launch(out, F, a.pad);
  return out;
}

// -> (dpair, dW1 (64,64), db1, dgamma, dbeta, dw2 (64 each), db2 (1)); the
// parameter gradients fp32
std::vector<at::Tensor> pair_dist_backward(
    at::Tensor grad, at::Tensor pair, std::optional<at::Tensor> pad,
    at::Tensor W1, at::Tensor b1, at::Tensor gamma, at::Tensor beta,
    at::Tensor w2, at::Tensor b2, double eps) {
  const PairDistArgs a = check_pair_dist("pair_dist_backward", pair, pad, W1,
                                         b1, gamma, beta, w2, b2);
  TORCH_CHECK(grad.device() == pair.device() &&
                  grad.scalar_type() == at::kFloat && grad.dim() == 3 &&
                  grad.size(0) == a.B && grad.size(1) == a.L &&
                  grad.size(2) == a.L && grad.is_contiguous(),
              "pair_dist_backward: grad must be contiguous fp32 (B, L, L) = (",
              a.B, ", ", a.L, ", ", a.L, ") on the device of pair, got ",
              grad.scalar_type(), " sizes ", grad.sizes(), " strides ",
              grad.strides(), " on ", grad.device());
  auto dpair = at::empty_like(pair);
  const int64_t C = pair_dist_h64_wgrad_cols();
  auto fold = a.B > 0 ? at::empty({C}, W1.options()) : at::zeros({C}, W1.options());
  if (a.B > 0) {
    auto dF = at::empty_like(grad);
    pair_dist_sym_launch(dF, grad, a.pad);
    pair_dist_h64_backward_launch(dpair, fold, dF, pair, a.pad, W1, b1, gamma,
                                  beta, w2, (float)eps);
  }
  const int64_t H = 64, HH = H * H;
  return {dpair,
          fold.narrow(0, 0, HH).view({H, H}),
          fold.narrow(0, HH, H),
          fold.narrow(0, HH + H, H),
          fold.narrow(0, HH + 2 * H, H),
          fold.narrow(0, HH + 3 * H, H),
          fold.narrow(0, HH + 4 * H, 1)};
}

// ---------------------------------------------------------------------------
// Uni-Mol pair embedding (pair_gauss_h64.hip): the entries and their host
// checks
// ---------------------------------------------------------------------------

bool pair_gauss_supported(int64_t K, int64_t H, int64_t L) {
  return K == 128 && H == 64 && L >= 8 && L % 8 == 0;
}

namespace {

struct PairGaussArgs {
  int64_t B, L;
  const uint8_t* pad;
  at::Tensor padc;
};

PairGaussArgs check_pair_gauss(const char* name, const at::Tensor& coords,
                               const at::Tensor& a, const at::Tensor& b,
                               const std::optional<at::Tensor>& pad,
                               const at::Tensor& means, const at::Tensor& stds,
                               const at::Tensor& W1, const at::Tensor& b1,
                               const at::Tensor& W2, const at::Tensor* b2) {
  TORCH_CHECK(coords.is_cuda(), name, ": coords must be on the GPU, got device ",
              coords.device());
  TORCH_CHECK(coords.scalar_type() == at::kFloat && coords.dim() == 3 &&
                  coords.size(2) == 3 && coords.is_contiguous(),
              name, ": coords must be contiguous fp32 (B, L, 3), got ",
              coords.scalar_type(), " sizes ", coords.sizes(), " strides ",
              coords.strides());
  PairGaussArgs r;
  r.B = coords.size(0);
  r.L = coords.size(1);
  TORCH_CHECK(W1.scalar_type() == at::kBFloat16, name,
              ": the kernels serve a bf16 module, got linear1.weight in ",
              W1.scalar_type());
  TORCH_CHECK(means.dim() == 1 && means.size(0) == 128, name,
              ": the kernels serve K = 128 gaussians, got means of sizes ",
              means.sizes());
  TORCH_CHECK(W2.dim() == 2 && W2.size(0) == 64, name,
              ": the kernels serve H = 64 heads, got linear2.weight of sizes ",
              W2.sizes());
  TORCH_CHECK(r.L >= 8 && r.L % 8 == 0, name,
              ": needs L a multiple of 8 and >= 8, got L = ", r.L);
  TORCH_CHECK(r.B * r.L <= 0x7fffffffLL, name, ": B * L = ", r.B * r.L,
              " does not fit 31 bits");
  auto check_t = [&](const char* tn, const at::Tensor& t, at::ScalarType st,
                     at::IntArrayRef shape) {
    TORCH_CHECK(t.device() == coords.device(), name, ": ", tn,
                " must be on the device of coords, got ", t.device(), " vs ",
                coords.device());
    TORCH_CHECK(t.scalar_type() == st, name, ": ", tn, " must be ", st,
                ", got ", t.scalar_type());
    TORCH_CHECK(t.sizes() == shape && t.is_contiguous(), name, ": ", tn,
                " must be contiguous ", shape, ", got sizes ", t.sizes(),
                " strides ", t.strides());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
                ": ", tn, " must be 16 B-aligned, got address ", t.data_ptr());
  };
  check_t("a", a, at::kFloat, {r.B, r.L, r.L});
  check_t("b", b, at::kFloat, {r.B, r.L, r.L});
  check_t("means", means, at::kFloat, {128});
  check_t("stds", stds, at::kFloat, {128});
  check_t("linear1.weight", W1, at::kBFloat16, {128, 128});
  check_t("linear1.bias", b1, at::kBFloat16, {128});
  check_t("linear2.weight", W2, at::kBFloat16, {64, 128});
  if (b2 != nullptr) check_t("linear2.bias", *b2, at::kBFloat16, {64});
  r.pad = nullptr;
  if (pad.has_value()) {
    TORCH_CHECK(pad->device() == coords.device() &&
                    pad->scalar_type() == at::kBool && pad->dim() == 2 &&
                    pad->size(0) == r.B && pad->size(1) == r.L,
                name, ": padding_mask must be bool (B, L) = (", r.B, ", ", r.L,
                ") on the device of coords, got ", pad->scalar_type(),
                " sizes ", pad->sizes(), " on ", pad->device());
    r.padc = pad->contiguous();
    // the backward kernels read eight pad bytes as one word
    if (reinterpret_cast<uintptr_t>(r.padc.data_ptr()) % 8 != 0)
      r.padc = r.padc.clone();
    r.pad = (const uint8_t*)r.padc.data_ptr<bool>();
  }
  return r;
}

}  // namespace

// -> (B, 64, L, L) bf16, fill at padded keys
at::Tensor pair_gauss_forward(at::Tensor coords, at::Tensor a, at::Tensor b,
                              std::optional<at::Tensor> pad, at::Tensor means,
                              at::Tensor stds, at::Tensor W1, at::Tensor b1,
                              at::Tensor W2, at::Tensor b2, double fill) {
  const PairGaussArgs r = check_pair_gauss("pair_gauss_forward", coords, a, b,
                                           pad, means, stds, W1, b1, W2, &b2);
  auto out = at::empty({r.B, 64, r.L, r.L}, W1.options());
  if (r.B == 0) return out;
  pair_gauss_h64_forward_launch(out, coords, a, b, r.pad, means, stds, W1, b1,
                                W2, b2, (float)fill);
  return out;
}

// -> (d_a, d_b (B, L, L), d_means, d_stds (128), dW1 (128,128), db1 (128),
// dW2 (64,128), db2 (64)), all fp32
std::vector<at::Tensor> pair_gauss_backward(
    at::Tensor grad, at::Tensor coords, at::Tensor a, at::Tensor b,
    std::optional<at::Tensor> pad, at::Tensor means, at::Tensor stds,
    at::Tensor W1, at::Tensor b1, at::Tensor W2) {
  const PairGaussArgs r = check_pair_gauss("pair_gauss_backward", coords, a, b,
                                           pad, means, stds, W1, b1, W2,
                                           nullptr);
  TORCH_CHECK(grad.device() == coords.device() &&
                  grad.scalar_type() == at::kBFloat16 && grad.dim() == 4 &&
                  grad.size(0) == r.B && grad.size(1) == 64 &&
                  grad.size(2) == r.L && grad.size(3) == r.L &&
                  grad.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(grad.data_ptr()) % 16 == 0,
              "pair_gauss_backward: grad must be contiguous, 16 B-aligned bf16 "
              "(B, 64, L, L) = (", r.B, ", 64, ", r.L, ", ", r.L,
              ") on the device of coords, got ", grad.scalar_type(), " sizes ",
              grad.sizes(), " strides ", grad.strides(), " on ", grad.device());
  const int64_t K = 128, H = 64, C = pair_gauss_h64_wgrad_cols();
  auto d_a = at::empty_like(a);
  auto d_b = at::empty_like(b);
  auto sf = r.B > 0 ? at::empty({2 * K}, a.options()) : at::zeros({2 * K}, a.options());
  auto wf = r.B > 0 ? at::empty({C}, a.options()) : at::zeros({C}, a.options());
  if (r.B > 0)
    pair_gauss_h64_backward_launch(d_a, d_b, sf, wf, grad, coords, a, b, r.pad,
                                   means, stds, W1, b1, W2);
  return {d_a,
          d_b,
          sf.narrow(0, 0, K),
          sf.narrow(0, K, K),
          wf.narrow(0, 0, K * K).view({K, K}),
          wf.narrow(0, K * K, K),
          wf.narrow(0, K * K + K, H * K).view({H, K}),
          wf.narrow(0, K * K + K + H * K, H)};
}

// ---------------------------------------------------------------------------
// Uni-Mol norm regularisers (pair_norm.hip): the entries and their host
// checks
// ---------------------------------------------------------------------------

bool pair_norm_supported(int64_t H, int64_t L) {
  return H >= 4 && H % 4 == 0 && L >= 8 && L % 8 == 0;
}

namespace {

struct NormPad {
  const uint8_t* ptr = nullptr;
  at::Tensor keep;
};

// bool mask of `shape` on the device of ref; the pair kernel reads eight pad
// bytes as one word
NormPad check_norm_pad(const char* name, const std::optional<at::Tensor>& pad,
                       const at::Tensor& ref, at::IntArrayRef shape) {
  NormPad r;
  if (!pad.has_value()) return r;
  TORCH_CHECK(pad->device() == ref.device() &&
                  pad->scalar_type() == at::kBool && pad->sizes() == shape,
              name, ": padding_mask must be bool ", shape,
              " on the device of the input, got ", pad->scalar_type(),
              " sizes ", pad->sizes(), " on ", pad->device());
  r.keep = pad->contiguous();
  if (reinterpret_cast<uintptr_t>(r.keep.data_ptr()) % 8 != 0)
    r.keep = r.keep.clone();
  r.ptr = (const uint8_t*)r.keep.data_ptr<bool>();
  return r;
}

void check_norm_tensor(const char* name, const char* tn, const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), name, ": ", tn, " must be on the GPU, got device ",
              t.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat ||
                  t.scalar_type() == at::kBFloat16,
              name, ": ", tn, " must be fp32 or bf16, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": ", tn,
              " must be contiguous, got sizes ", t.sizes(), " strides ",
              t.strides());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, ": ",
              tn, " must be 16 B-aligned, got address ", t.data_ptr());
}

void check_norm_f32(const char* name, const char* tn, const at::Tensor& t,
                    const at::Tensor& ref, at::IntArrayRef shape) {
  TORCH_CHECK(t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.sizes() == shape && t.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, ": ", tn, " must be contiguous, 16 B-aligned fp32 ", shape,
              " on the device of the input, got ", t.scalar_type(), " sizes ",
              t.sizes(), " strides ", t.strides(), " on ", t.device());
}

void check_pair_norm(const char* name, const at::Tensor& pair,
                     const at::Tensor& bias) {
  check_norm_tensor(name, "pair", pair);
  TORCH_CHECK(pair.dim() == 4 && pair.size(2) == pair.size(3), name,
              ": pair must be (B, H, L, L), got sizes ", pair.sizes());
  TORCH_CHECK(bias.sizes() == pair.sizes(), name,
              ": pair and bias must have one shape, got pair ", pair.sizes(),
              " and bias ", bias.sizes());
  TORCH_CHECK(bias.scalar_type() == pair.scalar_type() &&
                  bias.device() == pair.device(),
              name, ": pair and bias must have one dtype and device, got ",
              pair.scalar_type(), " on ", pair.device(), " and ",
              bias.scalar_type(), " on ", bias.device());
  check_norm_tensor(name, "bias", bias);
  const int64_t H = pair.size(1), L = pair.size(3);
  TORCH_CHECK(H >= 4 && H % 4 == 0, name,
              ": needs H a multiple of 4 and >= 4, got H = ", H);
  TORCH_CHECK(L >= 8 && L % 8 == 0, name,
              ": needs L a multiple of 8 and >= 8, got L = ", L);
  // the kernels index 8-position units with 32 bits
  const int64_t units = pair.size(0) * H * L * (L / 8);
  TORCH_CHECK(units <= 0x7fffff00LL, name, ": B * H * L * L / 8 = ", units,
              " units do not fit 31 bits");
}

void check_row_norm(const char* name, const at::Tensor& x) {
  check_norm_tensor(name, "x", x);
  TORCH_CHECK(x.dim() == 2, name, ": x must be (N, E), got sizes ", x.sizes());
  const int64_t E = x.size(1);
  TORCH_CHECK(E >= 8 && E % 8 == 0 && E <= kRowNormMaxE, name,
              ": needs E a multiple of 8 in [8, ", kRowNormMaxE,
              "], got E = ", E);
}

}  // namespace

// -> (coef (B, L, L), rowerr (B, L)), fp32; 0 where i or j is padded
std::vector<at::Tensor> pair_norm_forward(at::Tensor pair, at::Tensor bias,
                                          std::optional<at::Tensor> pad) {
  check_pair_norm("pair_norm_forward", pair, bias);
  const int64_t B = pair.size(0), L = pair.size(3);
  const NormPad p = check_norm_pad("pair_norm_forward", pad, pair, {B, L});
  const auto f32 = pair.options().dtype(at::kFloat);
  auto coef = at::empty({B, L, L}, f32);
  auto uerr = at::empty({B, L, L / 8}, f32);
  if (B > 0) pair_norm_forward_launch(coef, uerr, pair, bias, p.ptr);
  return {coef, uerr.sum(-1)};
}

// -> (d_pair, d_bias = -d_pair), as pair
std::vector<at::Tensor> pair_norm_backward(at::Tensor gscale, at::Tensor coef,
                                           at::Tensor pair, at::Tensor bias) {
  check_pair_norm("pair_norm_backward", pair, bias);
  const int64_t B = pair.size(0), L = pair.size(3);
  check_norm_f32("pair_norm_backward", "gscale", gscale, pair, {B});
  check_norm_f32("pair_norm_backward", "coef", coef, pair, {B, L, L});
  auto d_pair = at::empty_like(pair);
  auto d_bias = at::empty_like(pair);
  if (B > 0)
    pair_norm_backward_launch(d_pair, d_bias, gscale, coef, pair, bias);
  return {d_pair, d_bias};
}

// x (N, E) -> (coef (N), err (N)), fp32; 0 at padded rows
std::vector<at::Tensor> row_norm_forward(at::Tensor x,
                                         std::optional<at::Tensor> pad) {
  check_row_norm("row_norm_forward", x);
  const int64_t N = x.size(0);
  const NormPad p = check_norm_pad("row_norm_forward", pad, x, {N});
  const auto f32 = x.options().dtype(at::kFloat);
  auto coef = at::empty({N}, f32);
  auto err = at::empty({N}, f32);
  if (N > 0) row_norm_forward_launch(coef, err, x, p.ptr);
  return {coef, err};
}

// -> dx = g_row[n] * coef[n] * x, as x
at::Tensor row_norm_backward(at::Tensor g_row, at::Tensor coef, at::Tensor x) {
  check_row_norm("row_norm_backward", x);
  const int64_t N = x.size(0);
  check_norm_f32("row_norm_backward", "g_row", g_row, x, {N});
  check_norm_f32("row_norm_backward", "coef", coef, x, {N});
  auto dx = at::empty_like(x);
  if (N > 0) row_norm_backward_launch(dx, g_row, coef, x);
  return dx;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("softmax_dropout_forward", &softmax_dropout_forward,
        "fused softmax(+mask,+bias)+dropout forward (gfx950)");
  m.def("softmax_dropout_backward_bias", &softmax_dropout_backward_bias,
        "fused softmax backward + broadcast bias gradient");
  m.def("softmax_dropout_backward_bias_supported",
        &softmax_dropout_backward_bias_supported,
        "fused bias-grad backward supports this shape");
  m.def("softmax_dropout_backward", &softmax_dropout_backward,
        "fused softmax+dropout backward, in-place on grad");
  m.def("layernorm_forward", &layernorm_forward, "fused LayerNorm forward");
  m.def("layernorm_backward", &layernorm_backward,
        "fused LayerNorm backward -> (dx, dgamma, dbeta)");
  m.def("rmsnorm_forward", &rmsnorm_forward, "fused RMSNorm forward");
  m.def("rmsnorm_backward", &rmsnorm_backward,
        "fused RMSNorm backward -> (dx, dgamma)");
  m.def("adam", &fused_adam, "fused AdamW step (in-place)");
  m.def("multi_tensor_l2norm", &multi_tensor_l2norm,
        "global L2 norm over a tensor list");
  m.def("fp32_to_bf16_sr", &fp32_to_bf16_sr,
        "stochastic-rounding fp32 -> bf16 copy");
  m.def("qkv_split_forward", &qkv_split_forward,
        "fused QKV head-split + q-scale -> (q, k, v) each (B*H, L, D)");
  m.def("qkv_split_backward", &qkv_split_backward,
        "fused QKV head-split backward -> dqkv (B, L, 3E)");
  m.def("gated_mul_forward", &gated_mul_forward,
        "fused (x+bx)*sigmoid(g+bg)");
  m.def("gated_mul_backward", &gated_mul_backward,
        "gated-mul backward -> (dx, dg[, bias colsums])");
  m.def("msa_arrange", &msa_arrange,
        "(B,S,L,H*D) <-> row/col head-major MSA layouts, 16 B both sides");
  m.def("attn_merge", &attn_merge,
        "(B*H, L, D) <-> (B, L, H*D) vectorized permute-copy");
  m.def("gelu_dropout_forward", &gelu_dropout_forward,
        "fused exact-GELU + bitfield dropout forward");
  m.def("gelu_dropout_backward", &gelu_dropout_backward,
        "fused GELU + dropout backward (recomputes gelu grad)");
  m.def("mfma_gemm_16x16x32", &mfma_gemm_16x16x32,
        "one-wave bf16 MFMA probe (fragment-layout unit test)");
  m.def("mfma_gemm_16x16x4_f32", &mfma_gemm_16x16x4_f32,
        "one-wave fp32 MFMA probe (fragment-layout unit test)");
  m.def("flash_attn_forward", &flash_attn_forward,
        "flash attention forward (bf16, D=64) -> (o, lse, seed)");
  m.def("flash_attn_backward", &flash_attn_backward,
        "flash attention backward -> (dq, dk, dv[, dS])");
  m.def("evo_attn_forward", &evo_attn_forward,
        "Evoformer attention forward (bf16, D=32, T<=512) -> (o, lse, seed)");
  m.def("evo_attn_backward", &evo_attn_backward,
        "Evoformer attention backward -> (dq, dk, dv[, dbias])");
  m.def("evo_attn_supported", &evo_attn_supported,
        "the shape / dtype checks of the Evoformer attention entries");
  m.def("pair_attn_forward", &pair_attn_forward,
        "pair-track attention forward (bf16, D=64, L<=512) -> (o, logits, "
        "lse, seed)");
  m.def("pair_attn_backward", &pair_attn_backward,
        "pair-track attention backward -> (dq, dk, dv, dbias)");
  m.def("pair_attn_supported", &pair_attn_supported,
        "the shape / dtype checks of the pair-track attention entries");
  m.def("dropout_add_ln_forward", &dropout_add_ln_forward,
        "fused dropout+residual+LayerNorm forward");
  m.def("dropout_add_forward", &dropout_add_forward,
        "fused dropout + residual add forward");
  m.def("dropout_add_backward", &dropout_add_backward,
        "fused dropout + residual add backward (dx only; d_res = grad)");
  m.def("embedding_backward", &embedding_backward,
        "atomic-scatter embedding gradient (fp32 accumulate)");
  m.def("cross_entropy_forward", &cross_entropy_forward,
        "fused online-logsumexp token cross entropy -> (loss, lse)");
  m.def("gaussian_basis_forward", &gaussian_basis_forward,
        "fused gaussian pair-basis from coords");
  m.def("gaussian_basis_backward", &gaussian_basis_backward,
        "gaussian pair-basis backward (d_coords, d_means, d_stds)");
  m.def("gaussian_basis_supported", &gaussian_basis_supported,
        "kernel supports this K");
  m.def("gaussian_pair_bias_forward", &gaussian_pair_bias_forward,
        "fully-fused gaussian pair bias: coords -> (B,H,L,L)");
  m.def("gaussian_pair_bias_backward", &gaussian_pair_bias_backward,
        "fused pair-bias backward (d_coords, d_means, d_stds, dW, db)");
  m.def("gaussian_pair_bias_supported", &gaussian_pair_bias_supported,
        "fused pair-bias kernel supports this K/H");
  m.def("cross_entropy_backward", &cross_entropy_backward,
        "cross entropy backward (softmax - onehot, no materialized fp32)");
  m.def("tri_contract", &tri_contract,
        "channel-last triangle contraction: (B,X,Z,C) x (B,Y,Z,C) -> (B,X,Y,C)");
  m.def("opm_forward", &opm_forward,
        "outer product mean: (B,S,I,32) x (B,S,J,32) -> (B,I,J,32,32)");
  m.def("opm_backward_a", &opm_backward_a,
        "outer product mean, gradient of a: (B,I,J,32,32) x (B,S,J,32) -> (B,S,I,32)");
  m.def("opm_backward_b", &opm_backward_b,
        "outer product mean, gradient of b: (B,I,J,32,32) x (B,S,I,32) -> (B,S,J,32)");
  m.def("opm_forward_w", &opm_forward_w,
        "opm_forward with an fp32 (B,I,J) weight in place of the scale");
  m.def("opm_backward_a_w", &opm_backward_a_w,
        "opm_backward_a with an fp32 (B,I,J) weight in place of the scale");
  m.def("opm_backward_b_w", &opm_backward_b_w,
        "opm_backward_b with an fp32 (B,I,J) weight in place of the scale");
  m.def("gated_mul_masked_forward", &gated_mul_masked_forward,
        "fused (x+bx)*sigmoid(g+bg)*m[row]");
  m.def("gated_mul_masked_backward", &gated_mul_masked_backward,
        "row-masked gated-mul backward -> (dx, dg[, bias colsums])");
  m.def("pair_arrange", &pair_arrange,
        "triangle attention: (B,I,J,H*D) view -> (B,H,R,T,D), optionally transposed");
  m.def("pair_merge", &pair_merge,
        "triangle attention: (B*H*R,T,D) -> (B,I,J,H*D), inverse of pair_arrange");
  m.def("pair_bias_arrange", &pair_bias_arrange,
        "triangle attention bias: (B,L,L,H) -> (B,H,L,L), optionally transposed");
  m.def("pair_bias_arrange_bwd", &pair_bias_arrange_bwd,
        "triangle attention bias gradient: (B,H,L,L) -> (B,L,L,H)");
  m.def("shared_dropout_add_forward", &shared_dropout_add_forward,
        "dropout shared along dim 1 or 2 of (B,R,T,C) + residual add -> (out, mask)");
  m.def("shared_dropout_add_ln_forward", &shared_dropout_add_ln_forward,
        "shared-axis dropout + residual + LayerNorm -> (normed, summed, mask, mean, invvar)");
  m.def("shared_dropout_add_backward", &shared_dropout_add_backward,
        "shared-axis dropout backward through the small mask -> (dx, dbias)");
  m.def("pair_coord_forward", &pair_coord_forward,
        "equivariant coordinate head: (B,H,L,L) pair track -> (B,L,3) update");
  m.def("pair_coord_backward", &pair_coord_backward,
        "coordinate head backward -> (dpair, dW1, db1, dW2, db2)");
  m.def("pair_coord_supported", &pair_coord_supported,
        "coordinate head kernel supports this head count (and, at 64 heads, L)");
  m.def("pair_dist_forward", &pair_dist_forward,
        "pair distance head: (B,64,L,L) pair track -> (B,L,L) fp32 distances");
  m.def("pair_dist_backward", &pair_dist_backward,
        "distance head backward -> (dpair, dW1, db1, dgamma, dbeta, dw2, db2)");
  m.def("pair_gauss_forward", &pair_gauss_forward,
        "Uni-Mol pair embedding forward, K = 128, H = 64, bf16 (gfx950)");
  m.def("pair_gauss_backward", &pair_gauss_backward,
        "Uni-Mol pair embedding backward: d_a, d_b and the parameter gradients");
  m.def("pair_gauss_supported", &pair_gauss_supported,
        "pair embedding kernels serve this (K, H, L)");
  m.def("pair_dist_supported", &pair_dist_supported,
        "distance head kernels serve this head count and L");
  m.def("pair_norm_forward", &pair_norm_forward,
        "pair norm regulariser: (B,H,L,L) pair, bias -> (coef (B,L,L), rowerr (B,L))");
  m.def("pair_norm_backward", &pair_norm_backward,
        "pair norm regulariser backward -> (d_pair, d_bias = -d_pair)");
  m.def("pair_norm_supported", &pair_norm_supported,
        "pair norm kernels serve this head count and L");
  m.def("row_norm_forward", &row_norm_forward,
        "row norm regulariser: (N,E) -> (coef (N), err (N))");
  m.def("row_norm_backward", &row_norm_backward,
        "row norm regulariser backward -> dx");
}
