// Python bindings for the skypilot_amd CDNA4 kernels.
//
// Compiled with hipcc against libtorch; kernels live in the .hip TUs and
// are reached through extern "C" launch functions so this TU only needs
// the HIP runtime + torch headers.
#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <limits>
#include <vector>

#include "attn_append.h"
#include "attn_launch.h"
#include "kv_fp8_launch.h"

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")
#define CHECK_BF16(x) \
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, #x " must be bf16")

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// ---- extern "C" launchers from the .hip files -----------------------------
extern "C" {
void rmsnorm_fwd_launch(const void*, const void*, void*, float*, long long,
                        int, float, hipStream_t);
void rmsnorm_bwd_launch(const void*, const void*, const void*, const float*,
                        void*, float*, long long, int, hipStream_t);
void rope_launch(const void*, void*, const float*, const float*, const int*,
                 long long, int, int, bool, hipStream_t);
void adamw_launch(void*, float*, const void*, float*, float*, long long,
                  float, float, float, float, float, int, float, hipStream_t);
void cross_entropy_launch(void*, const int*, float*, long long, int, float,
                          int, hipStream_t);
void mfma_probe_launch(const void*, const void*, float*, hipStream_t);
void mfma32_probe_launch(const void*, const void*, float*, hipStream_t);
void trb16_probe_launch(float*, int, hipStream_t);
void permlane_probe_launch(float*, hipStream_t);
void skinny_gemm_launch(const void*, const void*, void*, int, int, int,
                        hipStream_t);
void skinny_gemm_swiglu_launch(const void*, const void*, void*, int, int,
                               int, hipStream_t);
void transpose_bf16_launch(const void*, void*, int, int, hipStream_t);
void skinny_gemm_fp8_launch(const void*, const float*, const void*, void*,
                            int, int, int, hipStream_t);
void gemm_nt_launch(const void*, const void*, void*, int, int, long long,
                    hipStream_t);
void adamw_mt_launch(const void*, const void*, const void*, const void*,
                     const void*, long long, float, float, float, float,
                     int, float, hipStream_t);
void decode_advance_launch(const void*, long long, void*, long long,
                           void*, const void*, int, hipStream_t);
void sample_tokens_launch(const void*, int, long long, const void*,
                          const void*, void*, void*, hipStream_t);
void token_logprobs_launch(const void*, int, long long, const void*,
                           const void*, void*, void*, void*, hipStream_t);
void decode_logprobs_launch(const void*, int, const void*, long long,
                            const void*, void*, void*, void*, const void*,
                            int, hipStream_t);
void decode_sample_advance_launch(const void*, int, void*, long long, void*,
                                  const void*, int, const void*,
                                  hipStream_t);
void rmsnorm_res_launch(const void*, const void*, const void*, void*, void*,
                        int, int, float, hipStream_t);
void rope_kvwrite_launch(const void*, void*, void*, void*, const void*,
                         const void*, const void*, const void*, int, int,
                         int, int, int, hipStream_t);
void swiglu_fwd_launch(const void*, void*, long long, int, hipStream_t);
void swiglu_bwd_launch(const void*, const void*, void*, long long, int,
                       hipStream_t);
void skinny_gemm_fp8_norm_launch(const void*, const float*, const void*,
                                 const void*, const void*, void*, float,
                                 void*, int, int, int, hipStream_t);
void attn_decode_qkv_launch(const void*, void*, void*, void*, const void*,
                            const void*, const int*, const int*,
                            const int*, int, int, int, int, float,
                            hipStream_t);
void attn_decode_launch(const void*, const void*, const void*, void*,
                        const int*, const int*, int, int, int, int, float,
                        hipStream_t);
}

// ---- RMSNorm --------------------------------------------------------------
torch::Tensor rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                          torch::Tensor inv_rms, double eps) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_GPU(w); CHECK_CONTIG(w); CHECK_BF16(w);
  const int H = (int)x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(w.numel() == H, "rmsnorm_fwd: w must have H = ", H,
              " elements, got ", w.numel());
  long long rows = x.numel() / H;
  CHECK_GPU(inv_rms); CHECK_CONTIG(inv_rms);
  TORCH_CHECK(inv_rms.scalar_type() == at::kFloat && inv_rms.numel() == rows,
              "rmsnorm_fwd: inv_rms must be fp32 with one entry per row");
  auto y = torch::empty_like(x);
  rmsnorm_fwd_launch(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     inv_rms.data_ptr<float>(), rows, H, (float)eps,
                     cur_stream());
  return y;
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor x, torch::Tensor w,
                                       torch::Tensor dy,
                                       torch::Tensor inv_rms) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_GPU(w); CHECK_CONTIG(w); CHECK_BF16(w);
  CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
  CHECK_GPU(inv_rms); CHECK_CONTIG(inv_rms);
  const int H = (int)x.size(-1);
  // The kernel keeps a row's columns in registers: 8 vectors of 8 per
  // thread at block=256 is its widest instantiation.
  TORCH_CHECK(H % 8 == 0 && H <= 16384,
              "rmsnorm_bwd: hidden dim must be a multiple of 8 and at most "
              "16384, got ", H);
  TORCH_CHECK(w.numel() == H, "rmsnorm_bwd: w must have H = ", H,
              " elements, got ", w.numel());
  TORCH_CHECK(dy.sizes() == x.sizes(), "rmsnorm_bwd: dy must have x's shape");
  long long rows = x.numel() / H;
  TORCH_CHECK(inv_rms.scalar_type() == at::kFloat && inv_rms.numel() == rows,
              "rmsnorm_bwd: inv_rms must be fp32 with one entry per row");
  auto dx = torch::empty_like(x);
  auto dw = torch::zeros({(long)H},
                         x.options().dtype(at::kFloat));
  rmsnorm_bwd_launch(x.data_ptr(), w.data_ptr(), dy.data_ptr(),
                     inv_rms.data_ptr<float>(), dx.data_ptr(),
                     dw.data_ptr<float>(), rows, H, cur_stream());
  return {dx, dw};
}

// ---- RoPE -----------------------------------------------------------------
torch::Tensor rope(torch::Tensor x, torch::Tensor cos_tab,
                   torch::Tensor sin_tab, torch::Tensor positions,
                   bool backward) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
  TORCH_CHECK(positions.scalar_type() == at::kInt,
              "rope: positions must be int32");
  CHECK_GPU(positions); CHECK_CONTIG(positions);
  TORCH_CHECK(x.dim() >= 2, "rope: x must be [..., heads, head_dim]");
  const int D = (int)x.size(-1);
  const int H = (int)x.size(-2);
  TORCH_CHECK(D % 2 == 0, "rope: head dim must be even, got ", D);
  long long n_tokens = x.numel() / ((long long)H * D);
  TORCH_CHECK(positions.numel() == n_tokens, "rope: need one position per "
              "token: ", n_tokens, " tokens, ", positions.numel(),
              " positions");
  for (const torch::Tensor& t : {cos_tab, sin_tab}) {
    CHECK_GPU(t); CHECK_CONTIG(t);
    TORCH_CHECK(t.scalar_type() == at::kFloat, "rope: cos/sin must be fp32");
    TORCH_CHECK(t.dim() >= 1 && t.size(-1) == D / 2,
                "rope: cos/sin last dim must be head_dim/2 = ", D / 2);
  }
  auto y = torch::empty_like(x);
  rope_launch(x.data_ptr(), y.data_ptr(), cos_tab.data_ptr<float>(),
              sin_tab.data_ptr<float>(), positions.data_ptr<int>(), n_tokens,
              H, D, backward, cur_stream());
  return y;
}

// ---- AdamW ----------------------------------------------------------------
void adamw_step(std::vector<torch::Tensor> params_bf16,
                std::vector<torch::Tensor> params_master,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> exp_avg,
                std::vector<torch::Tensor> exp_avg_sq, double lr, double beta1,
                double beta2, double eps, double weight_decay, int64_t step,
                double grad_scale, std::vector<bool> decay_mask) {
  auto stream = cur_stream();
  for (size_t i = 0; i < params_bf16.size(); ++i) {
    auto& p = params_bf16[i];
    long long n = p.numel();
    float wd = decay_mask.empty() || decay_mask[i] ? (float)weight_decay : 0.f;
    adamw_launch(p.data_ptr(), params_master[i].data_ptr<float>(),
                 grads[i].data_ptr(), exp_avg[i].data_ptr<float>(),
                 exp_avg_sq[i].data_ptr<float>(), n, (float)lr, (float)beta1,
                 (float)beta2, (float)eps, wd, (int)step, (float)grad_scale,
                 stream);
  }
}

// ---- Cross entropy --------------------------------------------------------
torch::Tensor cross_entropy_fused(torch::Tensor logits, torch::Tensor targets,
                                  double grad_scale, int64_t ignore_index) {
  CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
  TORCH_CHECK(targets.scalar_type() == at::kInt);
  const int V = (int)logits.size(-1);
  long long N = logits.numel() / V;
  auto loss = torch::empty({(long)N}, logits.options().dtype(at::kFloat));
  cross_entropy_launch(logits.data_ptr(), targets.data_ptr<int>(),
                       loss.data_ptr<float>(), N, V, (float)grad_scale,
                       (int)ignore_index, cur_stream());
  return loss;
}

// ---- Attention ------------------------------------------------------------
// The kernels index every tensor as dense [B,S,H,128] and tile S by 64:
// anything else would read or write the wrong elements, so it is
// rejected here.  `op` names the binding in the messages.
static void check_attn_qkv(const char* op, const torch::Tensor& Q,
                           const torch::Tensor& K, const torch::Tensor& V) {
  const torch::Tensor* ts[] = {&Q, &K, &V};
  const char* names[] = {"Q", "K", "V"};
  for (int i = 0; i < 3; ++i) {
    const torch::Tensor& t = *ts[i];
    TORCH_CHECK(t.is_cuda(), op, ": ", names[i], " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", names[i],
                " must be bf16, got ", t.scalar_type());
    TORCH_CHECK(t.dim() == 4, op, ": ", names[i],
                " must be [B, S, heads, 128], got ", t.dim(), " dims");
    TORCH_CHECK(t.is_contiguous(), op, ": ", names[i],
                " must be contiguous, got strides ", t.strides());
    TORCH_CHECK(t.size(3) == ATT_D, op, ": ", names[i],
                " head dim must be 128, got ", t.size(3));
  }
  const int64_t B = Q.size(0), S = Q.size(1), Hq = Q.size(2);
  TORCH_CHECK(S % 64 == 0, op, ": seq len must be a multiple of 64, got ", S);
  TORCH_CHECK(K.size(0) == B && K.size(1) == S, op,
              ": K must be [B, S, Hkv, 128] with Q's B = ", B, " and S = ", S,
              ", got ", K.sizes());
  TORCH_CHECK(V.sizes() == K.sizes(), op, ": V must have K's shape ",
              K.sizes(), ", got ", V.sizes());
  const int64_t Hkv = K.size(2);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, op, ": Hq = ", Hq,
              " must be a multiple of Hkv = ", Hkv);
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor Q, torch::Tensor K,
                                    torch::Tensor V, double scale,
                                    bool causal) {
  check_attn_qkv("attn_fwd", Q, K, V);
  const int B = (int)Q.size(0), S = (int)Q.size(1), Hq = (int)Q.size(2);
  const int Hkv = (int)K.size(2);
  auto O = torch::empty_like(Q);
  auto lse = torch::empty({B, Hq, S}, Q.options().dtype(at::kFloat));
  attn_fwd_launch(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(),
                  lse.data_ptr<float>(), B, S, Hq, Hkv, (float)scale, causal,
                  cur_stream());
  return {O, lse};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor Q, torch::Tensor K,
                                    torch::Tensor V, torch::Tensor O,
                                    torch::Tensor dO, torch::Tensor lse,
                                    double scale, bool causal,
                                    int64_t dkv_variant,
                                    int64_t dq_variant) {
  // dkv_variant: -1 = default (the shipped kernel, 2); 0 = v3 dkv,
  // 1 = pipelined v3 dkv, 2 = pipelined + heavy-first grid.
  // dq_variant: -1 = default (the shipped kernel); 0 = v3 dq,
  // 1 = pipelined v3 dq.
  check_attn_qkv("attn_bwd", Q, K, V);
  TORCH_CHECK(dkv_variant >= -1 && dkv_variant <= 2,
              "attn_bwd: dkv_variant must be -1, 0, 1 or 2");
  TORCH_CHECK(dq_variant >= -1 && dq_variant <= 1,
              "attn_bwd: dq_variant must be -1, 0 or 1");
  const int B = (int)Q.size(0), S = (int)Q.size(1), Hq = (int)Q.size(2);
  const int Hkv = (int)K.size(2);
  const torch::Tensor* outs[] = {&O, &dO};
  const char* out_names[] = {"O", "dO"};
  for (int i = 0; i < 2; ++i) {
    const torch::Tensor& t = *outs[i];
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, "attn_bwd: ",
                out_names[i], " must be bf16 on GPU, got ", t.scalar_type());
    TORCH_CHECK(t.sizes() == Q.sizes(), "attn_bwd: ", out_names[i],
                " must have Q's shape ", Q.sizes(), ", got ", t.sizes());
    TORCH_CHECK(t.is_contiguous(), "attn_bwd: ", out_names[i],
                " must be contiguous, got strides ", t.strides());
  }
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat,
              "attn_bwd: lse must be fp32 on GPU, got ", lse.scalar_type());
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == Hq &&
                  lse.size(2) == S,
              "attn_bwd: lse must be [B, Hq, S] = [", B, ", ", Hq, ", ", S,
              "], got ", lse.sizes());
  TORCH_CHECK(lse.is_contiguous(),
              "attn_bwd: lse must be contiguous, got strides ", lse.strides());
  auto dQ = torch::empty_like(Q);
  auto dK = torch::empty_like(K);
  auto dV = torch::empty_like(V);
  auto Dvec = torch::empty({(long)B * S * Hq}, Q.options().dtype(at::kFloat));
  attn_bwd_launch(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(),
                  dO.data_ptr(), lse.data_ptr<float>(),
                  Dvec.data_ptr<float>(), dQ.data_ptr(), dK.data_ptr(),
                  dV.data_ptr(), B, S, Hq, Hkv, (float)scale, causal,
                  (int)dkv_variant, (int)dq_variant, cur_stream());
  return {dQ, dK, dV};
}

// ---- argument checks of the decode-step bindings --------------------------
// The decode kernels index every tensor as dense memory of one fixed
// element type, so each tensor argument is checked here for device,
// dtype, contiguity, rank and shape before anything is launched; `op`
// and `name` go into the message.  VALUES held in device memory (slot
// ids, positions, kv lengths) are NOT validated: reading them back would
// put a host sync into the captured decode graph.  The caller owns them:
// 0 <= slot < slots, 0 <= position < S_max, 0 <= kv_len <= S_max.
static void check_dense(const char* op, const char* name,
                        const torch::Tensor& t, at::ScalarType dtype,
                        const torch::Tensor& first) {
  TORCH_CHECK(t.defined(), op, ": ", name, " must be a tensor");
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on GPU");
  TORCH_CHECK(t.device() == first.device(), op, ": ", name, " is on ",
              t.device(), " but the first tensor is on ", first.device());
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name,
              " must be contiguous, got sizes ", t.sizes(), " strides ",
              t.strides());
}

// Kc / Vc: dense bf16 [slots, S_max, Hkv, 128] of one shape.
static void check_kv_cache(const char* op, const torch::Tensor& Kc,
                           const torch::Tensor& Vc, int64_t Hq, int64_t Hkv,
                           const torch::Tensor& first) {
  const torch::Tensor* ts[] = {&Kc, &Vc};
  const char* names[] = {"Kc", "Vc"};
  for (int i = 0; i < 2; ++i) {
    check_dense(op, names[i], *ts[i], at::kBFloat16, first);
    TORCH_CHECK(ts[i]->dim() == 4, op, ": ", names[i],
                " must be [slots, S_max, Hkv, 128], got ", ts[i]->dim(),
                " dims");
    TORCH_CHECK(ts[i]->size(3) == ATT_D, op, ": ", names[i],
                " head dim must be 128, got ", ts[i]->size(3));
  }
  TORCH_CHECK(Vc.sizes() == Kc.sizes(), op, ": Vc must have Kc's shape ",
              Kc.sizes(), ", got ", Vc.sizes());
  TORCH_CHECK(Kc.size(0) > 0 && Kc.size(1) > 0 &&
                  Kc.size(1) <= std::numeric_limits<int>::max(),
              op, ": Kc must hold at least one slot and one row, got ",
              Kc.sizes());
  TORCH_CHECK(Hkv > 0 && Hkv == Kc.size(2), op, ": Hkv = ", Hkv,
              " must equal Kc.size(2) = ", Kc.size(2));
  TORCH_CHECK(Hq > 0 && Hq % Hkv == 0, op, ": Hq = ", Hq,
              " must be a positive multiple of Hkv = ", Hkv);
}

// One int32 entry per sequence, on the device.
static void check_index(const char* op, const char* name,
                        const torch::Tensor& t, int64_t B,
                        const torch::Tensor& first) {
  check_dense(op, name, t, at::kInt, first);
  TORCH_CHECK(t.dim() == 1 && t.size(0) == B, op, ": ", name,
              " must be a [B] = [", B, "] tensor, got ", t.sizes());
}

// cos / sin: fp32 [rows >= S_max, 64], row p for position p.
static void check_rope_tables(const char* op, const torch::Tensor& cos_tab,
                              const torch::Tensor& sin_tab, int64_t S_max,
                              const torch::Tensor& first) {
  const torch::Tensor* ts[] = {&cos_tab, &sin_tab};
  const char* names[] = {"cos", "sin"};
  for (int i = 0; i < 2; ++i) {
    check_dense(op, names[i], *ts[i], at::kFloat, first);
    TORCH_CHECK(ts[i]->dim() == 2 && ts[i]->size(1) == ATT_D / 2, op, ": ",
                names[i], " must be [rows, 64], got ", ts[i]->sizes());
    TORCH_CHECK(ts[i]->size(0) >= S_max, op, ": ", names[i], " has ",
                ts[i]->size(0), " rows, fewer than the cache's S_max = ",
                S_max);
  }
}

// One block per (sequence, q head) in grid.x.
static void check_grid(const char* op, int64_t B, int64_t Hq) {
  TORCH_CHECK(B * Hq <= std::numeric_limits<int>::max(), op, ": B * Hq = ",
              B * Hq, " exceeds the grid limit 2^31 - 1");
}

// The packed [B, (Hq + 2 Hkv) * 128] q|k|v rows of a decode step.
static void check_packed_qkv(const char* op, const torch::Tensor& qkv,
                             int64_t Hq, int64_t Hkv) {
  check_dense(op, "qkv", qkv, at::kBFloat16, qkv);
  TORCH_CHECK(Hq > 0 && Hkv > 0, op, ": Hq = ", Hq, " and Hkv = ", Hkv,
              " must be positive");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (Hq + 2 * Hkv) * ATT_D, op,
              ": qkv must be [B, (Hq + 2 * Hkv) * 128] = [B, ",
              (Hq + 2 * Hkv) * ATT_D, "], got ", qkv.sizes());
}

torch::Tensor attn_decode(torch::Tensor Q, torch::Tensor Kc,
                          torch::Tensor Vc, torch::Tensor kv_lens,
                          torch::Tensor slot_ids, double scale) {
  // decode attention over the slot KV cache (attention_decode.hip)
  const char* op = "attn_decode";
  check_dense(op, "Q", Q, at::kBFloat16, Q);
  TORCH_CHECK(Q.dim() == 3 && Q.size(2) == ATT_D, op,
              ": Q must be [B, Hq, 128], got ", Q.sizes());
  const int64_t B = Q.size(0), Hq = Q.size(1);
  check_kv_cache(op, Kc, Vc, Hq, Kc.dim() == 4 ? Kc.size(2) : 0, Q);
  check_index(op, "kv_lens", kv_lens, B, Q);
  check_index(op, "slot_ids", slot_ids, B, Q);
  check_grid(op, B, Hq);
  const int S_max = (int)Kc.size(1), Hkv = (int)Kc.size(2);
  auto O = torch::empty_like(Q);
  if (B > 0)
    attn_decode_launch(Q.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                       O.data_ptr(), kv_lens.data_ptr<int>(),
                       slot_ids.data_ptr<int>(), (int)B, S_max, (int)Hq,
                       Hkv, (float)scale, cur_stream());
  return O;
}

// Append attention over the slot KV cache (attention_append.hip): Sq new
// rows per sequence against cache rows [0, q_start + q_len).  The kernel
// indexes Q as dense [n,Sq,Hq,128] and the caches as dense
// [slots,S_max,Hkv,128]; the index tensors stay on the device.
torch::Tensor attn_append(torch::Tensor Q, torch::Tensor Kc,
                          torch::Tensor Vc, torch::Tensor slot_ids,
                          torch::Tensor q_start, torch::Tensor q_lens,
                          double scale) {
  const char* op = "attn_append";
  const torch::Tensor* ts[] = {&Q, &Kc, &Vc};
  const char* names[] = {"Q", "Kc", "Vc"};
  for (int i = 0; i < 3; ++i) {
    const torch::Tensor& t = *ts[i];
    TORCH_CHECK(t.is_cuda(), op, ": ", names[i], " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", names[i],
                " must be bf16, got ", t.scalar_type());
    TORCH_CHECK(t.dim() == 4, op, ": ", names[i],
                " must have 4 dims [.., .., heads, 128], got ", t.dim());
    TORCH_CHECK(t.is_contiguous(), op, ": ", names[i],
                " must be contiguous, got strides ", t.strides());
    TORCH_CHECK(t.size(3) == ATT_D, op, ": ", names[i],
                " head dim must be 128, got ", t.size(3));
  }
  const int64_t n = Q.size(0), Sq = Q.size(1), Hq = Q.size(2);
  const int64_t slots = Kc.size(0), S_max = Kc.size(1), Hkv = Kc.size(2);
  TORCH_CHECK(Sq > 0 && Sq % 64 == 0, op,
              ": chunk length Sq must be a positive multiple of 64, got ",
              Sq);
  TORCH_CHECK(Vc.sizes() == Kc.sizes(), op, ": Vc must have Kc's shape ",
              Kc.sizes(), ", got ", Vc.sizes());
  TORCH_CHECK(slots > 0 && S_max > 0, op,
              ": the cache must hold at least one slot and one row, got ",
              Kc.sizes());
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, op, ": Hq = ", Hq,
              " must be a multiple of Hkv = ", Hkv);
  TORCH_CHECK(n > 0 && n * Hq <= 65535, op, ": n * Hq = ", n * Hq,
              " must be in [1, 65535] (one grid row per sequence and head)");
  TORCH_CHECK(Q.device() == Kc.device() && Q.device() == Vc.device(), op,
              ": Q, Kc and Vc must be on one device");
  const torch::Tensor* idx[] = {&slot_ids, &q_start, &q_lens};
  const char* idx_names[] = {"slot_ids", "q_start", "q_lens"};
  for (int i = 0; i < 3; ++i) {
    const torch::Tensor& t = *idx[i];
    TORCH_CHECK(t.is_cuda() && t.device() == Q.device(), op, ": ",
                idx_names[i], " must be on Q's GPU");
    TORCH_CHECK(t.scalar_type() == at::kInt, op, ": ", idx_names[i],
                " must be int32, got ", t.scalar_type());
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.is_contiguous(), op,
                ": ", idx_names[i], " must be a contiguous [n] = [", n,
                "] tensor, got ", t.sizes());
  }
  auto O = torch::empty_like(Q);
  attn_append_launch(Q.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                     O.data_ptr(), slot_ids.data_ptr<int>(),
                     q_start.data_ptr<int>(), q_lens.data_ptr<int>(), (int)n,
                     (int)Sq, (int)Hq, (int)Hkv, (int)slots, (int)S_max,
                     (float)scale, cur_stream());
  return O;
}

torch::Tensor attn_decode_qkv(torch::Tensor qkv, torch::Tensor Kc,
                              torch::Tensor Vc, torch::Tensor cos_tab,
                              torch::Tensor sin_tab,
                              torch::Tensor positions,
                              torch::Tensor kv_lens,
                              torch::Tensor slot_ids, int64_t Hq,
                              int64_t Hkv, double scale) {
  // fused rope + cache-write + decode attention (attention_decode.hip)
  const char* op = "attn_decode_qkv";
  check_packed_qkv(op, qkv, Hq, Hkv);
  const int64_t B = qkv.size(0);
  check_kv_cache(op, Kc, Vc, Hq, Hkv, qkv);
  const int S_max = (int)Kc.size(1);
  check_rope_tables(op, cos_tab, sin_tab, S_max, qkv);
  check_index(op, "positions", positions, B, qkv);
  check_index(op, "kv_lens", kv_lens, B, qkv);
  check_index(op, "slot_ids", slot_ids, B, qkv);
  check_grid(op, B, Hq);
  auto O = torch::empty({B, Hq, (int64_t)ATT_D}, qkv.options());
  if (B > 0)
    attn_decode_qkv_launch(qkv.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                           O.data_ptr(), cos_tab.data_ptr(),
                           sin_tab.data_ptr(), positions.data_ptr<int>(),
                           kv_lens.data_ptr<int>(),
                           slot_ids.data_ptr<int>(), (int)B, S_max, (int)Hq,
                           (int)Hkv, (float)scale, cur_stream());
  return O;
}

// ---- FP8 KV cache (kv_fp8.h) ------------------------------------------------
// Code tensors uint8 [slots, S_max, Hkv, 128] and exponent tensors uint8
// [slots, S_max, Hkv], all four dense and of one cache.
static void check_kv_cache_fp8(const char* op, const torch::Tensor& Kc,
                               const torch::Tensor& Vc,
                               const torch::Tensor& Ke,
                               const torch::Tensor& Ve, int64_t Hq,
                               int64_t Hkv, const torch::Tensor& first) {
  const torch::Tensor* cs[] = {&Kc, &Vc};
  const char* cnames[] = {"Kc", "Vc"};
  for (int i = 0; i < 2; ++i) {
    check_dense(op, cnames[i], *cs[i], at::kByte, first);
    TORCH_CHECK(cs[i]->dim() == 4, op, ": ", cnames[i],
                " must be [slots, S_max, Hkv, 128], got ", cs[i]->dim(),
                " dims");
    TORCH_CHECK(cs[i]->size(3) == ATT_D, op, ": ", cnames[i],
                " head dim must be 128, got ", cs[i]->size(3));
  }
  TORCH_CHECK(Vc.sizes() == Kc.sizes(), op, ": Vc must have Kc's shape ",
              Kc.sizes(), ", got ", Vc.sizes());
  TORCH_CHECK(Kc.size(0) > 0 && Kc.size(1) > 0 &&
                  Kc.size(0) <= std::numeric_limits<int>::max() &&
                  Kc.size(1) <= std::numeric_limits<int>::max(),
              op, ": Kc must hold at least one slot and one row, got ",
              Kc.sizes());
  const torch::Tensor* es[] = {&Ke, &Ve};
  const char* enames[] = {"Ke", "Ve"};
  for (int i = 0; i < 2; ++i) {
    check_dense(op, enames[i], *es[i], at::kByte, first);
    TORCH_CHECK(es[i]->dim() == 3 && es[i]->size(0) == Kc.size(0) &&
                    es[i]->size(1) == Kc.size(1) &&
                    es[i]->size(2) == Kc.size(2),
                op, ": ", enames[i], " must be [slots, S_max, Hkv] = [",
                Kc.size(0), ", ", Kc.size(1), ", ", Kc.size(2), "], got ",
                es[i]->sizes());
  }
  TORCH_CHECK(Hkv > 0 && Hkv == Kc.size(2), op, ": Hkv = ", Hkv,
              " must equal Kc.size(2) = ", Kc.size(2));
  TORCH_CHECK(Hq > 0 && Hq % Hkv == 0, op, ": Hq = ", Hq,
              " must be a positive multiple of Hkv = ", Hkv);
}

// Quantising cache write of prefill / append rows (kv_write_fp8.hip):
// row i < lens[b] of k, v [n, S, Hkv, 128] goes to
// [slot_ids[b], starts[b] + i].
void kv_write_fp8(torch::Tensor k, torch::Tensor v, torch::Tensor Kc,
                  torch::Tensor Vc, torch::Tensor Ke, torch::Tensor Ve,
                  torch::Tensor slot_ids, torch::Tensor starts,
                  torch::Tensor lens) {
  const char* op = "kv_write_fp8";
  const torch::Tensor* ts[] = {&k, &v};
  const char* names[] = {"k", "v"};
  for (int i = 0; i < 2; ++i) {
    check_dense(op, names[i], *ts[i], at::kBFloat16, k);
    TORCH_CHECK(ts[i]->dim() == 4 && ts[i]->size(3) == ATT_D, op, ": ",
                names[i], " must be [n, S, Hkv, 128], got ", ts[i]->sizes());
  }
  TORCH_CHECK(v.sizes() == k.sizes(), op, ": v must have k's shape ",
              k.sizes(), ", got ", v.sizes());
  const int64_t n = k.size(0), S = k.size(1), Hkv = k.size(2);
  check_kv_cache_fp8(op, Kc, Vc, Ke, Ve, Hkv, Hkv, k);
  check_index(op, "slot_ids", slot_ids, n, k);
  check_index(op, "starts", starts, n, k);
  check_index(op, "lens", lens, n, k);
  TORCH_CHECK(S <= std::numeric_limits<int>::max() &&
                  n * S * Hkv <= std::numeric_limits<int>::max(),
              op, ": n * S * Hkv = ", n * S * Hkv,
              " exceeds the grid limit 2^31 - 1");
  if (n * S * Hkv > 0)
    kv_write_fp8_launch(k.data_ptr(), v.data_ptr(), Kc.data_ptr(),
                        Vc.data_ptr(), Ke.data_ptr(), Ve.data_ptr(),
                        slot_ids.data_ptr<int>(), starts.data_ptr<int>(),
                        lens.data_ptr<int>(), (int)n, (int)S, (int)Hkv,
                        (int)Kc.size(0), (int)Kc.size(1), cur_stream());
}

// attn_append over the FP8 KV cache (attention_append.hip).
torch::Tensor attn_append_fp8(torch::Tensor Q, torch::Tensor Kc,
                              torch::Tensor Vc, torch::Tensor Ke,
                              torch::Tensor Ve, torch::Tensor slot_ids,
                              torch::Tensor q_start, torch::Tensor q_lens,
                              double scale) {
  const char* op = "attn_append_fp8";
  check_dense(op, "Q", Q, at::kBFloat16, Q);
  TORCH_CHECK(Q.dim() == 4 && Q.size(3) == ATT_D, op,
              ": Q must be [n, Sq, Hq, 128], got ", Q.sizes());
  const int64_t n = Q.size(0), Sq = Q.size(1), Hq = Q.size(2);
  TORCH_CHECK(Sq > 0 && Sq % 64 == 0, op,
              ": chunk length Sq must be a positive multiple of 64, got ",
              Sq);
  check_kv_cache_fp8(op, Kc, Vc, Ke, Ve, Hq, Kc.dim() == 4 ? Kc.size(2) : 0,
                     Q);
  TORCH_CHECK(n > 0 && n * Hq <= 65535, op, ": n * Hq = ", n * Hq,
              " must be in [1, 65535] (one grid row per sequence and head)");
  check_index(op, "slot_ids", slot_ids, n, Q);
  check_index(op, "q_start", q_start, n, Q);
  check_index(op, "q_lens", q_lens, n, Q);
  auto O = torch::empty_like(Q);
  attn_append_fp8_launch(Q.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                         Ke.data_ptr(), Ve.data_ptr(), O.data_ptr(),
                         slot_ids.data_ptr<int>(), q_start.data_ptr<int>(),
                         q_lens.data_ptr<int>(), (int)n, (int)Sq, (int)Hq,
                         (int)Kc.size(2), (int)Kc.size(0), (int)Kc.size(1),
                         (float)scale, cur_stream());
  return O;
}

// Fused rope + cache write + decode attention over the FP8 KV cache
// (attention_decode_fp8.hip); the contract of attn_decode_qkv.
torch::Tensor attn_decode_qkv_fp8(torch::Tensor qkv, torch::Tensor Kc,
                                  torch::Tensor Vc, torch::Tensor Ke,
                                  torch::Tensor Ve, torch::Tensor cos_tab,
                                  torch::Tensor sin_tab,
                                  torch::Tensor positions,
                                  torch::Tensor kv_lens,
                                  torch::Tensor slot_ids, int64_t Hq,
                                  int64_t Hkv, double scale) {
  const char* op = "attn_decode_qkv_fp8";
  check_packed_qkv(op, qkv, Hq, Hkv);
  const int64_t B = qkv.size(0);
  check_kv_cache_fp8(op, Kc, Vc, Ke, Ve, Hq, Hkv, qkv);
  const int S_max = (int)Kc.size(1);
  check_rope_tables(op, cos_tab, sin_tab, S_max, qkv);
  check_index(op, "positions", positions, B, qkv);
  check_index(op, "kv_lens", kv_lens, B, qkv);
  check_index(op, "slot_ids", slot_ids, B, qkv);
  check_grid(op, B, Hq);
  auto O = torch::empty({B, Hq, (int64_t)ATT_D}, qkv.options());
  if (B > 0)
    attn_decode_qkv_fp8_launch(
        qkv.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), Ke.data_ptr(),
        Ve.data_ptr(), O.data_ptr(), cos_tab.data_ptr(), sin_tab.data_ptr(),
        positions.data_ptr<int>(), kv_lens.data_ptr<int>(),
        slot_ids.data_ptr<int>(), (int)B, S_max, (int)Hq, (int)Hkv,
        (float)scale, cur_stream());
  return O;
}

// W8 [O, I] e4m3fn bytes with one fp32 scale per output row.
static void check_fp8_weight(const char* op, const torch::Tensor& W8,
                             const torch::Tensor& scale, int64_t I,
                             const torch::Tensor& first) {
  TORCH_CHECK(W8.defined() && (W8.scalar_type() == at::kByte ||
                               W8.scalar_type() == at::kFloat8_e4m3fn),
              op, ": W8 must be uint8 or float8_e4m3fn, got ",
              W8.scalar_type());
  check_dense(op, "W8", W8, W8.scalar_type(), first);
  TORCH_CHECK(W8.dim() == 2 && W8.size(1) == I, op,
              ": W8 must be [O, I] with I = ", I, ", got ", W8.sizes());
  TORCH_CHECK(W8.size(0) >= 1 &&
                  W8.size(0) <= std::numeric_limits<int>::max(),
              op, ": W8 must have at least one row, got ", W8.sizes());
  check_dense(op, "scale", scale, at::kFloat, first);
  TORCH_CHECK(scale.numel() == W8.size(0), op, ": scale must have O = ",
              W8.size(0), " elements, got ", scale.numel());
}

std::vector<torch::Tensor> skinny_gemm_fp8_norm(
    torch::Tensor x, torch::Tensor res, torch::Tensor nw, double eps,
    torch::Tensor W8, torch::Tensor scale, bool want_xout) {
  // norm-fused fp8 GEMV (skinny_gemm.hip): y = rmsnorm(x+res)*nw @ W8^T
  const char* op = "skinny_gemm_fp8_norm";
  check_dense(op, "x", x, at::kBFloat16, x);
  TORCH_CHECK(x.dim() == 2, op, ": x must be [N, I], got ", x.sizes());
  const int N = (int)x.size(0), I = (int)x.size(1);
  TORCH_CHECK(I >= 1024 && I <= 4096 && I % 1024 == 0, op,
              ": I must be 1024, 2048, 3072 or 4096, got ", I);
  TORCH_CHECK(N >= 1 && N <= 2, op, ": N must be 1 or 2, got ", N);
  check_fp8_weight(op, W8, scale, I, x);
  const int O = (int)W8.size(0);
  TORCH_CHECK(O % 2 == 0, op, ": O must be even, got ", O);
  check_dense(op, "nw", nw, at::kBFloat16, x);
  TORCH_CHECK(nw.numel() == I, op, ": nw must have I = ", I,
              " elements, got ", nw.numel());
  const bool has_res = res.defined() && res.numel() > 0;
  if (has_res) {
    check_dense(op, "res", res, at::kBFloat16, x);
    TORCH_CHECK(res.sizes() == x.sizes(), op, ": res must be empty or have "
                "x's shape ", x.sizes(), ", got ", res.sizes());
  }
  auto y = torch::empty({N, O}, x.options());
  torch::Tensor xout;
  if (want_xout) xout = torch::empty_like(x);
  skinny_gemm_fp8_norm_launch(
      W8.data_ptr(), scale.data_ptr<float>(), x.data_ptr(),
      has_res ? res.data_ptr() : nullptr, nw.data_ptr(),
      want_xout ? xout.data_ptr() : nullptr, (float)eps, y.data_ptr(),
      N, I, O, cur_stream());
  if (!want_xout) xout = x;
  return {xout, y};
}

void adamw_step_mt(torch::Tensor ptrs, torch::Tensor wd_arr,
                   torch::Tensor sizes, torch::Tensor chunk_tensor,
                   torch::Tensor chunk_start, double lr, double beta1,
                   double beta2, double eps, int64_t step,
                   double grad_scale) {
  // One launch for the whole parameter list (adamw.hip multi-tensor).
  CHECK_GPU(ptrs); CHECK_GPU(chunk_tensor);
  adamw_mt_launch(ptrs.data_ptr(), wd_arr.data_ptr(), sizes.data_ptr(),
                  chunk_tensor.data_ptr(), chunk_start.data_ptr(),
                  (long long)chunk_tensor.numel(), (float)lr, (float)beta1,
                  (float)beta2, (float)eps, (int)step, (float)grad_scale,
                  cur_stream());
}

torch::Tensor skinny_gemm_swiglu(torch::Tensor GU, torch::Tensor W) {
  // Y[N,O] = silu(G)*U @ W^T where GU = [N, 2M] packed gate|up.
  CHECK_GPU(GU); CHECK_CONTIG(GU); CHECK_BF16(GU);
  CHECK_GPU(W); CHECK_CONTIG(W); CHECK_BF16(W);
  const int N = (int)GU.size(0), M = (int)GU.size(1) / 2;
  const int O = (int)W.size(0);
  TORCH_CHECK(W.size(1) == M, "skinny_gemm_swiglu: dims mismatch");
  TORCH_CHECK(N >= 1 && N <= 4, "skinny_gemm_swiglu: N must be 1..4");
  TORCH_CHECK(M % 512 == 0, "skinny_gemm_swiglu: M %% 512 != 0");
  auto y = torch::empty({N, O}, GU.options());
  skinny_gemm_swiglu_launch(W.data_ptr(), GU.data_ptr(), y.data_ptr(), N,
                            M, O, cur_stream());
  return y;
}

// Transpose-then-NT weight-gradient GEMM (wgrad_gemm.hip).
// The kernel moves whole 64x64 tiles of a 2-D tensor, takes int dims and
// reads and writes 16-byte vectors.
static bool tile_dims(const torch::Tensor& X) {
  return X.size(0) > 0 && X.size(1) > 0 && X.size(0) % 64 == 0 &&
         X.size(1) % 64 == 0 &&
         X.size(0) <= std::numeric_limits<int>::max() &&
         X.size(1) <= std::numeric_limits<int>::max();
}
static bool aligned16(const torch::Tensor& X) {
  return reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0;
}
static bool transposable(const torch::Tensor& X) {
  return tile_dims(X) && aligned16(X);
}

static void check_transpose_arg(const char* op, const char* name,
                                const torch::Tensor& X,
                                const torch::Tensor& first) {
  check_dense(op, name, X, at::kBFloat16, first);
  TORCH_CHECK(X.dim() == 2, op, ": ", name, " must be 2-D, got ", X.sizes());
  TORCH_CHECK(aligned16(X), op, ": ", name, " must start on a 16-byte "
              "boundary (storage offset ", X.storage_offset(), ")");
}

static void check_transpose_src(const char* op, const char* name,
                                const torch::Tensor& X,
                                const torch::Tensor& first) {
  check_transpose_arg(op, name, X, first);
  TORCH_CHECK(tile_dims(X), op, ": ", name, " dims must be positive "
              "multiples of 64 (dims % 64), got ", X.sizes());
}

torch::Tensor transpose_bf16(torch::Tensor X) {
  check_transpose_src("transpose_bf16", "X", X, X);
  int R = X.size(0), C = X.size(1);
  auto Y = torch::empty({C, R}, X.options());
  transpose_bf16_launch(X.data_ptr(), Y.data_ptr(), R, C, cur_stream());
  return Y;
}

// Y[c, r] = X[r, c] into a caller's contiguous [C, R] tensor, which may
// be a row range of a larger buffer.
void transpose_bf16_out(torch::Tensor X, torch::Tensor Y) {
  const char* op = "transpose_bf16_out";
  check_transpose_src(op, "X", X, X);
  check_transpose_arg(op, "Y", Y, X);
  TORCH_CHECK(Y.size(0) == X.size(1) &&
              Y.size(1) == X.size(0), op, ": Y must be [", X.size(1), ", ",
              X.size(0), "] for X ", X.sizes(), ", got ", Y.sizes());
  transpose_bf16_launch(X.data_ptr(), Y.data_ptr(), (int)X.size(0),
                        (int)X.size(1), cur_stream());
}

torch::Tensor gemm_nt(torch::Tensor A, torch::Tensor B) {
  // C[i,j] = sum_m A[i,m] * B[j,m]
  CHECK_GPU(A); CHECK_CONTIG(A); CHECK_BF16(A);
  CHECK_GPU(B); CHECK_CONTIG(B); CHECK_BF16(B);
  long long M = A.size(1);
  int I = A.size(0), J = B.size(0);
  TORCH_CHECK(B.size(1) == M, "gemm_nt: inner dims mismatch");
  TORCH_CHECK(M % 64 == 0, "gemm_nt: M % 64 != 0");
  TORCH_CHECK(I % 128 == 0 && J % 256 == 0, "gemm_nt: I%128/J%256");
  auto C = torch::empty({I, J}, A.options());
  gemm_nt_launch(A.data_ptr(), B.data_ptr(), C.data_ptr(), I, J, M,
                 cur_stream());
  return C;
}

torch::Tensor wgrad_tn(torch::Tensor dy, torch::Tensor x) {
  // dW[i,j] = sum_m dy[m,i] * x[m,j]  (nn.Linear weight grad).
  CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
  long long M = dy.size(0);
  int I = dy.size(1), J = x.size(1);
  TORCH_CHECK(x.size(0) == M, "wgrad_tn: token dims mismatch");
  auto dyT = transpose_bf16(dy);
  auto xT = transpose_bf16(x);
  return gemm_nt(dyT, xT);
}

// ---- Weight gradient of a linear layer ------------------------------------
// dW [out, in] = dy^T x, dy [M, out], x [M, in], by the library GEMM in
// one of three operand layouts (docs/KERNELS.md "Weight gradients"):
//   0  at::mm(dy.t(), x)      the call autograd makes: neither operand is
//                             contiguous along the contraction M
//   1  at::linear(dyT, xT)    both transposed first: the forward's layout
//   2  at::mm(dyT, x)         dy transposed only: the dgrad layout
// Transposed copies are scratch from the caching allocator, freed on
// return.  kWgradRoutes holds the layout measured fastest, transposes
// included, per (sum of outs, in) on MI355X at M = 24,576 (bench_wgrad_
// layouts.py; docs/BENCHMARKS.md "Weight-gradient layouts"; ms per call,
// GEMM + transposes).  The same entries also win at M = 8,192, the other
// token count measured (docs/KERNELS.md), so the table applies from
// kWgradMinTokens = 8,192 up; nothing below was measured.  Everything not
// listed, and every shape the transpose kernel cannot take, is 0.
struct WgradRoute {
  int64_t out, in;
  int route;
};
static const WgradRoute kWgradRoutes[] = {
    // gate|up: library 4.782, route 1 4.451, route 2 4.653
    {28672, 4096, 1},
    // down: library 2.910, route 1 2.961, route 2 2.668
    {4096, 14336, 2},
    // o (4096 x 4096) stays on the library: 0.671 against 0.727 and 0.666
    // q|k|v (6144 x 4096), which ops.qkv_linear hands over already packed,
    // stays on the library: 1.045 against 1.077 and 1.061 (as the three
    // separate products autograd made it was 1.391)
};
static const int64_t kWgradMinTokens = 8192;

static int wgrad_table_route(int64_t M, int64_t out, int64_t in) {
  if (M < kWgradMinTokens) return 0;
  for (const auto& r : kWgradRoutes)
    if (r.out == out && r.in == in) return r.route;
  return 0;
}

// Several dy that share one x (dq, dk, dv): one [sum out, M] transposed
// buffer, one GEMM, row views of one [sum out, in] result.
std::vector<torch::Tensor> linear_wgrad_packed(std::vector<torch::Tensor> dys,
                                               torch::Tensor x,
                                               int64_t route) {
  const char* op = "linear_wgrad";
  TORCH_CHECK(route >= -1 && route <= 2, op, ": route must be -1 (table), "
              "0 (library), 1 (both transposed) or 2 (dy transposed), got ",
              route);
  TORCH_CHECK(!dys.empty(), op, ": needs at least one dy");
  check_dense(op, "x", x, at::kBFloat16, x);
  TORCH_CHECK(x.dim() == 2, op, ": x must be [M, in], got ", x.sizes());
  const int64_t M = x.size(0), in = x.size(1);
  int64_t total = 0;
  // One rule for both routes: route 2 never transposes x, but a shape
  // with any dim off the 64-tile was not measured on any route, so it
  // takes the library call as well.
  bool tiles = transposable(x);
  for (const auto& dy : dys) {
    check_dense(op, "dy", dy, at::kBFloat16, x);
    TORCH_CHECK(dy.dim() == 2 && dy.size(0) == M, op, ": dy must be [M = ",
                M, ", out], got ", dy.sizes());
    total += dy.size(1);
    tiles = tiles && transposable(dy);
  }
  if (route < 0) route = wgrad_table_route(M, total, in);
  std::vector<torch::Tensor> dWs;
  if (route == 0 || !tiles) {
    for (const auto& dy : dys) dWs.push_back(at::mm(dy.t(), x));
    return dWs;
  }
  auto dyT = at::empty({total, M}, x.options());
  int64_t off = 0;
  for (const auto& dy : dys) {
    transpose_bf16_out(dy, dyT.narrow(0, off, dy.size(1)));
    off += dy.size(1);
  }
  auto dW = route == 1 ? at::linear(dyT, transpose_bf16(x)) : at::mm(dyT, x);
  if (dys.size() == 1) return {dW};
  off = 0;
  for (const auto& dy : dys) {
    dWs.push_back(dW.narrow(0, off, dy.size(1)));
    off += dy.size(1);
  }
  return dWs;
}

torch::Tensor linear_wgrad(torch::Tensor dy, torch::Tensor x, int64_t route) {
  return linear_wgrad_packed({dy}, x, route)[0];
}

torch::Tensor skinny_gemm_fp8(torch::Tensor X, torch::Tensor W8,
                              torch::Tensor scale) {
  // Y[N,O] = X[N,I] @ (scale[o] * W8[O,I])^T ; W8 = OCP e4m3fn bytes.
  const char* op = "skinny_gemm_fp8";
  check_dense(op, "X", X, at::kBFloat16, X);
  TORCH_CHECK(X.dim() == 2, op, ": X must be [N, I], got ", X.sizes());
  const int64_t N = X.size(0), I = X.size(1);
  TORCH_CHECK(N >= 1 && N <= 8, op, ": N must be 1..8, got ", N);
  TORCH_CHECK(I >= 16 && I % 16 == 0 &&
                  I <= std::numeric_limits<int>::max(),
              op, ": I must be a positive multiple of 16, got ", I);
  check_fp8_weight(op, W8, scale, I, X);
  const int64_t O = W8.size(0);
  auto y = torch::empty({N, O}, X.options());
  skinny_gemm_fp8_launch(W8.data_ptr(), scale.data_ptr<float>(),
                         X.data_ptr(), y.data_ptr(), (int)N, (int)I, (int)O,
                         cur_stream());
  return y;
}

torch::Tensor skinny_gemm(torch::Tensor X, torch::Tensor W) {
  // Y[N,O] = X[N,I] @ W[O,I]^T (decode GEMV; see skinny_gemm.hip)
  CHECK_GPU(X); CHECK_CONTIG(X); CHECK_BF16(X);
  CHECK_GPU(W); CHECK_CONTIG(W); CHECK_BF16(W);
  const int N = (int)X.size(0), I = (int)X.size(1), O = (int)W.size(0);
  TORCH_CHECK(W.size(1) == I, "skinny_gemm: inner dims mismatch");
  TORCH_CHECK(N >= 1 && N <= 8, "skinny_gemm: N must be 1..8");
  TORCH_CHECK(I % 512 == 0, "skinny_gemm: I must be a multiple of 512");
  auto y = torch::empty({N, O}, X.options());
  skinny_gemm_launch(W.data_ptr(), X.data_ptr(), y.data_ptr(), N, I, O,
                     cur_stream());
  return y;
}

std::vector<torch::Tensor> rmsnorm_res(torch::Tensor x, torch::Tensor res,
                                       torch::Tensor w, double eps) {
  // (x + res, rmsnorm(x + res) * w) in one kernel (decode_fused.hip)
  const char* op = "rmsnorm_res";
  check_dense(op, "x", x, at::kBFloat16, x);
  TORCH_CHECK(x.dim() >= 1, op, ": x must be [..., H], got a scalar");
  const int64_t H = x.size(-1);
  TORCH_CHECK(H >= 256 && H % 256 == 0 && H <= 8192, op,
              ": H must be a multiple of 256 and <= 8192, got ", H);
  check_dense(op, "res", res, at::kBFloat16, x);
  TORCH_CHECK(res.sizes() == x.sizes(), op, ": res must have x's shape ",
              x.sizes(), ", got ", res.sizes());
  check_dense(op, "w", w, at::kBFloat16, x);
  TORCH_CHECK(w.numel() == H, op, ": w must have H = ", H,
              " elements, got ", w.numel());
  const int64_t rows = x.numel() / H;
  TORCH_CHECK(rows <= std::numeric_limits<int>::max(), op, ": ", rows,
              " rows exceed the grid limit 2^31 - 1");
  auto x_out = torch::empty_like(x);
  auto h_out = torch::empty_like(x);
  if (rows > 0)
    rmsnorm_res_launch(x.data_ptr(), res.data_ptr(), w.data_ptr(),
                       x_out.data_ptr(), h_out.data_ptr(), (int)rows, (int)H,
                       (float)eps, cur_stream());
  return {x_out, h_out};
}

void decode_advance(torch::Tensor logits, torch::Tensor stage,
                    torch::Tensor ring, torch::Tensor ctr) {
  // fused greedy argmax + in-graph decode state bump (decode_fused.hip)
  const char* op = "decode_advance";
  check_dense(op, "logits", logits, at::kBFloat16, logits);
  TORCH_CHECK(logits.dim() >= 1, op,
              ": logits must be [b, V], got a scalar");
  const int64_t V = logits.size(-1);
  TORCH_CHECK(V >= 1 && V <= std::numeric_limits<int>::max(), op,
              ": V must be in [1, 2^31 - 1], got ", V);
  const int64_t b = logits.numel() / V;
  check_dense(op, "stage", stage, at::kInt, logits);
  TORCH_CHECK(stage.dim() == 2 && stage.size(0) == 6 && stage.size(1) == b,
              op, ": stage must be [6, b] = [6, ", b, "], got ",
              stage.sizes());
  check_dense(op, "ring", ring, at::kLong, logits);
  TORCH_CHECK(ring.dim() == 2 && ring.size(0) >= 1 &&
                  ring.size(0) <= std::numeric_limits<int>::max() &&
                  ring.size(1) == b,
              op, ": ring must be [chunk >= 1, b] = [chunk, ", b, "], got ",
              ring.sizes());
  check_dense(op, "ctr", ctr, at::kLong, logits);
  TORCH_CHECK(ctr.numel() == 1, op, ": ctr must hold one element, got ",
              ctr.sizes());
  TORCH_CHECK(b <= std::numeric_limits<int>::max(), op, ": b = ", b,
              " rows exceed the grid limit 2^31 - 1");
  if (b > 0)
    decode_advance_launch(logits.data_ptr(), V, stage.data_ptr(), b,
                          ring.data_ptr(), ctr.data_ptr(),
                          (int)ring.size(0), cur_stream());
}

// ---- seeded decode sampling (decode_sample.hip) ---------------------------
// The kernel sums 2^40-scaled 64-bit weights, at most V * 2^40 per row:
// V <= 2^23 keeps every sum below 2^63.
static const long long kSampleMaxV = 1ll << 23;

std::vector<torch::Tensor> sample_tokens(torch::Tensor logits,
                                         torch::Tensor samp,
                                         torch::Tensor counter) {
  CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
  CHECK_GPU(samp); CHECK_CONTIG(samp);
  CHECK_GPU(counter); CHECK_CONTIG(counter);
  TORCH_CHECK(logits.dim() == 2, "sample_tokens: logits must be [n, V]");
  TORCH_CHECK(samp.dtype() == torch::kInt32, "sample_tokens: samp int32");
  TORCH_CHECK(counter.dtype() == torch::kInt32,
              "sample_tokens: counter int32");
  const long long n = logits.size(0);
  const long long V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= kSampleMaxV,
              "sample_tokens: V must be in [1, 2^23], got ", V);
  TORCH_CHECK(samp.dim() == 2 && samp.size(0) == 5 && samp.size(1) == n,
              "sample_tokens: samp must be [5, n]");
  TORCH_CHECK(counter.dim() == 1 && counter.size(0) == n,
              "sample_tokens: counter must be [n]");
  auto tokens = torch::empty({n}, logits.options().dtype(torch::kInt64));
  auto tau = torch::empty({n}, logits.options().dtype(torch::kFloat));
  if (n > 0)
    sample_tokens_launch(logits.data_ptr(), (int)V, n, samp.data_ptr(),
                         counter.data_ptr(), tokens.data_ptr(),
                         tau.data_ptr(), cur_stream());
  return {tokens, tau};
}

void decode_sample_advance(torch::Tensor logits, torch::Tensor stage,
                           torch::Tensor ring, torch::Tensor ctr,
                           torch::Tensor samp) {
  // seeded sampling + in-graph decode state bump (decode_sample.hip)
  CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
  CHECK_GPU(stage); CHECK_CONTIG(stage);
  CHECK_GPU(ring); CHECK_CONTIG(ring);
  CHECK_GPU(ctr); CHECK_CONTIG(ctr);
  CHECK_GPU(samp); CHECK_CONTIG(samp);
  TORCH_CHECK(stage.dtype() == torch::kInt32,
              "decode_sample_advance: stage int32");
  TORCH_CHECK(ring.dtype() == torch::kInt64,
              "decode_sample_advance: ring int64");
  TORCH_CHECK(ctr.dtype() == torch::kInt64 && ctr.numel() == 1,
              "decode_sample_advance: ctr int64 [1]");
  TORCH_CHECK(samp.dtype() == torch::kInt32,
              "decode_sample_advance: samp int32");
  const long long V = logits.size(-1);
  TORCH_CHECK(V >= 1 && V <= kSampleMaxV,
              "decode_sample_advance: V must be in [1, 2^23], got ", V);
  const long long b = logits.numel() / V;
  TORCH_CHECK(stage.dim() == 2 && stage.size(0) == 6 && stage.size(1) == b,
              "decode_sample_advance: stage must be [6, b]");
  TORCH_CHECK(samp.dim() == 2 && samp.size(0) == 5 && samp.size(1) == b,
              "decode_sample_advance: samp must be [5, b]");
  TORCH_CHECK(ring.dim() == 2 && ring.size(0) >= 1 && ring.size(1) == b,
              "decode_sample_advance: ring must be [chunk, b]");
  if (b > 0)
    decode_sample_advance_launch(logits.data_ptr(), (int)V, stage.data_ptr(),
                                 b, ring.data_ptr(), ctr.data_ptr(),
                                 (int)ring.size(0), samp.data_ptr(),
                                 cur_stream());
}

// ---- token log-probabilities (decode_sample.hip) --------------------------
static const int64_t kLogprobTop = 20;

// logits [rows, V] with V in [1, 2^23] (the fixed-point sum's bound, as
// for the sampler); returns V.
static int64_t check_logprob_logits(const char* op,
                                    const torch::Tensor& logits) {
  check_dense(op, "logits", logits, at::kBFloat16, logits);
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be [n, V], got ",
              logits.sizes());
  const int64_t V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= kSampleMaxV, op,
              ": V must be in [1, 2^23], got ", V);
  TORCH_CHECK(logits.size(0) <= std::numeric_limits<int>::max(), op, ": ",
              logits.size(0), " rows exceed the grid limit 2^31 - 1");
  return V;
}

// Writes lp [n], top_lp [n, 20] and top_ids [n, 20] in place; rows with
// n_top < 0 are left as they are.  The values of ids and n_top are not
// read on the host.
void token_logprobs(torch::Tensor logits, torch::Tensor ids,
                    torch::Tensor n_top, torch::Tensor lp,
                    torch::Tensor top_lp, torch::Tensor top_ids) {
  const char* op = "token_logprobs";
  const int64_t V = check_logprob_logits(op, logits);
  const int64_t n = logits.size(0);
  check_dense(op, "ids", ids, at::kLong, logits);
  TORCH_CHECK(ids.dim() == 1 && ids.size(0) == n, op, ": ids must be [n] = [",
              n, "], got ", ids.sizes());
  check_index(op, "n_top", n_top, n, logits);
  check_dense(op, "lp", lp, at::kFloat, logits);
  TORCH_CHECK(lp.dim() == 1 && lp.size(0) == n, op, ": lp must be [n] = [", n,
              "], got ", lp.sizes());
  check_dense(op, "top_lp", top_lp, at::kFloat, logits);
  check_dense(op, "top_ids", top_ids, at::kInt, logits);
  TORCH_CHECK(top_lp.dim() == 2 && top_lp.size(0) == n &&
                  top_lp.size(1) == kLogprobTop,
              op, ": top_lp must be [n, 20] = [", n, ", 20], got ",
              top_lp.sizes());
  TORCH_CHECK(top_ids.dim() == 2 && top_ids.size(0) == n &&
                  top_ids.size(1) == kLogprobTop,
              op, ": top_ids must be [n, 20] = [", n, ", 20], got ",
              top_ids.sizes());
  if (n > 0)
    token_logprobs_launch(logits.data_ptr(), (int)V, n, ids.data_ptr(),
                          n_top.data_ptr(), lp.data_ptr(), top_lp.data_ptr(),
                          top_ids.data_ptr(), cur_stream());
}

void decode_logprobs(torch::Tensor logits, torch::Tensor stage,
                     torch::Tensor n_top, torch::Tensor lp_ring,
                     torch::Tensor top_lp_ring, torch::Tensor top_id_ring,
                     torch::Tensor ctr) {
  // in-graph log-probabilities of the token the advance kernel chose
  const char* op = "decode_logprobs";
  const int64_t V = check_logprob_logits(op, logits);
  const int64_t b = logits.size(0);
  check_dense(op, "stage", stage, at::kInt, logits);
  TORCH_CHECK(stage.dim() == 2 && stage.size(0) == 6 && stage.size(1) == b,
              op, ": stage must be [6, b] = [6, ", b, "], got ",
              stage.sizes());
  check_index(op, "n_top", n_top, b, logits);
  check_dense(op, "lp_ring", lp_ring, at::kFloat, logits);
  TORCH_CHECK(lp_ring.dim() == 2 && lp_ring.size(0) >= 1 &&
                  lp_ring.size(0) <= std::numeric_limits<int>::max() &&
                  lp_ring.size(1) == b,
              op, ": lp_ring must be [chunk >= 1, b] = [chunk, ", b,
              "], got ", lp_ring.sizes());
  const int64_t chunk = lp_ring.size(0);
  check_dense(op, "top_lp_ring", top_lp_ring, at::kFloat, logits);
  check_dense(op, "top_id_ring", top_id_ring, at::kInt, logits);
  TORCH_CHECK(top_lp_ring.dim() == 3 && top_lp_ring.size(0) == chunk &&
                  top_lp_ring.size(1) == b &&
                  top_lp_ring.size(2) == kLogprobTop,
              op, ": top_lp_ring must be [chunk, b, 20] = [", chunk, ", ", b,
              ", 20], got ", top_lp_ring.sizes());
  TORCH_CHECK(top_id_ring.dim() == 3 && top_id_ring.size(0) == chunk &&
                  top_id_ring.size(1) == b &&
                  top_id_ring.size(2) == kLogprobTop,
              op, ": top_id_ring must be [chunk, b, 20] = [", chunk, ", ", b,
              ", 20], got ", top_id_ring.sizes());
  check_dense(op, "ctr", ctr, at::kLong, logits);
  TORCH_CHECK(ctr.numel() == 1, op, ": ctr must hold one element, got ",
              ctr.sizes());
  if (b > 0)
    decode_logprobs_launch(logits.data_ptr(), (int)V, stage.data_ptr(), b,
                           n_top.data_ptr(), lp_ring.data_ptr(),
                           top_lp_ring.data_ptr(), top_id_ring.data_ptr(),
                           ctr.data_ptr(), (int)chunk, cur_stream());
}

torch::Tensor rope_kvwrite(torch::Tensor qkv, torch::Tensor kc,
                           torch::Tensor vc, torch::Tensor cos_tab,
                           torch::Tensor sin_tab, torch::Tensor positions,
                           torch::Tensor slot_ids, int64_t Hq,
                           int64_t Hkv) {
  // packed-qkv rope + KV-cache scatter (decode_fused.hip)
  const char* op = "rope_kvwrite";
  check_packed_qkv(op, qkv, Hq, Hkv);
  const int64_t n = qkv.size(0);
  check_kv_cache(op, kc, vc, Hq, Hkv, qkv);
  const int S_max = (int)kc.size(1);
  check_rope_tables(op, cos_tab, sin_tab, S_max, qkv);
  check_index(op, "positions", positions, n, qkv);
  check_index(op, "slot_ids", slot_ids, n, qkv);
  // 16 lanes per (token, head) row, 256 per block
  TORCH_CHECK(n * (Hq + 2 * Hkv) <= std::numeric_limits<int>::max(), op,
              ": n * (Hq + 2 * Hkv) = ", n * (Hq + 2 * Hkv),
              " exceeds the grid limit 2^31 - 1");
  auto q = torch::empty({n, Hq, (int64_t)ATT_D}, qkv.options());
  if (n > 0)
    rope_kvwrite_launch(qkv.data_ptr(), q.data_ptr(), kc.data_ptr(),
                        vc.data_ptr(), cos_tab.data_ptr(),
                        sin_tab.data_ptr(), positions.data_ptr(),
                        slot_ids.data_ptr(), (int)n, (int)Hq, (int)Hkv,
                        ATT_D, S_max, cur_stream());
  return q;
}

torch::Tensor swiglu_fwd(torch::Tensor gu) {
  CHECK_GPU(gu); CHECK_CONTIG(gu); CHECK_BF16(gu);
  const int M2 = (int)gu.size(-1);
  TORCH_CHECK(M2 % 16 == 0, "swiglu_fwd: last dim must be 2*M with "
              "M % 8 == 0, got ", M2);
  long long rows = gu.numel() / M2;
  auto sizes = gu.sizes().vec();
  sizes.back() = M2 / 2;
  auto y = torch::empty(sizes, gu.options());
  swiglu_fwd_launch(gu.data_ptr(), y.data_ptr(), rows, M2 / 2,
                    cur_stream());
  return y;
}

torch::Tensor swiglu_bwd(torch::Tensor gu, torch::Tensor dy) {
  CHECK_GPU(gu); CHECK_CONTIG(gu); CHECK_BF16(gu);
  CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
  const int M2 = (int)gu.size(-1);
  TORCH_CHECK(M2 % 16 == 0, "swiglu_bwd: last dim must be 2*M with "
              "M % 8 == 0, got ", M2);
  auto ysizes = gu.sizes().vec();
  ysizes.back() = M2 / 2;
  TORCH_CHECK(dy.sizes() == at::IntArrayRef(ysizes),
              "swiglu_bwd: dy must have the shape of swiglu_fwd(gu)");
  long long rows = gu.numel() / M2;
  auto dgu = torch::empty_like(gu);
  swiglu_bwd_launch(gu.data_ptr(), dy.data_ptr(), dgu.data_ptr(), rows,
                    M2 / 2, cur_stream());
  return dgu;
}

// ---- MFMA layout probe (used by tests/test_gpu_mfma.py) -------------------
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  CHECK_GPU(A); CHECK_BF16(A); CHECK_CONTIG(A); CHECK_CONTIG(B);
  TORCH_CHECK(A.size(0) == 16 && A.size(1) == 32);
  TORCH_CHECK(B.size(0) == 32 && B.size(1) == 16);
  auto C = torch::zeros({16, 16}, A.options().dtype(at::kFloat));
  mfma_probe_launch(A.data_ptr(), B.data_ptr(), C.data_ptr<float>(),
                    cur_stream());
  return C;
}

torch::Tensor mfma32_probe(torch::Tensor A, torch::Tensor B) {
  CHECK_GPU(A); CHECK_BF16(A); CHECK_CONTIG(A); CHECK_CONTIG(B);
  TORCH_CHECK(A.size(0) == 32 && A.size(1) == 16);
  TORCH_CHECK(B.size(0) == 16 && B.size(1) == 32);
  auto C = torch::zeros({32, 32}, A.options().dtype(at::kFloat));
  mfma32_probe_launch(A.data_ptr(), B.data_ptr(), C.data_ptr<float>(),
                      cur_stream());
  return C;
}

torch::Tensor trb16_probe(int64_t mode, torch::Tensor ref_dev) {
  auto out = torch::zeros({64, 4}, ref_dev.options().dtype(at::kFloat));
  trb16_probe_launch(out.data_ptr<float>(), (int)mode, cur_stream());
  return out;
}

torch::Tensor permlane_probe(torch::Tensor ref_dev) {
  auto out = torch::zeros({64, 2}, ref_dev.options().dtype(at::kFloat));
  permlane_probe_launch(out.data_ptr<float>(), cur_stream());
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("rope", &rope);
  m.def("adamw_step", &adamw_step);
  m.def("cross_entropy_fused", &cross_entropy_fused);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd, py::arg("Q"), py::arg("K"), py::arg("V"),
        py::arg("O"), py::arg("dO"), py::arg("lse"), py::arg("scale"),
        py::arg("causal"), py::arg("dkv_variant") = -1,
        py::arg("dq_variant") = -1);
  m.def("attn_decode", &attn_decode);
  m.def("attn_append", &attn_append);
  m.def("skinny_gemm", &skinny_gemm);
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8);
  m.def("transpose_bf16", &transpose_bf16);
  m.def("gemm_nt", &gemm_nt);
  m.def("wgrad_tn", &wgrad_tn);
  m.def("transpose_bf16_out", &transpose_bf16_out);
  m.def("linear_wgrad", &linear_wgrad, py::arg("dy"), py::arg("x"),
        py::arg("route") = -1);
  m.def("linear_wgrad_packed", &linear_wgrad_packed, py::arg("dys"),
        py::arg("x"), py::arg("route") = -1);
  m.def("adamw_step_mt", &adamw_step_mt);
  m.def("skinny_gemm_swiglu", &skinny_gemm_swiglu);
  m.def("rmsnorm_res", &rmsnorm_res);
  m.def("rope_kvwrite", &rope_kvwrite);
  m.def("decode_advance", &decode_advance);
  m.def("sample_tokens", &sample_tokens);
  m.def("decode_sample_advance", &decode_sample_advance);
  m.def("token_logprobs", &token_logprobs);
  m.def("decode_logprobs", &decode_logprobs);
  m.def("attn_decode_qkv", &attn_decode_qkv);
  m.def("kv_write_fp8", &kv_write_fp8);
  m.def("attn_decode_qkv_fp8", &attn_decode_qkv_fp8);
  m.def("attn_append_fp8", &attn_append_fp8);
  m.def("skinny_gemm_fp8_norm", &skinny_gemm_fp8_norm);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("mfma_probe", &mfma_probe);
  m.def("mfma32_probe", &mfma32_probe);
  m.def("trb16_probe", &trb16_probe);
  m.def("permlane_probe", &permlane_probe);
}
