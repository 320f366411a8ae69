// Python bindings for the gfx950 kernel extension.
#include <torch/extension.h>

torch::Tensor group_norm_fused(torch::Tensor x, int64_t groups,
                               torch::Tensor weight, torch::Tensor bias,
                               double eps, bool fuse_silu);
torch::Tensor layer_norm_bf16(torch::Tensor x, torch::Tensor gamma,
                              torch::Tensor beta, double eps);
std::tuple<torch::Tensor, torch::Tensor> layer_norm_fp8(torch::Tensor x,
                                                        torch::Tensor gamma,
                                                        torch::Tensor beta,
                                                        double eps);
torch::Tensor act_mul_bf16(torch::Tensor a, torch::Tensor b, bool gelu);
torch::Tensor extract_resize(torch::Tensor src, int64_t x1, int64_t y1,
                             int64_t x2, int64_t y2, int64_t ow, int64_t oh);
void blend_tile(torch::Tensor canvas, torch::Tensor tile, int64_t x1,
                int64_t y1, int64_t x2, int64_t y2, int64_t mx1, int64_t my1,
                int64_t mx2, int64_t my2, double sigma);
torch::Tensor attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                       int64_t heads, int64_t kv_heads, int64_t nk_real,
                       double scale);
torch::Tensor attn_fwd_packed(torch::Tensor q, torch::Tensor k,
                              torch::Tensor v, int64_t heads,
                              int64_t kv_heads, double scale);
torch::Tensor attn_fwd_qkv(torch::Tensor qkv, int64_t heads, double scale);
torch::Tensor attn_fwd_q_kv(torch::Tensor q, torch::Tensor kv, int64_t heads,
                            double scale);
torch::Tensor mfma_selftest(torch::Tensor a, torch::Tensor b);
torch::Tensor conv_nhwc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                        int64_t B, int64_t H, int64_t W, int64_t C, int64_t K,
                        int64_t rs, bool fuse_silu);
torch::Tensor group_norm_nhwc(torch::Tensor x, int64_t groups,
                              torch::Tensor weight, torch::Tensor bias,
                              double eps, bool fuse_silu,
                              c10::optional<torch::Tensor> addend);
std::vector<int64_t> group_norm_nhwc_plan(int64_t B, int64_t HW, int64_t C);
torch::Tensor conv_smallc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                          int64_t B, int64_t H, int64_t W, int64_t C,
                          int64_t K, int64_t rs, bool fuse_silu);
void conv_dense(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                torch::Tensor out, c10::optional<torch::Tensor> res1,
                c10::optional<torch::Tensor> res2, bool lrelu, double slope,
                double alpha, double beta1, bool up2);
torch::Tensor gemm256_bf16(torch::Tensor x, torch::Tensor w,
                           torch::Tensor bias, bool fuse_silu);
torch::Tensor gemm256_linear(torch::Tensor x, torch::Tensor w,
                             torch::Tensor bias, torch::Tensor res,
                             bool fuse_silu);
torch::Tensor gemm256_linear_ex(torch::Tensor x, torch::Tensor w,
                                torch::Tensor bias, torch::Tensor res,
                                bool fuse_silu, int64_t bn, int64_t split_k,
                                int64_t dp_tiles, int64_t sk_wgs);
std::tuple<int64_t, int64_t, int64_t, int64_t> gemm256_linear_plan(
    int64_t M, int64_t N, int64_t K);
torch::Tensor gemm_geglu(torch::Tensor x, torch::Tensor w_packed,
                         torch::Tensor bias_packed);
torch::Tensor gemm_geglu_ex(torch::Tensor x, torch::Tensor w_packed,
                            torch::Tensor bias_packed, int64_t bn);
torch::Tensor conv256_nhwc(torch::Tensor x, torch::Tensor wt,
                           torch::Tensor bias, torch::Tensor residual,
                           int64_t B, int64_t H,
                           int64_t W, int64_t C, int64_t K, int64_t rs,
                           int64_t stride, bool up2, bool fuse_silu);
torch::Tensor conv256_nhwc_ex(torch::Tensor x, torch::Tensor wt,
                              torch::Tensor bias, torch::Tensor residual,
                              int64_t B, int64_t H,
                              int64_t W, int64_t C, int64_t K, int64_t rs,
                              int64_t stride, bool up2, bool fuse_silu,
                              int64_t bn, int64_t split_k);
std::tuple<int64_t, int64_t> conv256_plan(int64_t M, int64_t K_out,
                                          int64_t Kdim);
torch::Tensor conv256_nhwc_sk(torch::Tensor x, torch::Tensor wt,
                              torch::Tensor bias, torch::Tensor residual,
                              int64_t B, int64_t H,
                              int64_t W, int64_t C, int64_t K, int64_t rs,
                              int64_t stride, bool up2, bool fuse_silu,
                              int64_t bn, int64_t dp_tiles, int64_t sk_wgs);
std::tuple<int64_t, int64_t, int64_t, int64_t> conv256_sched(int64_t M,
                                                             int64_t K_out,
                                                             int64_t Kdim);
std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t>>
conv256_sk_segments(int64_t tiles, int64_t kt, int64_t dp_tiles,
                    int64_t sk_wgs);
void qk_norm_rope(torch::Tensor q, torch::Tensor k, torch::Tensor q_weight,
                  torch::Tensor k_weight, torch::Tensor cos, torch::Tensor sin,
                  torch::Tensor out_q, torch::Tensor out_k, int64_t heads,
                  double eps, int64_t token_offset);
torch::Tensor norm_modulate(torch::Tensor x, torch::Tensor weight,
                            torch::Tensor scale, torch::Tensor shift,
                            double eps);
std::tuple<torch::Tensor, torch::Tensor> norm_modulate_fp8(
    torch::Tensor x, torch::Tensor weight, torch::Tensor scale,
    torch::Tensor shift, double eps);
torch::Tensor gated_residual(torch::Tensor x, torch::Tensor gate,
                             torch::Tensor y);
std::tuple<torch::Tensor, torch::Tensor> quant_rows_fp8(torch::Tensor x);
torch::Tensor gemm_fp8(torch::Tensor qa, torch::Tensor sa, torch::Tensor qw,
                       torch::Tensor sw, torch::Tensor bias, int64_t act);
std::tuple<torch::Tensor, torch::Tensor> quant_rows_fp8_pad(torch::Tensor x);
torch::Tensor gemm_geglu_fp8(torch::Tensor qa, torch::Tensor sa,
                             torch::Tensor qw_packed, torch::Tensor sw_packed,
                             torch::Tensor bias_packed);
std::tuple<torch::Tensor, torch::Tensor> quant_rows_mxfp8(torch::Tensor x);
torch::Tensor gemm_mxfp8(torch::Tensor qa, torch::Tensor ea, torch::Tensor qw,
                         torch::Tensor sw, torch::Tensor bias, int64_t act);
std::tuple<torch::Tensor, torch::Tensor> gemm_mxfp8_emit(
    torch::Tensor qa, torch::Tensor ea, torch::Tensor qw, torch::Tensor sw,
    torch::Tensor bias, int64_t act);
std::vector<torch::Tensor> attn_quant_fp8(torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, int64_t heads);
torch::Tensor attn_fwd_fp8(torch::Tensor qq, torch::Tensor qs,
                           torch::Tensor kc, torch::Tensor ks,
                           torch::Tensor vc, torch::Tensor vs, int64_t nk,
                           double scale);
torch::Tensor attn_fwd_fp8_sparse(torch::Tensor qq, torch::Tensor qs,
                                  torch::Tensor kc, torch::Tensor ks,
                                  torch::Tensor vc, torch::Tensor vs,
                                  int64_t nk, double scale, torch::Tensor idx,
                                  torch::Tensor cnt);
int64_t attn_fp8_qrows();
int64_t attn_fp8_sp();
std::tuple<torch::Tensor, torch::Tensor> quant_nhwc_fp8(torch::Tensor x);
torch::Tensor conv_fp8_nhwc(torch::Tensor q, torch::Tensor sa, torch::Tensor qw,
                            torch::Tensor sw, torch::Tensor bias,
                            torch::Tensor res, int64_t B, int64_t H, int64_t W,
                            int64_t C, int64_t K_out, int64_t RS,
                            int64_t stride, bool fuse_silu);
torch::Tensor conv_fp8_nhwc_ex(torch::Tensor q, torch::Tensor sa,
                               torch::Tensor qw, torch::Tensor sw,
                               torch::Tensor bias, torch::Tensor res,
                               int64_t B, int64_t H, int64_t W, int64_t C,
                               int64_t K_out, int64_t RS, int64_t stride,
                               bool fuse_silu, int64_t bn);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("group_norm_fused", &group_norm_fused,
        "fused GroupNorm(+SiLU), NCHW bf16");
  m.def("layer_norm", &layer_norm_bf16, "LayerNorm over last dim, bf16");
  m.def("layer_norm_fp8", &layer_norm_fp8,
        "quant_rows_fp8_pad(layer_norm(...)) in one launch -> (float8_e4m3fn "
        "[..., Cp], fp32 row scale [...]); C % 64 == 0, C <= 2048");
  m.def("act_mul", &act_mul_bf16, "a * act(b) elementwise, bf16");
  m.def("extract_resize", &extract_resize,
        "crop region of [B,H,W,C] f32 -> Lanczos-3 resample");
  m.def("blend_tile", &blend_tile,
        "fused resample + blurred-rect mask + composite (in-place canvas)");
  m.def("attn_fwd", &attn_fwd, "flash attention forward, bf16 MFMA");
  m.def("attn_fwd_packed", &attn_fwd_packed,
        "flash attention on packed [B,N,H*D] QKV (no host reshapes)");
  m.def("attn_fwd_qkv", &attn_fwd_qkv,
        "self-attention on fused [B,N,3*H*D] projection output");
  m.def("attn_fwd_q_kv", &attn_fwd_q_kv,
        "cross-attention on q [B,Nq,H*D] + fused kv [B,Nk,2*H*D]");
  m.def("mfma_selftest", &mfma_selftest,
        "single-wave 16x16x32 bf16 MFMA with the kernel fragment layouts");
  m.def("conv_nhwc", &conv_nhwc,
        "implicit-GEMM 3x3/1x1 NHWC bf16 conv on MFMA (+fused SiLU)");
  m.def("group_norm_nhwc", &group_norm_nhwc,
        "fused GroupNorm(+SiLU), NHWC bf16; addend [B, C] bf16 is added per "
        "sample (rounded to bf16) before the statistics",
        py::arg("x"), py::arg("groups"), py::arg("weight"), py::arg("bias"),
        py::arg("eps"), py::arg("fuse_silu"), py::arg("addend") = py::none());
  m.def("group_norm_nhwc_plan", &group_norm_nhwc_plan,
        "(B, HW, C) -> (threads, pixels per step, slots per lane, blocks per "
        "image, pixels per block) of the two-pass NHWC GroupNorm; launches "
        "nothing");
  m.def("conv_smallc", &conv_smallc,
        "small-C NHWC conv (stem convs, C <= 8)");
  m.def("conv_dense", &conv_dense,
        "3x3 NHWC bf16 conv for K_out <= 64 on channel-slice views: out = "
        "bf16(alpha * lrelu(conv(x) + bias) + beta1 * res1 + res2), written "
        "in place into `out`; up2 fuses a nearest 2x upsample of x",
        py::arg("x"), py::arg("wt"), py::arg("bias"), py::arg("out"),
        py::arg("res1") = py::none(), py::arg("res2") = py::none(),
        py::arg("lrelu") = false, py::arg("slope") = 0.0,
        py::arg("alpha") = 1.0, py::arg("beta1") = 1.0,
        py::arg("up2") = false);
  m.def("gemm256_bf16", &gemm256_bf16,
        "256x256x64 glds-staged MFMA GEMM, torch-Linear layout (+SiLU)");
  m.def("gemm256_linear", &gemm256_linear,
        "torch-Linear on the 256-tile GEMM with the N-tile width, K split and "
        "stream-K tail chosen per call: act(x W^T + bias) + res, x [M,K], "
        "w [N,K], res [M,N] bf16 or empty");
  m.def("gemm256_linear_ex", &gemm256_linear_ex,
        "gemm256_linear with the variant pinned: bn in {128, 256, 320} and "
        "split_k (0 = chooser), or with sk_wgs >= 1 the stream-K schedule "
        "(bn, dp_tiles, sk_wgs) as conv256_nhwc_sk");
  m.def("gemm256_linear_plan", &gemm256_linear_plan,
        "(M, N, K) -> (bn, split_k, dp_tiles, sk_wgs) gemm256_linear runs; "
        "launches nothing");
  m.def("gemm_geglu", &gemm_geglu,
        "(x W_value^T + b_value) * gelu_tanh(x W_gate^T + b_gate) on the "
        "256-tile GEMM: x [M,K] bf16, weight [2*inner,K] bf16 and fp32 bias "
        "(or empty) as dispatch.pack_geglu_weight pairs them -> [M,inner]");
  m.def("gemm_geglu_ex", &gemm_geglu_ex,
        "gemm_geglu with the N-tile width pinned: bn in {128, 256}; 0 = "
        "chooser");
  m.def("conv256_nhwc", &conv256_nhwc,
        "256-tile implicit-GEMM 3x3/1x1 NHWC conv on the same template; "
        "N-tile width and K split chosen per call");
  m.def("conv256_nhwc_ex", &conv256_nhwc_ex,
        "conv256_nhwc with the variant pinned: bn in {128, 256, 320} and "
        "split_k (clamped to the K-tile count); 0 = chooser");
  m.def("conv256_plan", &conv256_plan,
        "(M, K_out, Kdim) -> (bn, split_k) of the round-counting plan (the "
        "one used with the stream-K tail off); launches nothing");
  m.def("conv256_sched", &conv256_sched,
        "(M, K_out, Kdim) -> (bn, split_k, dp_tiles, sk_wgs) conv256_nhwc "
        "runs; sk_wgs = 0: no stream-K tail; launches nothing");
  m.def("conv256_nhwc_sk", &conv256_nhwc_sk,
        "conv256_nhwc with the schedule pinned: bn, the first dp_tiles tiles "
        "whole, the rest cut into sk_wgs ranges of K-tile steps");
  m.def("conv256_sk_segments", &conv256_sk_segments,
        "(tiles, kt, dp_tiles, sk_wgs) -> [(range, tile, kt0, kt1, slot)] "
        "of the stream-K tail, slot -1 = whole tile; launches nothing");
  m.def("qk_norm_rope", &qk_norm_rope,
        "per-head RMSNorm + RoPE of strided q/k views into [B,Ntot,H*D] "
        "buffers at a token offset");
  m.def("norm_modulate", &norm_modulate,
        "row RMSNorm (fp32 weight) or affine-free LayerNorm (empty weight) "
        "+ optional adaLN (1+scale)/shift");
  m.def("norm_modulate_fp8", &norm_modulate_fp8,
        "quant_rows_fp8(norm_modulate(...)) in one launch -> (float8_e4m3fn "
        "[B,N,C], fp32 row scale [B,N]); C % 128 == 0, C <= 8192");
  m.def("gated_residual", &gated_residual, "x + gate[b] * y, bf16");
  m.def("quant_rows_fp8", &quant_rows_fp8,
        "bf16 [M,K] -> (float8_e4m3fn [M,K], fp32 row scale [M] = amax/448)");
  m.def("gemm_fp8", &gemm_fp8,
        "act((qa . qw^T) * sa[m] * sw[n] + bias[n]) -> bf16 on the block-"
        "scaled 16x16x128 MFMA; act 0 none, 1 SiLU, 2 GELU-tanh");
  m.def("quant_rows_fp8_pad", &quant_rows_fp8_pad,
        "quant_rows_fp8 for K % 64 == 0: q [M,Kp] at the pitch Kp = K rounded "
        "up to 128, zero bytes in [K, Kp); the scale is of the K real elements");
  m.def("gemm_geglu_fp8", &gemm_geglu_fp8,
        "(a * sa * sw_a + b_a) * gelu_tanh(g * sa * sw_g + b_g) -> bf16 "
        "[M,inner]: qw [2*inner,K] e4m3, sw and bias [2*inner] as "
        "dispatch.pack_geglu_weight pairs value and gate rows");
  m.def("quant_rows_mxfp8", &quant_rows_mxfp8,
        "bf16 [M,K] -> (float8_e4m3fn [M,K], uint8 E8M0 block scales "
        "[M,K/32]): one power-of-two scale per 32 adjacent elements");
  m.def("gemm_mxfp8", &gemm_mxfp8,
        "act((sum_kb 2^exp[m][kb] * dot32(qa, qw)) * sw[n] + bias[n]) -> bf16 "
        "with the block scales applied by the 16x16x128 MFMA; act as gemm_fp8");
  m.def("gemm_mxfp8_emit", &gemm_mxfp8_emit,
        "quant_rows_mxfp8(gemm_mxfp8(...)) in the GEMM epilogue -> "
        "(float8_e4m3fn [M,N], uint8 [M,N/32]); N % 32 == 0");
  m.def("attn_quant_fp8", &attn_quant_fp8,
        "bf16 q [B,Nq,H*128], k, v [B,Nk,H*128] -> (q codes, q scale "
        "[B,Nq,H], k codes [B,H,Np,128] with the channel mean removed, k "
        "scale [B,H,Np/128], v codes [B,H,128,Np] keys permuted per 128-tile, "
        "v scale [B,H,128], k mean [B,H*128]); Np = Nk rounded up to 128");
  m.def("attn_fwd_fp8", &attn_fwd_fp8,
        "e4m3 flash attention forward on attn_quant_fp8's buffers -> bf16 "
        "[B,Nq,H*128]; both products on the 16x16x128 MFMA");
  m.def("attn_fwd_fp8_sparse", &attn_fwd_fp8_sparse,
        "attn_fwd_fp8 over a key-tile list per 256-row q-block: int32 idx "
        "[nqb, maxc] ascending 128-key tile numbers, cnt [nqb] valid entries");
  m.def("quant_nhwc_fp8", &quant_nhwc_fp8,
        "bf16 [B,H,W,C] -> (float8_e4m3fn [B,H,W,C], fp32 image scale [B] = "
        "amax/448 over the image)");
  m.def("conv_fp8_nhwc", &conv_fp8_nhwc,
        "act(conv(q, qw) * sa[image] * sw[n] + bias[n]) + res -> bf16 "
        "[B,Ho,Wo,K_out] on the block-scaled 16x16x128 MFMA: q [B,H,W,C] e4m3, "
        "qw [K_out, RS*C rounded up to 128] e4m3 (c innermost); 3x3 pad 1 "
        "stride 1 / 2 or 1x1, C % 64 == 0");
  m.def("conv_fp8_nhwc_ex", &conv_fp8_nhwc_ex,
        "conv_fp8_nhwc with the N-tile width pinned: bn in {256, 320}; 0 = "
        "chooser");
  m.attr("ATTN_FP8_QROWS") = attn_fp8_qrows();
  m.attr("ATTN_FP8_SP") = attn_fp8_sp();
}
