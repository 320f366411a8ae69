// Python bindings for the gfx950 kernel extension.
#include <torch/extension.h>

torch::Tensor group_norm_fused(torch::Tensor x, int64_t groups,
                               torch::Tensor weight, torch::Tensor bias,
                               double eps, bool fuse_silu);
torch::Tensor layer_norm_bf16(torch::Tensor x, torch::Tensor gamma,
                              torch::Tensor beta, double eps);
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
torch::Tensor gemm256_bf16(torch::Tensor x, torch::Tensor w,
                           torch::Tensor bias, bool fuse_silu);
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

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("group_norm_fused", &group_norm_fused,
        "fused GroupNorm(+SiLU), NCHW bf16");
  m.def("layer_norm", &layer_norm_bf16, "LayerNorm over last dim, bf16");
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
  m.def("gemm256_bf16", &gemm256_bf16,
        "256x256x64 glds-staged MFMA GEMM, torch-Linear layout (+SiLU)");
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
}
