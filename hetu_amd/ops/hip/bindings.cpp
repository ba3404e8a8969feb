// pybind bindings for the _hetu_hip extension (gfx950 kernels).
#include <torch/extension.h>

#include <vector>

// norms.hip
std::vector<torch::Tensor> norm_fwd(torch::Tensor x,
                                    c10::optional<torch::Tensor> resid,
                                    torch::Tensor w,
                                    c10::optional<torch::Tensor> b,
                                    double eps);
std::vector<torch::Tensor> norm_bwd(torch::Tensor dy, torch::Tensor x,
                                    torch::Tensor w,
                                    c10::optional<torch::Tensor> mean,
                                    torch::Tensor rstd,
                                    c10::optional<torch::Tensor> dresid);
// reduce.hip
torch::Tensor colsum(torch::Tensor x);
// ltgemm.cpp
std::vector<torch::Tensor> lt_linear_gelu_aux(torch::Tensor x,
                                              torch::Tensor w,
                                              torch::Tensor b);
std::vector<torch::Tensor> lt_dgelu_bgrad(torch::Tensor dy, torch::Tensor w,
                                          torch::Tensor aux);
// swiglu.hip
torch::Tensor swiglu_fwd(torch::Tensor x);
torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor x);
// activations.hip
torch::Tensor gelu_fwd(torch::Tensor x);
torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x);
torch::Tensor silu_fwd(torch::Tensor x);
torch::Tensor silu_bwd(torch::Tensor dy, torch::Tensor x);
// rope.hip
torch::Tensor rope_fwd(torch::Tensor x, torch::Tensor cos, torch::Tensor sin);
torch::Tensor rope_bwd(torch::Tensor dy, torch::Tensor cos, torch::Tensor sin);
// softmax.hip
torch::Tensor softmax_fwd(torch::Tensor x);
torch::Tensor softmax_bwd(torch::Tensor dy, torch::Tensor y);
// ce.hip
std::vector<torch::Tensor> softmax_ce_fwd(torch::Tensor logits,
                                          torch::Tensor labels,
                                          int64_t ignore_index);
torch::Tensor softmax_ce_bwd(torch::Tensor dloss, torch::Tensor logits,
                             torch::Tensor labels, torch::Tensor lse,
                             int64_t ignore_index);
torch::Tensor vp_sumexp(torch::Tensor logits, torch::Tensor gmax);
torch::Tensor vp_ce_bwd(torch::Tensor gy, torch::Tensor logits,
                        torch::Tensor labels, torch::Tensor lse,
                        int64_t vstart, int64_t vend, int64_t ignore);
std::vector<torch::Tensor> vp_ce_local(torch::Tensor logits,
                                       torch::Tensor labels,
                                       int64_t vocab_start,
                                       int64_t vocab_end,
                                       int64_t ignore_index);
// dropout.hip
std::vector<torch::Tensor> dropout_fwd(torch::Tensor x, double p,
                                       int64_t seed, int64_t offset);
torch::Tensor dropout_bwd(torch::Tensor dy, torch::Tensor mask, double p,
                          int64_t seed, int64_t offset);
// embedding.hip
torch::Tensor embedding_fwd(torch::Tensor table, torch::Tensor ids);
torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor ids,
                            int64_t num_rows);
// adam.hip
void adam_step(torch::Tensor param32, torch::Tensor grad, torch::Tensor m,
               torch::Tensor v, double lr, double beta1, double beta2,
               double eps, double weight_decay, int64_t step,
               torch::Tensor out16, torch::Tensor bc_dev);
// gemm.hip
torch::Tensor gemm_bf16(torch::Tensor x, torch::Tensor w, bool trans_w);
// gemm_wgrad.hip
torch::Tensor gemm_wgrad_bf16(torch::Tensor gy, torch::Tensor x);
std::vector<torch::Tensor> gemm_wgrad_bias_bf16(torch::Tensor gy,
                                                torch::Tensor x);
// transpose.hip
torch::Tensor transpose2d(torch::Tensor w, c10::optional<torch::Tensor> out,
                          int64_t order);
// quant.hip
std::vector<torch::Tensor> quantize_blockwise(torch::Tensor x,
                                              std::string qtype,
                                              int64_t blocksize);
torch::Tensor dequantize_blockwise(torch::Tensor q, torch::Tensor absmax,
                                   std::string qtype, int64_t blocksize,
                                   int64_t numel,
                                   torch::ScalarType out_dtype);
// galvatron_dp.cpp
std::pair<double, std::vector<int64_t>> galvatron_dp(
    std::vector<double> times, std::vector<double> mems, int64_t L,
    int64_t S, double cap, int64_t buckets);
// attention.hip: the dense [B,H,S,D] entries and the variant choice
// (impl 0 = by shape, 1/2/3 = exactly that kernel generation)
std::vector<torch::Tensor> flash_attn_fwd(torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, bool causal,
                                          double scale, int64_t impl);
std::vector<torch::Tensor> flash_attn_bwd(torch::Tensor dout,
                                          torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, torch::Tensor out,
                                          torch::Tensor lse, bool causal,
                                          double scale, int64_t impl);
// attention_v2.hip: fused-qkv and packed-varlen forward
std::vector<torch::Tensor> flash_attn_fwd_qkv(torch::Tensor qkv, int64_t H,
                                              int64_t Hkv, int64_t D,
                                              bool causal, double scale);
std::vector<torch::Tensor> flash_attn_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor cu,
    int64_t max_seqlen, bool causal, double scale);
// attention_bwd_v2.hip: fused-qkv and packed-varlen backward
torch::Tensor flash_attn_bwd_qkv(torch::Tensor dout, torch::Tensor qkv,
                                 torch::Tensor out, torch::Tensor lse,
                                 int64_t H, int64_t Hkv, int64_t D,
                                 bool causal, double scale);
std::vector<torch::Tensor> flash_attn_varlen_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, torch::Tensor cu,
    int64_t max_seqlen, bool causal, double scale);
// rope.hip
void rope_qk_inplace(torch::Tensor qkv, torch::Tensor cs, torch::Tensor sn,
                     int64_t n_rot, int64_t D, int64_t sign);
// moe.hip
std::vector<torch::Tensor> moe_topk(torch::Tensor probs, int64_t K);
std::vector<torch::Tensor> moe_assign_slots(torch::Tensor idx,
                                            torch::Tensor w, int64_t E,
                                            int64_t C);
torch::Tensor moe_dispatch_rows(torch::Tensor x, torch::Tensor pos,
                                c10::optional<torch::Tensor> out);
torch::Tensor moe_dispatch_rows_bwd(torch::Tensor gsend,
                                    torch::Tensor slot_of);
torch::Tensor moe_gate_bwd(torch::Tensor g_w, torch::Tensor slot_of,
                           torch::Tensor probs, int64_t C);
torch::Tensor moe_combine_rows(torch::Tensor recv, torch::Tensor wk,
                               torch::Tensor slot_of);
std::vector<torch::Tensor> moe_combine_rows_bwd(
    torch::Tensor gy, torch::Tensor recv, torch::Tensor wk,
    torch::Tensor pos, torch::Tensor slot_of,
    c10::optional<torch::Tensor> out);
int64_t moe_gate_max_blocks();
int64_t moe_gate_tokens_per_block(int64_t E);
std::vector<torch::Tensor> moe_gate_fwd(torch::Tensor logits, int64_t K);
torch::Tensor moe_gate_grad(c10::optional<torch::Tensor> g_probs,
                            c10::optional<torch::Tensor> g_aux,
                            c10::optional<torch::Tensor> g_z,
                            torch::Tensor logits, torch::Tensor lse,
                            torch::Tensor cnt);
// attention_decode.hip
int64_t decode_attn_tile();
int64_t decode_attn_num_splits(int64_t B, int64_t Hkv, int64_t L,
                               int64_t cus);
std::vector<torch::Tensor> flash_attn_decode(torch::Tensor q,
                                             torch::Tensor k_cache,
                                             torch::Tensor v_cache,
                                             torch::Tensor kv_len,
                                             double scale,
                                             int64_t num_splits);

// embed_cache.cpp
void register_embed_cache(pybind11::module& m);
// dataloader.cpp
void register_dataloader(pybind11::module& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_embed_cache(m);
  register_dataloader(m);
  m.def("norm_fwd", &norm_fwd);
  m.def("norm_bwd", &norm_bwd);
  m.def("colsum", &colsum);
  m.def("lt_linear_gelu_aux", &lt_linear_gelu_aux);
  m.def("lt_dgelu_bgrad", &lt_dgelu_bgrad);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("silu_fwd", &silu_fwd);
  m.def("silu_bwd", &silu_bwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("rope_bwd", &rope_bwd);
  m.def("softmax_fwd", &softmax_fwd);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("softmax_ce_fwd", &softmax_ce_fwd);
  m.def("softmax_ce_bwd", &softmax_ce_bwd);
  m.def("vp_ce_local", &vp_ce_local);
  m.def("vp_sumexp", &vp_sumexp);
  m.def("vp_ce_bwd", &vp_ce_bwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_bwd", &dropout_bwd);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("adam_step", &adam_step);
  m.def("gemm_bf16", &gemm_bf16);
  m.def("gemm_wgrad_bf16", &gemm_wgrad_bf16);
  m.def("gemm_wgrad_bias_bf16", &gemm_wgrad_bias_bf16);
  m.def("transpose2d", &transpose2d, py::arg("w"),
        py::arg("out") = py::none(), py::arg("order") = 1);
  m.def("quantize_blockwise", &quantize_blockwise);
  m.def("dequantize_blockwise", &dequantize_blockwise);
  m.def("galvatron_dp", &galvatron_dp);
  m.def("flash_attn_fwd", &flash_attn_fwd, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("causal"), py::arg("scale"),
        py::arg("impl") = 0);
  m.def("flash_attn_bwd", &flash_attn_bwd, py::arg("dout"), py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"),
        py::arg("causal"), py::arg("scale"), py::arg("impl") = 0);
  m.def("flash_attn_fwd_qkv", &flash_attn_fwd_qkv);
  m.def("flash_attn_varlen_fwd", &flash_attn_varlen_fwd);
  m.def("flash_attn_varlen_bwd", &flash_attn_varlen_bwd);
  m.def("flash_attn_bwd_qkv", &flash_attn_bwd_qkv);
  m.def("rope_qk_inplace", &rope_qk_inplace);
  m.def("moe_topk", &moe_topk);
  m.def("moe_assign_slots", &moe_assign_slots);
  m.def("moe_dispatch_rows", &moe_dispatch_rows, pybind11::arg("x"),
        pybind11::arg("pos"), pybind11::arg("out") = pybind11::none());
  m.def("moe_dispatch_rows_bwd", &moe_dispatch_rows_bwd);
  m.def("moe_gate_bwd", &moe_gate_bwd);
  m.def("moe_combine_rows", &moe_combine_rows);
  m.def("moe_combine_rows_bwd", &moe_combine_rows_bwd, pybind11::arg("gy"),
        pybind11::arg("recv"), pybind11::arg("wk"), pybind11::arg("pos"),
        pybind11::arg("slot_of"), pybind11::arg("out") = pybind11::none());
  m.def("moe_gate_max_blocks", &moe_gate_max_blocks);
  m.def("moe_gate_tokens_per_block", &moe_gate_tokens_per_block);
  m.def("moe_gate_fwd", &moe_gate_fwd);
  m.def("moe_gate_grad", &moe_gate_grad);
  m.def("decode_attn_tile", &decode_attn_tile);
  m.def("decode_attn_num_splits", &decode_attn_num_splits);
  m.def("flash_attn_decode", &flash_attn_decode, py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"),
        py::arg("scale"), py::arg("num_splits") = 0);
}
