// What the two decode-attention translation units share: attention_decode.hip
// (VALU kernel; it defines everything declared here) and
// attention_decode_mfma.hip (MFMA kernel for wide GQA groups).
#pragma once
#include <vector>
#include <torch/extension.h>
#include "common.h"

constexpr int DEC_BN = 64;             // split unit: splits own whole 64-key units
constexpr int DEC_MAX_SPLITS = 64;

struct DecArgs {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  const int* kv_len;
  bf16* out;          // [B, H, D]
  float* lse;         // [B, H]
  float* ws_o;        // [B, H, ns, D], normalised partial outputs
  float* ws_lse;      // [B, H, ns]
  long long q_bs, q_hs;
  long long k_bs, k_hs, k_rs;
  long long v_bs, v_hs, v_rs;
  int H, Hkv, L, ns;
  float scale;
};

// a checked call, its outputs and the split workspace (undefined at ns == 1)
struct DecCall {
  DecArgs a;
  torch::Tensor out, lse, ws;
  int64_t B, H, Hkv, D;
  bool empty;         // B == 0 or H == 0: nothing to launch
};

int64_t decode_attn_num_splits(int64_t B, int64_t Hkv, int64_t L,
                               int64_t cus);
void dec_check_strides(const torch::Tensor& t, const char* what);
// every TORCH_CHECK of flash_attn_decode, then out / lse / workspace and the
// kernel arguments; key_tile is the caller's block tile (bounds L)
DecCall dec_prepare(const torch::Tensor& q, const torch::Tensor& k_cache,
                    const torch::Tensor& v_cache, const torch::Tensor& kv_len,
                    double scale, int64_t num_splits, int key_tile);
// fa_decode_merge_kernel over the [B, H, ns, D + 1] workspace (ns > 1 only)
void dec_merge_launch(const DecCall& c, hipStream_t stream);
