// What the decode-attention translation units share: attention_decode.hip
// (VALU kernel; it defines everything declared here), attention_decode_mfma.hip
// (MFMA kernel for wide GQA groups) and attention_decode_paged.hip (the VALU
// kernel over a paged cache; attention_decode_valu.h holds the kernel itself).
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

// Paged cache: a.k / a.v are the pools [P, Hkv, PS, D], k_bs / v_bs the page
// strides and L = MP * PS the logical capacity.  Key j of row b lives in page
// table[b * MP + j / PS], row j % PS; PS = 1 << ps_shift >= 32, so the keys a
// wave takes from a tile (16 or 32, aligned to their count) share one page.
// An entry outside [0, P) is a page of masked keys.  The dense kernels keep
// DecArgs as their argument block.
struct DecPagedArgs : DecArgs {
  const int* table;   // [B, MP]
  int MP, P, ps_shift;
};

// the block-table entry of the page that holds `key` of row b, as a scalar
// (key is wave-uniform and < MP * PS).  The table is not written while a
// decode kernel runs, so it is read through the constant address space: a
// uniform index then makes the load a scalar one (s_load_dword, counted by
// lgkmcnt and waited for at the first use, not in the vector memory queue
// whose count the MFMA kernel's pipeline relies on).
DEV int dec_page_of(const DecPagedArgs& a, int b, int key) {
  typedef const __attribute__((address_space(4))) int* const_int_p;
  const int64_t idx = (int64_t)b * a.MP + (key >> a.ps_shift);
  return __builtin_amdgcn_readfirstlane(((const_int_p)a.table)[idx]);
}

// Scalar loads return out of order, so a wait for one id is a wait for every
// id in flight.  This goes between the id a tile is about to use (`page`,
// requested a tile ago, so the wait it takes here is free) and the request of
// the next one: `next_key`, the argument of that request, is tied behind the
// wait, so the new load cannot be issued in front of it and then be waited
// for by the first use of `page`.
DEV void dec_page_landed(int& page, int& next_key) {
  asm volatile("" : "+s"(page), "+s"(next_key));
}

// a checked call, its outputs and the split workspace (undefined at ns == 1)
struct DecCall {
  DecArgs a;
  torch::Tensor out, lse, ws;
  int64_t B, H, Hkv, D;
  bool empty;         // B == 0 or H == 0: nothing to launch
  // set by dec_prepare with a block_table
  const int* table = nullptr;
  int MP = 0, P = 0, ps_shift = 0;
  DecPagedArgs paged() const {
    DecPagedArgs p;
    static_cast<DecArgs&>(p) = a;
    p.table = table; p.MP = MP; p.P = P; p.ps_shift = ps_shift;
    return p;
  }
};

int64_t decode_attn_num_splits(int64_t B, int64_t Hkv, int64_t L,
                               int64_t cus);
void dec_check_strides(const torch::Tensor& t, const char* what);
// every TORCH_CHECK of flash_attn_decode, then out / lse / workspace and the
// kernel arguments; key_tile is the caller's block tile (bounds L).  With a
// block_table [B, MP] the caches are pools [P, Hkv, PS, D] and L = MP * PS.
// fp8: the caches hold e4m3 codes, strides are bytes and the caller checks
// them (attention_decode_fp8.hip).
DecCall dec_prepare(const torch::Tensor& q, const torch::Tensor& k_cache,
                    const torch::Tensor& v_cache, const torch::Tensor& kv_len,
                    double scale, int64_t num_splits, int key_tile,
                    const torch::Tensor* block_table = nullptr,
                    bool fp8 = false);
// fa_decode_merge_kernel over the [B, H, ns, D + 1] workspace (ns > 1 only)
void dec_merge_launch(const DecCall& c, hipStream_t stream);
