// Split-KV decode attention over a paged bf16 KV cache, VALU kernel: the
// contract, grid, split rule, workspace and merge of flash_attn_decode
// (attention_decode.hip) with the cache addressed through a block table.
//
//   q [B, H, D], k_pool / v_pool [P, Hkv, PS, D] (element strides; a layer
//   slice of [n_layer, P, Hkv, PS, D] is read in place), block_table int32
//   [B, MP] and kv_len int32 [B] on the device
//   -> out [B, H, D] bf16, lse [B, H] fp32
//
// Key j of row b is row j % PS of page block_table[b, j / PS]; PS is 32, 64,
// 128 or 256 and the logical capacity is L = MP * PS.  Entries past
// ceil(kv_len[b] / PS) are never read.  A needed entry outside [0, P) is a
// page of masked keys: nothing is loaded through it.  The kernel is
// fa_decode_kernel<D, GC, PAGED = true> (attention_decode_valu.h, which says
// how the page id stays a prefetched scalar); the MFMA variant lives with its
// dense sibling in attention_decode_mfma.hip.
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include "attention_decode.h"
#include "attention_decode_valu.h"

std::vector<torch::Tensor> flash_attn_decode_paged(torch::Tensor q,
                                                   torch::Tensor k_pool,
                                                   torch::Tensor v_pool,
                                                   torch::Tensor block_table,
                                                   torch::Tensor kv_len,
                                                   double scale,
                                                   int64_t num_splits) {
  // the id prefetch forms keys up to two tiles past the last one
  DecCall c = dec_prepare(q, k_pool, v_pool, kv_len, scale, num_splits,
                          3 * DEC_BN, &block_table);
  if (c.empty) return {c.out, c.lse};
  const DecPagedArgs a = c.paged();
  const int64_t D = c.D, G = c.H / c.Hkv;
  const int gc = G >= 5 ? 8 : G >= 3 ? 4 : (int)G;
  auto stream = hetu_current_stream();
  const dim3 grid(a.ns, (unsigned)c.Hkv, (unsigned)c.B);
#define DEC_LAUNCH(DD, GG)                                                 \
  hipLaunchKernelGGL((fa_decode_kernel<DD, GG, true>), grid,               \
                     dim3(DEC_THREADS), 0, stream, a)
#define DEC_LAUNCH_D(DD)                                                   \
  do {                                                                     \
    if (gc == 1) DEC_LAUNCH(DD, 1);                                        \
    else if (gc == 2) DEC_LAUNCH(DD, 2);                                   \
    else if (gc == 4) DEC_LAUNCH(DD, 4);                                   \
    else DEC_LAUNCH(DD, DEC_MAX_GC);                                       \
  } while (0)
  if (D == 128) DEC_LAUNCH_D(128);
  else DEC_LAUNCH_D(64);
#undef DEC_LAUNCH_D
#undef DEC_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (a.ns > 1) dec_merge_launch(c, stream);
  return {c.out, c.lse};
}
