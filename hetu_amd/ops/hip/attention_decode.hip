// Split-KV decode attention for gfx950: one query token per sequence against
// a bf16 KV cache read in place.
//
//   q [B, H, D], k_cache / v_cache [B, Hkv, L, D] (element strides, last dim
//   contiguous), kv_len int32 [B] on the device
//   -> out [B, H, D] bf16, lse [B, H] fp32 = log sum_j exp(scale * q.k_j)
//
// A block owns one (batch row, KV head, split) and serves all G = H / Hkv
// query heads of that KV head from ONE 16-byte load of each K and V row
// slice.  Plain VALU, no MFMA and no LDS in the key loop (docs/KERNELS.md,
// "Decode attention", says why):
//   * a K / V row is spread over LPR = D / 8 lanes, 16 B each, so one wave
//     load instruction fetches KPI = 64 / LPR whole rows;
//   * a lane keeps the same 8 dims of q (packed bf16) for every head of the
//     chunk, forms its partial dot with v_dot2c_f32_bf16 and the LPR lanes
//     of the row add up with DPP (no LDS traffic);
//   * every lane of the row group then knows the score, and holds the
//     matching 8 dims of the V row, so P.V is lane-local as well.
// Each row group (KPI per wave, 4 waves) is an independent online-softmax
// stream over the keys it meets; the streams merge once per head chunk:
// across row groups with shuffles, across waves through LDS in wave order.
// Heads are taken in chunks of GC <= 8 (register budget); a KV head with
// more query heads re-reads its key range once per chunk.
//
// kv_len is read in the kernel and clamped to [0, L].  A row index is
// clamped to kv - 1 before it is used as an address and the score of a key
// >= kv is SELECTED to -inf (p = 0): nothing past kv_len is ever loaded, so
// whatever the cache holds there (NaN included) cannot reach the result.
// The grid depends on B, Hkv, L and the CU count only.
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include "attention_decode.h"
#include "attention_decode_valu.h"   // fa_decode_kernel<D, GC>

// out[row] = sum_s exp(lse_s - lse) * o_s over the non-empty splits, in
// split order; one block per (b, h), one thread per dim
__global__ void fa_decode_merge_kernel(const float* __restrict__ ws_o,
                                       const float* __restrict__ ws_lse,
                                       bf16* __restrict__ out,
                                       float* __restrict__ lse, int ns,
                                       int D) {
  const int64_t row = blockIdx.x;
  const int d = threadIdx.x;
  const float* pl = ws_lse + row * ns;
  float mx = -INFINITY;
  for (int s = 0; s < ns; ++s) mx = fmaxf(mx, pl[s]);
  float sum = 0.f, o = 0.f;
  if (mx != -INFINITY) {
    for (int s = 0; s < ns; ++s) {
      const float ls = pl[s];
      if (ls == -INFINITY) continue;   // empty split: its o was never written
      const float w = __expf(ls - mx);
      sum += w;
      o += w * ws_o[(row * ns + s) * D + d];
    }
    o /= sum;
  }
  reinterpret_cast<unsigned short*>(out)[row * D + d] = f2bf(o);
  if (d == 0) lse[row] = mx == -INFINITY ? -INFINITY : mx + logf(sum);
}

static bool dec_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

void dec_check_strides(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.stride(-1) == 1, "flash_attn_decode: ", what,
              " needs a contiguous last dim");
  for (int64_t i = 0; i + 1 < t.dim(); ++i)    // size-1 dims: stride unused
    TORCH_CHECK(t.size(i) == 1 || t.stride(i) % 8 == 0,
                "flash_attn_decode: ", what,
                " stride ", i, " (", t.stride(i),
                ") is not a multiple of 8 elements");
  TORCH_CHECK(dec_aligned16(t.data_ptr()), "flash_attn_decode: ", what,
              " is not 16-byte aligned");
}

int64_t decode_attn_tile() { return DEC_BN; }

// the launcher's split count: B, Hkv, L and the CU count only (never the
// values of kv_len), so the grid is the same on every replay of a capture
int64_t decode_attn_num_splits(int64_t B, int64_t Hkv, int64_t L,
                               int64_t cus) {
  const int64_t tiles = std::max<int64_t>((L + DEC_BN - 1) / DEC_BN, 1);
  const int64_t blocks = std::max<int64_t>(B * Hkv, 1);
  const int64_t want = (2 * cus + blocks - 1) / blocks;   // two blocks per CU
  return std::max<int64_t>(
      1, std::min<int64_t>({want, tiles, (int64_t)DEC_MAX_SPLITS}));
}

DecCall dec_prepare(const torch::Tensor& q, const torch::Tensor& k_cache,
                    const torch::Tensor& v_cache, const torch::Tensor& kv_len,
                    double scale, int64_t num_splits, int key_tile,
                    const torch::Tensor* block_table, bool fp8) {
  const bool paged = block_table != nullptr;
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
              kv_len.is_cuda(),
              "flash_attn_decode: q, k_cache, v_cache and kv_len must be on "
              "the GPU");
  TORCH_CHECK(q.device() == k_cache.device() &&
              q.device() == v_cache.device() && q.device() == kv_len.device(),
              "flash_attn_decode: all tensors must share one device");
  TORCH_CHECK(!paged || (block_table->is_cuda() &&
                         block_table->device() == q.device()),
              "flash_attn_decode: block_table must be on q's GPU");
  const auto cache_type = fp8 ? at::kFloat8_e4m3fn : at::kBFloat16;
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
              k_cache.scalar_type() == cache_type &&
              v_cache.scalar_type() == cache_type,
              fp8 ? "flash_attn_decode (fp8 cache): q must be bf16, k_cache "
                    "and v_cache float8_e4m3fn"
                  : "flash_attn_decode: q, k_cache and v_cache must be bf16");
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4,
              "flash_attn_decode: need q [B, H, D] and caches "
              "[B, Hkv, L, D] (pools [P, Hkv, PS, D] with a block_table)");
  const int64_t B = q.size(0), H = q.size(1), D = q.size(2);
  const int64_t Hkv = k_cache.size(1);
  const int64_t P = k_cache.size(0), PS = k_cache.size(2);   // paged only
  int64_t MP = 0, L = k_cache.size(2);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() &&
              (paged || k_cache.size(0) == B) && k_cache.size(3) == D,
              "flash_attn_decode: cache shapes do not match q");
  if (paged) {
    TORCH_CHECK(PS == 32 || PS == 64 || PS == 128 || PS == 256,
                "flash_attn_decode: the page size of k_pool / v_pool (dim 2) "
                "must be 32, 64, 128 or 256, got ", PS);
    TORCH_CHECK(block_table->scalar_type() == at::kInt &&
                block_table->dim() == 2 && block_table->size(0) == B &&
                block_table->is_contiguous(),
                "flash_attn_decode: block_table must be a contiguous int32 "
                "[B, MP]");
    MP = block_table->size(1);
    TORCH_CHECK(P < ((int64_t)1 << 31) && MP < ((int64_t)1 << 31) / PS,
                "flash_attn_decode: block_table covers MP * PS keys, too "
                "many for int");
    L = MP * PS;
  }
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_decode: D must be 64 or 128, "
              "got ", D);
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, "flash_attn_decode: H (", H,
              ") is not a multiple of Hkv (", Hkv, ")");
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.dim() == 1 &&
              kv_len.size(0) == B && kv_len.is_contiguous(),
              "flash_attn_decode: kv_len must be a contiguous int32 [B]");
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 &&
              L < ((int64_t)1 << 31) - key_tile,
              "flash_attn_decode: B, Hkv or L too large");
  TORCH_CHECK(num_splits >= 0, "flash_attn_decode: num_splits must be >= 0");
  DecCall c;
  c.B = B; c.H = H; c.Hkv = Hkv; c.D = D;
  c.out = torch::empty({B, H, D}, q.options());
  c.lse = torch::empty({B, H}, q.options().dtype(at::kFloat));
  c.empty = B == 0 || H == 0;
  if (c.empty) return c;
  dec_check_strides(q, "q");
  if (!fp8) {
    dec_check_strides(k_cache, "k_cache");
    dec_check_strides(v_cache, "v_cache");
  }

  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int ns = (int)(num_splits > 0
                           ? std::min<int64_t>(num_splits, 1 << 16)
                           : decode_attn_num_splits(B, Hkv, L, cus));
  DecArgs& a = c.a;
  a.q = (const bf16*)q.data_ptr();
  a.k = (const bf16*)k_cache.data_ptr();
  a.v = (const bf16*)v_cache.data_ptr();
  a.kv_len = kv_len.data_ptr<int>();
  a.out = (bf16*)c.out.data_ptr();
  a.lse = c.lse.data_ptr<float>();
  a.ws_o = nullptr;
  a.ws_lse = nullptr;
  if (ns > 1) {                        // caching allocator, stream-ordered
    c.ws = torch::empty({B * H * ns * (D + 1)}, c.lse.options());
    a.ws_o = c.ws.data_ptr<float>();
    a.ws_lse = a.ws_o + B * H * ns * D;
  }
  a.q_bs = q.stride(0); a.q_hs = q.stride(1);
  a.k_bs = k_cache.stride(0); a.k_hs = k_cache.stride(1);
  a.k_rs = k_cache.stride(2);
  a.v_bs = v_cache.stride(0); a.v_hs = v_cache.stride(1);
  a.v_rs = v_cache.stride(2);
  a.H = (int)H; a.Hkv = (int)Hkv; a.L = (int)L; a.ns = ns;
  a.scale = (float)scale;
  if (paged) {
    c.table = block_table->data_ptr<int>();
    c.MP = (int)MP; c.P = (int)P;
    c.ps_shift = __builtin_ctzll((unsigned long long)PS);
  }
  return c;
}

void dec_merge_launch(const DecCall& c, hipStream_t stream) {
  hipLaunchKernelGGL(fa_decode_merge_kernel, dim3((unsigned)(c.B * c.H)),
                     dim3((unsigned)c.D), 0, stream, c.a.ws_o, c.a.ws_lse,
                     c.a.out, c.a.lse, c.a.ns, (int)c.D);
  HIP_CHECK(hipGetLastError());
}

std::vector<torch::Tensor> flash_attn_decode(torch::Tensor q,
                                             torch::Tensor k_cache,
                                             torch::Tensor v_cache,
                                             torch::Tensor kv_len,
                                             double scale,
                                             int64_t num_splits) {
  DecCall c = dec_prepare(q, k_cache, v_cache, kv_len, scale, num_splits,
                          DEC_BN);
  if (c.empty) return {c.out, c.lse};
  const DecArgs& a = c.a;
  const int64_t D = c.D, G = c.H / c.Hkv;
  const int gc = G >= 5 ? 8 : G >= 3 ? 4 : (int)G;
  auto stream = hetu_current_stream();
  const dim3 grid(a.ns, (unsigned)c.Hkv, (unsigned)c.B);
#define DEC_LAUNCH(DD, GG)                                                 \
  hipLaunchKernelGGL((fa_decode_kernel<DD, GG>), grid, dim3(DEC_THREADS),  \
                     0, stream, a)
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
