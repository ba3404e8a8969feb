// Append into a paged KV cache for gfx950: a 2-byte-element row copy through
// a block table that lives on the device.
//
//   k_new / v_new [B, S, Hkv, D] (element strides, last dim contiguous: views
//   into a fused qkv output are read in place), k_pool / v_pool
//   [P, Hkv, PS, D] of the same 2-byte dtype (with their strides: a layer
//   slice is written in place), block_table int32 [B, MP], end int32 [B]
//
// Row s of batch b goes to logical position j = end[b] - S + s, which is row
// j % PS of page block_table[b, j / PS].  A row with j outside [0, MP * PS),
// or whose page id is outside [0, P), is dropped: no table entry is read for
// the first kind and no address is formed from either.  Nothing else in the
// pools is written, and with distinct pages in the table every written row
// has one writer.
//
// One launch serves K and V.  A row is spread over D / 8 lanes, 16 bytes per
// lane: one 16-byte load and one 16-byte store, no arithmetic on the values
// (the copy is blind to the dtype).  Position and page come from the device,
// so the launch is capturable; no atomics, no host sync.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "common.h"

namespace {

constexpr int KP_THREADS = 256;

struct KvpSide {
  const bf16* src;            // [B, S, Hkv, D]
  bf16* dst;                  // [P, Hkv, PS, D]
  long long s_bs, s_ss, s_hs;
  long long d_ps, d_hs, d_rs;
};

struct KvpArgs {
  KvpSide side[2];            // K, V
  const int* table;           // [B, MP]
  const int* end;             // [B]
  int S, Hkv, LPR;            // LPR = D / 8 lanes per row
  int MP, P, ps_shift;
  long long rows;             // B * S * Hkv, per side
};

__global__ __launch_bounds__(KP_THREADS)
void kv_cache_append_paged_kernel(KvpArgs a) {
  const long long gid = (long long)blockIdx.x * KP_THREADS + threadIdx.x;
  const long long row = gid / a.LPR;
  const int part = (int)(gid % a.LPR);
  if (row >= 2 * a.rows) return;
  // a select of the two argument blocks, not an indexed copy in scratch
  const KvpSide sd = row >= a.rows ? a.side[1] : a.side[0];
  long long r = row >= a.rows ? row - a.rows : row;
  const int h = (int)(r % a.Hkv);
  r /= a.Hkv;
  const int s = (int)(r % a.S);
  const int b = (int)(r / a.S);

  const long long tgt = (long long)a.end[b] - a.S + s;
  if (tgt < 0 || tgt >= ((long long)a.MP << a.ps_shift)) return;
  const int page = a.table[(long long)b * a.MP + (tgt >> a.ps_shift)];
  if ((unsigned)page >= (unsigned)a.P) return;
  const int prow = (int)tgt & ((1 << a.ps_shift) - 1);
  const uint4 x = *reinterpret_cast<const uint4*>(
      sd.src + b * sd.s_bs + s * sd.s_ss + h * sd.s_hs + 8 * part);
  *reinterpret_cast<uint4*>(sd.dst + page * sd.d_ps + h * sd.d_hs +
                            prow * sd.d_rs + 8 * part) = x;
}

KvpSide kvp_side(const torch::Tensor& x, const torch::Tensor& pool,
                 const char* xn, const char* pn, const torch::Tensor& k_new,
                 const torch::Tensor& k_pool) {
  const char* fn = "kv_cache_append_paged: ";
  TORCH_CHECK(x.is_cuda() && pool.is_cuda(), fn, xn, " and ", pn,
              " must be on the GPU");
  TORCH_CHECK(x.device() == k_new.device() && pool.device() == k_new.device(),
              fn, "all tensors must share one device");
  TORCH_CHECK(x.element_size() == 2 && pool.scalar_type() == x.scalar_type(),
              fn, xn, " and ", pn, " must share one 2-byte dtype");
  TORCH_CHECK(x.sizes() == k_new.sizes(), fn, xn,
              " must be [B, S, Hkv, D] like k_new");
  TORCH_CHECK(pool.sizes() == k_pool.sizes(), fn, pn,
              " must be [P, Hkv, PS, D] like k_pool");
  TORCH_CHECK(x.stride(3) == 1 && pool.stride(3) == 1, fn, xn, " and ", pn,
              " need a contiguous last dim");
  for (int i = 0; i < 3; ++i) {
    TORCH_CHECK(x.size(i) == 1 || x.stride(i) % 8 == 0, fn, xn, " stride ",
                i, " is not a multiple of 8 elements");
    TORCH_CHECK(pool.size(i) == 1 || pool.stride(i) % 8 == 0, fn, pn,
                " stride ", i, " is not a multiple of 8 elements");
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, fn, xn,
              " is not 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pool.data_ptr()) % 16 == 0, fn, pn,
              " is not 16-byte aligned");
  KvpSide sd;
  sd.src = (const bf16*)x.data_ptr();
  sd.dst = (bf16*)pool.data_ptr();
  sd.s_bs = x.stride(0); sd.s_ss = x.stride(1); sd.s_hs = x.stride(2);
  sd.d_ps = pool.stride(0); sd.d_hs = pool.stride(1);
  sd.d_rs = pool.stride(2);
  return sd;
}

// ---- packed rows ----------------------------------------------------------
//   k_new / v_new [T, Hkv, D] packed over sequences, cu_q int32 [B + 1]
// Row t of sequence b (n_b = cu_q[b + 1] - cu_q[b] rows from cu_q[b]) goes to
// position end[b] - n_b + (t - cu_q[b]); the drop rules are the ones above.
// Grid (b, row tile): it depends on shapes and the max_q hint only, the
// chunk bounds are read on the device.  A block takes KPP_ROWS rows of one
// sequence, K and V, all KV heads; its threads walk (side, row, head, 16 B).
constexpr int KPP_ROWS = 16;

struct KvpPackedArgs {
  KvpSide side[2];            // s_bs unused, s_ss = row stride
  const int* table;
  const int* end;
  const int* cu_q;            // [B + 1]
  int T, Hkv, LPR, MP, P, ps_shift;
};

__global__ __launch_bounds__(KP_THREADS)
void kv_cache_append_paged_packed_kernel(KvpPackedArgs a) {
  const int b = blockIdx.x;
  const int row0 = min(max(a.cu_q[b], 0), a.T);
  const int n_b = min(max(a.cu_q[b + 1], row0), a.T) - row0;
  const int s0 = blockIdx.y * KPP_ROWS;
  if (s0 >= n_b) return;
  const int rows = min(KPP_ROWS, n_b - s0);
  const long long end = a.end[b];
  const int per_row = a.Hkv * a.LPR;
  const int per_side = rows * per_row;
  for (int i = threadIdx.x; i < 2 * per_side; i += KP_THREADS) {
    const KvpSide sd = i >= per_side ? a.side[1] : a.side[0];
    int j = i >= per_side ? i - per_side : i;
    const int part = j % a.LPR;
    j /= a.LPR;
    const int h = j % a.Hkv;
    const int s = s0 + j / a.Hkv;
    const long long tgt = end - n_b + s;
    if (tgt < 0 || tgt >= ((long long)a.MP << a.ps_shift)) continue;
    const int page = a.table[(long long)b * a.MP + (tgt >> a.ps_shift)];
    if ((unsigned)page >= (unsigned)a.P) continue;
    const int prow = (int)tgt & ((1 << a.ps_shift) - 1);
    const uint4 x = *reinterpret_cast<const uint4*>(
        sd.src + (long long)(row0 + s) * sd.s_ss + h * sd.s_hs + 8 * part);
    *reinterpret_cast<uint4*>(sd.dst + page * sd.d_ps + h * sd.d_hs +
                              prow * sd.d_rs + 8 * part) = x;
  }
}

KvpSide kvp_side_packed(const torch::Tensor& x, const torch::Tensor& pool,
                        const char* xn, const char* pn,
                        const torch::Tensor& k_new,
                        const torch::Tensor& k_pool) {
  const char* fn = "kv_cache_append_paged: ";
  TORCH_CHECK(x.is_cuda() && pool.is_cuda(), fn, xn, " and ", pn,
              " must be on the GPU");
  TORCH_CHECK(x.device() == k_new.device() && pool.device() == k_new.device(),
              fn, "all tensors must share one device");
  TORCH_CHECK(x.element_size() == 2 && pool.scalar_type() == x.scalar_type(),
              fn, xn, " and ", pn, " must share one 2-byte dtype");
  TORCH_CHECK(x.sizes() == k_new.sizes(), fn, xn,
              " must be [T, Hkv, D] like k_new");
  TORCH_CHECK(pool.sizes() == k_pool.sizes(), fn, pn,
              " must be [P, Hkv, PS, D] like k_pool");
  TORCH_CHECK(x.stride(2) == 1 && pool.stride(3) == 1, fn, xn, " and ", pn,
              " need a contiguous last dim");
  for (int i = 0; i < 2; ++i)
    TORCH_CHECK(x.size(i) == 1 || x.stride(i) % 8 == 0, fn, xn, " stride ",
                i, " is not a multiple of 8 elements");
  for (int i = 0; i < 3; ++i)
    TORCH_CHECK(pool.size(i) == 1 || pool.stride(i) % 8 == 0, fn, pn,
                " stride ", i, " is not a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, fn, xn,
              " is not 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pool.data_ptr()) % 16 == 0, fn, pn,
              " is not 16-byte aligned");
  KvpSide sd;
  sd.src = (const bf16*)x.data_ptr();
  sd.dst = (bf16*)pool.data_ptr();
  sd.s_bs = 0; sd.s_ss = x.stride(0); sd.s_hs = x.stride(1);
  sd.d_ps = pool.stride(0); sd.d_hs = pool.stride(1);
  sd.d_rs = pool.stride(2);
  return sd;
}

}  // namespace

void kv_cache_append_paged_packed(torch::Tensor k_new, torch::Tensor v_new,
                                  torch::Tensor k_pool, torch::Tensor v_pool,
                                  torch::Tensor block_table,
                                  torch::Tensor end, torch::Tensor cu_q,
                                  int64_t max_q) {
  const char* fn = "kv_cache_append_paged: ";
  TORCH_CHECK(k_new.dim() == 3 && k_pool.dim() == 4, fn,
              "with cu_q need k_new [T, Hkv, D] and k_pool [P, Hkv, PS, D]");
  const int64_t T = k_new.size(0), Hkv = k_new.size(1), D = k_new.size(2);
  const int64_t P = k_pool.size(0), PS = k_pool.size(2);
  TORCH_CHECK(k_pool.size(1) == Hkv && k_pool.size(3) == D, fn,
              "k_pool must be [P, Hkv, PS, D] with k_new's Hkv and D");
  TORCH_CHECK(D >= 8 && D % 8 == 0, fn, "D must be a multiple of 8, got ", D);
  TORCH_CHECK(PS == 32 || PS == 64 || PS == 128 || PS == 256, fn,
              "the page size of k_pool / v_pool (dim 2) must be 32, 64, 128 "
              "or 256, got ", PS);
  KvpPackedArgs a;
  a.side[0] = kvp_side_packed(k_new, k_pool, "k_new", "k_pool", k_new,
                              k_pool);
  a.side[1] = kvp_side_packed(v_new, v_pool, "v_new", "v_pool", k_new,
                              k_pool);
  const auto index_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == k_new.device() &&
           t.scalar_type() == at::kInt && t.is_contiguous();
  };
  TORCH_CHECK(index_ok(block_table) && block_table.dim() == 2, fn,
              "block_table must be a contiguous int32 [B, MP] on the GPU");
  const int64_t B = block_table.size(0), MP = block_table.size(1);
  TORCH_CHECK(index_ok(end) && end.dim() == 1 && end.size(0) == B, fn,
              "end must be a contiguous int32 [B] on the GPU");
  TORCH_CHECK(index_ok(cu_q) && cu_q.dim() == 1 && cu_q.size(0) == B + 1, fn,
              "cu_q must be a contiguous int32 [B + 1] on the GPU");
  const int64_t lim = (int64_t)1 << 31;
  TORCH_CHECK(P < lim && MP < lim / PS && T < lim && B < lim &&
              Hkv * (D / 8) * KPP_ROWS < lim / 2, fn,
              "P, T, B, Hkv * D or MP * PS too large for int");
  a.table = block_table.data_ptr<int>();
  a.end = end.data_ptr<int>();
  a.cu_q = cu_q.data_ptr<int>();
  a.T = (int)T; a.Hkv = (int)Hkv; a.LPR = (int)(D / 8);
  a.MP = (int)MP; a.P = (int)P;
  a.ps_shift = __builtin_ctzll((unsigned long long)PS);
  if (T == 0 || B == 0 || Hkv == 0 || MP == 0) return;
  max_q = std::min(std::max<int64_t>(max_q, 1), T);
  const int64_t gy = (max_q + KPP_ROWS - 1) / KPP_ROWS;
  TORCH_CHECK(gy <= 65535, fn, "max_q too large for one launch");
  hipLaunchKernelGGL(kv_cache_append_paged_packed_kernel,
                     dim3((unsigned)B, (unsigned)gy), dim3(KP_THREADS), 0,
                     hetu_current_stream(), a);
  HIP_CHECK(hipGetLastError());
}

void kv_cache_append_paged(torch::Tensor k_new, torch::Tensor v_new,
                           torch::Tensor k_pool, torch::Tensor v_pool,
                           torch::Tensor block_table, torch::Tensor end) {
  const char* fn = "kv_cache_append_paged: ";
  TORCH_CHECK(k_new.dim() == 4 && k_pool.dim() == 4, fn,
              "need k_new [B, S, Hkv, D] and k_pool [P, Hkv, PS, D]");
  const int64_t B = k_new.size(0), S = k_new.size(1), Hkv = k_new.size(2);
  const int64_t D = k_new.size(3);
  const int64_t P = k_pool.size(0), PS = k_pool.size(2);
  TORCH_CHECK(k_pool.size(1) == Hkv && k_pool.size(3) == D, fn,
              "k_pool must be [P, Hkv, PS, D] with k_new's Hkv and D");
  TORCH_CHECK(D >= 8 && D % 8 == 0, fn, "D must be a multiple of 8, got ", D);
  TORCH_CHECK(PS == 32 || PS == 64 || PS == 128 || PS == 256, fn,
              "the page size of k_pool / v_pool (dim 2) must be 32, 64, 128 "
              "or 256, got ", PS);
  KvpArgs a;
  a.side[0] = kvp_side(k_new, k_pool, "k_new", "k_pool", k_new, k_pool);
  a.side[1] = kvp_side(v_new, v_pool, "v_new", "v_pool", k_new, k_pool);
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == k_new.device()
              && block_table.scalar_type() == at::kInt &&
              block_table.dim() == 2 && block_table.size(0) == B &&
              block_table.is_contiguous(), fn,
              "block_table must be a contiguous int32 [B, MP] on the GPU");
  TORCH_CHECK(end.is_cuda() && end.device() == k_new.device() &&
              end.scalar_type() == at::kInt && end.dim() == 1 &&
              end.size(0) == B && end.is_contiguous(), fn,
              "end must be a contiguous int32 [B] on the GPU");
  const int64_t MP = block_table.size(1);
  TORCH_CHECK(P < ((int64_t)1 << 31) && MP < ((int64_t)1 << 31) / PS &&
              S < ((int64_t)1 << 31), fn,
              "P, S or MP * PS too large for int");
  a.table = block_table.data_ptr<int>();
  a.end = end.data_ptr<int>();
  a.S = (int)S; a.Hkv = (int)Hkv; a.LPR = (int)(D / 8);
  a.MP = (int)MP; a.P = (int)P;
  a.ps_shift = __builtin_ctzll((unsigned long long)PS);
  a.rows = B * S * Hkv;
  if (a.rows == 0 || MP == 0) return;
  const int64_t threads = 2 * a.rows * (D / 8);
  const int64_t blocks = (threads + KP_THREADS - 1) / KP_THREADS;
  TORCH_CHECK(blocks < ((int64_t)1 << 31), fn,
              "too many rows for one launch");
  hipLaunchKernelGGL(kv_cache_append_paged_kernel, dim3((unsigned)blocks),
                     dim3(KP_THREADS), 0, hetu_current_stream(), a);
  HIP_CHECK(hipGetLastError());
}
