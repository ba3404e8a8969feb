// Quantizing append into an fp8 (OCP e4m3) KV cache for gfx950.
//
//   k_new / v_new [B, S, Hkv, D] bf16 (element strides, last dim contiguous)
//   k_cache / v_cache [B, Hkv, L, D] e4m3 bytes, k_scale / v_scale
//   [B, Hkv, L] fp32 (all with their strides), end int32 [B] on the device
//
// Row s of batch b goes to cache row end[b] - S + s.  Per cached row:
//   scale = amax(|x|) / 448 (fp32, IEEE division; 0 for a row of zeros)
//   code  = rne_e4m3(clamp(x / scale, -448, 448)), 0 where scale == 0
// so the value of an element is float(code) * scale[row].
//
// One launch serves K and V.  A row is spread over LPR = D / 8 lanes, the
// decode VALU kernel's row spread: one 16-byte load per lane, |x| joined
// over the row's lanes with the DPP steps of that kernel's dot product, four
// v_cvt_pk_fp8_f32 and one 8-byte store per lane; lane 0 of the row stores
// the scale.  Every lane stays active through the DPP steps: a thread past
// the last row re-reads that row, and a row whose target is outside [0, L)
// is dropped at the stores (no address is formed from it).  The row index
// comes from the device, so the launch is capturable; no atomics.
//
// Paged (kv_cache_append_paged_fp8): the caches are code pools
// [P, Hkv, PS, D] and the scales pools [P, Hkv, PS] behind block_table int32
// [B, MP] (kv_cache_paged.hip's layout).  The same lanes and arithmetic; the
// row goes to position j = end[b] - S + s, row j % PS of page
// block_table[b, j / PS] in all four pools.  A row with j outside
// [0, MP * PS) is dropped before the table is read, one behind an id outside
// [0, P) before any address is formed.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "common.h"

namespace {

constexpr int KQ_THREADS = 256;

struct KvqSide {
  const bf16* src;            // [B, S, Hkv, D]
  unsigned char* dst;         // [B, Hkv, L, D]
  float* scale;               // [B, Hkv, L]
  long long s_bs, s_ss, s_hs;
  long long d_bs, d_hs, d_rs;
  long long c_bs, c_hs, c_rs;
};

struct KvqArgs {
  KvqSide side[2];            // K, V
  const int* end;
  int S, Hkv, L;
  long long rows;             // B * S * Hkv, per side
};

template <int CTRL>
DEV float kvq_dpp_max(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf,
                                            0xf, false);
  return fmaxf(x, __int_as_float(y));
}

// max over the LPR (8 or 16) consecutive lanes of a row, on every lane
template <int LPR>
DEV float kvq_row_max(float x) {
  x = kvq_dpp_max<0xB1>(x);            // quad_perm [1,0,3,2]
  x = kvq_dpp_max<0x4E>(x);            // quad_perm [2,3,0,1]
  x = kvq_dpp_max<0x141>(x);           // row_half_mirror
  if constexpr (LPR == 16) x = kvq_dpp_max<0x140>(x);   // row_mirror
  return x;
}

// the lane's 8 elements of a row quantized: the row's scale and the 8 codes
template <int LPR>
DEV float kvq_quantize(const bf16* src, int& w0, int& w1) {
  const ushort8 u = *reinterpret_cast<const ushort8*>(src);
  float x[8], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = bf2f(u.v[j]);
    amax = fmaxf(amax, fabsf(x[j]));
  }
  amax = kvq_row_max<LPR>(amax);
  const float scale = __fdiv_rn(amax, 448.f);
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = __fdiv_rn(x[j], scale);
    y[j] = scale == 0.f ? 0.f : fminf(fmaxf(t, -448.f), 448.f);
  }
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
  return scale;
}

template <int D>
__global__ __launch_bounds__(KQ_THREADS)
void kv_cache_append_fp8_kernel(KvqArgs a) {
  constexpr int LPR = D / 8;
  const long long gid = (long long)blockIdx.x * KQ_THREADS + threadIdx.x;
  const long long row_raw = gid / LPR;
  const int part = (int)(gid % LPR);
  const bool live = row_raw < 2 * a.rows;
  const long long row = live ? row_raw : 2 * a.rows - 1;
  // a select of the two argument blocks, not an indexed copy in scratch
  const KvqSide sd = row >= a.rows ? a.side[1] : a.side[0];
  long long r = row >= a.rows ? row - a.rows : row;
  const int h = (int)(r % a.Hkv);
  r /= a.Hkv;
  const int s = (int)(r % a.S);
  const int b = (int)(r / a.S);

  int w0, w1;
  const float scale = kvq_quantize<LPR>(
      sd.src + b * sd.s_bs + s * sd.s_ss + h * sd.s_hs + 8 * part, w0, w1);

  const long long tgt = (long long)a.end[b] - a.S + s;
  if (live && tgt >= 0 && tgt < a.L) {
    *reinterpret_cast<uint2*>(sd.dst + b * sd.d_bs + h * sd.d_hs +
                              tgt * sd.d_rs + 8 * part) =
        make_uint2((unsigned)w0, (unsigned)w1);
    if (part == 0) sd.scale[b * sd.c_bs + h * sd.c_hs + tgt * sd.c_rs] = scale;
  }
}

// pools: KvqSide's d_bs / c_bs are page strides
struct KvqPagedArgs {
  KvqSide side[2];            // K, V
  const int* table;           // [B, MP]
  const int* end;
  int S, Hkv, MP, P, ps_shift;
  long long rows;             // B * S * Hkv, per side
};

template <int D>
__global__ __launch_bounds__(KQ_THREADS)
void kv_cache_append_paged_fp8_kernel(KvqPagedArgs a) {
  constexpr int LPR = D / 8;
  const long long gid = (long long)blockIdx.x * KQ_THREADS + threadIdx.x;
  const long long row_raw = gid / LPR;
  const int part = (int)(gid % LPR);
  const bool live = row_raw < 2 * a.rows;
  const long long row = live ? row_raw : 2 * a.rows - 1;
  const KvqSide sd = row >= a.rows ? a.side[1] : a.side[0];
  long long r = row >= a.rows ? row - a.rows : row;
  const int h = (int)(r % a.Hkv);
  r /= a.Hkv;
  const int s = (int)(r % a.S);
  const int b = (int)(r / a.S);

  int w0, w1;
  const float scale = kvq_quantize<LPR>(
      sd.src + b * sd.s_bs + s * sd.s_ss + h * sd.s_hs + 8 * part, w0, w1);

  // the DPP steps are behind: lanes may leave
  const long long tgt = (long long)a.end[b] - a.S + s;
  if (!live || tgt < 0 || tgt >= ((long long)a.MP << a.ps_shift)) return;
  const int page = a.table[(long long)b * a.MP + (tgt >> a.ps_shift)];
  if ((unsigned)page >= (unsigned)a.P) return;
  const int prow = (int)tgt & ((1 << a.ps_shift) - 1);
  *reinterpret_cast<uint2*>(sd.dst + page * sd.d_bs + h * sd.d_hs +
                            prow * sd.d_rs + 8 * part) =
      make_uint2((unsigned)w0, (unsigned)w1);
  if (part == 0)
    sd.scale[page * sd.c_bs + h * sd.c_hs + prow * sd.c_rs] = scale;
}

bool kvq_is_fp8(const torch::Tensor& t) {
  return t.scalar_type() == at::kFloat8_e4m3fn;
}

// cache [C0, Hkv, L, D] and scale [C0, Hkv, L]: C0 = B, or (paged) C0 = P and
// L = PS
KvqSide kvq_side(const torch::Tensor& x, const torch::Tensor& cache,
                 const torch::Tensor& scale, const char* xn, const char* cn,
                 const char* sn, int64_t B, int64_t S, int64_t Hkv,
                 int64_t L, int64_t D, bool paged = false) {
  const char* fn = paged ? "kv_cache_append_paged (fp8 pools): "
                         : "kv_cache_append_fp8: ";
  const int64_t C0 = paged ? cache.size(0) : B;
  TORCH_CHECK(x.is_cuda() && cache.is_cuda() && scale.is_cuda(), fn, xn, ", ",
              cn, " and ", sn, " must be on the GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, fn, xn, " must be bf16");
  TORCH_CHECK(cache.scalar_type() != at::kByte, fn, cn, " is uint8: pass "
              "it as .view(torch.float8_e4m3fn)");
  TORCH_CHECK(kvq_is_fp8(cache), fn, cn, " must be float8_e4m3fn");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, fn, sn, " must be fp32");
  TORCH_CHECK(x.dim() == 4 && x.size(0) == B && x.size(1) == S &&
              x.size(2) == Hkv && x.size(3) == D,
              fn, xn, " must be [B, S, Hkv, D] like k_new");
  TORCH_CHECK(cache.dim() == 4 && cache.size(0) == C0 &&
              cache.size(1) == Hkv && cache.size(2) == L && cache.size(3) == D,
              fn, cn, paged ? " must be [P, Hkv, PS, D]"
                            : " must be [B, Hkv, L, D]");
  TORCH_CHECK(scale.dim() == 3 && scale.size(0) == C0 &&
              scale.size(1) == Hkv && scale.size(2) == L, fn, sn,
              paged ? " must be [P, Hkv, PS]" : " must be [B, Hkv, L]");
  TORCH_CHECK(x.stride(3) == 1 && cache.stride(3) == 1, fn, xn, " and ", cn,
              " need a contiguous last dim");
  for (int i = 0; i < 3; ++i) {
    TORCH_CHECK(x.size(i) == 1 || x.stride(i) % 8 == 0, fn, xn, " stride ",
                i, " is not a multiple of 8 elements");
    TORCH_CHECK(cache.size(i) == 1 || cache.stride(i) % 8 == 0, fn, cn,
                " stride ", i, " is not a multiple of 8 bytes");
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, fn, xn,
              " is not 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(cache.data_ptr()) % 8 == 0, fn, cn,
              " is not 8-byte aligned");
  KvqSide sd;
  sd.src = (const bf16*)x.data_ptr();
  sd.dst = (unsigned char*)cache.data_ptr();
  sd.scale = scale.data_ptr<float>();
  sd.s_bs = x.stride(0); sd.s_ss = x.stride(1); sd.s_hs = x.stride(2);
  sd.d_bs = cache.stride(0); sd.d_hs = cache.stride(1);
  sd.d_rs = cache.stride(2);
  sd.c_bs = scale.stride(0); sd.c_hs = scale.stride(1);
  sd.c_rs = scale.stride(2);
  return sd;
}

}  // namespace

void kv_cache_append_fp8(torch::Tensor k_new, torch::Tensor v_new,
                         torch::Tensor k_cache, torch::Tensor v_cache,
                         torch::Tensor k_scale, torch::Tensor v_scale,
                         torch::Tensor end) {
  TORCH_CHECK(k_new.dim() == 4 && k_cache.dim() == 4,
              "kv_cache_append_fp8: need k_new [B, S, Hkv, D] and k_cache "
              "[B, Hkv, L, D]");
  const int64_t B = k_new.size(0), S = k_new.size(1), Hkv = k_new.size(2);
  const int64_t D = k_new.size(3), L = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128, "kv_cache_append_fp8: D must be 64 or "
              "128, got ", D);
  TORCH_CHECK(L < ((int64_t)1 << 31) && S < ((int64_t)1 << 31),
              "kv_cache_append_fp8: L or S too large");
  KvqArgs a;
  a.side[0] = kvq_side(k_new, k_cache, k_scale, "k_new", "k_cache", "k_scale",
                       B, S, Hkv, L, D);
  a.side[1] = kvq_side(v_new, v_cache, v_scale, "v_new", "v_cache", "v_scale",
                       B, S, Hkv, L, D);
  TORCH_CHECK(end.is_cuda() && end.scalar_type() == at::kInt &&
              end.dim() == 1 && end.size(0) == B && end.is_contiguous(),
              "kv_cache_append_fp8: end must be a contiguous int32 [B] on "
              "the GPU");
  TORCH_CHECK(end.device() == k_new.device() &&
              k_cache.device() == k_new.device() &&
              v_cache.device() == k_new.device(),
              "kv_cache_append_fp8: all tensors must share one device");
  a.end = end.data_ptr<int>();
  a.S = (int)S; a.Hkv = (int)Hkv; a.L = (int)L;
  a.rows = B * S * Hkv;
  if (a.rows == 0) return;
  const int64_t threads = 2 * a.rows * (D / 8);
  const int64_t blocks = (threads + KQ_THREADS - 1) / KQ_THREADS;
  TORCH_CHECK(blocks < ((int64_t)1 << 31), "kv_cache_append_fp8: too many "
              "rows for one launch");
  auto stream = hetu_current_stream();
  if (D == 128)
    hipLaunchKernelGGL(kv_cache_append_fp8_kernel<128>, dim3((unsigned)blocks),
                       dim3(KQ_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(kv_cache_append_fp8_kernel<64>, dim3((unsigned)blocks),
                       dim3(KQ_THREADS), 0, stream, a);
  HIP_CHECK(hipGetLastError());
}

void kv_cache_append_paged_fp8(torch::Tensor k_new, torch::Tensor v_new,
                               torch::Tensor k_pool, torch::Tensor v_pool,
                               torch::Tensor k_scale, torch::Tensor v_scale,
                               torch::Tensor block_table, torch::Tensor end) {
  const char* fn = "kv_cache_append_paged (fp8 pools): ";
  TORCH_CHECK(k_new.dim() == 4 && k_pool.dim() == 4, fn,
              "need k_new [B, S, Hkv, D] and k_pool [P, Hkv, PS, D]");
  const int64_t B = k_new.size(0), S = k_new.size(1), Hkv = k_new.size(2);
  const int64_t D = k_new.size(3);
  const int64_t P = k_pool.size(0), PS = k_pool.size(2);
  TORCH_CHECK(D == 64 || D == 128, fn, "D must be 64 or 128, got ", D);
  TORCH_CHECK(PS == 32 || PS == 64 || PS == 128 || PS == 256, fn,
              "the page size of k_pool / v_pool (dim 2) must be 32, 64, 128 "
              "or 256, got ", PS);
  TORCH_CHECK(v_pool.dim() == 4 && v_pool.size(0) == P, fn,
              "v_pool must be [P, Hkv, PS, D] like k_pool");
  KvqPagedArgs a;
  a.side[0] = kvq_side(k_new, k_pool, k_scale, "k_new", "k_pool", "k_scale",
                       B, S, Hkv, PS, D, true);
  a.side[1] = kvq_side(v_new, v_pool, v_scale, "v_new", "v_pool", "v_scale",
                       B, S, Hkv, PS, D, true);
  const auto index_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == k_new.device() &&
           t.scalar_type() == at::kInt && t.is_contiguous();
  };
  TORCH_CHECK(index_ok(block_table) && block_table.dim() == 2 &&
              block_table.size(0) == B, fn,
              "block_table must be a contiguous int32 [B, MP] on the GPU");
  TORCH_CHECK(index_ok(end) && end.dim() == 1 && end.size(0) == B, fn,
              "end must be a contiguous int32 [B] on the GPU");
  TORCH_CHECK(k_pool.device() == k_new.device() &&
              v_pool.device() == k_new.device() &&
              k_scale.device() == k_new.device() &&
              v_scale.device() == k_new.device() &&
              v_new.device() == k_new.device(), fn,
              "all tensors must share one device");
  const int64_t MP = block_table.size(1);
  TORCH_CHECK(P < ((int64_t)1 << 31) && MP < ((int64_t)1 << 31) / PS &&
              S < ((int64_t)1 << 31), fn,
              "P, S or MP * PS too large for int");
  a.table = block_table.data_ptr<int>();
  a.end = end.data_ptr<int>();
  a.S = (int)S; a.Hkv = (int)Hkv; a.MP = (int)MP; a.P = (int)P;
  a.ps_shift = __builtin_ctzll((unsigned long long)PS);
  a.rows = B * S * Hkv;
  if (a.rows == 0 || MP == 0 || P == 0) return;
  const int64_t threads = 2 * a.rows * (D / 8);
  const int64_t blocks = (threads + KQ_THREADS - 1) / KQ_THREADS;
  TORCH_CHECK(blocks < ((int64_t)1 << 31), fn, "too many rows for one launch");
  auto stream = hetu_current_stream();
  if (D == 128)
    hipLaunchKernelGGL(kv_cache_append_paged_fp8_kernel<128>,
                       dim3((unsigned)blocks), dim3(KQ_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(kv_cache_append_paged_fp8_kernel<64>,
                       dim3((unsigned)blocks), dim3(KQ_THREADS), 0, stream, a);
  HIP_CHECK(hipGetLastError());
}
