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

namespace {

constexpr int DEC_BN = 64;             // keys per block tile
constexpr int DEC_WAVES = 4;           // 16 keys of the tile each
constexpr int DEC_THREADS = DEC_WAVES * WAVE;
constexpr int DEC_WKEYS = DEC_BN / DEC_WAVES;
constexpr int DEC_MAX_GC = 8;          // query heads per pass
constexpr int DEC_MAX_SPLITS = 64;

template <int CTRL>
DEV float dec_dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf,
                                            0xf, false);
  return x + __int_as_float(y);
}

// sum over the LPR (8 or 16) consecutive lanes of a row; every lane of the
// group gets the total.  xor 1, xor 2, then the two mirrors (after the quad
// steps all lanes of a quad agree, so a mirror is as good as an xor).
template <int LPR>
DEV float dec_row_sum(float x) {
  x = dec_dpp_add<0xB1>(x);            // quad_perm [1,0,3,2]
  x = dec_dpp_add<0x4E>(x);            // quad_perm [2,3,0,1]
  x = dec_dpp_add<0x141>(x);           // row_half_mirror
  if constexpr (LPR == 16) x = dec_dpp_add<0x140>(x);   // row_mirror
  return x;
}

DEV float dec_dot2(u32 a, u32 b, float acc) {
  typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, a),
                                         __builtin_bit_cast(v2bf, b), acc,
                                         false);
}

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

template <int D, int GC>
__global__ __launch_bounds__(DEC_THREADS)
void fa_decode_kernel(DecArgs a) {
  constexpr int LPR = D / 8;           // lanes per row
  constexpr int KPI = WAVE / LPR;      // rows per wave load
  constexpr int NI = DEC_WKEYS / KPI;  // loads per wave per tile
  __shared__ float s_o[DEC_WAVES][GC][D];
  __shared__ float s_m[DEC_WAVES][GC];
  __shared__ float s_l[DEC_WAVES][GC];

  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int G = a.H / a.Hkv;
  const int ns = a.ns;
  const int kv = min(max(a.kv_len[b], 0), a.L);
  const int n_tiles = (kv + DEC_BN - 1) / DEC_BN;
  const int tps = (n_tiles + ns - 1) / ns;
  const int t0 = split * tps;
  const int t1 = min(n_tiles, t0 + tps);
  const int64_t row0 = (int64_t)b * a.H + (int64_t)hkv * G;   // (b, head 0)

  if (t0 >= t1) {                      // block-uniform: no loads, no barrier
    for (int g = threadIdx.x; g < G; g += DEC_THREADS) {
      if (ns == 1) a.lse[row0 + g] = -INFINITY;
      else a.ws_lse[(row0 + g) * ns + split] = -INFINITY;
    }
    if (ns == 1) {                     // kv == 0: the row's output is zero
      ushort8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z.v[j] = 0;
      for (int i = threadIdx.x; i < G * LPR; i += DEC_THREADS)
        *reinterpret_cast<ushort8*>(a.out + row0 * D + (int64_t)i * 8) = z;
    }
    return;
  }

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x >> 6;
  const int rg = lane / LPR;           // row of a wave load
  const int ds = (lane % LPR) * 8;     // this lane's 8 dims
  const bf16* kb = a.k + (int64_t)b * a.k_bs + (int64_t)hkv * a.k_hs + ds;
  const bf16* vb = a.v + (int64_t)b * a.v_bs + (int64_t)hkv * a.v_hs + ds;
  const float scale = a.scale;

  for (int c0 = 0; c0 < G; c0 += GC) {
    uint4 qf[GC];
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      qf[g] = make_uint4(0, 0, 0, 0);
      if (c0 + g < G)
        qf[g] = *reinterpret_cast<const uint4*>(
            a.q + (int64_t)b * a.q_bs +
            (int64_t)(hkv * G + c0 + g) * a.q_hs + ds);
    }
    float m[GC], l[GC], acc[GC][8];
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      m[g] = -INFINITY;
      l[g] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }

    for (int t = t0; t < t1; ++t) {
      const int kbase = t * DEC_BN + wave * DEC_WKEYS;
      if (kbase >= kv) continue;       // wave-uniform: all 16 keys masked
      uint4 kf[NI], vf[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int row = min(kbase + i * KPI + rg, kv - 1);
        kf[i] = *reinterpret_cast<const uint4*>(kb + (int64_t)row * a.k_rs);
        vf[i] = *reinterpret_cast<const uint4*>(vb + (int64_t)row * a.v_rs);
      }
      float s[GC][NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const bool valid = kbase + i * KPI + rg < kv;
#pragma unroll
        for (int g = 0; g < GC; ++g) {
          float d = dec_dot2(kf[i].x, qf[g].x, 0.f);
          d = dec_dot2(kf[i].y, qf[g].y, d);
          d = dec_dot2(kf[i].z, qf[g].z, d);
          d = dec_dot2(kf[i].w, qf[g].w, d);
          d = dec_row_sum<LPR>(d) * scale;
          s[g][i] = valid ? d : -INFINITY;
        }
      }
      float alpha[GC], ms[GC];
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        float mn = m[g];
#pragma unroll
        for (int i = 0; i < NI; ++i) mn = fmaxf(mn, s[g][i]);
        ms[g] = mn == -INFINITY ? 0.f : mn;
        alpha[g] = __expf(m[g] - ms[g]);
        m[g] = mn;
        l[g] *= alpha[g];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] *= alpha[g];
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const bool valid = kbase + i * KPI + rg < kv;
        float vv[8];
        const u32 w[4] = {vf[i].x, vf[i].y, vf[i].z, vf[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          vv[2 * j] = __uint_as_float(w[j] << 16);
          vv[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
#pragma unroll
        for (int g = 0; g < GC; ++g) {
          const float p = valid ? __expf(s[g][i] - ms[g]) : 0.f;
          l[g] += p;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[g][j] += p * vv[j];
        }
      }
    }

    // merge the row groups of the wave (butterfly: every lane ends with the
    // wave's stream)
#pragma unroll
    for (int off = LPR; off < WAVE; off <<= 1) {
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const float mo = __shfl_xor(m[g], off, WAVE);
        const float lo = __shfl_xor(l[g], off, WAVE);
        const float mn = fmaxf(m[g], mo);
        const float msafe = mn == -INFINITY ? 0.f : mn;
        const float wa = __expf(m[g] - msafe), wb = __expf(mo - msafe);
        l[g] = l[g] * wa + lo * wb;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[g][j] = acc[g][j] * wa + __shfl_xor(acc[g][j], off, WAVE) * wb;
        m[g] = mn;
      }
    }
    if (rg == 0) {
#pragma unroll
      for (int g = 0; g < GC; ++g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s_o[wave][g][ds + j] = acc[g][j];
        if (lane == 0) {
          s_m[wave][g] = m[g];
          s_l[wave][g] = l[g];
        }
      }
    }
    __syncthreads();
    // the waves in wave order; thread = (head of the chunk, 8 dims).  The
    // split is not empty, so at least one wave met a valid key: mx is finite.
    if (threadIdx.x < GC * LPR) {
      const int g = threadIdx.x / LPR;
      const int d0 = (threadIdx.x % LPR) * 8;
      if (c0 + g < G) {
        float mx = s_m[0][g];
#pragma unroll
        for (int w = 1; w < DEC_WAVES; ++w) mx = fmaxf(mx, s_m[w][g]);
        float lt = 0.f, o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
          const float ww = __expf(s_m[w][g] - mx);
          lt += s_l[w][g] * ww;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += s_o[w][g][d0 + j] * ww;
        }
        const float inv = 1.f / lt;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] *= inv;
        const int64_t row = row0 + c0 + g;
        const float ls = mx + logf(lt);
        if (ns == 1) {
          bf16* dst = a.out + row * D + d0;
          fa_store4_bf16(dst, o[0], o[1], o[2], o[3]);
          fa_store4_bf16(dst + 4, o[4], o[5], o[6], o[7]);
          if (d0 == 0) a.lse[row] = ls;
        } else {
          float* dst = a.ws_o + (row * ns + split) * D + d0;
          VecIO<float>::store(dst, o);
          VecIO<float>::store(dst + 4, o + 4);
          if (d0 == 0) a.ws_lse[row * ns + split] = ls;
        }
      }
    }
    __syncthreads();                   // s_o is reused by the next chunk
  }
}

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

bool dec_aligned16(const void* p) {
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

}  // namespace

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

std::vector<torch::Tensor> flash_attn_decode(torch::Tensor q,
                                             torch::Tensor k_cache,
                                             torch::Tensor v_cache,
                                             torch::Tensor kv_len,
                                             double scale,
                                             int64_t num_splits) {
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
              kv_len.is_cuda(),
              "flash_attn_decode: q, k_cache, v_cache and kv_len must be on "
              "the GPU");
  TORCH_CHECK(q.device() == k_cache.device() &&
              q.device() == v_cache.device() && q.device() == kv_len.device(),
              "flash_attn_decode: all tensors must share one device");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
              k_cache.scalar_type() == at::kBFloat16 &&
              v_cache.scalar_type() == at::kBFloat16,
              "flash_attn_decode: q, k_cache and v_cache must be bf16");
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4,
              "flash_attn_decode: need q [B, H, D] and caches "
              "[B, Hkv, L, D]");
  const int64_t B = q.size(0), H = q.size(1), D = q.size(2);
  const int64_t Hkv = k_cache.size(1), L = k_cache.size(2);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B &&
              k_cache.size(3) == D,
              "flash_attn_decode: cache shapes do not match q");
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_decode: D must be 64 or 128, "
              "got ", D);
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, "flash_attn_decode: H (", H,
              ") is not a multiple of Hkv (", Hkv, ")");
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.dim() == 1 &&
              kv_len.size(0) == B && kv_len.is_contiguous(),
              "flash_attn_decode: kv_len must be a contiguous int32 [B]");
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 && L < ((int64_t)1 << 31) - DEC_BN,
              "flash_attn_decode: B, Hkv or L too large");
  TORCH_CHECK(num_splits >= 0, "flash_attn_decode: num_splits must be >= 0");
  auto out = torch::empty({B, H, D}, q.options());
  auto lse = torch::empty({B, H}, q.options().dtype(at::kFloat));
  if (B == 0 || H == 0) return {out, lse};
  dec_check_strides(q, "q");
  dec_check_strides(k_cache, "k_cache");
  dec_check_strides(v_cache, "v_cache");

  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int ns = (int)(num_splits > 0
                           ? std::min<int64_t>(num_splits, 1 << 16)
                           : decode_attn_num_splits(B, Hkv, L, cus));
  torch::Tensor ws;
  DecArgs a;
  a.q = (const bf16*)q.data_ptr();
  a.k = (const bf16*)k_cache.data_ptr();
  a.v = (const bf16*)v_cache.data_ptr();
  a.kv_len = kv_len.data_ptr<int>();
  a.out = (bf16*)out.data_ptr();
  a.lse = lse.data_ptr<float>();
  a.ws_o = nullptr;
  a.ws_lse = nullptr;
  if (ns > 1) {                        // caching allocator, stream-ordered
    ws = torch::empty({B * H * ns * (D + 1)}, lse.options());
    a.ws_o = ws.data_ptr<float>();
    a.ws_lse = a.ws_o + B * H * ns * D;
  }
  a.q_bs = q.stride(0); a.q_hs = q.stride(1);
  a.k_bs = k_cache.stride(0); a.k_hs = k_cache.stride(1);
  a.k_rs = k_cache.stride(2);
  a.v_bs = v_cache.stride(0); a.v_hs = v_cache.stride(1);
  a.v_rs = v_cache.stride(2);
  a.H = (int)H; a.Hkv = (int)Hkv; a.L = (int)L; a.ns = ns;
  a.scale = (float)scale;

  const int64_t G = H / Hkv;
  const int gc = G >= 5 ? 8 : G >= 3 ? 4 : (int)G;
  auto stream = hetu_current_stream();
  const dim3 grid(ns, (unsigned)Hkv, (unsigned)B);
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
  if (ns > 1) {
    hipLaunchKernelGGL(fa_decode_merge_kernel, dim3((unsigned)(B * H)),
                       dim3((unsigned)D), 0, stream, a.ws_o, a.ws_lse, a.out,
                       a.lse, ns, (int)D);
    HIP_CHECK(hipGetLastError());
  }
  return {out, lse};
}
