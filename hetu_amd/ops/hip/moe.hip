// MoE routing / layout kernels: top-k gate selection, capacity slot
// assignment, and the dispatch / combine row movement with their backwards.
// Reference parity: hetu/impl/kernel TopKIdx.cu, LayoutTransform.cu,
// ReverseLayoutTransform; written for wave64 from scratch.
//
// Layout: N tokens, E experts, C slots per expert, K choices per token.
//   pos     [E, C] int64   token held by a slot, -1 if the slot is empty
//   slot_of [N, K] int64   flat slot (e*C + q) of a token's k-th choice,
//                          -1 if that choice was dropped
// A token holds at most K slots and a slot holds at most one token, so every
// row kernel below is a gather: one block per OUTPUT row, no atomics, fp32
// accumulation in k order, one rounding.  Every output is a pure function of
// the inputs.
#include <torch/extension.h>
#include <c10/util/Optional.h>
#include "ext_stream.h"
#include "common.h"

// fp16 rows: 8 halves per 16 B lane, same shape as the bf16 VecIO
template <> struct VecIO<__half> {
  static constexpr int VEC = 8;
  DEV static void load(const __half* p, float* out) {
    ushort8 u = *reinterpret_cast<const ushort8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      out[i] = __half2float(__ushort_as_half(u.v[i]));
  }
  DEV static void store(__half* p, const float* in) {
    ushort8 u;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      u.v[i] = __half_as_ushort(__float2half_rn(in[i]));
    *reinterpret_cast<ushort8*>(p) = u;
  }
};

namespace {

constexpr int MOE_MAX_K = 8;
constexpr int MOE_MAX_E = 2048;

// scalar element <-> fp32 (same roundings as the vector paths)
DEV float ld1(const float* p) { return *p; }
DEV float ld1(const bf16* p) {
  return bf2f(*reinterpret_cast<const unsigned short*>(p));
}
DEV float ld1(const __half* p) { return __half2float(*p); }
DEV void st1(float* p, float v) { *p = v; }
DEV void st1(bf16* p, float v) {
  *reinterpret_cast<unsigned short*>(p) = f2bf(v);
}
DEV void st1(__half* p, float v) { *p = __float2half_rn(v); }

#define MOE_DISPATCH(TENSOR, NAME, ...)                                    \
  do {                                                                     \
    if ((TENSOR).scalar_type() == at::kBFloat16) {                         \
      using scalar_t = bf16; __VA_ARGS__();                                \
    } else if ((TENSOR).scalar_type() == at::kFloat) {                     \
      using scalar_t = float; __VA_ARGS__();                               \
    } else if ((TENSOR).scalar_type() == at::kHalf) {                      \
      using scalar_t = __half; __VA_ARGS__();                              \
    } else {                                                               \
      TORCH_CHECK(false, NAME, ": unsupported dtype");                     \
    }                                                                      \
  } while (0)

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// block per row: enough lanes for one 16 B access each, whole waves
int row_block(int64_t h, int vec) {
  int64_t lanes = (h + vec - 1) / vec;
  int64_t b = ((lanes + WAVE - 1) / WAVE) * WAVE;
  return (int)std::min<int64_t>(std::max<int64_t>(b, WAVE), 256);
}

int row_grid(int64_t rows) {
  return (int)std::min<int64_t>(std::max<int64_t>(rows, 1), 1 << 18);
}

// ---------------------------------------------------------------------------
// (a) top-k: one wave per token.  Round k takes the largest not yet taken
// element under the total order (value desc, expert index asc); the order
// is carried as one 64-bit key so the cross-lane arg-max is a plain max.
// Values compare as fp32 (-0 == +0; NaN sorts above +inf, as torch.topk).
// The row is re-read each round (K*E cached reads) instead of held in
// registers, so there is no dynamically indexed register array.
// ---------------------------------------------------------------------------
DEV u64 topk_key(float f, int e) {
  if (f == 0.f) f = 0.f;                       // -0 -> +0
  u32 b = __float_as_uint(f);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)b << 32) | (u64)(0xFFFFFFFFu - (u32)e);
}

template <typename T>
__global__ void moe_topk_kernel(const T* __restrict__ probs,
                                int64_t* __restrict__ idx,
                                float* __restrict__ w,
                                int64_t N, int E, int K) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wpb = blockDim.x >> 6;
  for (int64_t t = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); t < N;
       t += (int64_t)gridDim.x * wpb) {
    const T* row = probs + t * E;
    u64 prev = 0;
    for (int k = 0; k < K; ++k) {
      u64 best = 0;                            // every real key is > 0
      for (int e = lane; e < E; e += WAVE) {
        const u64 key = topk_key(ld1(row + e), e);
        if ((k == 0 || key < prev) && key > best) best = key;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(best, off, WAVE);
        best = o > best ? o : best;
      }
      prev = best;
      if (lane == 0) {
        // K <= E, so a candidate always exists (best != 0) and e < E
        const int e = best ? (int)(0xFFFFFFFFu - (u32)best) : 0;
        idx[t * K + k] = e;
        w[t * K + k] = ld1(row + e);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// (b) slot assignment: one block per expert.  Rounds k = 0..K-1 in order;
// within a round tokens queue in increasing token index.  A chunk is
// ASSIGN_BLOCK * ASSIGN_T consecutive tokens: each wave owns 64 * ASSIGN_T
// of them and ranks them with ASSIGN_T ballots + popcount, a double-buffered
// LDS array carries the wave totals, and `filled` (block-uniform) carries
// the count across chunks and rounds.
// ---------------------------------------------------------------------------
constexpr int ASSIGN_BLOCK = 1024;
constexpr int ASSIGN_WAVES = ASSIGN_BLOCK / WAVE;
constexpr int ASSIGN_T = 4;

__global__ __launch_bounds__(ASSIGN_BLOCK)
void moe_assign_slots_kernel(const int64_t* __restrict__ idx,
                             const float* __restrict__ w,
                             int64_t* __restrict__ pos,
                             int64_t* __restrict__ slot_of,
                             float* __restrict__ wk,
                             int64_t N, int K, int64_t C) {
  __shared__ int wave_tot[2][ASSIGN_WAVES];
  const int64_t e = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const u64 below = lane == 0 ? 0ull : (~0ull >> (WAVE - lane));
  constexpr int64_t CHUNK = (int64_t)ASSIGN_BLOCK * ASSIGN_T;
  int64_t filled = 0;                          // queue length so far
  int buf = 0;
  for (int k = 0; k < K; ++k) {
    for (int64_t c0 = 0; c0 < N; c0 += CHUNK, buf ^= 1) {
      const int64_t w0 = c0 + (int64_t)wid * (WAVE * ASSIGN_T);
      bool mine[ASSIGN_T];
      int rank[ASSIGN_T];
      int run = 0;                             // wave-uniform
#pragma unroll
      for (int j = 0; j < ASSIGN_T; ++j) {
        const int64_t t = w0 + j * WAVE + lane;
        mine[j] = t < N && idx[t * K + k] == e;
        const u64 m = __ballot(mine[j]);
        rank[j] = run + __popcll(m & below);
        run += __popcll(m);
      }
      if (lane == 0) wave_tot[buf][wid] = run;
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int i = 0; i < ASSIGN_WAVES; ++i) {
        const int v = wave_tot[buf][i];
        before += i < wid ? v : 0;
        total += v;
      }
#pragma unroll
      for (int j = 0; j < ASSIGN_T; ++j) {
        if (!mine[j]) continue;
        const int64_t t = w0 + j * WAVE + lane;
        const int64_t q = filled + before + rank[j];
        const bool keep = q < C;
        slot_of[t * K + k] = keep ? e * C + q : -1;
        wk[t * K + k] = keep ? w[t * K + k] : 0.f;
        if (keep) pos[e * C + q] = t;
      }
      filled += total;
    }
  }
  for (int64_t q = (filled < C ? filled : C) + threadIdx.x; q < C;
       q += ASSIGN_BLOCK)
    pos[e * C + q] = -1;
}

// ---------------------------------------------------------------------------
// (c) dispatch: send[s] = x[pos[s]] or zeros.  Pure copy, dtype-agnostic:
// 16 B units when the row size and the base pointers allow, else elements.
// ---------------------------------------------------------------------------
template <typename U>
__global__ void moe_dispatch_rows_kernel(const U* __restrict__ x,
                                         const int64_t* __restrict__ pos,
                                         U* __restrict__ send,
                                         int64_t S, int64_t N, int64_t hu) {
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const int64_t t = pos[s];
    U* dst = send + s * hu;
    if ((u64)t < (u64)N) {
      const U* src = x + t * hu;
      for (int64_t i = threadIdx.x; i < hu; i += blockDim.x) dst[i] = src[i];
    } else {
      for (int64_t i = threadIdx.x; i < hu; i += blockDim.x) dst[i] = U{};
    }
  }
}

// ---------------------------------------------------------------------------
// (d) / (f) token-major weighted gather:
//   out[t] = sum_k wt[t,k] * src[slot_of[t,k]]   over kept k, fp32, k order
// WEIGHTED=false is the dispatch backward (all weights 1).
// ---------------------------------------------------------------------------
template <typename T, bool VECIO, bool WEIGHTED>
__global__ void moe_gather_sum_kernel(const T* __restrict__ src,
                                      const float* __restrict__ wt,
                                      const int64_t* __restrict__ slot_of,
                                      T* __restrict__ out,
                                      int64_t N, int64_t S, int K,
                                      int64_t h) {
  constexpr int V = VECIO ? VecIO<T>::VEC : 1;
  for (int64_t t = blockIdx.x; t < N; t += gridDim.x) {
    int64_t sl[MOE_MAX_K];
    float wv[MOE_MAX_K];
#pragma unroll
    for (int k = 0; k < MOE_MAX_K; ++k) {
      sl[k] = -1;
      wv[k] = 0.f;
      if (k < K) {
        const int64_t s = slot_of[t * K + k];
        if ((u64)s < (u64)S) {
          sl[k] = s;
          wv[k] = WEIGHTED ? wt[t * K + k] : 1.f;
        }
      }
    }
    T* dst = out + t * h;
    for (int64_t i = (int64_t)threadIdx.x * V; i < h;
         i += (int64_t)blockDim.x * V) {
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < MOE_MAX_K; ++k) {
        if (sl[k] < 0) continue;               // block-uniform
        float r[V];
        if constexpr (VECIO) VecIO<T>::load(src + sl[k] * h + i, r);
        else r[0] = ld1(src + sl[k] * h + i);
#pragma unroll
        for (int j = 0; j < V; ++j)
          acc[j] = WEIGHTED ? acc[j] + wv[k] * r[j] : acc[j] + r[j];
      }
      if constexpr (VECIO) VecIO<T>::store(dst + i, acc);
      else st1(dst + i, acc[0]);
    }
  }
}

// ---------------------------------------------------------------------------
// (e) gate backward: dprobs[t, slot_of[t,k] / C] = g_w[t,k] for kept k,
// zero elsewhere.  One thread per dprobs element.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void moe_gate_bwd_kernel(const float* __restrict__ g_w,
                                    const int64_t* __restrict__ slot_of,
                                    T* __restrict__ dprobs,
                                    int64_t N, int E, int K, int64_t C) {
  const int64_t total = N * E;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / E;
    const int64_t e = i - t * E;
    float v = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t s = slot_of[t * K + k];
      if (s >= 0 && s / C == e) v = g_w[t * K + k];
    }
    st1(dprobs + i, v);
  }
}

// ---------------------------------------------------------------------------
// (g) combine backward, slot-major, with dwk folded in: the block of slot s
// (token t = pos[s], choice k found by a <= K step search) writes
//   d_recv[s] = gy[t] * wk[t,k]        and       dwk[t,k] = <gy[t], recv[s]>
// from one read of gy[t] and recv[s].  Empty slots write zero rows; dwk is
// zero-filled by the host wrapper for the dropped entries no block owns.
// ---------------------------------------------------------------------------
template <typename T, bool VECIO>
__global__ void moe_combine_bwd_kernel(const T* __restrict__ gy,
                                       const T* __restrict__ recv,
                                       const float* __restrict__ wk,
                                       const int64_t* __restrict__ pos,
                                       const int64_t* __restrict__ slot_of,
                                       T* __restrict__ d_recv,
                                       float* __restrict__ dwk,
                                       int64_t S, int64_t N, int K,
                                       int64_t h) {
  constexpr int V = VECIO ? VecIO<T>::VEC : 1;
  __shared__ float red[16];
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const int64_t t = pos[s];
    int kk = -1;
    if ((u64)t < (u64)N) {
      for (int k = 0; k < K; ++k)
        if (slot_of[t * K + k] == s) { kk = k; break; }
    }
    T* dst = d_recv + s * h;
    if (kk < 0) {                              // block-uniform
      for (int64_t i = (int64_t)threadIdx.x * V; i < h;
           i += (int64_t)blockDim.x * V) {
        float z[V];
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] = 0.f;
        if constexpr (VECIO) VecIO<T>::store(dst + i, z);
        else st1(dst + i, 0.f);
      }
      continue;
    }
    const float wgt = wk[t * K + kk];
    const T* g = gy + t * h;
    const T* r = recv + s * h;
    float dot = 0.f;
    for (int64_t i = (int64_t)threadIdx.x * V; i < h;
         i += (int64_t)blockDim.x * V) {
      float gv[V], rv[V];
      if constexpr (VECIO) {
        VecIO<T>::load(g + i, gv);
        VecIO<T>::load(r + i, rv);
      } else {
        gv[0] = ld1(g + i);
        rv[0] = ld1(r + i);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        dot += gv[j] * rv[j];
        gv[j] *= wgt;
      }
      if constexpr (VECIO) VecIO<T>::store(dst + i, gv);
      else st1(dst + i, gv[0]);
    }
    dot = block_sum(dot, red);
    if (threadIdx.x == 0) dwk[t * K + kk] = dot;
  }
}

void check_routing(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kLong && t.dim() == 2,
              "moe: ", what, " must be a contiguous 2-d int64 GPU tensor");
}

void check_rows(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2,
              "moe: ", what, " must be a contiguous 2-d GPU tensor");
}

void check_k(int64_t K) {
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K, "moe: need 1 <= K <= 8, got ", K);
}

template <typename T>
bool can_vec(int64_t h, std::initializer_list<const void*> ptrs) {
  if (h % VecIO<T>::VEC) return false;
  for (const void* p : ptrs)
    if (!aligned16(p)) return false;
  return true;
}

}  // namespace

// probs [N, E] -> idx [N, K] int64 (descending value, ties to the lower
// expert index), w [N, K] fp32 (the selected probabilities, unnormalised)
std::vector<torch::Tensor> moe_topk(torch::Tensor probs, int64_t K) {
  check_rows(probs, "probs");
  const int64_t N = probs.size(0), E = probs.size(1);
  check_k(K);
  TORCH_CHECK(K <= E, "moe_topk: K (", K, ") > E (", E, ")");
  TORCH_CHECK(E <= MOE_MAX_E, "moe_topk: E (", E, ") > 2048");
  auto idx = torch::empty({N, K}, probs.options().dtype(at::kLong));
  auto w = torch::empty({N, K}, probs.options().dtype(at::kFloat));
  if (N == 0) return {idx, w};
  constexpr int BLOCK = 256;
  const int wpb = BLOCK / WAVE;
  const int grid = row_grid((N + wpb - 1) / wpb);
  auto stream = hetu_current_stream();
  MOE_DISPATCH(probs, "moe_topk", [&] {
    hipLaunchKernelGGL((moe_topk_kernel<scalar_t>), dim3(grid), dim3(BLOCK),
                       0, stream, (const scalar_t*)probs.data_ptr(),
                       idx.data_ptr<int64_t>(), w.data_ptr<float>(), N,
                       (int)E, (int)K);
  });
  return {idx, w};
}

// idx [N, K] (entries in [0, E)), w [N, K] fp32 -> pos [E, C],
// slot_of [N, K], wk [N, K] fp32.  Entries of idx outside [0, E) belong to
// no expert block and leave their slot_of / wk entries unwritten.
std::vector<torch::Tensor> moe_assign_slots(torch::Tensor idx,
                                            torch::Tensor w, int64_t E,
                                            int64_t C) {
  check_routing(idx, "idx");
  const int64_t N = idx.size(0), K = idx.size(1);
  check_k(K);
  TORCH_CHECK(K <= E, "moe_assign_slots: K (", K, ") > E (", E, ")");
  TORCH_CHECK(E <= MOE_MAX_E, "moe_assign_slots: E (", E, ") > 2048");
  TORCH_CHECK(C >= 1, "moe_assign_slots: C must be >= 1");
  TORCH_CHECK(N * K < (int64_t)1 << 31, "moe_assign_slots: N*K too large");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
              w.scalar_type() == at::kFloat && w.sizes() == idx.sizes(),
              "moe_assign_slots: w must be fp32 [N, K]");
  auto pos = torch::empty({E, C}, idx.options());
  auto slot_of = torch::empty({N, K}, idx.options());
  auto wk = torch::empty({N, K}, w.options());
  auto stream = hetu_current_stream();
  hipLaunchKernelGGL(moe_assign_slots_kernel, dim3((int)E),
                     dim3(ASSIGN_BLOCK), 0, stream, idx.data_ptr<int64_t>(),
                     w.data_ptr<float>(), pos.data_ptr<int64_t>(),
                     slot_of.data_ptr<int64_t>(), wk.data_ptr<float>(), N,
                     (int)K, C);
  return {pos, slot_of, wk};
}

// x [N, h], pos [E, C] -> send [E*C, h]
torch::Tensor moe_dispatch_rows(torch::Tensor x, torch::Tensor pos,
                                c10::optional<torch::Tensor> out) {
  check_rows(x, "x");
  check_routing(pos, "pos");
  const int64_t N = x.size(0), h = x.size(1), S = pos.numel();
  torch::Tensor send;
  if (out.has_value()) {
    send = *out;
    check_rows(send, "out");
    TORCH_CHECK(send.size(0) == S && send.size(1) == h &&
                send.scalar_type() == x.scalar_type(),
                "moe_dispatch_rows: out must be [E*C, h] of x's dtype");
  } else {
    send = torch::empty({S, h}, x.options());
  }
  if (S == 0 || h == 0) return send;
  const int64_t rb = h * x.element_size();
  auto stream = hetu_current_stream();
  const int grid = row_grid(S);
  if (rb % 16 == 0 && aligned16(x.data_ptr()) &&
      aligned16(send.data_ptr())) {
    const int64_t hu = rb / 16;
    hipLaunchKernelGGL((moe_dispatch_rows_kernel<float4v>), dim3(grid),
                       dim3(row_block(hu, 1)), 0, stream,
                       (const float4v*)x.data_ptr(),
                       pos.data_ptr<int64_t>(), (float4v*)send.data_ptr(),
                       S, N, hu);
  } else if (x.element_size() == 4) {
    hipLaunchKernelGGL((moe_dispatch_rows_kernel<u32>), dim3(grid),
                       dim3(row_block(h, 1)), 0, stream,
                       (const u32*)x.data_ptr(), pos.data_ptr<int64_t>(),
                       (u32*)send.data_ptr(), S, N, h);
  } else {
    TORCH_CHECK(x.element_size() == 2, "moe_dispatch_rows: unsupported dtype");
    hipLaunchKernelGGL((moe_dispatch_rows_kernel<unsigned short>),
                       dim3(grid), dim3(row_block(h, 1)), 0, stream,
                       (const unsigned short*)x.data_ptr(),
                       pos.data_ptr<int64_t>(),
                       (unsigned short*)send.data_ptr(), S, N, h);
  }
  return send;
}

namespace {
template <bool WEIGHTED>
torch::Tensor gather_sum(torch::Tensor src, const float* wt,
                         torch::Tensor slot_of, const char* name) {
  check_rows(src, "rows");
  check_routing(slot_of, "slot_of");
  const int64_t S = src.size(0), h = src.size(1);
  const int64_t N = slot_of.size(0), K = slot_of.size(1);
  check_k(K);
  auto out = torch::empty({N, h}, src.options());
  if (N == 0 || h == 0) return out;
  auto stream = hetu_current_stream();
  const int grid = row_grid(N);
  MOE_DISPATCH(src, name, [&] {
    const scalar_t* sp = (const scalar_t*)src.data_ptr();
    scalar_t* op = (scalar_t*)out.data_ptr();
    if (can_vec<scalar_t>(h, {sp, op})) {
      hipLaunchKernelGGL((moe_gather_sum_kernel<scalar_t, true, WEIGHTED>),
                         dim3(grid),
                         dim3(row_block(h, VecIO<scalar_t>::VEC)), 0, stream,
                         sp, wt, slot_of.data_ptr<int64_t>(), op, N, S,
                         (int)K, h);
    } else {
      hipLaunchKernelGGL((moe_gather_sum_kernel<scalar_t, false, WEIGHTED>),
                         dim3(grid), dim3(row_block(h, 1)), 0, stream, sp,
                         wt, slot_of.data_ptr<int64_t>(), op, N, S, (int)K,
                         h);
    }
  });
  return out;
}
}  // namespace

// gsend [E*C, h], slot_of [N, K] -> dx [N, h]
torch::Tensor moe_dispatch_rows_bwd(torch::Tensor gsend,
                                    torch::Tensor slot_of) {
  return gather_sum<false>(gsend, nullptr, slot_of, "moe_dispatch_rows_bwd");
}

// recv [E*C, h], wk [N, K] fp32, slot_of [N, K] -> y [N, h]
torch::Tensor moe_combine_rows(torch::Tensor recv, torch::Tensor wk,
                               torch::Tensor slot_of) {
  TORCH_CHECK(wk.is_cuda() && wk.is_contiguous() &&
              wk.scalar_type() == at::kFloat &&
              wk.sizes() == slot_of.sizes(),
              "moe_combine_rows: wk must be fp32 [N, K]");
  return gather_sum<true>(recv, wk.data_ptr<float>(), slot_of,
                          "moe_combine_rows");
}

// g_w [N, K] fp32, slot_of [N, K], probs [N, E] (shape and dtype only)
// -> dprobs [N, E]
torch::Tensor moe_gate_bwd(torch::Tensor g_w, torch::Tensor slot_of,
                           torch::Tensor probs, int64_t C) {
  check_routing(slot_of, "slot_of");
  check_rows(probs, "probs");
  const int64_t N = slot_of.size(0), K = slot_of.size(1);
  const int64_t E = probs.size(1);
  check_k(K);
  TORCH_CHECK(E <= MOE_MAX_E, "moe_gate_bwd: E (", E, ") > 2048");
  TORCH_CHECK(C >= 1 && probs.size(0) == N, "moe_gate_bwd: bad shapes");
  TORCH_CHECK(g_w.is_cuda() && g_w.is_contiguous() &&
              g_w.scalar_type() == at::kFloat &&
              g_w.sizes() == slot_of.sizes(),
              "moe_gate_bwd: g_w must be fp32 [N, K]");
  auto dprobs = torch::empty_like(probs);
  if (N * E == 0) return dprobs;
  constexpr int BLOCK = 256;
  const int grid = row_grid((N * E + BLOCK - 1) / BLOCK);
  auto stream = hetu_current_stream();
  MOE_DISPATCH(probs, "moe_gate_bwd", [&] {
    hipLaunchKernelGGL((moe_gate_bwd_kernel<scalar_t>), dim3(grid),
                       dim3(BLOCK), 0, stream, g_w.data_ptr<float>(),
                       slot_of.data_ptr<int64_t>(),
                       (scalar_t*)dprobs.data_ptr(), N, (int)E, (int)K, C);
  });
  return dprobs;
}

// gy [N, h], recv [E*C, h], wk [N, K] fp32, pos [E, C], slot_of [N, K]
// -> d_recv [E*C, h], dwk [N, K] fp32
std::vector<torch::Tensor> moe_combine_rows_bwd(
    torch::Tensor gy, torch::Tensor recv, torch::Tensor wk,
    torch::Tensor pos, torch::Tensor slot_of,
    c10::optional<torch::Tensor> out) {
  check_rows(gy, "gy");
  check_rows(recv, "recv");
  check_routing(pos, "pos");
  check_routing(slot_of, "slot_of");
  const int64_t N = gy.size(0), h = gy.size(1), S = pos.numel();
  const int64_t K = slot_of.size(1);
  check_k(K);
  TORCH_CHECK(recv.size(0) == S && recv.size(1) == h &&
              recv.scalar_type() == gy.scalar_type() &&
              slot_of.size(0) == N,
              "moe_combine_rows_bwd: bad shapes");
  TORCH_CHECK(wk.is_cuda() && wk.is_contiguous() &&
              wk.scalar_type() == at::kFloat &&
              wk.sizes() == slot_of.sizes(),
              "moe_combine_rows_bwd: wk must be fp32 [N, K]");
  torch::Tensor d_recv;
  if (out.has_value()) {
    d_recv = *out;
    check_rows(d_recv, "out");
    TORCH_CHECK(d_recv.sizes() == recv.sizes() &&
                d_recv.scalar_type() == recv.scalar_type(),
                "moe_combine_rows_bwd: out must match recv");
  } else {
    d_recv = torch::empty_like(recv);
  }
  auto dwk = torch::zeros_like(wk);
  if (S == 0 || h == 0) return {d_recv, dwk};
  auto stream = hetu_current_stream();
  const int grid = row_grid(S);
  MOE_DISPATCH(gy, "moe_combine_rows_bwd", [&] {
    const scalar_t* gp = (const scalar_t*)gy.data_ptr();
    const scalar_t* rp = (const scalar_t*)recv.data_ptr();
    scalar_t* dp = (scalar_t*)d_recv.data_ptr();
    if (can_vec<scalar_t>(h, {gp, rp, dp})) {
      hipLaunchKernelGGL((moe_combine_bwd_kernel<scalar_t, true>),
                         dim3(grid),
                         dim3(row_block(h, VecIO<scalar_t>::VEC)), 0, stream,
                         gp, rp, wk.data_ptr<float>(),
                         pos.data_ptr<int64_t>(),
                         slot_of.data_ptr<int64_t>(), dp,
                         dwk.data_ptr<float>(), S, N, (int)K, h);
    } else {
      hipLaunchKernelGGL((moe_combine_bwd_kernel<scalar_t, false>),
                         dim3(grid), dim3(row_block(h, 1)), 0, stream, gp,
                         rp, wk.data_ptr<float>(), pos.data_ptr<int64_t>(),
                         slot_of.data_ptr<int64_t>(), dp,
                         dwk.data_ptr<float>(), S, N, (int)K, h);
    }
  });
  return {d_recv, dwk};
}
