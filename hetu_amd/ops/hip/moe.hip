// MoE routing / layout kernels: top-k gate selection, capacity slot
// assignment, and the dispatch / combine row movement with their backwards.
// Section (h) adds the fused gate: softmax + top-k + the load-balance and
// router z-loss statistics, forward and backward.
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

// ---------------------------------------------------------------------------
// (h) fused gate: softmax + top-k + load-balance / z-loss statistics.
//   lse[t]  = logsumexp_e logits[t,e]          p32 = exp(logits - lse)
//   probs   = p32 rounded once to T            idx, w = moe_topk(probs)
//   psum[e] = sum_t p32[t,e]                   cnt[e] = #{(t,k): idx[t,k]==e}
//   aux = E/N^2 * sum_e psum[e]*cnt[e]         z = 1/N * sum_t lse[t]^2
// A group of gw lanes (a power of two, a whole wave once E > 32) owns a
// token; lane l of the group owns experts l, l+gw, ...  For E <= 256 the row
// lives in registers (R = 1, 2 or 4 elements per lane): one read of logits,
// one write of probs, and the K selection rounds of moe_topk run on the
// rounded values without touching memory.  Larger E takes the looping
// kernel, which re-reads the row as moe_topk does.  The grid is capped at
// GATE_MAX_BLOCKS and grid-strided.  Each group keeps an fp32 psum row and
// an int cnt row in LDS ([groups][E] each; 64 KiB at E = 2048); only the
// owning lane touches a column, so there are no conflicts and no atomics.
// The block adds its groups' rows in group order into one row of part_p /
// part_c / part_z; moe_gate_colsum_kernel sums the partial rows in a fixed
// order and (one block, E <= 64) also forms the scalars, else
// moe_gate_scalars_kernel does.  Grid and group shape depend on N and E
// only, so every output is a pure function of the inputs.
// ---------------------------------------------------------------------------
constexpr int GATE_BLOCK = 256;
constexpr int GATE_WAVES = GATE_BLOCK / WAVE;
constexpr int GATE_MAX_BLOCKS = 1024;
constexpr int GATE_REG_E = 256;                // largest E held in registers

// the value half of a topk_key (values here are probabilities, never -0)
DEV float topk_key_value(u64 key) {
  const u32 b = (u32)(key >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}

// what st1 stores, read back
DEV float stored(const float*, float v) { return v; }
DEV float stored(const bf16*, float v) { return bf2f(f2bf(v)); }
DEV float stored(const __half*, float v) {
  return __half2float(__float2half_rn(v));
}

// fixed-order fp64 block sum (<= 16 waves; smem holds 16 doubles); the
// result is valid on thread 0
DEV double block_sum_f64(double x, double* smem) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int nwaves = (blockDim.x + WAVE - 1) >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  if (lane == 0) smem[wid] = x;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < nwaves; ++i) r += smem[i];
  __syncthreads();
  return r;
}

// butterflies over a group of gw lanes: every lane gets the same bits
DEV float group_max(float x, int gw) {
  for (int off = gw >> 1; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, WAVE));
  return x;
}
DEV float group_sum(float x, int gw) {
  for (int off = gw >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}
DEV u64 group_max(u64 x, int gw) {
  for (int off = gw >> 1; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(x, off, WAVE);
    x = o > x ? o : x;
  }
  return x;
}

// lanes per token of the forward kernels
int gate_group_width(int64_t E) {
  int gw = 1;
  while (gw < E && gw < WAVE) gw <<= 1;
  return gw;
}

// block epilogue: rows of the block's groups -> one partial row, in group
// order; then the groups' z sums through the same LDS
DEV void gate_block_partials(float* lds, int groups, int E, int gid,
                             bool leader, float zacc,
                             float* __restrict__ part_p,
                             int* __restrict__ part_c,
                             float* __restrict__ part_z) {
  __syncthreads();
  const float* P = lds;
  const int* Cn = reinterpret_cast<const int*>(lds + (size_t)groups * E);
  for (int e = threadIdx.x; e < E; e += GATE_BLOCK) {
    float ps = P[e];
    int cs = Cn[e];
    for (int i = 1; i < groups; ++i) {
      ps += P[(size_t)i * E + e];
      cs += Cn[(size_t)i * E + e];
    }
    part_p[(int64_t)blockIdx.x * E + e] = ps;
    part_c[(int64_t)blockIdx.x * E + e] = cs;
  }
  __syncthreads();                             // rows consumed: reuse for z
  if (leader) lds[gid] = zacc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float zs = lds[0];
    for (int i = 1; i < groups; ++i) zs += lds[i];
    part_z[blockIdx.x] = zs;
  }
}

template <typename T, int R>
__global__ __launch_bounds__(GATE_BLOCK)
void moe_gate_fwd_kernel(const T* __restrict__ logits, T* __restrict__ probs,
                         int64_t* __restrict__ idx, float* __restrict__ w,
                         float* __restrict__ lse, float* __restrict__ part_p,
                         int* __restrict__ part_c, float* __restrict__ part_z,
                         int64_t N, int E, int K, int gw) {
  extern __shared__ float gate_lds[];          // [groups][E] fp32, then int
  const int groups = GATE_BLOCK / gw;
  const int gl = threadIdx.x & (gw - 1);
  const int gid = threadIdx.x / gw;
  float* sp = gate_lds + (size_t)gid * E;
  int* sc = reinterpret_cast<int*>(gate_lds + (size_t)groups * E) +
            (size_t)gid * E;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = gl + gw * r;
    if (e < E) {
      sp[e] = 0.f;
      sc[e] = 0;
    }
  }
  float zacc = 0.f;                            // group-uniform
  for (int64_t t = (int64_t)blockIdx.x * groups + gid; t < N;
       t += (int64_t)gridDim.x * groups) {
    const T* x = logits + t * E;
    T* pr = probs + t * E;
    float v[R];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = gl + gw * r;
      v[r] = e < E ? ld1(x + e) : -INFINITY;
      m = fmaxf(m, v[r]);
    }
    m = group_max(m, gw);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = expf(v[r] - m);                   // 0 beyond E
      s += v[r];
    }
    s = group_sum(s, gw);
    const float l = m + logf(s);
    u64 key[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = gl + gw * r;
      key[r] = 0;
      if (e < E) {
        const float p = v[r] / s;
        st1(pr + e, p);
        sp[e] += p;
        key[r] = topk_key(stored(pr, p), e);
      }
    }
    zacc += l * l;
    u64 prev = 0;
    for (int k = 0; k < K; ++k) {
      u64 best = 0;                            // every real key is > 0
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((k == 0 || key[r] < prev) && key[r] > best) best = key[r];
      best = group_max(best, gw);
      prev = best;
      const int e = best ? (int)(0xFFFFFFFFu - (u32)best) : 0;
      if ((e & (gw - 1)) == gl && e < E) sc[e] += 1;
      if (gl == 0) {
        idx[t * K + k] = e;
        w[t * K + k] = topk_key_value(best);
      }
    }
    if (gl == 0) lse[t] = l;
  }
  gate_block_partials(gate_lds, groups, E, gid, gl == 0, zacc, part_p,
                      part_c, part_z);
}

// E > GATE_REG_E: one wave per token, the row re-read per pass and round
template <typename T>
__global__ __launch_bounds__(GATE_BLOCK)
void moe_gate_fwd_loop_kernel(const T* __restrict__ logits, T* probs,
                              int64_t* __restrict__ idx,
                              float* __restrict__ w, float* __restrict__ lse,
                              float* __restrict__ part_p,
                              int* __restrict__ part_c,
                              float* __restrict__ part_z, int64_t N, int E,
                              int K) {
  extern __shared__ float gate_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  float* sp = gate_lds + (size_t)wid * E;
  int* sc = reinterpret_cast<int*>(gate_lds + (size_t)GATE_WAVES * E) +
            (size_t)wid * E;
  for (int e = lane; e < E; e += WAVE) {
    sp[e] = 0.f;
    sc[e] = 0;
  }
  float zacc = 0.f;                            // wave-uniform
  for (int64_t t = (int64_t)blockIdx.x * GATE_WAVES + wid; t < N;
       t += (int64_t)gridDim.x * GATE_WAVES) {
    const T* x = logits + t * E;
    T* pr = probs + t * E;
    float m = -INFINITY;
    for (int e = lane; e < E; e += WAVE) m = fmaxf(m, ld1(x + e));
    m = wave_max(m);
    float s = 0.f;
    for (int e = lane; e < E; e += WAVE) s += expf(ld1(x + e) - m);
    s = wave_sum(s);
    const float l = m + logf(s);
    for (int e = lane; e < E; e += WAVE) {
      const float p = expf(ld1(x + e) - m) / s;
      st1(pr + e, p);
      sp[e] += p;
    }
    zacc += l * l;
    // a lane re-reads only the elements it stored itself
    u64 prev = 0;
    for (int k = 0; k < K; ++k) {
      u64 best = 0;
      for (int e = lane; e < E; e += WAVE) {
        const u64 key = topk_key(ld1(pr + e), e);
        if ((k == 0 || key < prev) && key > best) best = key;
      }
      best = group_max(best, WAVE);
      prev = best;
      const int e = best ? (int)(0xFFFFFFFFu - (u32)best) : 0;
      if ((e & (WAVE - 1)) == lane && e < E) sc[e] += 1;
      if (lane == 0) {
        idx[t * K + k] = e;
        w[t * K + k] = topk_key_value(best);
      }
    }
    if (lane == 0) lse[t] = l;
  }
  gate_block_partials(gate_lds, GATE_WAVES, E, wid, lane == 0, zacc, part_p,
                      part_c, part_z);
}

// psum[e] = sum_g part_p[g,e], cnt[e] = sum_g part_c[g,e]: a block owns 64
// columns, wave i sums rows i, i+16, ... in order, wave 0 adds the sixteen.
// A grid of one block (E <= 64) forms aux and z as well.
constexpr int COLSUM_BLOCK = 1024;
constexpr int COLSUM_WAVES = COLSUM_BLOCK / WAVE;

__global__ __launch_bounds__(COLSUM_BLOCK)
void moe_gate_colsum_kernel(const float* __restrict__ part_p,
                            const int* __restrict__ part_c,
                            const float* __restrict__ part_z,
                            float* __restrict__ psum, int* __restrict__ cnt,
                            float* __restrict__ aux, float* __restrict__ z,
                            int G, int E, double aux_scale, double z_scale) {
  __shared__ float sp[COLSUM_WAVES][WAVE];
  __shared__ int sc[COLSUM_WAVES][WAVE];
  __shared__ double red[16];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int e = blockIdx.x * WAVE + lane;
  float ps = 0.f;
  int cs = 0;
  if (e < E) {
#pragma unroll 4
    for (int g = wid; g < G; g += COLSUM_WAVES) {
      ps += part_p[(int64_t)g * E + e];
      cs += part_c[(int64_t)g * E + e];
    }
  }
  sp[wid][lane] = ps;
  sc[wid][lane] = cs;
  __syncthreads();
  double a = 0.0;                              // aux, z: fp64, one rounding
  if (wid == 0 && e < E) {
#pragma unroll
    for (int i = 1; i < COLSUM_WAVES; ++i) {
      ps += sp[i][lane];
      cs += sc[i][lane];
    }
    psum[e] = ps;
    cnt[e] = cs;
    a = (double)ps * (double)cs;
  }
  if (gridDim.x == 1) {                        // block-uniform
    double zs = 0.0;
    for (int g = threadIdx.x; g < G; g += COLSUM_BLOCK) zs += part_z[g];
    a = block_sum_f64(a, red);
    zs = block_sum_f64(zs, red);
    if (threadIdx.x == 0) {
      aux[0] = (float)(a * aux_scale);
      z[0] = (float)(zs * z_scale);
    }
  }
}

// aux = aux_scale * sum_e psum[e]*cnt[e], z = z_scale * sum_g part_z[g]:
// one block, strided per-thread fp64 sums, then a fixed-order block sum.
__global__ __launch_bounds__(GATE_BLOCK)
void moe_gate_scalars_kernel(const float* __restrict__ psum,
                             const int* __restrict__ cnt,
                             const float* __restrict__ part_z,
                             float* __restrict__ aux, float* __restrict__ z,
                             int G, int E, double aux_scale,
                             double z_scale) {
  __shared__ double red[16];
  double a = 0.0, zs = 0.0;
  for (int e = threadIdx.x; e < E; e += GATE_BLOCK)
    a += (double)psum[e] * (double)cnt[e];
  for (int g = threadIdx.x; g < G; g += GATE_BLOCK) zs += part_z[g];
  a = block_sum_f64(a, red);
  zs = block_sum_f64(zs, red);
  if (threadIdx.x == 0) {
    aux[0] = (float)(a * aux_scale);
    z[0] = (float)(zs * z_scale);
  }
}

// gate backward: gw lanes per token (a power of two, enough for one 16 B
// access each up to a whole wave), p32 recomputed from logits and lse,
//   dp = g_probs + g_aux * aux_scale * cnt
//   dlogits = p32 * (dp - <p32, dp>) + g_z * z_scale * lse * p32
// g_probs / g_aux / g_z may be null (zero); the scalars are read here.
template <typename T, bool VECIO>
__global__ __launch_bounds__(GATE_BLOCK)
void moe_gate_grad_kernel(const T* __restrict__ g_probs,
                          const float* __restrict__ g_aux,
                          const float* __restrict__ g_z,
                          const T* __restrict__ logits,
                          const float* __restrict__ lse,
                          const int* __restrict__ cnt,
                          T* __restrict__ dlogits, int64_t N, int E,
                          float aux_scale, float z_scale, int gw) {
  constexpr int V = VECIO ? VecIO<T>::VEC : 1;
  const int groups = GATE_BLOCK / gw;
  const int gl = threadIdx.x & (gw - 1);
  const int gid = threadIdx.x / gw;
  const float ca = g_aux ? g_aux[0] * aux_scale : 0.f;
  const float cz = g_z ? g_z[0] * z_scale : 0.f;
  for (int64_t t = (int64_t)blockIdx.x * groups + gid; t < N;
       t += (int64_t)gridDim.x * groups) {
    const T* x = logits + t * E;
    const T* gp = g_probs ? g_probs + t * E : nullptr;
    T* dst = dlogits + t * E;
    const float l = lse[t];
    float dot = 0.f;
    for (int i = gl * V; i < E; i += gw * V) {
      float xv[V], gv[V];
      if constexpr (VECIO) VecIO<T>::load(x + i, xv);
      else xv[0] = ld1(x + i);
#pragma unroll
      for (int j = 0; j < V; ++j) gv[j] = 0.f;
      if (gp) {
        if constexpr (VECIO) VecIO<T>::load(gp + i, gv);
        else gv[0] = ld1(gp + i);
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        dot += expf(xv[j] - l) * (gv[j] + ca * (float)cnt[i + j]);
    }
    dot = group_sum(dot, gw);
    const float zl = cz * l;
    for (int i = gl * V; i < E; i += gw * V) {
      float xv[V], gv[V];
      if constexpr (VECIO) VecIO<T>::load(x + i, xv);
      else xv[0] = ld1(x + i);
#pragma unroll
      for (int j = 0; j < V; ++j) gv[j] = 0.f;
      if (gp) {
        if constexpr (VECIO) VecIO<T>::load(gp + i, gv);
        else gv[0] = ld1(gp + i);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float p = expf(xv[j] - l);
        const float dp = gv[j] + ca * (float)cnt[i + j];
        xv[j] = p * (dp - dot) + zl * p;
      }
      if constexpr (VECIO) VecIO<T>::store(dst + i, xv);
      else st1(dst + i, xv[0]);
    }
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

// the fused gate's grid cap and the tokens a block takes per pass: with
// N > 2 * tokens_per_block(E) * max_blocks every block loops at least twice
int64_t moe_gate_max_blocks() { return GATE_MAX_BLOCKS; }
int64_t moe_gate_tokens_per_block(int64_t E) {
  return E <= GATE_REG_E ? GATE_BLOCK / gate_group_width(E) : GATE_WAVES;
}

// logits [N, E] -> probs [N, E], idx [N, K] int64, w [N, K] fp32,
// lse [N] fp32, psum [E] fp32, cnt [E] int32, aux [] fp32, z [] fp32
std::vector<torch::Tensor> moe_gate_fwd(torch::Tensor logits, int64_t K) {
  check_rows(logits, "logits");
  const int64_t N = logits.size(0), E = logits.size(1);
  check_k(K);
  TORCH_CHECK(N >= 1, "moe_gate_fwd: no tokens");
  TORCH_CHECK(K <= E, "moe_gate_fwd: K (", K, ") > E (", E, ")");
  TORCH_CHECK(E <= MOE_MAX_E, "moe_gate_fwd: E (", E, ") > 2048");
  const int gw = gate_group_width(E);
  const int groups = (int)moe_gate_tokens_per_block(E);
  const int G = (int)std::min<int64_t>((N + groups - 1) / groups,
                                       GATE_MAX_BLOCKS);
  auto probs = torch::empty_like(logits);
  auto idx = torch::empty({N, K}, logits.options().dtype(at::kLong));
  // the fp32 outputs share one allocation; the [G, E] workspace is apart,
  // so a saved lse / aux does not keep it alive
  auto f32 = logits.options().dtype(at::kFloat);
  auto i32 = logits.options().dtype(at::kInt);
  auto fout = torch::empty({N * K + N + E + 2}, f32);
  int64_t off = 0;
  auto take = [&off](const torch::Tensor& buf, int64_t n) {
    auto t = buf.narrow(0, off, n);
    off += n;
    return t;
  };
  auto w = take(fout, N * K).view({N, K});
  auto lse = take(fout, N);
  auto psum = take(fout, E);
  auto aux = take(fout, 1).squeeze(0);
  auto z = take(fout, 1).squeeze(0);
  auto cnt = torch::empty({E}, i32);
  auto fwork = torch::empty({(int64_t)G * E + G}, f32);
  off = 0;
  auto part_p = take(fwork, (int64_t)G * E);
  auto part_z = take(fwork, G);
  auto part_c = torch::empty({(int64_t)G * E}, i32);
  const size_t lds = (size_t)groups * E * (sizeof(float) + sizeof(int));
  auto stream = hetu_current_stream();
#define GATE_FWD_ARGS                                                      \
  (const scalar_t*)logits.data_ptr(), (scalar_t*)probs.data_ptr(),         \
      idx.data_ptr<int64_t>(), w.data_ptr<float>(), lse.data_ptr<float>(), \
      part_p.data_ptr<float>(), part_c.data_ptr<int>(),                    \
      part_z.data_ptr<float>(), N, (int)E, (int)K
  MOE_DISPATCH(logits, "moe_gate_fwd", [&] {
    if (E <= WAVE) {
      hipLaunchKernelGGL((moe_gate_fwd_kernel<scalar_t, 1>), dim3(G),
                         dim3(GATE_BLOCK), lds, stream, GATE_FWD_ARGS, gw);
    } else if (E <= 2 * WAVE) {
      hipLaunchKernelGGL((moe_gate_fwd_kernel<scalar_t, 2>), dim3(G),
                         dim3(GATE_BLOCK), lds, stream, GATE_FWD_ARGS, gw);
    } else if (E <= GATE_REG_E) {
      hipLaunchKernelGGL((moe_gate_fwd_kernel<scalar_t, GATE_REG_E / WAVE>),
                         dim3(G), dim3(GATE_BLOCK), lds, stream,
                         GATE_FWD_ARGS, gw);
    } else {
      hipLaunchKernelGGL((moe_gate_fwd_loop_kernel<scalar_t>), dim3(G),
                         dim3(GATE_BLOCK), lds, stream, GATE_FWD_ARGS);
    }
  });
#undef GATE_FWD_ARGS
  HIP_CHECK(hipGetLastError());
  const double n = (double)N;
  const double aux_scale = (double)E / (n * n);
  const double z_scale = 1.0 / n;
  const int cgrid = (int)((E + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(moe_gate_colsum_kernel, dim3(cgrid), dim3(COLSUM_BLOCK),
                     0, stream, part_p.data_ptr<float>(),
                     part_c.data_ptr<int>(), part_z.data_ptr<float>(),
                     psum.data_ptr<float>(), cnt.data_ptr<int>(),
                     aux.data_ptr<float>(), z.data_ptr<float>(), G, (int)E,
                     aux_scale, z_scale);
  if (cgrid > 1)
    hipLaunchKernelGGL(moe_gate_scalars_kernel, dim3(1), dim3(GATE_BLOCK), 0,
                       stream, psum.data_ptr<float>(), cnt.data_ptr<int>(),
                       part_z.data_ptr<float>(), aux.data_ptr<float>(),
                       z.data_ptr<float>(), G, (int)E, aux_scale, z_scale);
  return {probs, idx, w, lse, psum, cnt, aux, z};
}

// g_probs [N, E] | none, g_aux [] fp32 | none, g_z [] fp32 | none (device
// scalars, read in the kernel), logits [N, E], lse [N] fp32, cnt [E] int32
// -> dlogits [N, E]
torch::Tensor moe_gate_grad(c10::optional<torch::Tensor> g_probs,
                            c10::optional<torch::Tensor> g_aux,
                            c10::optional<torch::Tensor> g_z,
                            torch::Tensor logits, torch::Tensor lse,
                            torch::Tensor cnt) {
  check_rows(logits, "logits");
  const int64_t N = logits.size(0), E = logits.size(1);
  TORCH_CHECK(N >= 1 && E >= 1, "moe_gate_grad: empty logits");
  TORCH_CHECK(E <= MOE_MAX_E, "moe_gate_grad: E (", E, ") > 2048");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
              lse.scalar_type() == at::kFloat && lse.dim() == 1 &&
              lse.size(0) == N, "moe_gate_grad: lse must be fp32 [N]");
  TORCH_CHECK(cnt.is_cuda() && cnt.is_contiguous() &&
              cnt.scalar_type() == at::kInt && cnt.dim() == 1 &&
              cnt.size(0) == E, "moe_gate_grad: cnt must be int32 [E]");
  const void* gp = nullptr;
  if (g_probs.has_value()) {
    check_rows(*g_probs, "g_probs");
    TORCH_CHECK(g_probs->sizes() == logits.sizes() &&
                g_probs->scalar_type() == logits.scalar_type(),
                "moe_gate_grad: g_probs must match logits");
    gp = g_probs->data_ptr();
  }
  auto scalar = [](const c10::optional<torch::Tensor>& t,
                   const char* what) -> const float* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                t->numel() == 1, "moe_gate_grad: ", what,
                " must be one fp32 value on the GPU");
    return t->data_ptr<float>();
  };
  const float* ga = scalar(g_aux, "g_aux");
  const float* gz = scalar(g_z, "g_z");
  auto dlogits = torch::empty_like(logits);
  const double n = (double)N;
  const float aux_scale = (float)((double)E / (n * n));
  const float z_scale = (float)(2.0 / n);
  auto stream = hetu_current_stream();
  MOE_DISPATCH(logits, "moe_gate_grad", [&] {
    const scalar_t* xp = (const scalar_t*)logits.data_ptr();
    scalar_t* dp = (scalar_t*)dlogits.data_ptr();
    const bool vec = gp ? can_vec<scalar_t>(E, {xp, dp, gp})
                        : can_vec<scalar_t>(E, {xp, dp});
    const int V = vec ? VecIO<scalar_t>::VEC : 1;
    const int gw = gate_group_width((E + V - 1) / V);
    const int groups = GATE_BLOCK / gw;
    const int grid = row_grid((N + groups - 1) / groups);
    if (vec) {
      hipLaunchKernelGGL((moe_gate_grad_kernel<scalar_t, true>), dim3(grid),
                         dim3(GATE_BLOCK), 0, stream, (const scalar_t*)gp,
                         ga, gz, xp, lse.data_ptr<float>(),
                         cnt.data_ptr<int>(), dp, N, (int)E, aux_scale,
                         z_scale, gw);
    } else {
      hipLaunchKernelGGL((moe_gate_grad_kernel<scalar_t, false>), dim3(grid),
                         dim3(GATE_BLOCK), 0, stream, (const scalar_t*)gp,
                         ga, gz, xp, lse.data_ptr<float>(),
                         cnt.data_ptr<int>(), dp, N, (int)E, aux_scale,
                         z_scale, gw);
    }
  });
  return dlogits;
}
