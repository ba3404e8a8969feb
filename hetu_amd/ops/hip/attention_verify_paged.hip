// Split-KV verification attention over a paged bf16 KV cache, for gfx950: a
// chunk of a few query tokens per sequence at the END of a long cached context
// (one verification step of speculative decoding, the last short round of a
// chunked prefill).  The contract is flash_attn_prefill_paged's
// (attention_prefill_paged.hip), the plan is the MFMA decode kernel's
// (attention_decode_mfma.hip).
//
//   q [T, H, D = 64 or 128] packed over sequences (element strides), k_pool /
//   v_pool [P, Hkv, PS, D] (with their strides), block_table int32 [B, MP],
//   cu_q int32 [B + 1] and kv_len int32 [B] on the device
//   -> out [T, H, D] bf16, lse [H, T] fp32
//
// n_b = cu_q[b + 1] - cu_q[b], kv_b = clamp(kv_len[b], 0, MP * PS); row i of
// sequence b stands at p = kv_b - n_b + i and attends keys 0 .. p.  Rows with
// p < 0 and rows at or past cu_q[B] come back 0 / -inf.
//
// A block (4 waves) owns (sequence, KV head, split) and reads the split's keys
// ONCE for all n_b tokens and all G = H / Hkv query heads of the KV head:
//  * M-rows are (token, head-in-group) pairs: row r is token r / G, head
//    hkv * G + r % G, R_b = n_b * G rows.  They sit on the 16-wide side of
//    v_mfma_f32_16x16x32_bf16, MT = 1, 2 or 4 row tiles of 16 sharing every K
//    and V fragment (spare rows: q = 0, not stored); more than 16 MT rows loop
//    over chunks and re-read the key range.  q stays in registers.
//  * Keys: splits own whole 64-key units of ceil(kv_b / 64), tiles are 128
//    keys, wave w owns keys [32 w, 32 w + 32) of each tile as its own
//    online-softmax stream with its own V ring; K comes straight from global
//    memory, V through global_load_lds into the swizzled image and back with
//    transposed reads (attention_decode_mfma.h).  No barrier in the key loop.
//  * Causal mask: in the S^T result a lane holds ONE M-row (lane & 15) and the
//    keys k0 + 16 c + 4 g + r, so the mask is one compare per element against
//    the lane's bound min(p(token of the row), last key of the split); spare
//    rows have bound -1.  That compare is the one the decode kernel spends on
//    the kv_b tail, so interior tiles cost what they cost there and there is
//    one stage, not two (a second, compare-free copy of the stage spilled at
//    MT = 4: profiles/r15_verify_paged.md).  The MT tokens of a lane travel as
//    one byte each in one register.
//  * A row may see no key in a wave's 32 keys, in a wave's stream or in a whole
//    split.  Its maximum stays -inf and is replaced by 0 before it enters
//    exp2, so l = 0, acc = 0 and the partial lse is -inf; the waves merge in
//    wave order and the splits in split order, empties skipped by selection.
//  * Pages as in the paged MFMA decode kernel: one scalar id per wave and
//    tile, two tiles ahead behind dec_page_landed; keys are clamped to the
//    split's last valid key before they become a table index or an address; an
//    id outside [0, P) means no K load, no DMA and no compute for the tile.
//  * Softmax in base 2 on fp32 scores (scale * log2(e) meets the scores in
//    fp32, q is not pre-scaled), the bare v_exp_f32.
//
// Grid (ns, Hkv, B + 1): shapes, max_q (through MT) and the CU count only.  A
// split with no keys writes lse = -inf to the workspace and returns before any
// load or barrier.  ns == 1 writes out / lse directly and the blocks of the
// pseudo-sequence b == B blank the rows past cu_q[B]; ns > 1 goes through the
// workspace [T, H, ns, D + 1] and fa_verify_merge_kernel, which decides those
// rows from cu_q.  No atomics, no host sync, bit-reproducible.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include "attention_decode.h"
#include "attention_decode_mfma.h"

// A row's result must not depend on MT (the same call with another max_q is
// bit-identical): no instantiation may fuse a multiply and an add that another
// one keeps apart.
#pragma clang fp contract(off)

namespace {

constexpr float VF_LN2 = 0.6931471805599453f;

// DecPagedArgs with q_bs the token stride of q, out [T, H, D], lse [H, T] and
// the workspace rows (t * H + h)
struct VfArgs : DecPagedArgs {
  const int* cu_q;    // [B + 1]
  int B, T;
  float scale_log2;   // scale * log2(e)
};

DEV void vf_zero_row(bf16* dst) {      // 16 B of a [.., D] bf16 row
  ushort8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z.v[j] = 0;
  *reinterpret_cast<ushort8*>(dst) = z;
}

// D = 128: one block per CU with two or four row tiles (512 registers a lane),
// two with one: what compiles without scratch (profiles/r15_verify_paged.md).
// D = 64 halves q, the K fragments and the accumulators and fits two blocks
// per CU at every MT (profiles/r16_paged_d64.md).
template <int MT, int D>
__global__ __launch_bounds__(DM_THREADS, (D == 128 && MT >= 2) ? 1 : 2)
void fa_verify_paged_kernel(VfArgs a) {
  constexpr int RB = 2 * D;
  constexpr int IMG = DM_WKEYS * RB;           // 8 KiB (D = 128) / 4 KiB
  constexpr int NV = IMG / 1024;               // DMA instructions per tile
  constexpr int KS = D / 32;
  constexpr int NDB = D / 16;
  constexpr int DP = D + 4;                    // merge row, floats
  constexpr int DPT = D / 16;                  // merge: dims per thread
  constexpr int RING_BYTES = DM_WAVES * DM_RING * IMG;
  constexpr int MERGE_BYTES = DM_WAVES * 16 * (DP + 2) * 4;
  // the rings; after the key loop the same bytes hold the waves' streams
  __shared__ __attribute__((aligned(1024))) char
      smem[RING_BYTES > MERGE_BYTES ? RING_BYTES : MERGE_BYTES];

  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int G = a.H / a.Hkv;
  const int ns = a.ns;
  const int tid = threadIdx.x;

  if (b == a.B) {
    // ns == 1 only: rows past cu_q[B], the G heads of this KV head
    if (ns > 1) return;
    const int t_end = min(max(a.cu_q[a.B], 0), a.T);
    const long long total = (long long)(a.T - t_end) * G * (D / 8);
    for (long long i = tid; i < total; i += DM_THREADS) {
      const int t = t_end + (int)(i / (G * (D / 8)));
      const int rest = (int)(i % (G * (D / 8)));
      const int h = hkv * G + rest / (D / 8), ch = rest % (D / 8);
      vf_zero_row(a.out + ((int64_t)t * a.H + h) * D + ch * 8);
      if (ch == 0) a.lse[(int64_t)h * a.T + t] = -INFINITY;
    }
    return;
  }

  // the chunk, clamped into the packed rows whatever cu_q holds
  const int row0 = min(max(a.cu_q[b], 0), a.T);
  const int n_b = min(max(a.cu_q[b + 1], row0), a.T) - row0;
  if (n_b == 0) return;                // block-uniform: no rows to write
  const int R = n_b * G;               // M-rows of this (sequence, KV head)
  const int kv = min(max(a.kv_len[b], 0), a.L);
  const int diag = kv - n_b;           // position of the chunk's token 0
  const int n_tiles = (kv + DEC_BN - 1) / DEC_BN;      // 64-key split units
  const int tps = (n_tiles + ns - 1) / ns;
  const int t0 = split * tps;
  const int t1 = min(n_tiles, t0 + tps);
  // M-row r -> (token, head): the rows of out / the workspace and of lse
  const auto out_row = [&](int r) {
    return (int64_t)(row0 + r / G) * a.H + hkv * G + r % G;
  };
  const auto lse_row = [&](int r) {
    return (int64_t)(hkv * G + r % G) * a.T + row0 + r / G;
  };

  if (t0 >= t1) {                      // block-uniform: no loads, no barrier
    for (int r = tid; r < R; r += DM_THREADS) {
      if (ns == 1) a.lse[lse_row(r)] = -INFINITY;
      else a.ws_lse[out_row(r) * ns + split] = -INFINITY;
    }
    if (ns == 1)                       // kv == 0: the rows' output is zero
      for (int64_t i = tid; i < (int64_t)R * (D / 8); i += DM_THREADS)
        vf_zero_row(a.out + out_row((int)(i / (D / 8))) * D +
                    (i % (D / 8)) * 8);
    return;
  }

  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane & 15;            // M-row column / key row of a fragment
  const int lg = lane >> 4;            // lane group
  const bf16* kb = a.k + (int64_t)hkv * a.k_hs;
  const bf16* vb = a.v + (int64_t)hkv * a.v_hs;
  const auto kpage = [&](int page) { return kb + (int64_t)page * a.k_bs; };
  const auto vpage = [&](int page) { return vb + (int64_t)page * a.v_bs; };
  const int rmask = (1 << a.ps_shift) - 1;     // row within the page
  const float sl2 = a.scale_log2;
  // this split's keys; every address is clamped to klast < kv <= L
  const int kend = min(t1 * DEC_BN, kv), klast = kend - 1;
  const int kw0 = t0 * DEC_BN + wave * DM_WKEYS;
  const int nt = kw0 < kend ? (kend - kw0 + DM_BN - 1) / DM_BN : 0;
  char* ring = smem + wave * (DM_RING * IMG);
  float* s_o = reinterpret_cast<float*>(smem);         // [wave][16][DP]
  float* s_m = s_o + DM_WAVES * 16 * DP;               // [wave][16]
  float* s_l = s_m + DM_WAVES * 16;

  for (int c0 = 0; c0 < R; c0 += 16 * MT) {
    bf16x8 qf[MT][KS];                 // B fragments: M-row column hi
    // the token of each of the lane's MT rows, relative to the chunk's first
    // token (one byte each, they span < 64 tokens); 255: a spare row
    const int tok0 = c0 / G;
    unsigned toks = 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int r = c0 + 16 * mt + hi;
      const int rc = min(r, R - 1);
      const int tok = rc / G;
      toks |= (r < R ? (unsigned)(tok - tok0) : 255u) << (8 * mt);
      const bf16* qrow = a.q + (int64_t)(row0 + tok) * a.q_bs +
                         (int64_t)(hkv * G + rc - tok * G) * a.q_hs + 8 * lg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        uint4 w = *reinterpret_cast<const uint4*>(qrow + 32 * ks);
        if (r >= R) w = make_uint4(0, 0, 0, 0);
        qf[mt][ks] = __builtin_bit_cast(bf16x8, w);
      }
    }
    float m[MT], l[MT];                // base-2 running max and sum
    f32x4 acc[MT][NDB];                // O^T: row hi, dims 16 db + 4 lg + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      m[mt] = -INFINITY;
      l[mt] = 0.f;
#pragma unroll
      for (int db = 0; db < NDB; ++db) acc[mt][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    bf16x8 kf[2][KS];
    // the page id of tile i + 1 and whether tile i has a page at all
    int page_nx = 0;
    bool ok = true;
    {
      const int page = dec_page_of(a, b, min(kw0, klast));
      page_nx = dec_page_of(a, b, min(kw0 + DM_BN, klast));
      ok = (unsigned)page < (unsigned)a.P;
      if (nt > 0 && ok) {
        dm_load_k<D>(kf, kpage(page), a.k_rs, kw0, klast, rmask, lane);
        dm_stage_v<D>(vpage(page), a.v_rs, kw0, klast, rmask, ring, lane);
      }
    }
    for (int i = 0; i < nt; ++i) {     // wave-uniform trip count
      const int k0 = kw0 + i * DM_BN;
      const bool last = i + 1 == nt;
      const char* img = ring + (i & 1) * IMG;
      // tile i + 2's id: first used one trip from here
      int key_nn = min(k0 + 2 * DM_BN, klast);
      dec_page_landed(page_nx, key_nn);
      const int page_nn = dec_page_of(a, b, key_nn);
      // tile i + 1 is loaded in this trip
      const bool more = !last && (unsigned)page_nx < (unsigned)a.P;
      if (more)
        dm_stage_v<D>(vpage(page_nx), a.v_rs, k0 + DM_BN, klast, rmask,
                      ring + ((i + 1) & 1) * IMG, lane);
      if (!ok) {                       // 32 masked keys: nothing was loaded
        if (more)
          dm_load_k<D>(kf, kpage(page_nx), a.k_rs, k0 + DM_BN, klast, rmask,
                       lane);
        page_nx = page_nn;
        ok = more;
        continue;
      }
      fa_wait_tile<NV>(!more);         // K(i) and V(i) are in
      __builtin_amdgcn_sched_barrier(0);   // no MFMA above the DMA issue

      f32x4 s[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          s[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            s[mt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kf[c][ks], qf[mt][ks], s[mt][c], 0, 0, 0);
        }
      if (more)
        dm_load_k<D>(kf, kpage(page_nx), a.k_rs, k0 + DM_BN, klast, rmask,
                     lane);

      // lane (lg, hi) holds keys k0 + 16 c + 4 lg + r of M-row hi: key
      // 16 c + r of the lane is visible iff <= rel.  A row without a visible
      // key so far keeps m = -inf and takes 0 into exp2.
      const int kl = k0 + 4 * lg;
      bf16x8 pf[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int t = (toks >> (8 * mt)) & 255;
        const int rel = (t == 255 ? -1 : min(diag + tok0 + t, klast)) - kl;
        float sv[8];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sv[j] = 16 * (j >> 2) + (j & 3) <= rel
                      ? s[mt][j >> 2][j & 3] * sl2 : -INFINITY;
          mx = fmaxf(mx, sv[j]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        const float mn = fmaxf(m[mt], mx);
        const float mu = mn == -INFINITY ? 0.f : mn;
        const float alpha = __builtin_amdgcn_exp2f(m[mt] - mu);
        m[mt] = mn;
        float p[8], psum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          p[j] = __builtin_amdgcn_exp2f(sv[j] - mu);     // exp2(-inf) = 0
          psum += p[j];                // l sums the fp32 p, before rounding
        }
        l[mt] = l[mt] * alpha + psum;
        union { unsigned u[4]; bf16x8 v; } pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) pk.u[j] = fa_cvt_pk(p[2 * j], p[2 * j + 1]);
        pf[mt] = pk.v;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][db][r] *= alpha;
      }

#pragma unroll
      for (int q4 = 0; q4 < NDB / 4; ++q4) {
        bf16x8 vt[4];
        dm_tr_v4<D>(vt, img, 4 * q4, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][4 * q4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                vt[j], pf[mt], acc[mt][4 * q4 + j], 0, 0, 0);
      }
      page_nx = page_nn;
      ok = more;
    }

    // the wave's stream: l over the lane groups (m is already common)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      l[mt] += __shfl_xor(l[mt], 16, WAVE);
      l[mt] += __shfl_xor(l[mt], 32, WAVE);
    }
    // merge the waves in wave order, one row tile at a time, through the
    // bytes of the rings; thread = (row of the tile, DPT dims).  A stream
    // with m = -inf is empty (l = 0, acc = 0) and is skipped by selection.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      __syncthreads();                 // rings / the previous tile are done
#pragma unroll
      for (int db = 0; db < NDB; ++db)
        *reinterpret_cast<f32x4*>(s_o + (wave * 16 + hi) * DP + 16 * db +
                                  4 * lg) = acc[mt][db];
      if (lg == 0) {
        s_m[wave * 16 + hi] = m[mt];
        s_l[wave * 16 + hi] = l[mt];
      }
      __syncthreads();
      const int hh = tid >> 4;
      const int d0 = (tid & 15) * DPT;
      const int r = c0 + 16 * mt + hh;
      if (r < R) {
        float mx = s_m[hh];
#pragma unroll
        for (int w = 1; w < DM_WAVES; ++w) mx = fmaxf(mx, s_m[w * 16 + hh]);
        const bool none = mx == -INFINITY;
        float lt = 0.f, o[DPT];
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] = 0.f;
#pragma unroll
        for (int w = 0; w < DM_WAVES; ++w) {
          const float mw = s_m[w * 16 + hh];
          const float ww = mw == -INFINITY ? 0.f
                                           : __builtin_amdgcn_exp2f(mw - mx);
          lt += s_l[w * 16 + hh] * ww;
#pragma unroll
          for (int j = 0; j < DPT; ++j)
            o[j] += s_o[(w * 16 + hh) * DP + d0 + j] * ww;
        }
        const float inv = none ? 0.f : 1.f / lt;
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] *= inv;
        const float ls = none ? -INFINITY : (mx + __log2f(lt)) * VF_LN2;
        const int64_t row = out_row(r);
        if (ns == 1) {
          bf16* dst = a.out + row * D + d0;
#pragma unroll
          for (int j = 0; j < DPT; j += 4)
            fa_store4_bf16(dst + j, o[j], o[j + 1], o[j + 2], o[j + 3]);
          if (d0 == 0) a.lse[lse_row(r)] = ls;
        } else {
          float* dst = a.ws_o + (row * ns + split) * D + d0;
#pragma unroll
          for (int j = 0; j < DPT; j += 4) VecIO<float>::store(dst + j, o + j);
          if (d0 == 0) a.ws_lse[row * ns + split] = ls;
        }
      }
    }
    // the next chunk stages into the rings and counts its loads: the stores
    // above must not be among them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// out[t, h] = sum_s exp(lse_s - lse) * o_s over the non-empty splits, in split
// order, lse [H, T]; rows at or past cu_q[B] are 0 / -inf without a read of
// the workspace (no block wrote it).  One block per (t, h), one thread per dim.
template <int D>
__global__ void fa_verify_merge_kernel(const float* __restrict__ ws_o,
                                       const float* __restrict__ ws_lse,
                                       bf16* __restrict__ out,
                                       float* __restrict__ lse,
                                       const int* __restrict__ cu_q, int B,
                                       int T, int H, int ns) {
  const int64_t row = blockIdx.x;
  const int t = (int)(row / H), h = (int)(row % H);
  const int d = threadIdx.x;
  const float* pl = ws_lse + row * ns;
  float mx = -INFINITY;
  if (t < min(max(cu_q[B], 0), T))
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
  if (d == 0)
    lse[(int64_t)h * T + t] = mx == -INFINITY ? -INFINITY : mx + logf(sum);
}

void vf_check_strided(const torch::Tensor& t, const char* what) {
  const char* fn = "flash_attn_verify_paged: ";
  TORCH_CHECK(t.is_cuda(), fn, what, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, what, " must be bf16");
  TORCH_CHECK(t.stride(-1) == 1, fn, what, " needs a contiguous last dim");
  for (int i = 0; i + 1 < t.dim(); ++i)
    TORCH_CHECK(t.size(i) <= 1 || t.stride(i) % 8 == 0, fn, what, " stride ",
                i, " is not a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, what,
              " is not 16-byte aligned");
}

void vf_check_index(const torch::Tensor& t, const torch::Tensor& q,
                    const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device() &&
              t.scalar_type() == at::kInt && t.is_contiguous(),
              "flash_attn_verify_paged: ", what,
              " must be a contiguous int32 tensor on q's device");
}

}  // namespace

std::vector<torch::Tensor> flash_attn_verify_paged(
    torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
    torch::Tensor block_table, torch::Tensor cu_q, torch::Tensor kv_len,
    double scale, int64_t max_q, int64_t num_splits) {
  const char* fn = "flash_attn_verify_paged: ";
  TORCH_CHECK(q.dim() == 3 && k_pool.dim() == 4 && v_pool.dim() == 4 &&
              k_pool.sizes() == v_pool.sizes(), fn,
              "need q [T, H, D] and k_pool, v_pool [P, Hkv, PS, D]");
  const int64_t T = q.size(0), H = q.size(1), D = q.size(2);
  const int64_t P = k_pool.size(0), Hkv = k_pool.size(1);
  const int64_t PS = k_pool.size(2);
  TORCH_CHECK((D == 64 || D == 128) && k_pool.size(3) == D, fn,
              "D must be 64 or 128, got ", D, " and ", k_pool.size(3));
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, fn, "H (", H,
              ") is not a multiple of Hkv (", Hkv, ")");
  TORCH_CHECK(PS == 32 || PS == 64 || PS == 128 || PS == 256, fn,
              "the page size of k_pool / v_pool (dim 2) must be 32, 64, 128 "
              "or 256, got ", PS);
  vf_check_strided(q, "q");
  vf_check_strided(k_pool, "k_pool");
  vf_check_strided(v_pool, "v_pool");
  TORCH_CHECK(k_pool.device() == q.device() && v_pool.device() == q.device(),
              fn, "all tensors must share one device");
  vf_check_index(block_table, q, "block_table");
  vf_check_index(cu_q, q, "cu_q");
  vf_check_index(kv_len, q, "kv_len");
  TORCH_CHECK(block_table.dim() == 2 && cu_q.dim() == 1 && cu_q.size(0) >= 1,
              fn, "need block_table [B, MP] and cu_q [B + 1]");
  const int64_t B = block_table.size(0), MP = block_table.size(1);
  TORCH_CHECK(cu_q.size(0) == B + 1 && kv_len.dim() == 1 &&
              kv_len.size(0) == B, fn, "need cu_q [B + 1] and kv_len [B] "
              "with B = ", B, " rows of block_table");
  const int64_t lim = (int64_t)1 << 31;
  // the id prefetch forms keys up to two tiles past the last one
  TORCH_CHECK(T * H < lim && P < lim && MP * PS < lim - 3 * DM_BN, fn,
              "T * H, P or MP * PS too large for int");
  TORCH_CHECK(B < 65535 && Hkv <= 65535, fn, "B or Hkv too large");
  TORCH_CHECK(num_splits >= 0 && num_splits <= DEC_MAX_SPLITS, fn,
              "num_splits must be in [0, ", DEC_MAX_SPLITS, "], got ",
              num_splits);

  auto out = torch::empty({T, H, D}, q.options());
  auto lse = torch::empty({H, T}, q.options().dtype(at::kFloat));
  if (T == 0 || H == 0) return {out, lse};

  const int64_t G = H / Hkv;
  max_q = std::min(std::max<int64_t>(max_q, 1), T);
  const int mt = max_q * G <= 16 ? 1 : max_q * G <= 32 ? 2 : DM_MAX_MT;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int ns = (int)(num_splits > 0
                           ? num_splits
                           : decode_attn_num_splits(B, Hkv, MP * PS, cus));

  VfArgs a;
  a.q = (const bf16*)q.data_ptr();
  a.k = (const bf16*)k_pool.data_ptr();
  a.v = (const bf16*)v_pool.data_ptr();
  a.kv_len = kv_len.data_ptr<int>();
  a.out = (bf16*)out.data_ptr();
  a.lse = lse.data_ptr<float>();
  a.ws_o = nullptr;
  a.ws_lse = nullptr;
  torch::Tensor ws;
  if (ns > 1) {                        // caching allocator, stream-ordered
    ws = torch::empty({T * H * ns * (D + 1)}, lse.options());
    a.ws_o = ws.data_ptr<float>();
    a.ws_lse = a.ws_o + T * H * ns * D;
  }
  a.q_bs = q.stride(0); a.q_hs = q.stride(1);
  a.k_bs = k_pool.stride(0); a.k_hs = k_pool.stride(1);
  a.k_rs = k_pool.stride(2);
  a.v_bs = v_pool.stride(0); a.v_hs = v_pool.stride(1);
  a.v_rs = v_pool.stride(2);
  a.H = (int)H; a.Hkv = (int)Hkv; a.L = (int)(MP * PS); a.ns = ns;
  a.scale = (float)scale;
  a.table = block_table.data_ptr<int>();
  a.MP = (int)MP; a.P = (int)P;
  a.ps_shift = __builtin_ctzll((unsigned long long)PS);
  a.cu_q = cu_q.data_ptr<int>();
  a.B = (int)B; a.T = (int)T;
  a.scale_log2 = (float)(scale * 1.4426950408889634);

  auto stream = hetu_current_stream();
  const dim3 grid((unsigned)ns, (unsigned)Hkv, (unsigned)(B + 1));
#define VF_LAUNCH(MM, DD)                                                  \
  hipLaunchKernelGGL((fa_verify_paged_kernel<MM, DD>), grid,               \
                     dim3(DM_THREADS), 0, stream, a)
#define VF_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (mt == 1) VF_LAUNCH(1, DD);                                         \
    else if (mt == 2) VF_LAUNCH(2, DD);                                    \
    else VF_LAUNCH(DM_MAX_MT, DD);                                         \
    HIP_CHECK(hipGetLastError());                                          \
    if (ns > 1) {                                                          \
      hipLaunchKernelGGL(fa_verify_merge_kernel<DD>,                       \
                         dim3((unsigned)(T * H)), dim3(DD), 0, stream,     \
                         a.ws_o, a.ws_lse, a.out, a.lse, a.cu_q, a.B, a.T, \
                         a.H, ns);                                         \
      HIP_CHECK(hipGetLastError());                                        \
    }                                                                      \
  } while (0)
  if (D == 128) VF_LAUNCH_D(128);
  else VF_LAUNCH_D(64);
#undef VF_LAUNCH_D
#undef VF_LAUNCH
  return {out, lse};
}
