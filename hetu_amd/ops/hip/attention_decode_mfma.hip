// Split-KV decode attention for gfx950, MFMA variant for wide GQA groups
// and MQA: the contract of flash_attn_decode (attention_decode.hip), the
// same grid, split rule, workspace and merge kernel, another inner loop.
//
//   q [B, H, D], k_cache / v_cache [B, Hkv, L, D] (element strides), kv_len
//   int32 [B] on the device -> out [B, H, D] bf16, lse [B, H] fp32
//
// The G = H / Hkv query heads of a KV head are the 16-wide side of
// v_mfma_f32_16x16x32_bf16.  A head tile is 16 heads (spare rows: q = 0, not
// stored); MT = 1, 2 or 4 head tiles share every K and V fragment, so the
// key range of a (b, hkv, split) is read once for G <= 64.
//
// A block (4 waves) owns (batch row, KV head, split) and walks its keys in
// tiles of DM_BN = 128; wave w owns keys [32 w, 32 w + 32) of each tile and
// is its own online-softmax stream, with its own V ring: no barrier in the
// key loop.  Per wave and 32-key tile (lane = 16 g + i):
//   S^T = mfma(K, Q^T), twice 16 keys: the A operand of lane (g, i) is key
//     row i, dims 32 ks + 8 g .. + 8: one 16-byte global load, no LDS.  The
//     result holds head i in lane column i and keys 16 c + 4 g + r in
//     register r of score tile c, so max, exp, alpha and l are per-lane
//     values, joined over g by two shfl_xor (16, 32) per tile.
//   O^T += mfma(V^T, P^T), one 32-key step: contraction slot j of lane
//     group g is key 4 g + j (j < 4) or 16 + 4 g + j - 4: exactly the keys
//     whose p the lane holds, so the B operand is four v_cvt_pk_bf16_f32 and
//     no cross-lane move.  V is staged row-major with global_load_lds
//     (width 16) and read back transposed in that key order with two
//     ds_read_b64_tr_b16 per 16 dims (rows 4 g + .., then + 16).
// LDS image of a wave's tile: [32 keys][2 D bytes], the 32-byte slot of a
// row XORed with (row & 7) at D = 128 and ((row >> 1) & 3) at D = 64: the 8
// rows that a 32-lane half reads in one transposed read then fall on all 64
// banks once.  The XOR moves whole 32-byte slots, is folded into the DMA's
// source column, and is the same for rows r and r + 16 (second read = an
// immediate offset).
// Pipeline: V one tile ahead in a ring of 2 images per wave, K one tile
// ahead in registers (reloaded as soon as the score MFMAs have consumed
// it).  The loop head issues V(i + 1), then waits vmcnt(NV): K(i) and V(i)
// have landed, V(i + 1) flies under this tile's MFMAs; the last tile drains
// (fa_wait_tile).  No C++ access to LDS inside the loop (it would make the
// compiler wait vmcnt(0) for the DMA).
// Masking by selection: rows are clamped to the split's last valid key
// before they become addresses (K loads and each lane of the V DMA), so a
// staged image holds valid rows only (0 x NaN is NaN inside an MFMA); the
// score of a key past the end is selected to -inf and its p to 0; a wave
// whose 32 keys are all past the end skips the tile.
//
// PAGED (flash_attn_decode_paged_mfma): k / v are page pools [P, Hkv, PS, D]
// behind a block table (attention_decode.h).  A wave's 32 keys of a tile are
// aligned to 32 and PS >= 32, so they share one page: its id is a scalar that
// offsets the K row pointer and the per-lane source address of the V DMA;
// rows are clamped as above and then reduced mod PS.  The LDS image, swizzle,
// ring and waits are the dense kernel's.  Ids run two tiles ahead of the
// MFMAs: the trip of tile i issues V(i + 1) and reloads K(i + 1) with the id
// it already holds and requests the id of tile i + 2, so no K / V address
// waits for the table.  A page id outside [0, P) is 32 masked keys: the tile
// is neither loaded nor scored (the loop head then drains instead of counting
// a DMA that was not issued).  Same tiles, streams and merge order as the
// dense kernel: bit-identical results for the same values.
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include <type_traits>
#include "attention_decode.h"
#include "attention_decode_mfma.h"

namespace {

// two blocks per CU (2 waves / SIMD, 256 registers a lane) wherever that
// compiles without scratch: all but D = 128 with two or four head tiles
template <int D, int MT, bool PAGED = false>
__global__ __launch_bounds__(DM_THREADS, (D == 128 && MT >= 2) ? 1 : 2)
void fa_decode_mfma_kernel(std::conditional_t<PAGED, DecPagedArgs, DecArgs> a) {
  constexpr int RB = 2 * D;
  constexpr int IMG = DM_WKEYS * RB;           // 8 KiB (D = 128) / 4 KiB
  constexpr int NV = IMG / 1024;               // DMA instructions per tile
  constexpr int KS = D / 32;                   // k-steps of a score tile
  constexpr int NDB = D / 16;                  // 16-dim blocks of O^T
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
  const int kv = min(max(a.kv_len[b], 0), a.L);
  const int n_tiles = (kv + DEC_BN - 1) / DEC_BN;      // 64-key split units
  const int tps = (n_tiles + ns - 1) / ns;
  const int t0 = split * tps;
  const int t1 = min(n_tiles, t0 + tps);
  const int64_t row0 = (int64_t)b * a.H + (int64_t)hkv * G;   // (b, head 0)

  if (t0 >= t1) {                      // block-uniform: no loads, no barrier
    for (int g = threadIdx.x; g < G; g += DM_THREADS) {
      if (ns == 1) a.lse[row0 + g] = -INFINITY;
      else a.ws_lse[(row0 + g) * ns + split] = -INFINITY;
    }
    if (ns == 1) {                     // kv == 0: the row's output is zero
      ushort8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z.v[j] = 0;
      for (int i = threadIdx.x; i < G * (D / 8); i += DM_THREADS)
        *reinterpret_cast<ushort8*>(a.out + row0 * D + (int64_t)i * 8) = z;
    }
    return;
  }

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane & 15;            // head column / key row of a fragment
  const int lg = lane >> 4;            // lane group
  // dense: the batch row's cache; paged: the pool, kpage / vpage add the page
  const bf16* kb = a.k + (PAGED ? 0 : (int64_t)b * a.k_bs) +
                   (int64_t)hkv * a.k_hs;
  const bf16* vb = a.v + (PAGED ? 0 : (int64_t)b * a.v_bs) +
                   (int64_t)hkv * a.v_hs;
  const auto kpage = [&](int page) {
    if constexpr (PAGED) return kb + (int64_t)page * a.k_bs;
    else return kb;
  };
  const auto vpage = [&](int page) {
    if constexpr (PAGED) return vb + (int64_t)page * a.v_bs;
    else return vb;
  };
  int rmask = -1;                      // row within the page
  if constexpr (PAGED) rmask = (1 << a.ps_shift) - 1;
  const float scale = a.scale;
  // this split's keys; every address is clamped to klast < kv <= L
  const int kend = min(t1 * DEC_BN, kv), klast = kend - 1;
  const int kw0 = t0 * DEC_BN + wave * DM_WKEYS;
  const int nt = kw0 < kend ? (kend - kw0 + DM_BN - 1) / DM_BN : 0;
  char* ring = smem + wave * (DM_RING * IMG);
  float* s_o = reinterpret_cast<float*>(smem);         // [wave][16][DP]
  float* s_m = s_o + DM_WAVES * 16 * DP;               // [wave][16]
  float* s_l = s_m + DM_WAVES * 16;

  for (int c0 = 0; c0 < G; c0 += 16 * MT) {
    bf16x8 qf[MT][KS];                 // B fragments: head column hi
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int head = c0 + 16 * mt + hi;
      const bf16* qrow = a.q + (int64_t)b * a.q_bs +
                         (int64_t)(hkv * G + min(head, G - 1)) * a.q_hs +
                         8 * lg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        uint4 w = *reinterpret_cast<const uint4*>(qrow + 32 * ks);
        if (head >= G) w = make_uint4(0, 0, 0, 0);
        qf[mt][ks] = __builtin_bit_cast(bf16x8, w);
      }
    }
    float m[MT], l[MT];
    f32x4 acc[MT][NDB];                // O^T: head hi, dims 16 db + 4 lg + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      m[mt] = -INFINITY;
      l[mt] = 0.f;
#pragma unroll
      for (int db = 0; db < NDB; ++db) acc[mt][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    bf16x8 kf[2][KS];
    // paged: the page id of tile i + 1 and whether tile i has a page at all
    // (dense: no ids, every tile has)
    [[maybe_unused]] int page_nx = 0;
    bool ok = true;
    if constexpr (PAGED) {
      const int page = dec_page_of(a, b, min(kw0, klast));
      page_nx = dec_page_of(a, b, min(kw0 + DM_BN, klast));
      ok = (unsigned)page < (unsigned)a.P;
      if (nt > 0 && ok) {
        dm_load_k<D>(kf, kpage(page), a.k_rs, kw0, klast, rmask, lane);
        dm_stage_v<D>(vpage(page), a.v_rs, kw0, klast, rmask, ring, lane);
      }
    } else if (nt > 0) {
      dm_load_k<D>(kf, kb, a.k_rs, kw0, klast, rmask, lane);
      dm_stage_v<D>(vb, a.v_rs, kw0, klast, rmask, ring, lane);
    }
    for (int i = 0; i < nt; ++i) {     // wave-uniform trip count
      const int k0 = kw0 + i * DM_BN;
      const bool last = i + 1 == nt;
      const char* img = ring + (i & 1) * IMG;
      bool more = !last;               // tile i + 1 is loaded in this trip
      [[maybe_unused]] int page_nn = 0;
      if constexpr (PAGED) {
        // tile i + 2's id: first used one trip from here
        int key_nn = min(k0 + 2 * DM_BN, klast);
        dec_page_landed(page_nx, key_nn);
        page_nn = dec_page_of(a, b, key_nn);
        more = !last && (unsigned)page_nx < (unsigned)a.P;
      }
      if (more)
        dm_stage_v<D>(vpage(page_nx), a.v_rs, k0 + DM_BN, klast, rmask,
                      ring + ((i + 1) & 1) * IMG, lane);
      if constexpr (PAGED) {
        if (!ok) {                     // 32 masked keys: nothing was loaded
          if (more)
            dm_load_k<D>(kf, kpage(page_nx), a.k_rs, k0 + DM_BN, klast, rmask,
                         lane);
          page_nx = page_nn;
          ok = more;
          continue;
        }
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

      // lane (lg, hi) holds keys k0 + 16 c + 4 lg + r of head hi; the tile's
      // first key is valid, so every head's new maximum is finite
      const int nvalid = kend - (k0 + 4 * lg);   // key 16 c + r valid iff <
      bf16x8 pf[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        float sv[8];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool valid = 16 * (j >> 2) + (j & 3) < nvalid;
          sv[j] = valid ? s[mt][j >> 2][j & 3] * scale : -INFINITY;
          mx = fmaxf(mx, sv[j]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        const float mn = fmaxf(m[mt], mx);
        const float alpha = __expf(m[mt] - mn);
        m[mt] = mn;
        float p[8], psum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool valid = 16 * (j >> 2) + (j & 3) < nvalid;
          p[j] = valid ? __expf(sv[j] - mn) : 0.f;
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
      if constexpr (PAGED) {
        page_nx = page_nn;
        ok = more;
      }
    }

    // the wave's stream: l over the lane groups (m is already common)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      l[mt] += __shfl_xor(l[mt], 16, WAVE);
      l[mt] += __shfl_xor(l[mt], 32, WAVE);
    }
    // merge the waves in wave order, one head tile at a time, through the
    // bytes of the rings; thread = (head of the tile, DPT dims).  The split
    // is not empty, so wave 0 met a valid key: mx is finite (paged: unless
    // every page of the split is out of range; `none`).
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
      const int hh = threadIdx.x >> 4;
      const int d0 = (threadIdx.x & 15) * DPT;
      const int head = c0 + 16 * mt + hh;
      if (head < G) {
        float mx = s_m[hh];
#pragma unroll
        for (int w = 1; w < DM_WAVES; ++w) mx = fmaxf(mx, s_m[w * 16 + hh]);
        const bool none = PAGED && mx == -INFINITY;
        float lt = 0.f, o[DPT];
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] = 0.f;
#pragma unroll
        for (int w = 0; w < DM_WAVES; ++w) {
          const float ww = none ? 0.f : __expf(s_m[w * 16 + hh] - mx);
          lt += s_l[w * 16 + hh] * ww;
#pragma unroll
          for (int j = 0; j < DPT; ++j)
            o[j] += s_o[(w * 16 + hh) * DP + d0 + j] * ww;
        }
        const float inv = none ? 0.f : 1.f / lt;
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] *= inv;
        const int64_t row = row0 + head;
        const float ls = none ? -INFINITY : mx + logf(lt);
        if (ns == 1) {
          bf16* dst = a.out + row * D + d0;
#pragma unroll
          for (int j = 0; j < DPT; j += 4)
            fa_store4_bf16(dst + j, o[j], o[j + 1], o[j + 2], o[j + 3]);
          if (d0 == 0) a.lse[row] = ls;
        } else {
          float* dst = a.ws_o + (row * ns + split) * D + d0;
#pragma unroll
          for (int j = 0; j < DPT; j += 4) VecIO<float>::store(dst + j, o + j);
          if (d0 == 0) a.ws_lse[row * ns + split] = ls;
        }
      }
    }
    __syncthreads();                   // the next chunk stages into the rings
  }
}

}  // namespace

int64_t decode_attn_mfma_tile() { return DM_BN; }

std::vector<torch::Tensor> flash_attn_decode_mfma(torch::Tensor q,
                                                  torch::Tensor k_cache,
                                                  torch::Tensor v_cache,
                                                  torch::Tensor kv_len,
                                                  double scale,
                                                  int64_t num_splits) {
  DecCall c = dec_prepare(q, k_cache, v_cache, kv_len, scale, num_splits,
                          DM_BN);
  if (c.empty) return {c.out, c.lse};
  const DecArgs& a = c.a;
  const int64_t G = c.H / c.Hkv;
  const int mt = G <= 16 ? 1 : G <= 32 ? 2 : DM_MAX_MT;
  auto stream = hetu_current_stream();
  const dim3 grid(a.ns, (unsigned)c.Hkv, (unsigned)c.B);
#define DM_LAUNCH(DD, MM)                                                  \
  hipLaunchKernelGGL((fa_decode_mfma_kernel<DD, MM>), grid,                \
                     dim3(DM_THREADS), 0, stream, a)
#define DM_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (mt == 1) DM_LAUNCH(DD, 1);                                         \
    else if (mt == 2) DM_LAUNCH(DD, 2);                                    \
    else DM_LAUNCH(DD, DM_MAX_MT);                                         \
  } while (0)
  if (c.D == 128) DM_LAUNCH_D(128);
  else DM_LAUNCH_D(64);
#undef DM_LAUNCH_D
#undef DM_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (a.ns > 1) dec_merge_launch(c, stream);
  return {c.out, c.lse};
}

std::vector<torch::Tensor> flash_attn_decode_paged_mfma(
    torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
    torch::Tensor block_table, torch::Tensor kv_len, double scale,
    int64_t num_splits) {
  // the id prefetch forms keys up to two tiles past the last one
  DecCall c = dec_prepare(q, k_pool, v_pool, kv_len, scale, num_splits,
                          3 * DM_BN, &block_table);
  if (c.empty) return {c.out, c.lse};
  const DecPagedArgs a = c.paged();
  const int64_t G = c.H / c.Hkv;
  const int mt = G <= 16 ? 1 : G <= 32 ? 2 : DM_MAX_MT;
  auto stream = hetu_current_stream();
  const dim3 grid(a.ns, (unsigned)c.Hkv, (unsigned)c.B);
#define DM_LAUNCH(DD, MM)                                                  \
  hipLaunchKernelGGL((fa_decode_mfma_kernel<DD, MM, true>), grid,          \
                     dim3(DM_THREADS), 0, stream, a)
#define DM_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (mt == 1) DM_LAUNCH(DD, 1);                                         \
    else if (mt == 2) DM_LAUNCH(DD, 2);                                    \
    else DM_LAUNCH(DD, DM_MAX_MT);                                         \
  } while (0)
  if (c.D == 128) DM_LAUNCH_D(128);
  else DM_LAUNCH_D(64);
#undef DM_LAUNCH_D
#undef DM_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (a.ns > 1) dec_merge_launch(c, stream);
  return {c.out, c.lse};
}
