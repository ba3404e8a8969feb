// The split-KV VALU decode kernel, shared by attention_decode.hip (dense
// cache; the header comment there describes the design) and
// attention_decode_paged.hip (PAGED: the same key loop over a page pool).
//
// PAGED changes addresses only.  A wave's 16 keys of a tile lie in one page
// (PS >= 32), so the page id is a wave-uniform scalar: one block-table entry
// per wave and tile, read through a uniform address and readfirstlane, and
// requested one tile ahead: tile t + 1's entry is in flight while tile t's K
// and V rows are loaded and consumed, so no K / V address waits for the
// table.  The key whose entry is read is clamped to kv - 1 first: entries
// past the last needed page are never read.  A page id outside [0, P) masks
// the wave's 16 keys, which is the same as skipping them.  Tiles, streams and
// merges are the dense kernel's, operation for operation: for the same values
// the result is bit-identical.
#pragma once
#include <type_traits>
#include "attention_common.h"
#include "attention_decode.h"

namespace {

// DEC_BN (attention_decode.h) is the block's key tile here
constexpr int DEC_WAVES = 4;           // 16 keys of the tile each
constexpr int DEC_THREADS = DEC_WAVES * WAVE;
constexpr int DEC_WKEYS = DEC_BN / DEC_WAVES;
constexpr int DEC_MAX_GC = 8;          // query heads per pass

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

template <int D, int GC, bool PAGED = false>
__global__ __launch_bounds__(DEC_THREADS)
void fa_decode_kernel(std::conditional_t<PAGED, DecPagedArgs, DecArgs> a) {
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
  // dense: the batch row's cache; paged: the pool, the page comes per tile
  const bf16* kb = a.k + (PAGED ? 0 : (int64_t)b * a.k_bs) +
                   (int64_t)hkv * a.k_hs + ds;
  const bf16* vb = a.v + (PAGED ? 0 : (int64_t)b * a.v_bs) +
                   (int64_t)hkv * a.v_hs + ds;
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

    // paged: the wave's first key as a scalar, and the page id of the tile
    // about to be walked (kv >= 1 here)
    [[maybe_unused]] int wk0 = 0, page_next = 0;
    if constexpr (PAGED) {
      wk0 = __builtin_amdgcn_readfirstlane(wave) * DEC_WKEYS;
      page_next = dec_page_of(a, b, min(t0 * DEC_BN + wk0, kv - 1));
    }

    for (int t = t0; t < t1; ++t) {
      const int kbase = t * DEC_BN + wave * DEC_WKEYS;
      const bf16* kp = kb;
      const bf16* vp = vb;
      if constexpr (PAGED) {
        int page = page_next;
        // the next tile's entry, requested before this tile's rows are
        // loaded; past the last tile it re-reads the last needed entry
        int key_next = min((t + 1) * DEC_BN + wk0, kv - 1);
        dec_page_landed(page, key_next);
        page_next = dec_page_of(a, b, key_next);
        if (t * DEC_BN + wk0 >= kv) continue;
        if ((unsigned)page >= (unsigned)a.P) continue;   // 16 masked keys
        kp += (int64_t)page * a.k_bs;
        vp += (int64_t)page * a.v_bs;
      } else {
        if (kbase >= kv) continue;     // wave-uniform: all 16 keys masked
      }
      uint4 kf[NI], vf[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        int row = min(kbase + i * KPI + rg, kv - 1);
        // the clamped key stays within the wave's 16, so within the page
        if constexpr (PAGED) row &= (1 << a.ps_shift) - 1;
        kf[i] = *reinterpret_cast<const uint4*>(kp + (int64_t)row * a.k_rs);
        vf[i] = *reinterpret_cast<const uint4*>(vp + (int64_t)row * a.v_rs);
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
    // split is not empty, so at least one wave met a valid key: mx is finite
    // (paged: unless every page of the split is out of range; `none`).
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
        float ls = mx + logf(lt);
        // `none`: replace the NaN of exp(-inf + inf) after the fact, so that
        // the sums above stay the dense kernel's, operation for operation
        if constexpr (PAGED) {
          if (mx == -INFINITY) {
            ls = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = 0.f;
          }
        }
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

}  // namespace
