// Split-KV decode attention for gfx950 over an fp8 (OCP e4m3) KV cache with
// one fp32 scale per cached row: value = float(code) * scale[row].  The
// contract, grid, split rule, workspace and merge kernel of
// flash_attn_decode (attention_decode.hip); the plan of the MFMA variant
// (attention_decode_mfma.hip: heads are the 16-wide side of
// v_mfma_f32_16x16x32_bf16, MT = 1 or 2 head tiles share every K and V
// fragment, a wave owns 32 keys of each 128-key tile and is its own
// online-softmax stream), for every G = H / Hkv.
//
//   q [B, H, D] bf16, k_cache / v_cache [B, Hkv, L, D] e4m3 (byte strides),
//   k_scale / v_scale [B, Hkv, L] fp32, kv_len int32 [B] on the device
//   -> out [B, H, D] bf16, lse [B, H] fp32 over the dequantized values
//
// e4m3 converts to bf16 exactly (v_cvt_scalef32_pk_bf16_fp8 with scale 1,
// one instruction per two elements), so the MFMAs run in bf16 on the codes
// and the row scales enter in fp32, two multiplies per key and head:
//   K side: a lane's load is 16 bytes = 16 dims of one key row, and feeds
//     two k-steps (bytes 0-7, 8-15).  The contraction order of an MFMA is
//     free as long as both operands agree: slot j of lane group g in k-step
//     ks = 2 kl + h is dim 64 kl + 16 g + 8 h + j, and the q fragments are
//     loaded once in that order.  In the S^T C layout lane (g, i) holds
//     keys 16 c + 4 g + r of head i, so k_scale is one 16-byte load of four
//     floats per 16-key tile: score = acc * k_scale[key] * scale.
//   V side: p * v_scale[key] in fp32, then P is split into three bf16 parts
//     (a rounding, and twice the rounding of what is left) and each V^T
//     fragment meets all of them, three MFMAs: P.V is then an fp32 product.
//     With a single rounding of P the kernel and the fp32 torch branch
//     differ enough for a generator to quantize different rows on the two
//     sides (profiles/r10_decode_fp8.md, section 5).  l sums the unscaled
//     fp32 p.  The raw bytes are staged with
//     global_load_lds (images half the bf16 kernel's) and read back
//     transposed with ds_read_b64_tr_b8, then converted.  Measured
//     (scripts/probe_tr8.hip): lane 16 g + i receives, as byte j, byte
//     (i & 7) of the 8 bytes that lane 16 g + 2 j + (i >> 3) addresses:
//     lanes 2 j, 2 j + 1 of a group supply the halves of a 16-byte row j and
//     lane i gets column i of the 8 rows.  With lane a addressing key row
//     4 g + (j & 3) + 16 (j >> 2), j = (a >> 1) & 7, at dim 16 db + 8 (a & 1),
//     ONE read is the whole V^T fragment of dim block db in the key order of
//     the P fragment.
// LDS image of a wave's tile: [32 keys][D bytes]; the 16-byte slot of a row
// is XORed with ((row >> 1) & 3) | ((row >> 4) & 1) << 2 at D = 128 and
// ((row >> 2) & 1) | ((row >> 4) & 1) << 1 at D = 64, folded into the DMA's
// source column: the 16 rows that a 32-lane half reads then fall on 16
// different 16-byte columns of the 64 banks.
// Pipeline and masking as in the MFMA variant: V one tile ahead in a ring of
// two images per wave, K and the scales one tile ahead in registers, no C++
// access to LDS in the loop.  Row indices are clamped to the split's last
// valid key before they become addresses, for the scale loads too (a clamped
// row is valid, so its scale must be: 0 * NaN is NaN); a score past the end
// is selected to -inf and its p to 0.
//
// PAGED (flash_attn_decode_paged_fp8): k / v are code pools [P, Hkv, PS, D]
// and the scales pools [P, Hkv, PS] behind a block table (attention_decode.h).
// A wave's 32 keys of a tile are aligned to 32 and PS >= 32, so its two K
// loads, its four 16-byte scale loads and its V image come from one page: one
// scalar id per wave and tile offsets all four pools; rows are clamped as
// above (a clamped key stays in the wave's own 32 keys, so in the page the id
// was read for) and then reduced mod PS.  Ids run two tiles ahead as in the
// paged MFMA kernel: the trip of tile i stages V(i + 1) and reloads K(i + 1)
// and its scales with the id it already holds, and requests the id of tile
// i + 2.  A page id outside [0, P) is 32 masked keys: nothing is loaded for
// the tile and its compute is skipped, wave-uniformly (a stale image or stale
// registers may hold NaN, and 0 x NaN is NaN in an MFMA); the loop head then
// drains instead of counting a DMA that was not issued.  Same tiles, streams
// and merge order as the dense kernel: bit-identical results for the same
// values.
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include <type_traits>
#include "attention_decode.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef unsigned char u8;

constexpr int D8_WAVES = 4;
constexpr int D8_THREADS = D8_WAVES * WAVE;
constexpr int D8_WKEYS = 32;                   // keys per wave and tile
constexpr int D8_BN = D8_WAVES * D8_WKEYS;     // keys per block tile
constexpr int D8_RING = 2;                     // V images per wave
constexpr int D8_PP = 3;                       // bf16 parts of P: 24 bits
// 32 heads per pass: four head tiles (the bf16 MFMA kernel's ceiling) spill
// here at both D, the scales and the unconverted K take their registers; a
// KV head with more query heads re-reads its key range once per 32
constexpr int D8_MAX_MT = 2;
static_assert(D8_BN % DEC_BN == 0, "tiles are whole split units");

// A = DecPagedArgs: a.k / a.v are the code pools, ks / vs the scale pools
// [P, Hkv, PS] and every *_bs a page stride
template <class A>
struct Dec8ArgsT {
  A a;                        // a.k, a.v: the code bytes, strides in bytes
  const float* ks;            // [B, Hkv, L], last dim contiguous
  const float* vs;
  long long ks_bs, ks_hs, vs_bs, vs_hs;
  int ks_vec, vs_vec;         // every (b, hkv) row of scales is 16-B aligned
};
using Dec8Args = Dec8ArgsT<DecArgs>;
using Dec8PagedArgs = Dec8ArgsT<DecPagedArgs>;

template <int D>
DEV int d8_swz(int row) {
  return D == 128 ? (((row >> 1) & 3) | (((row >> 4) & 1) << 2))
                  : (((row >> 2) & 1) | (((row >> 4) & 1) << 1));
}

// 8 e4m3 bytes -> 8 bf16, exact
DEV bf16x8 d8_cvt8(unsigned lo, unsigned hi) {
  typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
  union { v2bf p[4]; bf16x8 v; } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return u.v;
}

// stage keys k0 .. k0 + 31 (clamped to klast) of V into a wave's image; a
// row index is taken & rmask (-1: dense; PS - 1: the row within vb's page)
template <int D>
DEV void d8_stage_v(const u8* vb, long long v_rs, int k0, int klast,
                    int rmask, char* img, int lane) {
#pragma unroll
  for (int i = 0; i < D8_WKEYS * D / 1024; ++i) {
    const int pos = (i * WAVE + lane) * 16;
    const int row = pos / D;
    const int col = (pos % D) ^ (d8_swz<D>(row) << 4);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(
            vb + (int64_t)(min(k0 + row, klast) & rmask) * v_rs + col),
        (__attribute__((address_space(3))) void*)(img + pos), 16, 0, 0);
  }
}

// the wave's 32 K rows, raw: kr[c][kl] = row 16 c + i, bytes
// 64 kl + 16 g .. + 16
template <int D>
DEV void d8_load_k(uint4 (&kr)[2][D / 64], const u8* kb, long long k_rs,
                   int k0, int klast, int rmask, int lane) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const u8* row = kb + (int64_t)(min(k0 + 16 * c + (lane & 15), klast) &
                                   rmask) * k_rs + 16 * (lane >> 4);
#pragma unroll
    for (int kl = 0; kl < D / 64; ++kl)
      kr[c][kl] = *reinterpret_cast<const uint4*>(row + 64 * kl);
  }
}

// the scales of keys kb .. kb + 3 (kb a multiple of 4), each index clamped
// to klast: one 16-byte load where all four are valid and the row of scales
// is aligned, else four clamped loads; indices & rmask as above (four keys
// from a multiple of 4 never straddle a page)
DEV f32x4 d8_load_scale(const float* sb, int kb, int klast, int rmask,
                        bool vec) {
  f32x4 r;
  if (vec && kb + 3 <= klast) {
    r = *reinterpret_cast<const f32x4*>(sb + (kb & rmask));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = sb[min(kb + j, klast) & rmask];
  }
  return r;
}

// the scales of the wave's 32 keys from k0: keys 16 c + 4 lg + r
DEV void d8_load_scales(f32x4 (&ksc)[2], f32x4 (&vsc)[2], const float* ksb,
                        const float* vsb, int k0, int klast, int rmask,
                        bool ks_vec, bool vs_vec, int lg) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int kn = k0 + 16 * c + 4 * lg;
    ksc[c] = d8_load_scale(ksb, kn, klast, rmask, ks_vec);
    vsc[c] = d8_load_scale(vsb, kn, klast, rmask, vs_vec);
  }
}

// V^T A fragments of d blocks db0 .. db0 + 3 (row d = 16 db + i, slots = the
// lane group's 8 keys) from a wave image: 4 transposed reads, one wait
template <int D>
DEV void d8_tr_v4(bf16x8 (&vt)[4], const char* img, int db0, int lane) {
  const int j = (lane >> 1) & 7;
  const int rl = 4 * (lane >> 4) + (j & 3) + 16 * (j >> 2);
  const int sw = d8_swz<D>(rl);
  const unsigned base = fa_lds_addr(img) + rl * D + 8 * (lane & 1);
  u32x2 x[4];
  asm volatile("ds_read_b64_tr_b8 %0, %4\n\t"
               "ds_read_b64_tr_b8 %1, %5\n\t"
               "ds_read_b64_tr_b8 %2, %6\n\t"
               "ds_read_b64_tr_b8 %3, %7\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3])
               : "v"(base + (((db0 + 0) ^ sw) << 4)),
                 "v"(base + (((db0 + 1) ^ sw) << 4)),
                 "v"(base + (((db0 + 2) ^ sw) << 4)),
                 "v"(base + (((db0 + 3) ^ sw) << 4))
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 4; ++t) vt[t] = d8_cvt8(x[t][0], x[t][1]);
}

// two blocks per CU wherever that compiles without scratch: all but D = 128
// with two head tiles
template <int D, int MT, bool PAGED = false>
__global__ __launch_bounds__(D8_THREADS, (D == 128 && MT >= 2) ? 1 : 2)
void fa_decode_fp8_kernel(
    std::conditional_t<PAGED, Dec8PagedArgs, Dec8Args> ar) {
  constexpr int IMG = D8_WKEYS * D;            // 4 KiB (D = 128) / 2 KiB
  constexpr int NV = IMG / 1024;               // DMA instructions per tile
  constexpr int KL = D / 64;                   // 16-byte K loads per row
  constexpr int KS = D / 32;                   // k-steps of a score tile
  constexpr int NDB = D / 16;                  // 16-dim blocks of O^T
  constexpr int DP = D + 4;                    // merge row, floats
  constexpr int DPT = D / 16;                  // merge: dims per thread
  constexpr int RING_BYTES = D8_WAVES * D8_RING * IMG;
  constexpr int MERGE_BYTES = D8_WAVES * 16 * (DP + 2) * 4;
  // the rings; after the key loop the same bytes hold the waves' streams
  __shared__ __attribute__((aligned(1024))) char
      smem[RING_BYTES > MERGE_BYTES ? RING_BYTES : MERGE_BYTES];

  const auto& a = ar.a;
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
    for (int g = threadIdx.x; g < G; g += D8_THREADS) {
      if (ns == 1) a.lse[row0 + g] = -INFINITY;
      else a.ws_lse[(row0 + g) * ns + split] = -INFINITY;
    }
    if (ns == 1) {                     // kv == 0: the row's output is zero
      ushort8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z.v[j] = 0;
      for (int i = threadIdx.x; i < G * (D / 8); i += D8_THREADS)
        *reinterpret_cast<ushort8*>(a.out + row0 * D + (int64_t)i * 8) = z;
    }
    return;
  }

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane & 15;            // head column / key row of a fragment
  const int lg = lane >> 4;            // lane group
  // dense: the batch row's caches and scales; paged: the pools, the *page
  // lambdas add the page
  const u8* kb = reinterpret_cast<const u8*>(a.k) +
                 (PAGED ? 0 : (int64_t)b * a.k_bs) + (int64_t)hkv * a.k_hs;
  const u8* vb = reinterpret_cast<const u8*>(a.v) +
                 (PAGED ? 0 : (int64_t)b * a.v_bs) + (int64_t)hkv * a.v_hs;
  const float* ksb = ar.ks + (PAGED ? 0 : (int64_t)b * ar.ks_bs) +
                     (int64_t)hkv * ar.ks_hs;
  const float* vsb = ar.vs + (PAGED ? 0 : (int64_t)b * ar.vs_bs) +
                     (int64_t)hkv * ar.vs_hs;
  const auto kpage = [&](int page) {
    if constexpr (PAGED) return kb + (int64_t)page * a.k_bs;
    else return kb;
  };
  const auto vpage = [&](int page) {
    if constexpr (PAGED) return vb + (int64_t)page * a.v_bs;
    else return vb;
  };
  const auto kspage = [&](int page) {
    if constexpr (PAGED) return ksb + (int64_t)page * ar.ks_bs;
    else return ksb;
  };
  const auto vspage = [&](int page) {
    if constexpr (PAGED) return vsb + (int64_t)page * ar.vs_bs;
    else return vsb;
  };
  int rmask = -1;                      // row within the page
  if constexpr (PAGED) rmask = (1 << a.ps_shift) - 1;
  const bool ks_vec = ar.ks_vec != 0, vs_vec = ar.vs_vec != 0;
  const float scale = a.scale;
  // this split's keys; every address is clamped to klast < kv <= L
  const int kend = min(t1 * DEC_BN, kv), klast = kend - 1;
  const int kw0 = t0 * DEC_BN + wave * D8_WKEYS;
  const int nt = kw0 < kend ? (kend - kw0 + D8_BN - 1) / D8_BN : 0;
  char* ring = smem + wave * (D8_RING * IMG);
  float* s_o = reinterpret_cast<float*>(smem);         // [wave][16][DP]
  float* s_m = s_o + D8_WAVES * 16 * DP;               // [wave][16]
  float* s_l = s_m + D8_WAVES * 16;

  for (int c0 = 0; c0 < G; c0 += 16 * MT) {
    // B fragments of head column hi, in the K loads' dim order: k-step
    // 2 kl + h holds dims 64 kl + 16 lg + 8 h .. + 8
    bf16x8 qf[MT][KS];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int head = c0 + 16 * mt + hi;
      const bf16* qrow = a.q + (int64_t)b * a.q_bs +
                         (int64_t)(hkv * G + min(head, G - 1)) * a.q_hs +
                         16 * lg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        uint4 w = *reinterpret_cast<const uint4*>(qrow + 64 * (ks >> 1) +
                                                  8 * (ks & 1));
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

    uint4 kr[2][KL];
    f32x4 ksc[2], vsc[2];              // scales of keys 16 c + 4 lg + r
    // paged: the page id of tile i + 1 and whether tile i has a page at all
    // (dense: no ids, every tile has)
    [[maybe_unused]] int page_nx = 0;
    bool ok = true;
    if constexpr (PAGED) {
      const int page = dec_page_of(a, b, min(kw0, klast));
      page_nx = dec_page_of(a, b, min(kw0 + D8_BN, klast));
      ok = (unsigned)page < (unsigned)a.P;
      if (nt > 0 && ok) {
        d8_load_k<D>(kr, kpage(page), a.k_rs, kw0, klast, rmask, lane);
        d8_load_scales(ksc, vsc, kspage(page), vspage(page), kw0, klast,
                       rmask, ks_vec, vs_vec, lg);
        d8_stage_v<D>(vpage(page), a.v_rs, kw0, klast, rmask, ring, lane);
      }
    } else if (nt > 0) {
      d8_load_k<D>(kr, kb, a.k_rs, kw0, klast, rmask, lane);
      d8_load_scales(ksc, vsc, ksb, vsb, kw0, klast, rmask, ks_vec, vs_vec,
                     lg);
      d8_stage_v<D>(vb, a.v_rs, kw0, klast, rmask, ring, lane);
    }
    for (int i = 0; i < nt; ++i) {     // wave-uniform trip count
      const int k0 = kw0 + i * D8_BN;
      const bool last = i + 1 == nt;
      const char* img = ring + (i & 1) * IMG;
      bool more = !last;               // tile i + 1 is loaded in this trip
      [[maybe_unused]] int page_nn = 0;
      if constexpr (PAGED) {
        // tile i + 2's id: first used one trip from here
        int key_nn = min(k0 + 2 * D8_BN, klast);
        dec_page_landed(page_nx, key_nn);
        page_nn = dec_page_of(a, b, key_nn);
        more = !last && (unsigned)page_nx < (unsigned)a.P;
      }
      if (more)
        d8_stage_v<D>(vpage(page_nx), a.v_rs, k0 + D8_BN, klast, rmask,
                      ring + ((i + 1) & 1) * IMG, lane);
      if constexpr (PAGED) {
        if (!ok) {                     // 32 masked keys: nothing was loaded
          if (more) {
            d8_load_k<D>(kr, kpage(page_nx), a.k_rs, k0 + D8_BN, klast,
                         rmask, lane);
            d8_load_scales(ksc, vsc, kspage(page_nx), vspage(page_nx),
                           k0 + D8_BN, klast, rmask, ks_vec, vs_vec, lg);
          }
          page_nx = page_nn;
          ok = more;
          continue;
        }
      }
      fa_wait_tile<NV>(!more);         // K(i), scales(i) and V(i) are in
      __builtin_amdgcn_sched_barrier(0);   // no MFMA above the DMA issue

      f32x4 s[MT][2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) s[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kl = 0; kl < KL; ++kl) {
          const bf16x8 ka = d8_cvt8(kr[c][kl].x, kr[c][kl].y);
          const bf16x8 kb2 = d8_cvt8(kr[c][kl].z, kr[c][kl].w);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            s[mt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                ka, qf[mt][2 * kl], s[mt][c], 0, 0, 0);
            s[mt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kb2, qf[mt][2 * kl + 1], s[mt][c], 0, 0, 0);
          }
        }
      }
      if (more)
        d8_load_k<D>(kr, kpage(page_nx), a.k_rs, k0 + D8_BN, klast, rmask,
                     lane);

      // lane (lg, hi) holds keys k0 + 16 c + 4 lg + r of head hi; the tile's
      // first key is valid, so every head's new maximum is finite
      const int nvalid = kend - (k0 + 4 * lg);   // key 16 c + r valid iff <
      bf16x8 pf[MT][D8_PP];            // P as a sum of bf16 parts
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        float sv[8];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool valid = 16 * (j >> 2) + (j & 3) < nvalid;
          sv[j] = valid ? s[mt][j >> 2][j & 3] * ksc[j >> 2][j & 3] * scale
                        : -INFINITY;
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
          psum += p[j];                // l sums the fp32 p, unscaled
          p[j] *= vsc[j >> 2][j & 3];   // v_scale in fp32, then the split
        }
        l[mt] = l[mt] * alpha + psum;
        // part t is the bf16 rounding of what parts 0 .. t - 1 left over
        // (the subtractions are exact), so the parts sum to p in fp32
#pragma unroll
        for (int t = 0; t < D8_PP; ++t) {
          union { unsigned u[4]; bf16x8 v; } pk;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned w = fa_cvt_pk(p[2 * j], p[2 * j + 1]);
            pk.u[j] = w;
            p[2 * j] -= __uint_as_float(w << 16);
            p[2 * j + 1] -= __uint_as_float(w & 0xffff0000u);
          }
          pf[mt][t] = pk.v;
        }
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][db][r] *= alpha;
      }
      if (more)                        // the scales are consumed: reload
        d8_load_scales(ksc, vsc, kspage(page_nx), vspage(page_nx),
                       k0 + D8_BN, klast, rmask, ks_vec, vs_vec, lg);

#pragma unroll
      for (int q4 = 0; q4 < NDB / 4; ++q4) {
        bf16x8 vt[4];
        d8_tr_v4<D>(vt, img, 4 * q4, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int t = D8_PP - 1; t >= 0; --t)     // small parts first
              acc[mt][4 * q4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  vt[j], pf[mt][t], acc[mt][4 * q4 + j], 0, 0, 0);
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
    // every page of the split is out of range; patched below).
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
        for (int w = 1; w < D8_WAVES; ++w) mx = fmaxf(mx, s_m[w * 16 + hh]);
        float lt = 0.f, o[DPT];
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] = 0.f;
#pragma unroll
        for (int w = 0; w < D8_WAVES; ++w) {
          const float ww = __expf(s_m[w * 16 + hh] - mx);
          lt += s_l[w * 16 + hh] * ww;
#pragma unroll
          for (int j = 0; j < DPT; ++j)
            o[j] += s_o[(w * 16 + hh) * DP + d0 + j] * ww;
        }
        const float inv = 1.f / lt;
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[j] *= inv;
        const int64_t row = row0 + head;
        float ls = mx + logf(lt);
        // no loaded key: replace the NaN of exp(-inf + inf) after the fact,
        // so that the sums above stay the dense kernel's, operation for
        // operation
        if constexpr (PAGED) {
          if (mx == -INFINITY) {
            ls = -INFINITY;
#pragma unroll
            for (int j = 0; j < DPT; ++j) o[j] = 0.f;
          }
        }
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

const char* D8_FN = "flash_attn_decode (fp8 cache): ";

void d8_check_cache(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.scalar_type() != at::kByte, D8_FN, what, " is uint8: pass it "
              "as .view(torch.float8_e4m3fn)");
  TORCH_CHECK(t.scalar_type() == at::kFloat8_e4m3fn, D8_FN, what,
              " must be float8_e4m3fn");
  TORCH_CHECK(t.stride(-1) == 1, D8_FN, what, " needs a contiguous last dim");
  for (int64_t i = 0; i + 1 < t.dim(); ++i)
    TORCH_CHECK(t.size(i) == 1 || t.stride(i) % 16 == 0, D8_FN, what,
                " stride ", i, " (", t.stride(i),
                ") is not a multiple of 16 bytes");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, D8_FN,
              what, " is not 16-byte aligned");
}

// checks a scale tensor (`shape` names the cache's first three dims); returns
// whether every (b, hkv) / (page, hkv) row is 16-B aligned
bool d8_check_scale(const torch::Tensor& s, const torch::Tensor& cache,
                    const char* what, const char* shape = "[B, Hkv, L]") {
  TORCH_CHECK(s.is_cuda() && s.device() == cache.device(), D8_FN, what,
              " must be on the caches' device");
  TORCH_CHECK(s.scalar_type() == at::kFloat, D8_FN, what, " must be fp32");
  TORCH_CHECK(s.dim() == 3 && s.size(0) == cache.size(0) &&
              s.size(1) == cache.size(1) && s.size(2) == cache.size(2),
              D8_FN, what, " must be ", shape);
  TORCH_CHECK(s.size(2) == 1 || s.stride(2) == 1, D8_FN, what,
              " needs a contiguous last dim");
  bool vec = reinterpret_cast<uintptr_t>(s.data_ptr()) % 16 == 0;
  for (int i = 0; i < 2; ++i)
    vec = vec && (s.size(i) == 1 || s.stride(i) % 4 == 0);
  return vec;
}

}  // namespace

int64_t decode_attn_fp8_tile() { return D8_BN; }

std::vector<torch::Tensor> flash_attn_decode_fp8(
    torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor k_scale, torch::Tensor v_scale, torch::Tensor kv_len,
    double scale, int64_t num_splits) {
  // dec_prepare's checks, for byte caches
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
              kv_len.is_cuda(), D8_FN,
              "q, k_cache, v_cache and kv_len must be on the GPU");
  TORCH_CHECK(q.device() == k_cache.device() &&
              q.device() == v_cache.device() && q.device() == kv_len.device(),
              D8_FN, "all tensors must share one device");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, D8_FN, "q must be bf16");
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4, D8_FN,
              "need q [B, H, D] and caches [B, Hkv, L, D]");
  const int64_t B = q.size(0), H = q.size(1), D = q.size(2);
  const int64_t Hkv = k_cache.size(1), L = k_cache.size(2);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B &&
              k_cache.size(3) == D, D8_FN, "cache shapes do not match q");
  TORCH_CHECK(D == 64 || D == 128, D8_FN, "D must be 64 or 128, got ", D);
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, D8_FN, "H (", H,
              ") is not a multiple of Hkv (", Hkv, ")");
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.dim() == 1 &&
              kv_len.size(0) == B && kv_len.is_contiguous(), D8_FN,
              "kv_len must be a contiguous int32 [B]");
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 && L < ((int64_t)1 << 31) - D8_BN,
              D8_FN, "B, Hkv or L too large");
  TORCH_CHECK(num_splits >= 0, D8_FN, "num_splits must be >= 0");
  DecCall c;
  c.B = B; c.H = H; c.Hkv = Hkv; c.D = D;
  c.out = torch::empty({B, H, D}, q.options());
  c.lse = torch::empty({B, H}, q.options().dtype(at::kFloat));
  c.empty = B == 0 || H == 0;
  if (c.empty) return {c.out, c.lse};
  dec_check_strides(q, "q");
  d8_check_cache(k_cache, "k_cache");
  d8_check_cache(v_cache, "v_cache");
  Dec8Args ar;
  ar.ks_vec = d8_check_scale(k_scale, k_cache, "k_scale");
  ar.vs_vec = d8_check_scale(v_scale, v_cache, "v_scale");

  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int ns = (int)(num_splits > 0
                           ? std::min<int64_t>(num_splits, 1 << 16)
                           : decode_attn_num_splits(B, Hkv, L, cus));
  DecArgs& a = ar.a;
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
  ar.ks = k_scale.data_ptr<float>();
  ar.vs = v_scale.data_ptr<float>();
  ar.ks_bs = k_scale.stride(0); ar.ks_hs = k_scale.stride(1);
  ar.vs_bs = v_scale.stride(0); ar.vs_hs = v_scale.stride(1);
  c.a = a;                             // the merge reads the workspace from c

  const int64_t G = H / Hkv;
  const int mt = G <= 16 ? 1 : D8_MAX_MT;
  auto stream = hetu_current_stream();
  const dim3 grid(a.ns, (unsigned)Hkv, (unsigned)B);
#define D8_LAUNCH(DD, MM)                                                  \
  hipLaunchKernelGGL((fa_decode_fp8_kernel<DD, MM>), grid,                 \
                     dim3(D8_THREADS), 0, stream, ar)
#define D8_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (mt == 1) D8_LAUNCH(DD, 1);                                         \
    else D8_LAUNCH(DD, D8_MAX_MT);                                         \
  } while (0)
  if (D == 128) D8_LAUNCH_D(128);
  else D8_LAUNCH_D(64);
#undef D8_LAUNCH_D
#undef D8_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (a.ns > 1) dec_merge_launch(c, stream);
  return {c.out, c.lse};
}

std::vector<torch::Tensor> flash_attn_decode_paged_fp8(
    torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
    torch::Tensor k_scale, torch::Tensor v_scale, torch::Tensor block_table,
    torch::Tensor kv_len, double scale, int64_t num_splits) {
  // the id prefetch forms keys up to two tiles past the last one
  DecCall c = dec_prepare(q, k_pool, v_pool, kv_len, scale, num_splits,
                          3 * D8_BN, &block_table, /*fp8=*/true);
  if (c.empty) return {c.out, c.lse};
  d8_check_cache(k_pool, "k_pool");
  d8_check_cache(v_pool, "v_pool");
  Dec8PagedArgs ar;
  ar.ks_vec = d8_check_scale(k_scale, k_pool, "k_scale", "[P, Hkv, PS]");
  ar.vs_vec = d8_check_scale(v_scale, v_pool, "v_scale", "[P, Hkv, PS]");
  ar.a = c.paged();
  ar.ks = k_scale.data_ptr<float>();
  ar.vs = v_scale.data_ptr<float>();
  ar.ks_bs = k_scale.stride(0); ar.ks_hs = k_scale.stride(1);
  ar.vs_bs = v_scale.stride(0); ar.vs_hs = v_scale.stride(1);
  const int64_t G = c.H / c.Hkv;
  const int mt = G <= 16 ? 1 : D8_MAX_MT;
  auto stream = hetu_current_stream();
  const dim3 grid(ar.a.ns, (unsigned)c.Hkv, (unsigned)c.B);
#define D8_LAUNCH(DD, MM)                                                  \
  hipLaunchKernelGGL((fa_decode_fp8_kernel<DD, MM, true>), grid,           \
                     dim3(D8_THREADS), 0, stream, ar)
#define D8_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (mt == 1) D8_LAUNCH(DD, 1);                                         \
    else D8_LAUNCH(DD, D8_MAX_MT);                                         \
  } while (0)
  if (c.D == 128) D8_LAUNCH_D(128);
  else D8_LAUNCH_D(64);
#undef D8_LAUNCH_D
#undef D8_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (ar.a.ns > 1) dec_merge_launch(c, stream);
  return {c.out, c.lse};
}
