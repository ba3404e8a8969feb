// Flash-attention primitives shared by the 8-wave 32x32-MFMA kernels for
// gfx950: attention_v2.hip (forward), attention_bwd_v2.hip (stride-aware
// backward) and attention_bwd_v3.hip (ring-staged dense backward).
//
// Every layout primitive lives here exactly once: the swizzled row-major
// LDS image, the V subtile image, global_load_lds staging, the
// cvt_pk + permlane32_swap fragment pack, the ds_read_b64_tr_b16 transpose
// reads, the row load / store helpers and the per-tile compute bodies of
// the two backward kernels.  Each is validated by scripts/probe_fa2.hip.
// All functions take lane / hi explicitly; nothing captures a local.
#pragma once
#include <cstdlib>
#include <torch/extension.h>
#include "common.h"

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

constexpr int FA_THREADS = 512;    // 8 waves x 32 rows per workgroup

// ---- LDS layouts and their sizes (the only source for launch sizing) -----
// Row-major tile image: [rows][256 B] (D=128 bf16), byte-in-row XOR
// ((row & 15) << 4): conflict-free ds_read_b128 and tr_b16 reads.
constexpr int FA_KV_IMG = 64 * 256;     // one 64-key K or V tile, 16 KiB
constexpr int FA_Q_IMG = 32 * 256;      // one 32-row Q or dO tile, 8 KiB
constexpr int FA_WAVE_V_IMG = 32 * 256; // dkv: a wave's own 32 V rows
constexpr int FA_P_IMG = 32 * 72;       // dkv: per-wave [32 q][32 key] bf16,
                                        // 72 B rows (64 B + pad)
constexpr int FA_RING = 3;              // K/V ring depth of fwd and v3 dq
constexpr size_t FA_FWD_LDS = 2 * FA_RING * (size_t)FA_KV_IMG;    // 96 KiB
constexpr size_t FA2_DQ_LDS = 2 * 2 * (size_t)FA_KV_IMG;          // 64 KiB
constexpr size_t FA3_DQ_LDS = 2 * FA_RING * (size_t)FA_KV_IMG;    // 96 KiB
// dkv (both generations): 2 Q + 2 dO buffers, then per wave a V image and
// a P' / dS' image pair
constexpr size_t FA_DKV_LDS =
    4 * (size_t)FA_Q_IMG + 8 * (size_t)FA_WAVE_V_IMG + 8 * 2 * (size_t)FA_P_IMG;

DEV int fa_swz_rm(int row, int byte_in_row) {
  return row * 256 + (byte_in_row ^ ((row & 15) << 4));
}

// inverse of fa_swz_rm for staging: the source element column whose 16 B
// land at linear image byte `pos` (row = pos >> 8)
DEV int fa_rm_src_col(int pos) {
  return ((pos & 255) ^ (((pos >> 8) & 15) << 4)) >> 1;
}

// V tile image of the forward: [kb][db] subtiles of [32 keys][16 d] bf16
// (1 KiB each, row stride 32 B): key k, dim d -> subtile (k>>5, d>>4)
DEV int fa_voff(int key, int d) {
  return ((key >> 5) * 8 + (d >> 4)) * 1024 + (key & 31) * 32 + (d & 15) * 2;
}

// 16-byte global -> LDS DMA; glds writes lane-linear (dest = base + lane*16)
// so any swizzle is folded into the SOURCE address
DEV void fa_glds16(const bf16* src, char* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// Loop-head wait of the counted-vmcnt pipelines: every load but the newest
// tile's N has landed.  On the last tile nothing newer is in flight, so
// the wait has to drain: a counted wait there returns while the tile's own
// N loads are still outstanding, and the tile would be read before it
// landed.
template <int N>
DEV void fa_wait_tile(bool last) {
  if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" :: "i"(N) : "memory");
}

// ds ops take a 32-bit LDS offset, not a generic 64-bit pointer
DEV unsigned fa_lds_addr(const char* p) {
  return (unsigned)(uintptr_t)(
      (const __attribute__((address_space(3))) char*)p);
}

DEV unsigned fa_cvt_pk(float a, float b) {
  unsigned w;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(a), "v"(b));
  return w;
}

// 4 floats -> 4 bf16, one 8-byte store
DEV void fa_store4_bf16(void* dst, float f0, float f1, float f2, float f3) {
  union { unsigned u[2]; uint2 v; } st;
  st.u[0] = fa_cvt_pk(f0, f1);
  st.u[1] = fa_cvt_pk(f2, f3);
  *reinterpret_cast<uint2*>(dst) = st.v;
}

// pack p[16] (C layout: col = q lane-local, rows = key crow) into a bf16
// A/B-fragment with own-index q, k = 8 keys starting at 8*hi within the
// 16-key slice held by registers rb..rb+7.  Half exchange: w0 <- keys
// {+0,+1}, w2 <- keys {+4,+5} (lo half keeps own, hi half receives the
// partner's).
DEV bf16x8 fa_pack_frag(const float (&p)[16], int rb) {
  unsigned w0 = fa_cvt_pk(p[rb + 0], p[rb + 1]);
  unsigned w2 = fa_cvt_pk(p[rb + 4], p[rb + 5]);
  unsigned w1 = fa_cvt_pk(p[rb + 2], p[rb + 3]);
  unsigned w3 = fa_cvt_pk(p[rb + 6], p[rb + 7]);
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1"
               : "+v"(w0), "+v"(w2));
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1"
               : "+v"(w1), "+v"(w3));
  union { unsigned u[4]; bf16x8 v; } pk;
  pk.u[0] = w0; pk.u[1] = w1; pk.u[2] = w2; pk.u[3] = w3;
  return pk.v;
}

DEV bf16x8 fa_join(u32x2 lo, u32x2 hi) {
  union { u32x2 u[2]; bf16x8 v; } f;
  f.u[0] = lo; f.u[1] = hi;
  return f.v;
}

// Measured tr_b16 semantics (scripts/probe_tr16): lane 16g+4r+c receives
// elem j from the address of lane 16g+4j+r, at +2c bytes.  So lane a
// supplies the row selected by (a>>2)&3 and the column block selected by
// a&3.  This is the column byte a lane supplies within a 64 B fragment.
DEV int fa_tr_colbyte(int lane) {
  return (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
}

// tr_b16 read of the 4 A/B fragments d[dt] (own = column 32*dt.., k = 8
// rows at rowb..) from a swizzled row-major image: 8 reads issued
// back-to-back under a single lgkmcnt wait instead of 4 round trips.
DEV void fa_tr_rm4(bf16x8 (&d)[4], const char* img, int rowb, int lane) {
  const int r1 = rowb + ((lane >> 2) & 3);
  const int r2 = r1 + 4;
  const unsigned b1 = fa_lds_addr(img + r1 * 256);
  const unsigned b2 = fa_lds_addr(img + r2 * 256);
  const int m1 = (r1 & 15) << 4, m2 = (r2 & 15) << 4;
  const int cb0 = fa_tr_colbyte(lane);
  u32x2 x[8];
  asm volatile("ds_read_b64_tr_b16 %0, %8\n\t"
               "ds_read_b64_tr_b16 %1, %9\n\t"
               "ds_read_b64_tr_b16 %2, %10\n\t"
               "ds_read_b64_tr_b16 %3, %11\n\t"
               "ds_read_b64_tr_b16 %4, %12\n\t"
               "ds_read_b64_tr_b16 %5, %13\n\t"
               "ds_read_b64_tr_b16 %6, %14\n\t"
               "ds_read_b64_tr_b16 %7, %15\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]),
                 "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7])
               : "v"(b1 + ((cb0 + 0) ^ m1)), "v"(b2 + ((cb0 + 0) ^ m2)),
                 "v"(b1 + ((cb0 + 64) ^ m1)), "v"(b2 + ((cb0 + 64) ^ m2)),
                 "v"(b1 + ((cb0 + 128) ^ m1)), "v"(b2 + ((cb0 + 128) ^ m2)),
                 "v"(b1 + ((cb0 + 192) ^ m1)), "v"(b2 + ((cb0 + 192) ^ m2)));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) d[dt] = fa_join(x[2 * dt], x[2 * dt + 1]);
}

// tr_b16 read of one fragment (own = key, k = 8 q rows at qb..) from a
// 72B-row [32 q][32 key] P' / dS' image.
DEV bf16x8 fa_tr_p(const char* img, int qb, int lane) {
  const int r1 = qb + ((lane >> 2) & 3);
  const unsigned a1 = fa_lds_addr(img + r1 * 72 + fa_tr_colbyte(lane));
  u32x2 x1, x2;
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
               "ds_read_b64_tr_b16 %1, %2 offset:288\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(x1), "=&v"(x2) : "v"(a1));
  __builtin_amdgcn_sched_barrier(0);
  return fa_join(x1, x2);
}

// forward: the 4 V^T fragments d[dt] (row d = 32dt + iq, k = keys
// 16ks + 8hi..) of one 16-key slot from the subtile image.  fa_voff is
// linear in the d-subtile index, so all 4 sit at static offsets
// (+2048*dt) from ONE address: 8 tr reads under a single lgkmcnt wait
// (the per-pair wait was the forward's biggest stall).
DEV void fa_tr_v4(bf16x8 (&d)[4], const char* v_img, int ks, int lane) {
  const int hi = lane >> 5;
  const int keyb = 16 * ks + 8 * hi + ((lane >> 2) & 3);
  const int dbase0 = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const unsigned a1 = fa_lds_addr(v_img + fa_voff(keyb, dbase0));
  u32x2 r1[4], r2[4];
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %8 offset:128\n\t"
      "ds_read_b64_tr_b16 %2, %8 offset:2048\n\t"
      "ds_read_b64_tr_b16 %3, %8 offset:2176\n\t"
      "ds_read_b64_tr_b16 %4, %8 offset:4096\n\t"
      "ds_read_b64_tr_b16 %5, %8 offset:4224\n\t"
      "ds_read_b64_tr_b16 %6, %8 offset:6144\n\t"
      "ds_read_b64_tr_b16 %7, %8 offset:6272\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r1[0]), "=&v"(r2[0]), "=&v"(r1[1]), "=&v"(r2[1]),
        "=&v"(r1[2]), "=&v"(r2[2]), "=&v"(r1[3]), "=&v"(r2[3])
      : "v"(a1));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) d[dt] = fa_join(r1[dt], r2[dt]);
}

// A lane's row as 8 MFMA fragments: frags[kk] = row[16*kk + 8*hi .. +8).
// The scaled form folds the softmax scale into Q (or K).
DEV void fa_load_row_frags(bf16x8 (&frags)[8], const bf16* row, int hi) {
#pragma unroll
  for (int kk = 0; kk < 8; ++kk)
    frags[kk] = *reinterpret_cast<const bf16x8*>(row + kk * 16 + hi * 8);
}
DEV void fa_load_row_frags(bf16x8 (&frags)[8], const bf16* row, int hi,
                           float scale) {
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    ushort8 u = *reinterpret_cast<const ushort8*>(row + kk * 16 + hi * 8);
    union { ushort8 us; bf16x8 v; } cvt;
#pragma unroll
    for (int j = 0; j < 8; ++j) cvt.us.v[j] = f2bf(bf2f(u.v[j]) * scale);
    frags[kk] = cvt.v;
  }
}

// O / dQ epilogue: row[d] = mul * acc^T[d][own row].  In the C layout a
// lane holds 4 runs of 4 contiguous d per 32-d block: (r&3) + 8*(r>>2).
DEV void fa_store_row_bf16(const f32x16 (&acc)[4], float mul, bf16* row,
                           int hi) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      fa_store4_bf16(row + 32 * dt + 8 * g + 4 * hi,
                     acc[dt][4 * g + 0] * mul, acc[dt][4 * g + 1] * mul,
                     acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
}

// dkv: stage the wave's own 32 V rows (8 KiB) into its row-major image;
// rows past Skv clamp to the last valid one
DEV void fa_stage_wave_v(const bf16* Vb, int64_t row_stride, int key0,
                         int Skv, char* vw_lds, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int pos = (i * 64 + lane) * 16;
    fa_glds16(Vb + (int64_t)min(key0 + (pos >> 8), Skv - 1) * row_stride +
                  fa_rm_src_col(pos),
              vw_lds + pos);
  }
}

// ---- causal tile bounds ---------------------------------------------------
// diag = Skv - S.  Number of 64-key tiles the 256-row q block at q0 visits:
DEV int fa_n_kv_tiles(int q0, int Skv, int diag, bool causal) {
  const int n = (Skv + 63) / 64;
  return causal ? min(n, max((q0 + 256 + diag + 63) / 64, 1)) : n;
}
// First 32-row q tile that any key of the 256-key block at kb0 can see:
DEV int fa_first_q_tile(int kb0, int diag, bool causal) {
  return causal ? max(0, (kb0 - diag) / 32) : 0;
}

// A tile of the forward and dq kernels needs the masked stage only where it
// crosses the key tail, the row tail or the causal diagonal of the wave's
// 32 rows; everywhere else every select of the mask is false and the plain
// stage computes the same bits without them.  Wave-uniform.  mask_all
// (HETU_AMD_FA_MASK_ALL=1) forces the masked stage.  Rows qw0..qw0+31
// against the 64-key tile at k0:
DEV bool fa_boundary_kv_tile(int qw0, int k0, int S, int Skv, int diag,
                             bool causal, bool mask_all) {
  qw0 = __builtin_amdgcn_readfirstlane(qw0);    // the wave index is a VGPR
  return mask_all || (k0 + 63 >= Skv) || (qw0 + 31 >= S) ||
         (causal && k0 + 63 > qw0 + diag);
}
// The masked bodies.  In the C layout register r of a lane holds key
// kbase + 4*hi + fa_crow(r) (+32 for a tile's second 32-key half).  The
// three tests (key tail, row tail, causal diagonal) fold into one per-lane
// bound, so an element costs a single compare against a constant:
// masked iff 4*hi-relative key index > fa_mask_bound(kbase + 4*hi, ...).
DEV constexpr int fa_crow(int r) { return (r & 3) + 8 * (r >> 2); }
DEV int fa_mask_bound(int kbase_lane, int my_q, int S, int Skv, int diag,
                      bool causal) {
  int last = Skv - 1;                           // last key this row may see
  if (causal) last = min(last, my_q + diag);
  return (my_q >= S) ? -1 : last - kbase_lane;  // -1: every key masked
}

// ---- backward tile bodies (shared by the v2 and v3 kernels) ---------------
// dq kernels, one 64-key tile: S^T = K Q_s^T and dP^T = V dO^T from the
// row-major K / V images, dS rebuilt from the saved lse and packed
// in-register into B-fragments, dQ^T += K^T dS.
// The one macro here, and it takes everything it touches as an argument.
// As an always-inline function the compiler turns the mask's exec branch
// into 32 v_cndmask, and fa3_bwd_dq_kernel, which sits at its 256-VGPR
// ceiling, then spills 88 B/lane to scratch; expanded in the kernel the
// code compiles exactly as it did when each kernel carried its own copy.
// `boundary` is wave-uniform (fa_boundary_kv_tile) and picks the dS stage;
// the MFMA phases around it exist once (two whole copies of the tile spill).
// The stage's two compile-time variants: the masked one, and the plain one
// without key index, compare or select.
#define FA_BWD_DQ_DS_MASKED(ds, sa, da, cbase, bound, lse_q, del_q)         \
  _Pragma("unroll")                                                         \
  for (int r = 0; r < 16; ++r) {                                            \
    bool masked_ = (cbase) + fa_crow(r) > (bound);                          \
    float pv_ = masked_ ? 0.f : __expf((sa)[r] - (lse_q));                  \
    (ds)[r] = masked_ ? 0.f : pv_ * ((da)[r] - (del_q));                    \
  }
#define FA_BWD_DQ_DS_PLAIN(ds, sa, da, lse_q, del_q)                        \
  _Pragma("unroll")                                                         \
  for (int r = 0; r < 16; ++r)                                              \
    (ds)[r] = __expf((sa)[r] - (lse_q)) * ((da)[r] - (del_q));
#define FA_BWD_DQ_TILE(boundary, k_img, v_img, qreg, doreg, dq_acc, k0,     \
                       my_q, S, Skv, diag, causal, lse_q, del_q, lane)      \
  do {                                                                      \
    const int iq_ = (lane) & 31;                                            \
    const int hi_ = (lane) >> 5;                                            \
    float ds_[2][16];                                                       \
    _Pragma("unroll")                                                       \
    for (int ct = 0; ct < 2; ++ct) {                                        \
      f32x16 sa_, da_;                                                      \
      _Pragma("unroll")                                                     \
      for (int r = 0; r < 16; ++r) { sa_[r] = 0.f; da_[r] = 0.f; }          \
      _Pragma("unroll")                                                     \
      for (int kk = 0; kk < 8; ++kk) {                                      \
        const int off_ = fa_swz_rm(32 * ct + iq_, kk * 32 + hi_ * 16);      \
        bf16x8 kf_ = *reinterpret_cast<const bf16x8*>((k_img) + off_);      \
        bf16x8 vf_ = *reinterpret_cast<const bf16x8*>((v_img) + off_);      \
        sa_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf_, (qreg)[kk], sa_, \
                                                      0, 0, 0);             \
        da_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf_, (doreg)[kk],     \
                                                      da_, 0, 0, 0);        \
      }                                                                     \
      if (boundary) {                                                       \
        const int bound_ = fa_mask_bound((k0) + 4 * hi_, my_q, S, Skv,      \
                                         diag, causal);                     \
        FA_BWD_DQ_DS_MASKED(ds_[ct], sa_, da_, 32 * ct, bound_, lse_q,      \
                            del_q)                                          \
      } else {                                                              \
        FA_BWD_DQ_DS_PLAIN(ds_[ct], sa_, da_, lse_q, del_q)                 \
      }                                                                     \
    }                                                                       \
    _Pragma("unroll")                                                       \
    for (int ks = 0; ks < 4; ++ks) {                                        \
      bf16x8 dsf_ = fa_pack_frag(ds_[ks >> 1], (ks & 1) * 8);               \
      bf16x8 kt_[4];                                                        \
      fa_tr_rm4(kt_, (k_img), 16 * ks + 8 * hi_, (lane));                   \
      _Pragma("unroll")                                                     \
      for (int dt = 0; dt < 4; ++dt)                                        \
        (dq_acc)[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(             \
            kt_[dt], dsf_, (dq_acc)[dt], 0, 0, 0);                          \
    }                                                                       \
  } while (0)

// dkv kernels, one 32-q tile for the wave's 32 exclusive keys key0..:
// S^T = K_s Q^T and dP^T = V dO^T, then P^T / dS^T round-trip through the
// wave's two 72B-row images (p_img, then dS' right behind it) so tr_b16
// can hand them back as A-fragments; dV += P^T dO, dK += dS^T Q.
// Every tile takes the masked form: a mask-free stage for interior tiles
// (as in the forward and dq) measured no faster here, the tile is bound by
// its LDS traffic (profiles/r07_fa_tiles.md).
DEV void fa_bwd_dkv_tile(const char* q_img, const char* do_img,
                         const char* vw_img, char* p_img,
                         const bf16x8 (&kreg)[8], f32x16 (&dk_acc)[4],
                         f32x16 (&dv_acc)[4], int qt0, int key0, int S,
                         int Skv, int diag, bool causal,
                         const float* lse_b, const float* del_b, int lane) {
  const int iq = lane & 31;        // own q column AND own key row
  const int hi = lane >> 5;
  char* ds_img = p_img + FA_P_IMG;
  const int my_q = qt0 + iq;
  const float lse_q = lse_b[min(my_q, S - 1)];
  const float del_q = del_b[min(my_q, S - 1)];
  f32x16 sa, da;
#pragma unroll
  for (int r = 0; r < 16; ++r) { sa[r] = 0.f; da[r] = 0.f; }
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    const int off = fa_swz_rm(iq, kk * 32 + hi * 16);
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(q_img + off);
    bf16x8 df = *reinterpret_cast<const bf16x8*>(do_img + off);
    bf16x8 vf = *reinterpret_cast<const bf16x8*>(vw_img + off);
    sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kreg[kk], qf, sa, 0, 0, 0);
    da = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, df, da, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
    bool masked = (key >= Skv) || (my_q >= S) ||
                  (causal && key > my_q + diag);
    float pv = masked ? 0.f : __expf(sa[r] - lse_q);
    sa[r] = pv;                                    // P^T
    da[r] = masked ? 0.f : pv * (da[r] - del_q);   // dS^T (no scale)
  }
#pragma unroll
  for (int rq = 0; rq < 4; ++rq) {     // 4 key-quads
    // row = q (iq), cols = keys keyb..keyb+3 (8 B)
    const int keyb = (8 * rq + 4 * hi) & 31;
    const unsigned pw0 = fa_cvt_pk(sa[4 * rq + 0], sa[4 * rq + 1]);
    const unsigned pw1 = fa_cvt_pk(sa[4 * rq + 2], sa[4 * rq + 3]);
    const unsigned dw0 = fa_cvt_pk(da[4 * rq + 0], da[4 * rq + 1]);
    const unsigned dw1 = fa_cvt_pk(da[4 * rq + 2], da[4 * rq + 3]);
    union { unsigned u[2]; uint2 v; } sp, sd;
    sp.u[0] = pw0; sp.u[1] = pw1;
    sd.u[0] = dw0; sd.u[1] = dw1;
    *reinterpret_cast<uint2*>(p_img + iq * 72 + keyb * 2) = sp.v;
    *reinterpret_cast<uint2*>(ds_img + iq * 72 + keyb * 2) = sd.v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int s = 0; s < 2; ++s) {        // k = q slices of 16
    bf16x8 ptf = fa_tr_p(p_img, 16 * s + 8 * hi, lane);
    bf16x8 dstf = fa_tr_p(ds_img, 16 * s + 8 * hi, lane);
    bf16x8 dof[4], qa[4];
    fa_tr_rm4(dof, do_img, 16 * s + 8 * hi, lane);
    fa_tr_rm4(qa, q_img, 16 * s + 8 * hi, lane);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dv_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          ptf, dof[dt], dv_acc[dt], 0, 0, 0);
      dk_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          dstf, qa[dt], dk_acc[dt], 0, 0, 0);
    }
  }
}

// HETU_AMD_FA_MASK_ALL=1 runs the masked body on every tile (read at each
// launch; for tests and for profiling both sides from one build)
inline bool fa_mask_all() {
  const char* e = std::getenv("HETU_AMD_FA_MASK_ALL");
  return e != nullptr && e[0] == '1';
}

// ---- host launchers shared across the attention translation units --------
// delta[row] = rowsum(dO * O); rows are LSE-ordered (b, h, s), dO / O
// addressed through `so` (BHSD or BS[HD]).  Defined in attention_bwd_v2.hip.
void fa_delta_launch(const bf16* dO, const bf16* O, float* delta,
                     int64_t rows, int D, int H, int S, FaStrides so,
                     hipStream_t stream);
// v2 forward over any layout; cu != nullptr selects the packed-varlen mode
// (B = segments, S = Skv = max_seqlen, lse [H, lse_T]).
void fa2_fwd_launch(const bf16* q, const bf16* k, const bf16* v, bf16* o,
                    float* lse, int B, int H, int Hkv, int S, int Skv,
                    float scale, bool causal, FaStrides sq, FaStrides skv,
                    FaStrides so, const int* cu, int lse_T,
                    hipStream_t stream);
// dense BHSD backward, one per generation (v3: D=128 and H == Hkv only)
std::vector<torch::Tensor> fa2_bwd_launch(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, bool causal, double scale);
std::vector<torch::Tensor> fa3_bwd_launch(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, bool causal, double scale);
