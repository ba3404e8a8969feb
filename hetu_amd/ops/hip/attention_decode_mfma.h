// The pieces of the MFMA decode kernel (attention_decode_mfma.hip) that the
// verification kernel (attention_verify_paged.hip) shares: the tile constants,
// the swizzled per-wave V image with its DMA staging and transposed reads, and
// the K fragment loads.  attention_decode_mfma.hip says how they fit together.
#pragma once
#include "attention_common.h"
#include "attention_decode.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DM_WAVES = 4;
constexpr int DM_THREADS = DM_WAVES * WAVE;
constexpr int DM_WKEYS = 32;                   // keys per wave and tile
constexpr int DM_BN = DM_WAVES * DM_WKEYS;     // keys per block tile
constexpr int DM_RING = 2;                     // V images per wave
constexpr int DM_MAX_MT = 4;                   // 64 heads per pass
static_assert(DM_BN % DEC_BN == 0, "tiles are whole split units");

template <int D>
DEV int dm_swz(int row) {
  return D == 128 ? (row & 7) : ((row >> 1) & 3);
}

// stage keys k0 .. k0 + 31 (clamped to klast) of V into a wave's image; a
// row index is taken & rmask (-1: dense; PS - 1: the row within vb's page)
template <int D>
DEV void dm_stage_v(const bf16* vb, long long v_rs, int k0, int klast,
                    int rmask, char* img, int lane) {
  constexpr int RB = 2 * D;
#pragma unroll
  for (int i = 0; i < DM_WKEYS * RB / 1024; ++i) {
    const int pos = (i * WAVE + lane) * 16;
    const int row = pos / RB;
    const int col = ((pos % RB) ^ (dm_swz<D>(row) << 5)) >> 1;
    fa_glds16(vb + (int64_t)(min(k0 + row, klast) & rmask) * v_rs + col,
              img + pos);
  }
}

// the wave's 32 K rows as A fragments: kf[c][ks] = row 16 c + i, dims
// 32 ks + 8 g .. + 8
template <int D>
DEV void dm_load_k(bf16x8 (&kf)[2][D / 32], const bf16* kb, long long k_rs,
                   int k0, int klast, int rmask, int lane) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const bf16* row = kb + (int64_t)(min(k0 + 16 * c + (lane & 15), klast) &
                                     rmask) * k_rs + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks)
      kf[c][ks] = *reinterpret_cast<const bf16x8*>(row + 32 * ks);
  }
}

// V^T A fragments of d blocks db0 .. db0 + 3 (row d = 16 db + i, slots =
// the lane group's 8 keys) from a wave image: 8 transposed reads, one wait.
// By the measured tr_b16 semantics lane a supplies the address of key row
// 4 g + ((a >> 2) & 3) at dim 16 db + 4 (a & 3).
template <int D>
DEV void dm_tr_v4(bf16x8 (&vt)[4], const char* img, int db0, int lane) {
  constexpr int RB = 2 * D;
  const int rl = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int sw = dm_swz<D>(rl);
  const unsigned base = fa_lds_addr(img) + rl * RB + 8 * (lane & 3);
  u32x2 x[8];
  asm volatile("ds_read_b64_tr_b16 %0, %8\n\t"
               "ds_read_b64_tr_b16 %1, %8 offset:%12\n\t"
               "ds_read_b64_tr_b16 %2, %9\n\t"
               "ds_read_b64_tr_b16 %3, %9 offset:%12\n\t"
               "ds_read_b64_tr_b16 %4, %10\n\t"
               "ds_read_b64_tr_b16 %5, %10 offset:%12\n\t"
               "ds_read_b64_tr_b16 %6, %11\n\t"
               "ds_read_b64_tr_b16 %7, %11 offset:%12\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]),
                 "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7])
               : "v"(base + (((db0 + 0) ^ sw) << 5)),
                 "v"(base + (((db0 + 1) ^ sw) << 5)),
                 "v"(base + (((db0 + 2) ^ sw) << 5)),
                 "v"(base + (((db0 + 3) ^ sw) << 5)), "i"(16 * RB)
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) vt[j] = fa_join(x[2 * j], x[2 * j + 1]);
}

}  // namespace
