// Flash-attention 2 forward, 8-wave 32x32-MFMA structure for gfx950.
//
// Replaces the reference's vendored CUTLASS flash-attn fwd
// (hetu/impl/kernel/FlashAttention.cu) with the CDNA4-native design from the
// MI355X kernel playbook (cdna_hip_programming.md Appendix B):
//  * 8 waves x 32 q-rows (BM=256), KV tiles of 64, mfma_f32_32x32x16_bf16.
//  * swapped QK^T: S^T = mfma(K, Q) puts a full P-row in each lane's
//    registers (col = lane&31 = q) -> softmax entirely in-register, the
//    only cross-lane step is a lane<->lane+32 half exchange.
//  * P -> bf16 A-fragments via cvt_pk + permlane32 swap (fa_pack_frag)
//    (no P round-trip through LDS).
//  * PV swapped too: O^T += mfma(V^T, P) keeps the softmax statistics
//    lane-local for the O rescale.
//  * K in LDS row-major XOR-swizzled (conflict-free ds_read_b128);
//    V in [32key][16d] subtiles consumed by the tr_b16 read (fa_tr_v4, the
//    4x4 hardware transpose read).
//  * register staging (T14): issue next tile's global loads before compute,
//    ds_write after the barrier; double-buffered LDS.
#include <torch/extension.h>
#include "ext_stream.h"
#include "attention_common.h"

namespace {

constexpr int BM = 256;       // q rows per workgroup (8 waves x 32)
constexpr int BN = 64;        // kv tile
constexpr int THREADS = FA_THREADS;   // one wave per 32 q rows
constexpr int NGLDS = FA_KV_IMG / (THREADS * 16);  // glds per lane per image
constexpr int NBUF = FA_RING; // KV ring depth (counted-vmcnt pipelining)

template <int D>  // D = head dim (128)
// 96 KiB LDS -> one workgroup per CU regardless; a 2-block register cap
// would only force tighter allocation for a block that cannot schedule
__global__ __launch_bounds__(THREADS, 1) void fa2_fwd_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O,
    float* __restrict__ LSE, int B, int H, int Hkv, int S, int Skv,
    float scale, bool causal, FaStrides sq, FaStrides skv, FaStrides so,
    const int* __restrict__ cu, int lse_T, bool mask_all) {
  static_assert(D == 128, "fa2 fwd: D=128 only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int b) -> char* { return smem + b * FA_KV_IMG; };
  auto v_lds = [&](int b) -> char* { return smem + (NBUF + b) * FA_KV_IMG; };

  // grid is (bh, q-block): consecutive blockIdx.x (-> XCD b%8 placement)
  // walk bh, so every CU samples ALL causal depths — with (q-block, bh)
  // each CU aliased onto ONE depth and causal ran as slow as non-causal
  const int bh = blockIdx.x;
  const int h = bh % H;
  const int b = bh / H;
  const int hkv = h / (H / Hkv);
  const int q0 = blockIdx.y * BM;
  // packed-varlen mode (reference mha_varlen_fwd): blockIdx "batch" is a
  // SEGMENT of the packed [T, H, D] layout; segment bounds come from the
  // device-side cu_seqlens — one launch covers every ragged segment, no
  // host loop, no host sync.
  int row0 = 0;
  if (cu != nullptr) {
    row0 = cu[b];
    S = cu[b + 1] - row0;
    Skv = S;
    if (q0 >= S) return;        // ragged tail tile of a shorter segment
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;      // this lane's q row within the wave block
  const int hi = lane >> 5;

  const int64_t qb_off = cu ? (int64_t)row0 * sq.rs : (int64_t)b * sq.bs;
  const int64_t kb_off = cu ? (int64_t)row0 * skv.rs
                            : (int64_t)b * skv.bs;
  const bf16* Qb = Q + qb_off + (int64_t)h * sq.hs;
  const bf16* Kb = K + kb_off + (int64_t)hkv * skv.hs;
  const bf16* Vb = V + kb_off + (int64_t)hkv * skv.hs;

  const int my_q = q0 + wid * 32 + iq;          // global q row (this lane)
  const int diag = Skv - S;                     // causal offset

  // ---- Q -> registers, prescaled by softmax scale --------------------
  // lane holds Q[my_q][16*kk + 8*hi .. +8) for kk = 0..7
  bf16x8 qreg[8];
  fa_load_row_frags(qreg, Qb + (int64_t)min(my_q, S - 1) * sq.rs, hi, scale);

  // ---- staging: global_load_lds DMA, swizzle folded into the SOURCE
  // address (rule 21: glds writes lane-linear, dest = base + lane*16).
  // Per tile: 16 KiB K + 16 KiB V = 16+16 glds instructions; each wave
  // issues 2 K + 2 V (1 KiB each).  For linear byte position `pos` in the
  // tile image, the source element is the inverse of the LDS layout:
  //   K (row-major [64][256B], XOR swizzle): row = pos>>8,
  //     bytecol = (pos&255) ^ ((row&15)<<4), d = bytecol>>1
  //   V ([kb][db] subtiles of [32key][16d]): subtile = pos>>10,
  //     key = (subtile>>3)*32 + ((pos>>5)&31),
  //     d = (subtile&7)*16 + ((pos>>4)&1)*8
  const int wlane16 = lane * 16;
#define ISSUE_GLDS(k0, buf)                                                 \
  do {                                                                      \
    _Pragma("unroll")                                                       \
    for (int i = 0; i < NGLDS; ++i) {                                       \
      int pos = (wid * NGLDS + i) * 1024 + wlane16;                         \
      fa_glds16(Kb + (int64_t)min((k0) + (pos >> 8), Skv - 1) * skv.rs      \
                    + fa_rm_src_col(pos),                                   \
                k_lds(buf) + pos);                                          \
      int st = pos >> 10;                                                   \
      int vkey = (st >> 3) * 32 + ((pos >> 5) & 31);                        \
      int vd = (st & 7) * 16 + ((pos >> 4) & 1) * 8;                        \
      fa_glds16(Vb + (int64_t)min((k0) + vkey, Skv - 1) * skv.rs + vd,      \
                v_lds(buf) + pos);                                          \
    }                                                                       \
  } while (0)

  // ---- accumulators ---------------------------------------------------
  f32x16 o_acc[4];                 // O^T[32*dt + crow(reg,hi)][q = iq]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] = 0.f;
  float m_i = -INFINITY, l_i = 0.f;

  const int wave_qmax = q0 + wid * 32 + 31;
  const int n_tiles = fa_n_kv_tiles(q0, Skv, diag, causal);

  // prologue: tiles 0 and 1 in flight (3-deep ring, counted vmcnt:
  // per wave each tile is 2*NGLDS glds; waiting vmcnt(2*NGLDS) at the
  // loop head means "tile t landed, tile t+1 still flying" — the DMA for
  // t+2 then issues after the barrier and lands under two tiles of MFMAs)
  ISSUE_GLDS(0, 0);
  // the counted wait below assumes a full tile's loads may trail behind
  // the newest ISSUE; with a single tile, issue a harmless duplicate so
  // tile 0 is guaranteed landed when its compute starts
  if (n_tiles > 1) ISSUE_GLDS(BN, 1);
  else ISSUE_GLDS(0, 1);

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * BN;
    const int cur = t % NBUF;
    fa_wait_tile<2 * NGLDS>(t + 1 >= n_tiles);
    __builtin_amdgcn_s_barrier();
    if (t + 2 < n_tiles) ISSUE_GLDS(k0 + 2 * BN, (t + 2) % NBUF);

    // does this wave have any unmasked key in this tile?
    const bool active = !causal || (k0 <= wave_qmax + diag);

    float p[2][16];                // P^T rows: p[ct][r] = P[q][32ct+crow]
    // mask + online softmax over p (all in-register; q = iq lane-local),
    // returns the O rescale.  MASK=false (interior tiles, see
    // fa_boundary_kv_tile) has no key index, no compare and no select
    // around exp; only this stage exists twice, the MFMA phases once.
    auto softmax = [&](auto mask_c) -> float {
      constexpr bool MASK = decltype(mask_c)::value;
      float pmax = -INFINITY;
      int bound = 0;
      if constexpr (MASK)
        bound = fa_mask_bound(k0 + 4 * hi, my_q, S, Skv, diag, causal);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if constexpr (MASK)
            if (32 * ct + fa_crow(r) > bound) p[ct][r] = -INFINITY;
          pmax = fmaxf(pmax, p[ct][r]);
        }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));
      float mn = fmaxf(m_i, pmax);
      float alpha = (m_i == -INFINITY || mn == -INFINITY)
                        ? ((m_i == -INFINITY) ? 0.f : 1.f)
                        : __expf(m_i - mn);
      m_i = mn;
      float psum = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pv;
          if constexpr (MASK)
            pv = (p[ct][r] == -INFINITY || mn == -INFINITY)
                     ? 0.f : __expf(p[ct][r] - mn);
          else
            pv = __expf(p[ct][r] - mn);
          p[ct][r] = pv;
          psum += pv;
        }
      psum += __shfl_xor(psum, 32, 64);
      l_i = l_i * alpha + psum;
      return alpha;
    };
    if (active) {
      // ---- S^T = K Q^T ------------------------------------------------
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          // A-frag: K rows 32*ct + (lane&31), d slice 16kk + 8hi..+8
          bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              k_lds(cur) + fa_swz_rm(32 * ct + iq, kk * 32 + hi * 16));
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qreg[kk], acc,
                                                        0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) p[ct][r] = acc[r];
      }

      const float alpha =
          fa_boundary_kv_tile(wave_qmax - 31, k0, S, Skv, diag, causal,
                              mask_all)
              ? softmax(std::true_type{}) : softmax(std::false_type{});
      // rescale O^T
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[dt][r] *= alpha;

      // ---- P -> bf16 A-fragments (cvt_pk + permlane32_swap), fused with
      // PV so only ONE pfrag is live at a time (register pressure).
      // frag[ks] (ks = key slot of 16): lane needs P[q][16ks + 8hi + j],
      // j = 0..7, as 4 u32 words.  O^T += mfma(Vfrag, Pfrag):
      // Vfrag(dt, ks): lane row d = 32dt + iq, k = key 16ks + 8hi + j via
      // the tr_b16 read: each 4-lane cluster reads a [4 key][4 d] tile;
      // lane (4c + j) supplies &V[key_base + j][d_base(cluster)] (8 B,
      // 4 contiguous d), lane (4c + k) receives column k = its own d.
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 pfrag = fa_pack_frag(p[ks >> 1], (ks & 1) * 8);
        bf16x8 vf[4];
        fa_tr_v4(vf, v_lds(cur), ks, lane);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              vf[dt], pfrag, o_acc[dt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue -------------------------------------------------------
  if (my_q < S) {
    float inv = (l_i > 0.f) ? 1.f / l_i : 0.f;
    bf16* orow = O + (cu ? (int64_t)row0 * so.rs : (int64_t)b * so.bs)
                 + (int64_t)h * so.hs + (int64_t)my_q * so.rs;
    fa_store_row_bf16(o_acc, inv, orow, hi);
    if (hi == 0) {
      int64_t li = cu ? ((int64_t)h * lse_T + row0 + my_q)
                      : ((int64_t)bh * S + my_q);
      LSE[li] = (l_i > 0.f) ? m_i + __logf(l_i) : -INFINITY;
    }
  }
}

}  // namespace

void fa2_fwd_launch(const bf16* q, const bf16* k, const bf16* v, bf16* o,
                    float* lse, int B, int H, int Hkv, int S, int Skv,
                    float scale, bool causal, FaStrides sq, FaStrides skv,
                    FaStrides so, const int* cu, int lse_T,
                    hipStream_t stream) {
  const bool mask_all = fa_mask_all();
  dim3 grid(B * H, (S + BM - 1) / BM);
  hipLaunchKernelGGL(fa2_fwd_kernel<128>, grid, dim3(THREADS), FA_FWD_LDS,
                     stream, q, k, v, o, lse, B, H, Hkv, S, Skv, scale,
                     causal, sq, skv, so, cu, lse_T, mask_all);
}

// Packed-varlen entry (reference FlashAttention.cu mha_varlen_fwd): ONE
// kernel launch over all ragged segments; q/k/v [T, H, D] packed, cu
// int32 [nseg+1] on DEVICE.  Returns (o [T, H, D], lse [H, T] fp32).
std::vector<torch::Tensor> flash_attn_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor cu,
    int64_t max_seqlen, bool causal, double scale) {
  TORCH_CHECK(q.dim() == 3 && q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous(), "varlen: q/k/v [T, H, D] contiguous");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "varlen: bf16 only");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.is_cuda() &&
              cu.is_contiguous(), "varlen: cu int32 on device");
  const int T = q.size(0), H = q.size(1), D = q.size(2);
  const int Hkv = k.size(1);
  TORCH_CHECK(D == 128, "fa2 varlen: D=128 only");
  const int nseg = cu.numel() - 1;
  auto o = torch::empty_like(q);
  auto lse = torch::empty({H, (int64_t)T},
                          q.options().dtype(at::kFloat));
  FaStrides sq{0, (int64_t)D, (int64_t)H * D};
  FaStrides skv{0, (int64_t)D, (int64_t)Hkv * D};
  fa2_fwd_launch((const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
                 (const bf16*)v.data_ptr(), (bf16*)o.data_ptr(),
                 lse.data_ptr<float>(), nseg, H, Hkv, (int)max_seqlen,
                 (int)max_seqlen, (float)scale, causal, sq, skv, sq,
                 cu.data_ptr<int>(), T, hetu_current_stream());
  return {o, lse};
}

// Fused-QKV entry: qkv [B, S, (H+2*Hkv)*D] straight from the column-
// parallel GEMM (q|k|v interleaved per token); no slice/transpose copies.
// Returns (o [B, S, H*D], lse [B, H, S]).
std::vector<torch::Tensor> flash_attn_fwd_qkv(torch::Tensor qkv, int64_t H,
                                              int64_t Hkv, int64_t D,
                                              bool causal, double scale) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous());
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "fa2 qkv: bf16 only");
  TORCH_CHECK(D == 128, "fa2 qkv: D=128 only");
  const int B = qkv.size(0), S = qkv.size(1);
  const int64_t C = (H + 2 * Hkv) * D;
  TORCH_CHECK(qkv.size(2) == C, "qkv width mismatch");
  auto o = torch::empty({B, (int64_t)S, H * D}, qkv.options());
  auto lse = torch::empty({B, H, S}, qkv.options().dtype(at::kFloat));
  const bf16* base = (const bf16*)qkv.data_ptr();
  FaStrides sqkv{(long long)S * C, (long long)D, (long long)C};
  FaStrides so{(long long)S * H * D, (long long)D, (long long)H * D};
  fa2_fwd_launch(base, base + H * D, base + (H + Hkv) * D,
                 (bf16*)o.data_ptr(), lse.data_ptr<float>(), B, H, Hkv, S, S,
                 (float)scale, causal, sqkv, sqkv, so, nullptr, 0,
                 hetu_current_stream());
  return {o, lse};
}
