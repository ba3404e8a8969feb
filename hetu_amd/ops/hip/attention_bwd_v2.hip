// Flash-attention 2 backward, 8-wave 32x32-MFMA structure for gfx950:
// the stride-aware generation (dense BHSD with GQA, fused-qkv, packed
// varlen).
//
// Two atomics-free kernels (the standard FA2 split; reference relied on
// vendored CUTLASS kernels — this is a from-scratch CDNA4 design):
//  * dq kernel: grid over q-blocks (8 waves x 32 q); K/V tiles stream
//    through LDS exactly like the fa2 forward; dS is rebuilt from the saved
//    lse and packed in-register (cvt_pk + permlane32_swap) into MFMA
//    B-fragments; dQ^T accumulates in registers, stores like the fwd O.
//  * dkv kernel: grid over kv-blocks (8 waves x 32 keys, keys exclusive per
//    wave); Q/dO tiles stream through LDS; P^T/dS^T round-trip through tiny
//    per-wave 72B-row LDS images consumed by tr_b16 transpose reads; dK/dV
//    accumulate in registers; plain stores (atomicAdd only under GQA).
// This file holds the skeletons (addressing, 2-buffer staging that drains
// vmcnt(0) every tile, epilogues); the per-tile compute bodies and every
// layout primitive are in attention_common.h, shared with
// attention_bwd_v3.hip.
#include <torch/extension.h>
#include "ext_stream.h"
#include "attention_common.h"

namespace {

constexpr int THREADS = FA_THREADS;

// ===========================================================================
// dq kernel: 8 waves x 32 q rows; loops over 64-key KV tiles.
// ===========================================================================
// VARLEN: packed [T, H(kv), D] layout, blockIdx.x = seg * H + h, segment
// bounds from the device-side cu_seqlens (same contract as the fa2 forward's
// varlen mode); LSE/DELTA are [H, lse_T].  A template flag, not a runtime
// branch, so the dense / fused-qkv instantiation compiles exactly as before.
template <int D, bool VARLEN>
__global__ __launch_bounds__(THREADS, 2) void fa2_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dQ, int B, int H, int Hkv, int S, int Skv,
    float scale, bool causal, FaStrides sq, FaStrides skv, FaStrides sdo,
    FaStrides sdq, const int* __restrict__ cu, int lse_T, bool mask_all) {
  static_assert(D == 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int b) -> char* { return smem + b * FA_KV_IMG; };
  auto v_lds = [&](int b) -> char* { return smem + (2 + b) * FA_KV_IMG; };

  // (bh, q-block) grid: spreads causal depths across CUs (see fwd note)
  const int bh = blockIdx.x;
  const int h = bh % H;
  const int b = bh / H;
  const int hkv = h / (H / Hkv);
  const int q0 = blockIdx.y * 256;
  int row0 = 0;
  if constexpr (VARLEN) {
    // b is the SEGMENT; block-uniform exit for empty segments and ragged
    // tail tiles, before any load, clamp or barrier
    row0 = cu[b];
    S = cu[b + 1] - row0;
    Skv = S;
    if (q0 >= S) return;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;
  const int hi = lane >> 5;

  const bf16* Qb = Q + (VARLEN ? (int64_t)row0 * sq.rs : (int64_t)b * sq.bs)
                 + (int64_t)h * sq.hs;
  const bf16* dOb = dO
      + (VARLEN ? (int64_t)row0 * sdo.rs : (int64_t)b * sdo.bs)
      + (int64_t)h * sdo.hs;
  const int64_t kb_off = VARLEN ? (int64_t)row0 * skv.rs
                                : (int64_t)b * skv.bs;
  const bf16* Kb = K + kb_off + (int64_t)hkv * skv.hs;
  const bf16* Vb = V + kb_off + (int64_t)hkv * skv.hs;

  const int my_q = q0 + wid * 32 + iq;
  const int diag = Skv - S;
  // LSE/DELTA rows: dense [B, H, S]; varlen [H, lse_T] at packed row
  const int64_t stat0 = VARLEN ? ((int64_t)h * lse_T + row0)
                               : ((int64_t)bh * S);
  const float lse_q = LSE[stat0 + min(my_q, S - 1)];
  const float del_q = DELTA[stat0 + min(my_q, S - 1)];

  // Q (scaled) and dO in registers
  bf16x8 qreg[8], doreg[8];
  fa_load_row_frags(qreg, Qb + (int64_t)min(my_q, S - 1) * sq.rs, hi, scale);
  fa_load_row_frags(doreg, dOb + (int64_t)min(my_q, S - 1) * sdo.rs, hi);

  const int wlane16 = lane * 16;
#define DQ_GLDS(k0, buf)                                                    \
  do {                                                                      \
    _Pragma("unroll")                                                       \
    for (int i = 0; i < 2; ++i) {                                           \
      int pos = (wid * 2 + i) * 1024 + wlane16;                             \
      int64_t roff = (int64_t)min((k0) + (pos >> 8), Skv - 1) * skv.rs      \
                   + fa_rm_src_col(pos);                                    \
      fa_glds16(Kb + roff, k_lds(buf) + pos);                               \
      fa_glds16(Vb + roff, v_lds(buf) + pos);                               \
    }                                                                       \
  } while (0)

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const int wave_qmax = q0 + wid * 32 + 31;
  const int n_tiles = fa_n_kv_tiles(q0, Skv, diag, causal);

  DQ_GLDS(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * 64;
    const int cur = t & 1;
    const bool have_next = (t + 1) < n_tiles;
    if (have_next) DQ_GLDS(k0 + 64, cur ^ 1);

    const bool active = !causal || (k0 <= wave_qmax + diag);
    if (active) {
      const bool boundary = fa_boundary_kv_tile(wave_qmax - 31, k0, S, Skv,
                                                diag, causal, mask_all);
      FA_BWD_DQ_TILE(boundary, k_lds(cur), v_lds(cur), qreg, doreg, dq_acc,
                     k0, my_q, S, Skv, diag, causal, lse_q, del_q, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef DQ_GLDS

  // ---- epilogue: dQ[my_q][d] = scale * dq^T[d][my_q] -------------------
  if (my_q < S) {
    bf16* qrow = dQ
        + (VARLEN ? (int64_t)row0 * sdq.rs : (int64_t)b * sdq.bs)
        + (int64_t)h * sdq.hs + (int64_t)my_q * sdq.rs;
    fa_store_row_bf16(dq_acc, scale, qrow, hi);
  }
}

// ===========================================================================
// dkv kernel: 8 waves x 32 keys (exclusive); loops over 32-q tiles.
// ===========================================================================
template <int D, bool VARLEN>   // VARLEN: see fa2_bwd_dq_kernel
// 132 KiB LDS -> occupancy 1 by LDS; see the fwd note on launch bounds
__global__ __launch_bounds__(THREADS, 1) void fa2_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    float* __restrict__ dK32, float* __restrict__ dV32,
    bf16* __restrict__ dK16, bf16* __restrict__ dV16,
    int B, int H, int Hkv, int S, int Skv, float scale, bool causal,
    FaStrides sq, FaStrides skv, FaStrides sdo, FaStrides sdkv,
    const int* __restrict__ cu, int lse_T) {
  static_assert(D == 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto q_lds = [&](int b) -> char* { return smem + b * FA_Q_IMG; };
  auto do_lds = [&](int b) -> char* { return smem + (2 + b) * FA_Q_IMG; };
  char* vw_base = smem + 4 * FA_Q_IMG;             // per-wave V images
  char* pw_base = vw_base + 8 * FA_WAVE_V_IMG;     // per-wave P'/dS' pairs

  // (bh, kv-block) grid: spreads causal depths across CUs (see fwd note)
  const int bh = blockIdx.x;
  const int h = bh % H;
  const int b = bh / H;
  const int hkv = h / (H / Hkv);
  const int kb0 = blockIdx.y * 256;
  int row0 = 0;
  if constexpr (VARLEN) {
    // b is the SEGMENT; block-uniform exit before any load or barrier
    row0 = cu[b];
    S = cu[b + 1] - row0;
    Skv = S;
    if (kb0 >= Skv) return;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;        // here: own q-col index AND own key row
  const int hi = lane >> 5;

  const bf16* Qb = Q + (VARLEN ? (int64_t)row0 * sq.rs : (int64_t)b * sq.bs)
                 + (int64_t)h * sq.hs;
  const bf16* dOb = dO
      + (VARLEN ? (int64_t)row0 * sdo.rs : (int64_t)b * sdo.bs)
      + (int64_t)h * sdo.hs;
  const int64_t kb_off = VARLEN ? (int64_t)row0 * skv.rs
                                : (int64_t)b * skv.bs;
  const bf16* Kb = K + kb_off + (int64_t)hkv * skv.hs;
  const bf16* Vb = V + kb_off + (int64_t)hkv * skv.hs;
  const int64_t stat0 = VARLEN ? ((int64_t)h * lse_T + row0)
                               : ((int64_t)bh * S);
  const float* lse_b = LSE + stat0;
  const float* del_b = DELTA + stat0;

  const int wave_kmin = kb0 + wid * 32;        // first key this wave owns
  const int my_key = wave_kmin + iq;           // lane's exclusive key row
  const int diag = Skv - S;

  char* vw_lds = vw_base + wid * FA_WAVE_V_IMG;
  char* p_lds = pw_base + wid * 2 * FA_P_IMG;

  // K (scaled) in registers; V in a per-wave swizzled row-major LDS image
  // (keeps the VGPR budget at 2 waves/SIMD without spills)
  bf16x8 kreg[8];
  fa_load_row_frags(kreg, Kb + (int64_t)min(my_key, Skv - 1) * skv.rs, hi,
                    scale);
  fa_stage_wave_v(Vb, skv.rs, wave_kmin, Skv, vw_lds, lane);

  // per tile: Qrm 8 KiB + dOrm 8 KiB; 512 lanes x 16 B covers 8 KiB, so one
  // glds per lane per image.
#define DKV_GLDS(qt0, buf)                                                  \
  do {                                                                      \
    int pos = tid * 16;                                                     \
    int qr_ = min((qt0) + (pos >> 8), S - 1);                               \
    int qd = fa_rm_src_col(pos);                                            \
    fa_glds16(Qb + (int64_t)qr_ * sq.rs + qd, q_lds(buf) + pos);            \
    fa_glds16(dOb + (int64_t)qr_ * sdo.rs + qd, do_lds(buf) + pos);         \
  } while (0)

  f32x16 dk_acc[4], dv_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk_acc[dt][r] = 0.f; dv_acc[dt][r] = 0.f; }

  const int n_q_tiles = (S + 31) / 32;
  const int t_start = fa_first_q_tile(kb0, diag, causal);

  DKV_GLDS(t_start * 32, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = t_start; t < n_q_tiles; ++t) {
    const int qt0 = t * 32;
    const int cur = (t - t_start) & 1;
    const bool have_next = (t + 1) < n_q_tiles;
    if (have_next) DKV_GLDS(qt0 + 32, cur ^ 1);

    // wave active if any of its keys can see this q tile
    const bool active = !causal || (qt0 + 31 >= wave_kmin - diag);
    if (active)
      fa_bwd_dkv_tile(q_lds(cur), do_lds(cur), vw_lds, p_lds, kreg, dk_acc,
                      dv_acc, qt0, wave_kmin, S, Skv, diag, causal, lse_b,
                      del_b, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef DKV_GLDS

  // ---- epilogue: dK = scale * acc; plain stores unless GQA -------------
  const bool gqa = (H != Hkv);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int key = wave_kmin + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (key < Skv) {
        float dkv_ = dk_acc[dt][r] * scale;
        float dvv_ = dv_acc[dt][r];
        if (gqa) {
          // f32 accumulation buffers: BHSD-contiguous (dense) or packed
          // [T, Hkv, D] (varlen)
          int64_t off32 =
              (VARLEN ? ((int64_t)(row0 + key) * Hkv + hkv)
                      : ((int64_t)(b * Hkv + hkv) * Skv + key)) * D
              + 32 * dt + iq;
          atomicAdd(dK32 + off32, dkv_);
          atomicAdd(dV32 + off32, dvv_);
        } else {
          int64_t off =
              (VARLEN ? (int64_t)row0 * sdkv.rs : (int64_t)b * sdkv.bs)
              + (int64_t)hkv * sdkv.hs + (int64_t)key * sdkv.rs
              + 32 * dt + iq;
          dK16[off] = (bf16)dkv_;
          dV16[off] = (bf16)dvv_;
        }
      }
    }
  }
}

// delta = rowsum(dO * O)
__global__ void fa2_delta_kernel(const bf16* __restrict__ dO,
                                 const bf16* __restrict__ O,
                                 float* __restrict__ delta,
                                 int64_t rows, int D, int H, int S,
                                 FaStrides so) {
  // delta rows are LSE-ordered (b, h, s); dO/O may be BHSD or BS[HD]
  // D == 128 fast path: 4 lanes per row (32 elems each, 16B vector
  // loads), quad shuffle reduction — pure bandwidth (the old one-block-
  // per-row version left 240/256 lanes idle: 580us vs the ~65us bound).
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (D == 128) {
    int64_t row = tid >> 2;
    const int q = tid & 3;
    const int64_t rstride = ((int64_t)gridDim.x * blockDim.x) >> 2;
    for (; row < rows; row += rstride) {
      const int64_t b = row / ((int64_t)H * S);
      const int64_t hh = (row / S) % H;
      const int64_t ss = row % S;
      const int64_t base = b * so.bs + hh * so.hs + ss * so.rs + q * 32;
      const bf16* a = dO + base;
      const bf16* bb = O + base;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 32; i += 8) {
        float av[8], bv[8];
        VecIO<bf16>::load(a + i, av);
        VecIO<bf16>::load(bb + i, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += av[j] * bv[j];
      }
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      if (q == 0) delta[row] = s;
    }
    return;
  }
  // generic fallback: one lane per row, scalar loads
  for (int64_t row = tid; row < rows;
       row += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = row / ((int64_t)H * S);
    const int64_t hh = (row / S) % H;
    const int64_t ss = row % S;
    const int64_t base = b * so.bs + hh * so.hs + ss * so.rs;
    const bf16* a = dO + base;
    const bf16* bb = O + base;
    float s = 0.f;
    for (int i = 0; i < D; ++i) s += (float)a[i] * (float)bb[i];
    delta[row] = s;
  }
}

template <bool VARLEN>
void fa2_bwd_kernels(const bf16* doutp, const bf16* qp, const bf16* kp,
                     const bf16* vp, const float* lse, const float* delta,
                     bf16* dqp, bf16* dk16p, bf16* dv16p, float* dk32p,
                     float* dv32p, int B, int H, int Hkv, int S, int Skv,
                     bool causal, float scale, FaStrides sq, FaStrides skv,
                     FaStrides sdo, FaStrides sdq, FaStrides sdkv,
                     const int* cu, int lse_T, hipStream_t stream) {
  const bool mask_all = fa_mask_all();
  hipLaunchKernelGGL((fa2_bwd_dq_kernel<128, VARLEN>),
                     dim3(B * H, (S + 255) / 256), dim3(THREADS), FA2_DQ_LDS,
                     stream, qp, kp, vp, doutp, lse, delta, dqp, B, H, Hkv,
                     S, Skv, scale, causal, sq, skv, sdo, sdq, cu, lse_T,
                     mask_all);
  hipLaunchKernelGGL((fa2_bwd_dkv_kernel<128, VARLEN>),
                     dim3(B * H, (Skv + 255) / 256), dim3(THREADS),
                     FA_DKV_LDS, stream, qp, kp, vp, doutp, lse, delta,
                     dk32p, dv32p, dk16p, dv16p, B, H, Hkv, S, Skv, scale,
                     causal, sq, skv, sdo, sdkv, cu, lse_T);
}

// delta + dq + dkv over arbitrary layouts.  Exactly one of the (dk16p,
// dv16p) / (dk32p, dv32p) pairs is non-null: bf16 plain stores, or fp32
// atomic accumulators under GQA.  cu != nullptr is the packed-varlen mode:
// B counts segments, S = Skv = max_seqlen only size the grid (the kernels
// read the real bounds from cu), and lse / delta are [H, lse_T].
void fa2_bwd_core(const bf16* doutp, const bf16* qp, const bf16* kp,
                  const bf16* vp, const bf16* outp, torch::Tensor lse,
                  int B, int H, int Hkv, int S, int Skv, int D, bool causal,
                  float scale, FaStrides sq, FaStrides skv, FaStrides sdo,
                  bf16* dqp, bf16* dk16p, bf16* dv16p, float* dk32p,
                  float* dv32p, FaStrides sdq, FaStrides sdkv,
                  const int* cu, int lse_T) {
  auto stream = hetu_current_stream();
  // varlen: [1, H, T] from packed dO/O, the dense kernel with B=1, S=T
  const int delta_S = cu ? lse_T : S;
  const int64_t rows = (int64_t)(cu ? 1 : B) * H * delta_S;
  auto delta = torch::empty({rows}, lse.options());
  fa_delta_launch(doutp, outp, delta.data_ptr<float>(), rows, D, H, delta_S,
                  sdo, stream);
  auto launch = cu ? fa2_bwd_kernels<true> : fa2_bwd_kernels<false>;
  launch(doutp, qp, kp, vp, lse.data_ptr<float>(), delta.data_ptr<float>(),
         dqp, dk16p, dv16p, dk32p, dv32p, B, H, Hkv, S, Skv, causal, scale,
         sq, skv, sdo, sdq, sdkv, cu, lse_T, stream);
}

// dK/dV outputs of one backward call: bf16 written in place, or fp32
// atomic accumulators under GQA that finish() rounds to the input dtype
struct DkvBuffers {
  torch::Tensor dk16, dv16, dk32, dv32;
  DkvBuffers(const torch::Tensor& k, const torch::Tensor& v, bool gqa,
             bool zero16) {
    if (gqa) {
      dk32 = torch::zeros_like(k, k.options().dtype(at::kFloat));
      dv32 = torch::zeros_like(v, v.options().dtype(at::kFloat));
    } else {
      dk16 = zero16 ? torch::zeros_like(k) : torch::empty_like(k);
      dv16 = zero16 ? torch::zeros_like(v) : torch::empty_like(v);
    }
  }
  bf16* k16() { return dk16.defined() ? (bf16*)dk16.data_ptr() : nullptr; }
  bf16* v16() { return dv16.defined() ? (bf16*)dv16.data_ptr() : nullptr; }
  float* k32() { return dk32.defined() ? dk32.data_ptr<float>() : nullptr; }
  float* v32() { return dv32.defined() ? dv32.data_ptr<float>() : nullptr; }
  std::vector<torch::Tensor> finish(torch::Tensor dq, at::ScalarType t) {
    if (dk32.defined()) return {dq, dk32.to(t), dv32.to(t)};
    return {dq, dk16, dv16};
  }
};

}  // namespace

void fa_delta_launch(const bf16* dO, const bf16* O, float* delta,
                     int64_t rows, int D, int H, int S, FaStrides so,
                     hipStream_t stream) {
  int grid = (int)std::min<int64_t>((rows * 4 + 255) / 256, 16384);
  hipLaunchKernelGGL(fa2_delta_kernel, dim3(grid), dim3(256), 0, stream,
                     dO, O, delta, rows, D, H, S, so);
}

std::vector<torch::Tensor> fa2_bwd_launch(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, bool causal, double scale) {
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hkv = k.size(1), Skv = k.size(2);
  auto dq = torch::empty_like(q);
  DkvBuffers d(k, v, H != Hkv, false);
  FaStrides sq{(long long)H * S * D, (long long)S * D, (long long)D};
  FaStrides skv{(long long)Hkv * Skv * D, (long long)Skv * D,
                (long long)D};
  fa2_bwd_core((const bf16*)dout.data_ptr(), (const bf16*)q.data_ptr(),
               (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
               (const bf16*)out.data_ptr(), lse, B, H, Hkv, S, Skv, D,
               causal, (float)scale, sq, skv, sq, (bf16*)dq.data_ptr(),
               d.k16(), d.v16(), d.k32(), d.v32(), sq, skv, nullptr, 0);
  return d.finish(dq, k.scalar_type());
}

// Packed-varlen backward (analogue of flash_attn_varlen_fwd): delta + dq +
// dkv, ONE launch each over all ragged segments; dout/q/k/v/out [T, H(kv), D]
// packed, lse [H, T] fp32, cu int32 [nseg+1] on DEVICE — no host sync.
// max_seqlen only sizes the grid and must be >= the longest segment.
// Rows outside every segment (t >= cu[-1]) come back zero.
std::vector<torch::Tensor> flash_attn_varlen_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, torch::Tensor cu,
    int64_t max_seqlen, bool causal, double scale) {
  TORCH_CHECK(q.dim() == 3 && q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous(), "varlen: q/k/v [T, H, D] contiguous");
  TORCH_CHECK(dout.is_contiguous() && out.is_contiguous() &&
              dout.sizes() == q.sizes() && out.sizes() == q.sizes(),
              "varlen: dout/out [T, H, D] contiguous");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
              k.scalar_type() == at::kBFloat16 &&
              v.scalar_type() == at::kBFloat16 &&
              dout.scalar_type() == at::kBFloat16 &&
              out.scalar_type() == at::kBFloat16, "varlen: bf16 only");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.is_cuda() &&
              cu.is_contiguous(), "varlen: cu int32 on device");
  const int T = q.size(0), H = q.size(1), D = q.size(2);
  const int Hkv = k.size(1);
  TORCH_CHECK(D == 128, "fa2 varlen: D=128 only");
  TORCH_CHECK(k.dim() == 3 && k.size(0) == T && k.size(2) == D &&
              v.sizes() == k.sizes() && Hkv > 0 && H % Hkv == 0,
              "varlen: k/v [T, Hkv, D]");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.dim() == 2 && lse.size(0) == H && lse.size(1) == T,
              "varlen: lse [H, T] fp32");
  const int nseg = cu.numel() - 1;
  // zero-filled: rows past cu[-1] belong to no segment and no block
  auto dq = torch::zeros_like(q);
  DkvBuffers d(k, v, H != Hkv, true);
  if (nseg > 0 && T > 0 && max_seqlen > 0) {
    FaStrides sq{0, (long long)D, (long long)H * D};
    FaStrides skv{0, (long long)D, (long long)Hkv * D};
    fa2_bwd_core((const bf16*)dout.data_ptr(), (const bf16*)q.data_ptr(),
                 (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                 (const bf16*)out.data_ptr(), lse, nseg, H, Hkv,
                 (int)max_seqlen, (int)max_seqlen, D, causal, (float)scale,
                 sq, skv, sq, (bf16*)dq.data_ptr(), d.k16(), d.v16(),
                 d.k32(), d.v32(), sq, skv, cu.data_ptr<int>(), T);
  }
  return d.finish(dq, k.scalar_type());
}

// Fused-QKV backward: dout/out [B,S,H*D], qkv [B,S,(H+2Hkv)*D] ->
// dqkv [B,S,(H+2Hkv)*D] written in place by the kernels (no slice or
// transpose copies).
torch::Tensor flash_attn_bwd_qkv(torch::Tensor dout, torch::Tensor qkv,
                                 torch::Tensor out, torch::Tensor lse,
                                 int64_t H, int64_t Hkv, int64_t D,
                                 bool causal, double scale) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous());
  TORCH_CHECK(dout.is_contiguous() && out.is_contiguous());
  const int B = qkv.size(0), S = qkv.size(1);
  const int64_t C = (H + 2 * Hkv) * D;
  const bool gqa = (H != Hkv);
  auto dqkv = torch::empty_like(qkv);
  torch::Tensor dk32, dv32;
  float *dk32p = nullptr, *dv32p = nullptr;
  if (gqa) {
    dk32 = torch::zeros({B, Hkv, (int64_t)S, D},
                        qkv.options().dtype(at::kFloat));
    dv32 = torch::zeros_like(dk32);
    dk32p = dk32.data_ptr<float>();
    dv32p = dv32.data_ptr<float>();
  }
  FaStrides sqkv{(long long)S * C, (long long)D, (long long)C};
  FaStrides so{(long long)S * H * D, (long long)D, (long long)H * D};
  const bf16* base = (const bf16*)qkv.data_ptr();
  bf16* dbase = (bf16*)dqkv.data_ptr();
  fa2_bwd_core((const bf16*)dout.data_ptr(), base, base + H * D,
               base + (H + Hkv) * D, (const bf16*)out.data_ptr(), lse,
               B, H, Hkv, S, S, D, causal, (float)scale, sqkv, sqkv, so,
               dbase,
               gqa ? nullptr : dbase + H * D,
               gqa ? nullptr : dbase + (H + Hkv) * D,
               dk32p, dv32p, sqkv, sqkv, nullptr, 0);
  if (gqa) {
    // scatter the fp32 accumulators into the k/v sections of dqkv
    auto dkv_view = dqkv.view({B, (int64_t)S, H + 2 * Hkv, D});
    dkv_view.narrow(2, H, Hkv).copy_(
        dk32.permute({0, 2, 1, 3}).to(qkv.scalar_type()));
    dkv_view.narrow(2, H + Hkv, Hkv).copy_(
        dv32.permute({0, 2, 1, 3}).to(qkv.scalar_type()));
  }
  return dqkv;
}
