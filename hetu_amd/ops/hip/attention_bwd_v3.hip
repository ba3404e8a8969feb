// Flash-attention backward v3: the default backward for dense (BHSD
// contiguous) non-GQA D=128 attention; flash_attn_bwd selects it whenever
// H == Hkv and D == 128 (attention.hip).
//
// Same math, layouts and per-tile compute bodies as attention_bwd_v2.hip
// (both call attention_common.h), bit-identical results; only the staging
// and the loop heads differ:
//   B1. dq: 3-deep K/V ring with a counted s_waitcnt vmcnt(N) at the loop
//       head (v2 drains vmcnt(0) every tile); dkv: 2-buffer ring, refilled
//       at the loop tail, with a counted wait.
//   B2. dq: walking-pointer glds source addressing with a clamped fallback
//       for the ragged tail (v2 recomputes min()*stride per tile).
//   B3. launch_bounds occupancy 1: at 96/132 KiB LDS only one block fits
//       per CU anyway.
#include <torch/extension.h>
#include "ext_stream.h"
#include "attention_common.h"

namespace {

constexpr int THREADS = FA_THREADS;
constexpr int NBUF = FA_RING;

// ===========================================================================
// dq kernel v3: 8 waves x 32 q rows; 3-ring KV staging, counted vmcnt.
// ===========================================================================
template <int D>
__global__ __launch_bounds__(THREADS, 1) void fa3_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dQ, int B, int H, int S, int Skv,
    float scale, bool causal, bool mask_all) {
  static_assert(D == 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int bb) -> char* { return smem + bb * FA_KV_IMG; };
  auto v_lds = [&](int bb) -> char* {
    return smem + (NBUF + bb) * FA_KV_IMG;
  };

  const int bh = blockIdx.x;
  const int q0 = blockIdx.y * 256;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;
  const int hi = lane >> 5;

  const bf16* Qb = Q + (int64_t)bh * S * D;
  const bf16* dOb = dO + (int64_t)bh * S * D;
  const bf16* Kb = K + (int64_t)bh * Skv * D;
  const bf16* Vb = V + (int64_t)bh * Skv * D;

  const int my_q = q0 + wid * 32 + iq;
  const int diag = Skv - S;
  const float lse_q = LSE[(int64_t)bh * S + min(my_q, S - 1)];
  const float del_q = DELTA[(int64_t)bh * S + min(my_q, S - 1)];

  bf16x8 qreg[8], doreg[8];
  fa_load_row_frags(qreg, Qb + (int64_t)min(my_q, S - 1) * D, hi, scale);
  fa_load_row_frags(doreg, dOb + (int64_t)min(my_q, S - 1) * D, hi);

  // B2: walking pointers (2 slots per lane, K and V share layout)
  const int wlane16 = lane * 16;
  int pos_c[2], krow_c[2], kd_c[2];
  const bf16* kp[2];
  const bf16* vp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int pos = (wid * 2 + i) * 1024 + wlane16;
    pos_c[i] = pos;
    krow_c[i] = pos >> 8;
    kd_c[i] = fa_rm_src_col(pos);
    kp[i] = Kb + (int64_t)krow_c[i] * D + kd_c[i];
    vp[i] = Vb + (int64_t)krow_c[i] * D + kd_c[i];
  }
  constexpr int64_t STEP = 64 * D;

#define DQ3_FAST(buf)                                                       \
  do {                                                                      \
    _Pragma("unroll")                                                       \
    for (int i = 0; i < 2; ++i) {                                           \
      fa_glds16(kp[i], k_lds(buf) + pos_c[i]);                              \
      fa_glds16(vp[i], v_lds(buf) + pos_c[i]);                              \
      kp[i] += STEP;                                                        \
      vp[i] += STEP;                                                        \
    }                                                                       \
  } while (0)

#define DQ3_CLAMPED(k0v, buf)                                               \
  do {                                                                      \
    _Pragma("unroll")                                                       \
    for (int i = 0; i < 2; ++i) {                                           \
      int64_t roff = (int64_t)min((k0v) + krow_c[i], Skv - 1) * D + kd_c[i];\
      fa_glds16(Kb + roff, k_lds(buf) + pos_c[i]);                          \
      fa_glds16(Vb + roff, v_lds(buf) + pos_c[i]);                          \
      kp[i] += STEP;                                                        \
      vp[i] += STEP;                                                        \
    }                                                                       \
  } while (0)

#define DQ3_ISSUE(k0v, buf)                                                 \
  do {                                                                      \
    if ((k0v) + 64 <= Skv) DQ3_FAST(buf);                                   \
    else DQ3_CLAMPED(k0v, buf);                                             \
  } while (0)

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const int wave_qmax = q0 + wid * 32 + 31;
  const int n_tiles = fa_n_kv_tiles(q0, Skv, diag, causal);

  DQ3_ISSUE(0, 0);
  if (n_tiles > 1) DQ3_ISSUE(64, 1);
  else DQ3_CLAMPED(0, 1);     // duplicate: keeps the counted wait sound

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * 64;
    const int cur = t % NBUF;
    // B1: allow the newest tile's 4 loads to stay in flight
    fa_wait_tile<4>(t + 1 >= n_tiles);
    __builtin_amdgcn_s_barrier();
    if (t + 2 < n_tiles) DQ3_ISSUE(k0 + 128, (t + 2) % NBUF);

    const bool active = !causal || (k0 <= wave_qmax + diag);
    if (active) {
      const bool boundary = fa_boundary_kv_tile(wave_qmax - 31, k0, S, Skv,
                                                diag, causal, mask_all);
      FA_BWD_DQ_TILE(boundary, k_lds(cur), v_lds(cur), qreg, doreg, dq_acc,
                     k0, my_q, S, Skv, diag, causal, lse_q, del_q, lane);
    }
  }
#undef DQ3_ISSUE
#undef DQ3_FAST
#undef DQ3_CLAMPED

  if (my_q < S)
    fa_store_row_bf16(dq_acc, scale, dQ + ((int64_t)bh * S + my_q) * D, hi);
}

// ===========================================================================
// dkv kernel v3: 8 waves x 32 keys; 2-ring Q/dO staging, counted vmcnt.
// ===========================================================================
template <int D>
__global__ __launch_bounds__(THREADS, 1) void fa3_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dK16, bf16* __restrict__ dV16,
    int B, int H, int S, int Skv, float scale, bool causal) {
  static_assert(D == 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // dkv uses a 2-buffer ring with issue-at-end + counted vmcnt (the 3rd
  // buffer's live state spilled past the 2-waves/SIMD VGPR budget)
  auto q_lds = [&](int bb) -> char* { return smem + bb * FA_Q_IMG; };
  auto do_lds = [&](int bb) -> char* { return smem + (2 + bb) * FA_Q_IMG; };
  char* vw_base = smem + 4 * FA_Q_IMG;
  char* pw_base = vw_base + 8 * FA_WAVE_V_IMG;

  const int bh = blockIdx.x;
  const int kb0 = blockIdx.y * 256;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;
  const int hi = lane >> 5;

  const bf16* Qb = Q + (int64_t)bh * S * D;
  const bf16* dOb = dO + (int64_t)bh * S * D;
  const bf16* Kb = K + (int64_t)bh * Skv * D;
  const bf16* Vb = V + (int64_t)bh * Skv * D;
  const float* lse_b = LSE + (int64_t)bh * S;
  const float* del_b = DELTA + (int64_t)bh * S;

  const int wave_kmin = kb0 + wid * 32;
  const int my_key = wave_kmin + iq;
  const int diag = Skv - S;

  char* vw_lds = vw_base + wid * FA_WAVE_V_IMG;
  char* p_lds = pw_base + wid * 2 * FA_P_IMG;

  bf16x8 kreg[8];
  fa_load_row_frags(kreg, Kb + (int64_t)min(my_key, Skv - 1) * D, hi, scale);
  fa_stage_wave_v(Vb, D, wave_kmin, Skv, vw_lds, lane);

  // one (q, do) pair per lane per tile
  const int pos0 = tid * 16;
  const int qrow_c = pos0 >> 8;
  const int qd_c = fa_rm_src_col(pos0);

  const int n_q_tiles = (S + 31) / 32;
  const int t_start = fa_first_q_tile(kb0, diag, causal);

  // dkv keeps v2-style clamped addressing (1 slot/lane, the address math
  // is cheap); the v3 win here is the counted-vmcnt pipeline — the kernel
  // sits exactly at the 2-waves/SIMD VGPR budget, so no walking pointers
#define DKV3_ISSUE(qt0, buf)                                                \
  do {                                                                      \
    int qr_ = min((qt0) + qrow_c, S - 1);                                   \
    fa_glds16(Qb + (int64_t)qr_ * D + qd_c, q_lds(buf) + pos0);             \
    fa_glds16(dOb + (int64_t)qr_ * D + qd_c, do_lds(buf) + pos0);           \
  } while (0)

  f32x16 dk_acc[4], dv_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk_acc[dt][r] = 0.f; dv_acc[dt][r] = 0.f; }

  DKV3_ISSUE(t_start * 32, 0);
  if (t_start + 1 < n_q_tiles) DKV3_ISSUE(t_start * 32 + 32, 1);
  else DKV3_ISSUE(t_start * 32, 1);   // duplicate keeps the wait sound

  for (int t = t_start; t < n_q_tiles; ++t) {
    const int qt0 = t * 32;
    const int cur = (t - t_start) & 1;
    // allow the newest issue's 2 loads to stay in flight; the V image
    // and tile t have landed once this retires
    fa_wait_tile<2>(t + 1 >= n_q_tiles);
    __builtin_amdgcn_s_barrier();

    const bool active = !causal || (qt0 + 31 >= wave_kmin - diag);
    if (active)
      fa_bwd_dkv_tile(q_lds(cur), do_lds(cur), vw_lds, p_lds, kreg, dk_acc,
                      dv_acc, qt0, wave_kmin, S, Skv, diag, causal, lse_b,
                      del_b, lane);
    // all waves done reading buffer `cur` -> refill it with tile t+2
    // (the DMA then lands under tile t+1's compute)
    __builtin_amdgcn_s_barrier();
    if (t + 2 < n_q_tiles) DKV3_ISSUE(qt0 + 64, cur);
  }
#undef DKV3_ISSUE

#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int key = wave_kmin + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (key < Skv) {
        int64_t off = ((int64_t)bh * Skv + key) * D + 32 * dt + iq;
        dK16[off] = (bf16)(dk_acc[dt][r] * scale);
        dV16[off] = (bf16)(dv_acc[dt][r]);
      }
    }
  }
}

}  // namespace

std::vector<torch::Tensor> fa3_bwd_launch(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, bool causal, double scale) {
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hkv = k.size(1), Skv = k.size(2);
  TORCH_CHECK(D == 128 && H == Hkv, "fa3 bwd: D=128, non-GQA only");
  auto stream = hetu_current_stream();
  auto delta = torch::empty({B, H, S}, q.options().dtype(at::kFloat));
  FaStrides so{(long long)H * S * D, (long long)S * D, (long long)D};
  fa_delta_launch((const bf16*)dout.data_ptr(), (const bf16*)out.data_ptr(),
                  delta.data_ptr<float>(), (int64_t)B * H * S, D, H, S, so,
                  stream);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  const bool mask_all = fa_mask_all();
  hipLaunchKernelGGL(fa3_bwd_dq_kernel<128>, dim3(B * H, (S + 255) / 256),
                     dim3(THREADS), FA3_DQ_LDS, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
                     (const bf16*)v.data_ptr(), (const bf16*)dout.data_ptr(),
                     lse.data_ptr<float>(), delta.data_ptr<float>(),
                     (bf16*)dq.data_ptr(), B, H, S, Skv, (float)scale,
                     causal, mask_all);
  hipLaunchKernelGGL(fa3_bwd_dkv_kernel<128>,
                     dim3(B * H, (Skv + 255) / 256), dim3(THREADS),
                     FA_DKV_LDS, stream, (const bf16*)q.data_ptr(),
                     (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     (const bf16*)dout.data_ptr(), lse.data_ptr<float>(),
                     delta.data_ptr<float>(), (bf16*)dk.data_ptr(),
                     (bf16*)dv.data_ptr(), B, H, S, Skv, (float)scale,
                     causal);
  return {dq, dk, dv};
}
