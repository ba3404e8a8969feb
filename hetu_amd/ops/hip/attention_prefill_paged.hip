// Causal attention of a packed, ragged batch of query chunks over a paged
// bf16 KV cache, for gfx950: the prefill (and chunked prefill) kernel behind
// the block-table decode kernels.
//
//   q [T, H, D = 64 or 128] packed over sequences (element strides: a view
//   into a fused qkv output is read in place), k_pool / v_pool [P, Hkv, PS, D]
//   (with their strides), block_table int32 [B, MP], cu_q int32 [B + 1] and
//   kv_len int32 [B] on the device -> out [T, H, D] bf16, lse [H, T] fp32
//
// n_b = cu_q[b + 1] - cu_q[b], kv_b = clamp(kv_len[b], 0, MP * PS): the chunk
// sits at the END of its sequence's cached keys, so row i of sequence b stands
// at position p = kv_b - n_b + i and attends keys 0 .. p; key j is row j % PS
// of page block_table[b, j / PS].  A row with p < 0 attends nothing (out 0,
// lse -inf), rows at or past cu_q[B] come back the same way.
//
// Geometry is the forward's (attention_v2.hip), so attention_common.h serves
// unchanged: 8 waves x 32 M-rows, 64-key tiles, S^T = mfma(K, Q) with the
// whole P row in a lane, fa_pack_frag for P, K row-major swizzled, V in
// [32 key][16 d] subtiles, global_load_lds staging into a 3-deep ring with a
// counted vmcnt.  What differs:
//  * An M-row is a (token, head-in-group) pair: the block serves GP query
//    heads of ONE KV head, row r = token q0 + r / GP, head hkv * G + c * GP +
//    r % GP.  One staged K / V tile feeds GP heads (the pages of a KV head
//    are read G / GP times, not G) and a short chunk still fills the waves.
//    The causal bound of a lane is that of its token.
//  * Staging goes through the block table.  A DMA instruction moves 1 KiB: 4
//    consecutive K rows or one 32-key group of a V subtile, both aligned, so
//    with PS >= 32 all of a wave's loads of a tile lie in ONE page (the
//    32-key group wid >> 2).  Its id is a scalar, read through the constant
//    address space one tile ahead of the DMA that needs it, i.e. three tiles
//    ahead of the compute.  Keys are clamped to the block's last needed key
//    before they become a table index or an address: no table entry past
//    ceil(kv_b / PS) and no pool row at or past kv_b is ever read.
//  * A page id outside [0, P) is 32 masked keys.  Its wave issues no DMA for
//    the group, and every wave (each reads both ids of a tile) masks the
//    group's scores by selection and skips its P.V MFMAs: the group's LDS
//    image is stale and 0 x NaN is NaN in an MFMA.  A wave that skipped its
//    DMA for tile t + 1 drains at the head of tile t instead of counting
//    loads it never issued.
//  * The softmax runs in base 2: scores are scaled by scale * log2(e) in
//    fp32 (q is NOT pre-scaled in bf16: that rounding moves lse by more than
//    the bound allows on a sharp row) and exp is the bare v_exp_f32.
//
// D = 64 keeps the 8 x 32 M-rows, the 16 KiB images, the ring and the counted
// wait, and changes what a byte of them means (the text above is D = 128):
//  * A K row is 128 B, so an image is a 128-KEY tile: four 32-key blocks of
//    S^T (p[4][16]) with 4 k-steps each, and two 32-d accumulator tiles of O.
//    The K image takes fa_swz_rm_d<64> (two rows per bank line, derived in
//    attention_common.h), the V image is [key group][d subtile] with four
//    d-subtiles per group.
//  * A 1 KiB DMA instruction is 8 consecutive K rows or one [32 key][16 d] V
//    subtile.  Wave w stages K rows 16 w .. 16 w + 15 and V subtiles 2 w and
//    2 w + 1: all in the 32-key group w >> 1, so it is still one page and one
//    scalar id per wave and tile.  Every wave consumes all four groups and
//    reads four ids per tile; the unloaded-group bits are four per tile.
//  * P.V takes a group at a time: both 16-key slots' V^T fragments come from
//    one fa_tr_v2x2 (8 transposed reads, one wait) and feed 4 MFMAs; the two
//    k-steps of an unloaded group are skipped together.
//
// Grid (B + 1) * Hkv * (G / GP) by ceil(max_q * GP / 256): sequence and head
// on blockIdx.x (docs/KERNELS.md, XCD grid order).  It depends on shapes and
// max_q only; blocks past a sequence's chunk return before any load or
// barrier, and the blocks of the pseudo-sequence b == B zero the rows past
// cu_q[B].  One launch, no atomics, no workspace, no host sync.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "ext_stream.h"
#include "attention_common.h"
#include "attention_decode.h"

namespace {

constexpr int PF_BM = 256;             // M-rows per block (8 waves x 32)
constexpr int PF_NGLDS = FA_KV_IMG / (FA_THREADS * 16);   // per lane and image
constexpr int PF_NBUF = FA_RING;

struct PfArgs {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  bf16* out;                  // [T, H, D]
  float* lse;                 // [H, T]
  const int* table;           // [B, MP]
  const int* cu_q;            // [B + 1]
  const int* kv_len;          // [B]
  long long q_ts, q_hs;
  long long k_ps, k_hs, k_rs;
  long long v_ps, v_hs, v_rs;
  int B, H, Hkv, T, MP, P, ps_shift;
  float scale_log2;           // scale * log2(e)
  bool mask_all;
};

// one bit per 32-key group of a tile (2 at D = 128, 4 at D = 64) whose page id
// is outside [0, P)
template <int NG>
DEV int pf_bad_bits(const int (&id)[NG], int P) {
  int bad = 0;
#pragma unroll
  for (int g = 0; g < NG; ++g)
    bad |= (unsigned)id[g] >= (unsigned)P ? 1 << g : 0;
  return bad;
}

template <int GP, int D>
__global__ __launch_bounds__(FA_THREADS, 1)
void fa_prefill_paged_kernel(PfArgs a) {
  static_assert(D == 64 || D == 128, "head dim");
  constexpr int PF_BN = FA_KV_IMG / (2 * D);   // key tile: 64 (D = 128) / 128
  constexpr int NG = PF_BN / 32;       // 32-key groups = S^T blocks of a tile
  constexpr int NKK = D / 16;          // k-steps of S^T
  constexpr int NDT = D / 32;          // 32-d accumulator tiles of O
  constexpr int GRP_SH = D == 128 ? 2 : 1;     // log2 of waves staging a group
  constexpr int KROW_SH = D == 128 ? 8 : 7;    // log2 of a K row's bytes
  constexpr int VSUB_SH = D == 128 ? 3 : 2;    // log2 of d-subtiles a group
  constexpr int ROW_CH = D / 8;        // 16-B chunks of an output row
  constexpr int ALL_BAD = (1 << NG) - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int i) -> char* { return smem + i * FA_KV_IMG; };
  auto v_lds = [&](int i) -> char* {
    return smem + (PF_NBUF + i) * FA_KV_IMG;
  };

  const int G = a.H / a.Hkv;
  const int NC = G / GP;               // head chunks per KV head
  const int c = blockIdx.x % NC;
  const int hkv = (blockIdx.x / NC) % a.Hkv;
  const int b = blockIdx.x / (NC * a.Hkv);
  const int head0 = hkv * G + c * GP;
  const int tid = threadIdx.x;

  if (b == a.B) {
    // rows past cu_q[B]: 16 B of zeros per thread and step, no loads
    const int t0 = min(max(a.cu_q[a.B], 0), a.T);
    const long long total = (long long)(a.T - t0) * (GP * ROW_CH);
    ushort8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z.v[j] = 0;
    for (long long i = (long long)blockIdx.y * FA_THREADS + tid; i < total;
         i += (long long)gridDim.y * FA_THREADS) {
      const int t = t0 + (int)(i / (GP * ROW_CH));
      const int h = head0 + (int)(i % (GP * ROW_CH)) / ROW_CH;
      const int ch = (int)(i % ROW_CH);
      *reinterpret_cast<ushort8*>(a.out + ((int64_t)t * a.H + h) * D +
                                  ch * 8) = z;
      if (ch == 0) a.lse[(int64_t)h * a.T + t] = -INFINITY;
    }
    return;
  }

  // the chunk, clamped into the packed rows whatever cu_q holds
  const int row0 = min(max(a.cu_q[b], 0), a.T);
  const int n_b = min(max(a.cu_q[b + 1], row0), a.T) - row0;
  const int q0 = blockIdx.y * (PF_BM / GP);     // first token of the block
  if (q0 >= n_b) return;               // block-uniform: no load, no barrier
  const int kv_b = min(max(a.kv_len[b], 0), a.MP << a.ps_shift);
  const int diag = kv_b - n_b;         // position of the chunk's token 0

  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int iq = lane & 31;
  const int hi = lane >> 5;
  const int r = blockIdx.y * PF_BM + wid * 32 + iq;       // M-row
  const int tok = r / GP;
  const int head = head0 + r % GP;
  const bool valid = tok < n_b;
  const int my_p = diag + tok;

  // wave-uniform: the wave's tokens, the block's key range
  const int wu = __builtin_amdgcn_readfirstlane(wid);
  const int grp = wu >> GRP_SH;        // the 32-key group this wave stages
  const int wtok0 = (blockIdx.y * PF_BM + wu * 32) / GP;
  const int wtok1 = (blockIdx.y * PF_BM + wu * 32 + 31) / GP;
  const bool w_any = wtok0 < n_b;
  const bool w_pad = wtok1 >= n_b;
  const int w_pmin = diag + wtok0;
  const int w_pmax = diag + min(wtok1, n_b - 1);
  const int kend = diag + min(q0 + PF_BM / GP, n_b);      // <= kv_b
  const int n_tiles = kend > 0 ? (kend + PF_BN - 1) / PF_BN : 0;
  const int klast = kend - 1;          // every key is clamped to it

  // Q -> registers, unscaled (the scale meets the scores in fp32)
  bf16x8 qreg[NKK];
  fa_load_row_frags_d<D>(qreg,
                         a.q + (int64_t)(row0 + min(tok, n_b - 1)) * a.q_ts +
                             (int64_t)head * a.q_hs, hi);

  typedef const __attribute__((address_space(4))) int* const_int_p;
  const const_int_p trow = (const_int_p)(a.table + (int64_t)b * a.MP);
  // the ids of the 32-key groups of the tile at k0 (klast >= 0 here)
  auto ids_of = [&](int k0, int (&id)[NG]) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
      id[g] = __builtin_amdgcn_readfirstlane(
          trow[min(k0 + 32 * g, klast) >> a.ps_shift]);
  };
  // the id of the wave's own group, by scalar selection (two levels on the
  // bits of grp; the readfirstlane keeps the four-way form in an SGPR, which
  // dec_page_landed requires)
  auto own_id = [&](const int (&id)[NG]) {
    if constexpr (NG == 2) {
      return grp ? id[1] : id[0];
    } else {
      const int lo = (grp & 1) ? id[1] : id[0];
      const int hi2 = (grp & 1) ? id[3] : id[2];
      return __builtin_amdgcn_readfirstlane((grp & 2) ? hi2 : lo);
    }
  };

  const bf16* kb = a.k + (int64_t)hkv * a.k_hs;
  const bf16* vb = a.v + (int64_t)hkv * a.v_hs;
  const int rmask = (1 << a.ps_shift) - 1;
  // the wave's 2 K + 2 V DMA instructions of one tile, all in `page`: the
  // clamped key stays in the wave's 32-key group or is klast itself, whose
  // page the id was read for
  auto stage = [&](int k0, int buf, int page) {
    const bf16* kp = kb + (int64_t)page * a.k_ps;
    const bf16* vp = vb + (int64_t)page * a.v_ps;
#pragma unroll
    for (int i = 0; i < PF_NGLDS; ++i) {
      const int pos = (wid * PF_NGLDS + i) * 1024 + lane * 16;
      const int krow = min(k0 + (pos >> KROW_SH), klast) & rmask;
      fa_glds16(kp + (int64_t)krow * a.k_rs + fa_rm_src_col_d<D>(pos),
                k_lds(buf) + pos);
      const int st = pos >> 10;
      const int vkey = (st >> VSUB_SH) * 32 + ((pos >> 5) & 31);
      const int vd = (st & (D / 16 - 1)) * 16 + ((pos >> 4) & 1) * 8;
      const int vrow = min(k0 + vkey, klast) & rmask;
      fa_glds16(vp + (int64_t)vrow * a.v_rs + vd, v_lds(buf) + pos);
    }
  };

  f32x16 o_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o_acc[dt][i] = 0.f;
  float m_i = -INFINITY, l_i = 0.f;    // base-2 running max and sum

  // prologue: tiles 0 and 1 in flight, the ids of tile 2 requested.
  // bad_c / bad_n: the unloaded groups of tiles t and t + 1.
  int bad_c = 0, bad_n = 0, id_n[NG] = {};
  if (n_tiles > 0) {
    int id[NG];
    ids_of(0, id);
    bad_c = pf_bad_bits(id, a.P);
    if (!((bad_c >> grp) & 1)) stage(0, 0, own_id(id));
    ids_of(PF_BN, id);
    bad_n = pf_bad_bits(id, a.P);
    if (n_tiles > 1 && !((bad_n >> grp) & 1))
      stage(PF_BN, 1, own_id(id));
    ids_of(2 * PF_BN, id_n);
  }

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * PF_BN;
    const int cur = t % PF_NBUF;
    // tile t landed, tile t + 1 may fly; drain where this wave issued
    // nothing for tile t + 1
    fa_wait_tile<2 * PF_NGLDS>(t + 1 >= n_tiles || ((bad_n >> grp) & 1));
    __builtin_amdgcn_s_barrier();
    const int bad_nn = pf_bad_bits(id_n, a.P);
    {
      int page = own_id(id_n);
      int key_nn = k0 + 3 * PF_BN;
      dec_page_landed(page, key_nn);   // old ids first, then the new request
      if (t + 2 < n_tiles && !((bad_nn >> grp) & 1))
        stage(k0 + 2 * PF_BN, (t + 2) % PF_NBUF, page);
      ids_of(key_nn, id_n);
    }

    // any row of the wave with an unmasked key in a loaded group?
    const bool active = w_any && k0 <= w_pmax && bad_c != ALL_BAD;
    if (active) {
      float p[NG][16];
#pragma unroll
      for (int ct = 0; ct < NG; ++ct) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              k_lds(cur) + fa_swz_rm_d<D>(32 * ct + iq, kk * 32 + hi * 16));
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qreg[kk], acc,
                                                        0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) p[ct][i] = acc[i] * a.scale_log2;
      }

      // mask + online softmax, lane-local; MASK = false has no key index,
      // compare or select.  Returns the O rescale.
      auto softmax = [&](auto mask_c) -> float {
        constexpr bool MASK = decltype(mask_c)::value;
        float pmax = -INFINITY;
        int bound[NG] = {};
        if constexpr (MASK) {
          // one compare per element: the lane's last key relative to its
          // first register's key; -1 masks a padded row or an unloaded group
          const int bl = valid ? my_p - (k0 + 4 * hi) : -1;
#pragma unroll
          for (int ct = 0; ct < NG; ++ct)
            bound[ct] = (bad_c & (1 << ct)) ? -1 : bl;
        }
#pragma unroll
        for (int ct = 0; ct < NG; ++ct)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if constexpr (MASK)
              if (32 * ct + fa_crow(i) > bound[ct]) p[ct][i] = -INFINITY;
            pmax = fmaxf(pmax, p[ct][i]);
          }
        pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));
        const float mn = fmaxf(m_i, pmax);
        const float alpha = (m_i == -INFINITY) ? 0.f
                            : __builtin_amdgcn_exp2f(m_i - mn);
        m_i = mn;
        float psum = 0.f;
#pragma unroll
        for (int ct = 0; ct < NG; ++ct)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float pv;
            if constexpr (MASK)
              pv = (p[ct][i] == -INFINITY || mn == -INFINITY)
                       ? 0.f : __builtin_amdgcn_exp2f(p[ct][i] - mn);
            else
              pv = __builtin_amdgcn_exp2f(p[ct][i] - mn);
            p[ct][i] = pv;
            psum += pv;
          }
        psum += __shfl_xor(psum, 32, 64);
        l_i = l_i * alpha + psum;
        return alpha;
      };
      // wave-uniform: the tile crosses the causal diagonal of the wave's
      // first token or the key tail, the wave holds padded rows, or a group
      // of the tile is not loaded
      const bool boundary = a.mask_all || k0 + (PF_BN - 1) > w_pmin ||
                            k0 + (PF_BN - 1) >= kv_b || w_pad || bad_c != 0;
      const float alpha = boundary ? softmax(std::true_type{})
                                   : softmax(std::false_type{});
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[dt][i] *= alpha;

      if constexpr (D == 128) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if ((bad_c >> (ks >> 1)) & 1) continue;   // stale V image: skip
          bf16x8 pfrag = fa_pack_frag(p[ks >> 1], (ks & 1) * 8);
          bf16x8 vf[4];
          fa_tr_v4(vf, v_lds(cur), ks, lane);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                vf[dt], pfrag, o_acc[dt], 0, 0, 0);
        }
      } else {
        // a 32-key group at a time: its two k-steps share one V read block
        // and are skipped together where the group was not loaded
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if ((bad_c >> g) & 1) continue;           // stale V image: skip
          bf16x8 vf[2][2];
          fa_tr_v2x2(vf, v_lds(cur), g, lane);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            bf16x8 pfrag = fa_pack_frag(p[g], s * 8);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
              o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  vf[s][dt], pfrag, o_acc[dt], 0, 0, 0);
          }
        }
      }
    }
    bad_c = bad_n;
    bad_n = bad_nn;
  }

  if (valid) {
    const float inv = (l_i > 0.f) ? 1.f / l_i : 0.f;
    fa_store_row_bf16_d<D>(
        o_acc, inv, a.out + ((int64_t)(row0 + tok) * a.H + head) * D, hi);
    if (hi == 0)
      a.lse[(int64_t)head * a.T + row0 + tok] =
          (l_i > 0.f) ? (m_i + __log2f(l_i)) * 0.6931471805599453f
                      : -INFINITY;
  }
}

void pf_check_strided(const torch::Tensor& t, const char* what) {
  const char* fn = "flash_attn_prefill_paged: ";
  TORCH_CHECK(t.is_cuda(), fn, what, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, what, " must be bf16");
  TORCH_CHECK(t.stride(-1) == 1, fn, what, " needs a contiguous last dim");
  for (int i = 0; i + 1 < t.dim(); ++i)
    TORCH_CHECK(t.size(i) <= 1 || t.stride(i) % 8 == 0, fn, what, " stride ",
                i, " is not a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, what,
              " is not 16-byte aligned");
}

void pf_check_index(const torch::Tensor& t, const torch::Tensor& q,
                    const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device() &&
              t.scalar_type() == at::kInt && t.is_contiguous(),
              "flash_attn_prefill_paged: ", what,
              " must be a contiguous int32 tensor on q's device");
}

}  // namespace

std::vector<torch::Tensor> flash_attn_prefill_paged(
    torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
    torch::Tensor block_table, torch::Tensor cu_q, torch::Tensor kv_len,
    double scale, int64_t max_q) {
  const char* fn = "flash_attn_prefill_paged: ";
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
  pf_check_strided(q, "q");
  pf_check_strided(k_pool, "k_pool");
  pf_check_strided(v_pool, "v_pool");
  TORCH_CHECK(k_pool.device() == q.device() && v_pool.device() == q.device(),
              fn, "all tensors must share one device");
  pf_check_index(block_table, q, "block_table");
  pf_check_index(cu_q, q, "cu_q");
  pf_check_index(kv_len, q, "kv_len");
  TORCH_CHECK(block_table.dim() == 2 && cu_q.dim() == 1 && cu_q.size(0) >= 1,
              fn, "need block_table [B, MP] and cu_q [B + 1]");
  const int64_t B = block_table.size(0), MP = block_table.size(1);
  TORCH_CHECK(cu_q.size(0) == B + 1 && kv_len.dim() == 1 &&
              kv_len.size(0) == B, fn, "need cu_q [B + 1] and kv_len [B] "
              "with B = ", B, " rows of block_table");
  const int64_t lim = (int64_t)1 << 31;
  // the id prefetch forms keys up to four 128-key tiles past the first
  TORCH_CHECK(T < lim && H < lim && P < lim && MP * PS < lim - 512 &&
              B < lim, fn, "T, H, B, P or MP * PS too large for int");

  auto out = torch::empty({T, H, D}, q.options());
  auto lse = torch::empty({H, T}, q.options().dtype(at::kFloat));
  if (T == 0 || H == 0) return {out, lse};

  const int64_t G = H / Hkv;
  const int gp = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
  max_q = std::min(std::max<int64_t>(max_q, 1), T);
  const int64_t gx = (B + 1) * Hkv * (G / gp);
  const int64_t gy = (max_q * gp + PF_BM - 1) / PF_BM;
  TORCH_CHECK(gx < lim && gy <= 65535, fn, "grid too large: ", gx, " x ", gy);

  PfArgs a;
  a.q = (const bf16*)q.data_ptr();
  a.k = (const bf16*)k_pool.data_ptr();
  a.v = (const bf16*)v_pool.data_ptr();
  a.out = (bf16*)out.data_ptr();
  a.lse = lse.data_ptr<float>();
  a.table = block_table.data_ptr<int>();
  a.cu_q = cu_q.data_ptr<int>();
  a.kv_len = kv_len.data_ptr<int>();
  a.q_ts = q.stride(0); a.q_hs = q.stride(1);
  a.k_ps = k_pool.stride(0); a.k_hs = k_pool.stride(1);
  a.k_rs = k_pool.stride(2);
  a.v_ps = v_pool.stride(0); a.v_hs = v_pool.stride(1);
  a.v_rs = v_pool.stride(2);
  a.B = (int)B; a.H = (int)H; a.Hkv = (int)Hkv; a.T = (int)T;
  a.MP = (int)MP; a.P = (int)P;
  a.ps_shift = __builtin_ctzll((unsigned long long)PS);
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.mask_all = fa_mask_all();

  const dim3 grid((unsigned)gx, (unsigned)gy);
  auto stream = hetu_current_stream();
#define PF_LAUNCH(GG, DD)                                                  \
  hipLaunchKernelGGL((fa_prefill_paged_kernel<GG, DD>), grid,              \
                     dim3(FA_THREADS), FA_FWD_LDS, stream, a)
#define PF_LAUNCH_D(DD)                                                    \
  do {                                                                     \
    if (gp == 8) PF_LAUNCH(8, DD);                                         \
    else if (gp == 4) PF_LAUNCH(4, DD);                                    \
    else if (gp == 2) PF_LAUNCH(2, DD);                                    \
    else PF_LAUNCH(1, DD);                                                 \
  } while (0)
  if (D == 128) PF_LAUNCH_D(128);
  else PF_LAUNCH_D(64);
#undef PF_LAUNCH_D
#undef PF_LAUNCH
  HIP_CHECK(hipGetLastError());
  return {out, lse};
}
