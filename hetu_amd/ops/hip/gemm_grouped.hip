// Grouped (per-expert) bf16 MFMA GEMMs for the MoE expert block on gfx950:
//   NN (forward):        out[g] = a[g] [M, K] @ b[g] [K, N]
//   NT (input gradient): out[g] = a[g] [M, K] @ b[g] [N, K]^T
// fp32 accumulate, one bf16 rounding.  Every operand is read where it lies:
// no transposed copy, no workspace, no atomics, no split-K, one launch.
//
// Rows of a[g] are P segments of `seg` slots (one segment per source rank of
// the expert-parallel all-to-all); segment s of group g holds counts[g, s]
// filled slots as a prefix, so row r is valid iff
//   (r % seg) < counts[g, r / seg].
// counts lives on the device and is read inside the kernel: the grid depends
// on shapes only, the call never syncs the host and can be captured.
// Every invalid output row is exactly zero and nothing an invalid input row
// holds reaches a valid row (row r of a only ever feeds row r of out).
//
// Structure (gemm.hip's skeleton, templated on how B is staged and read)
// ----------------------------------------------------------------------
//   * 128-row M tile, BN-column N tile (128 or 256), BK = 64.  One wave per
//     64x64 of the tile: 2 x BN/64 waves, 4x4 accumulators of 16x16 each.
//   * two LDS buffers of [A 16 KiB | B BN*128 B], staged with
//     global_load_lds width 16; tile t+1 is issued before tile t is
//     computed and the loop head waits vmcnt(loads of one tile), on the last
//     K-tile vmcnt(0) (fa_wait_tile: nothing newer is in flight there).
//   * A [128 rows][64 k] is K-major in both modes: 128-B image rows,
//     ds_read_b128 fragments, byte-in-row ^= (row & 7) << 4 as in gemm.hip.
//   * NT: B [BN n-rows][64 k] is the same image and the same reads.
//   * NN: B [64 k-rows][BN columns] is a plain row-major image and each
//     16-column x 32-k MFMA operand is two ds_read_b64_tr_b16 (semantics in
//     docs/KERNELS.md: lane 16g + 4q + p supplies row 8g + q at column bytes
//     c0 + 8p and receives column lane & 15 of the four rows of its group,
//     so two reads 4 rows apart give k = 8g .. 8g + 7 of one column).
//   * the MFMA takes the B fragment as its first operand, so a lane holds 4
//     consecutive output columns of one row: one 8-byte store per
//     accumulator and one validity test per (lane, 16-row block).
//
// NN image and its bank argument
// ------------------------------
// An image row is BN * 2 bytes: 256 B (BN = 128) or 512 B (BN = 256), in
// both cases a whole number of 256-B bank rows, so every image row starts
// on bank 0.  One tr read is served per 32-lane half; a half (g & 1 = 0, 1;
// q = 0..3) touches the 8 rows {r..r+3, r+8..r+11}, 32 B (4 p x 8 B) each,
// at the same column bytes c0..c0+31 with c0 % 32 == 0.  Unswizzled those
// are 8 rows on the same 8 banks: 8-way.  Swizzle: byte-in-row ^= f(t) << 5
// with f(t) = (t & 3) | ((t >> 3) & 1) << 2, which takes 8 distinct values
// on the 8 rows of a half.  It permutes the eight 32-B slots inside one
// 256-B bank row (bits 5..7), which exists for both row lengths because
// both are multiples of 256 B: the half then reads 8 distinct slots x 4
// distinct 8-B pieces = all 64 banks once.  Conflict-free.  gemm_wgrad's f
// is the same function; what had to be checked for this image is that the
// 256-B row keeps rows bank-aligned (it does: one bank row per image row)
// and that the XOR never leaves the row (bits 5..7 < 256).  f is unchanged
// by +4 and +32 rows, so the second read and the second k-step are
// immediate offsets on one address register per fragment.
// global_load_lds writes lane-linear, so the swizzle is applied to the
// per-lane SOURCE column, never to the LDS destination; the XOR moves whole
// 16-B chunks inside an aligned 256-B run, so the loads stay full-line.
//
// Ragged M and skipping
// ---------------------
// M = P * seg is arbitrary.  Staging clamps the row index to M - 1 before it
// becomes an address, so every lane always holds a valid address and EXEC is
// full in the main loop (the tr reads require that); only the epilogue's
// stores are predicated (row < M) and select zero for invalid rows.
// A block whose 128 rows are all invalid writes zeros with 16-B stores and
// returns before any load or barrier.  The test is block-uniform: a loop
// over the segments the tile overlaps, on scalar loads of counts.
//
// Block order
// -----------
// Bijective XCD remap as in gemm.hip: an XCD runs a contiguous chunk of work
// ids.  Ids are ordered group-major; inside a group in bands of 8 column
// tiles; inside a band row tile by row tile, the band's column tiles
// innermost.  The blocks an XCD holds at one time (64 at 2 per CU, 32 at 1)
// then cover a few consecutive row tiles of ONE band of ONE expert: the
// band's weight panel (K x 8 BN, 4 MB at K = 2048, BN = 128; streamed in
// K-step with the blocks, so the live part is far smaller) is fetched once
// and reused by every row tile of the expert, and an expert's weight (tens
// of MB) crosses HBM about once per launch.  The activations are the cheap
// side: a row panel is re-read once per band, from L2 / MALL.  With G a
// multiple of 8 each XCD owns whole experts.
#include "attention_common.h"
#include "ext_stream.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int GG_BM = 128, GG_BK = 64;
constexpr int GG_A_IMG = GG_BM * GG_BK * 2;     // 16 KiB
constexpr int GG_BAND = 8;                      // column tiles per band

// gemm.hip's swizzle of a K-major image (128-B rows)
DEV int gg_swz(int row, int byte_in_row) {
  return byte_in_row ^ ((row & 7) << 4);
}

// the NN image's swizzle value of k-row t
DEV int gg_f(int t) { return (t & 3) | (((t >> 3) & 1) << 2); }

// Stage ROWS rows of a K-major [rows][64 k] tile (A, or B in NT mode); the
// global row index is clamped to last_row.
template <int ROWS, int THREADS>
DEV void gg_stage_kmajor(const bf16* __restrict__ src, int64_t ld, int row0,
                         int last_row, char* lds, int tid) {
  constexpr int NINST = ROWS * GG_BK * 2 / (THREADS * 16);
#pragma unroll
  for (int t = 0; t < NINST; ++t) {
    const int lin = (t * THREADS + tid) * 16;
    const int row = lin >> 7;
    const int col = gg_swz(row, lin & 127) >> 1;
    fa_glds16(src + (int64_t)min(row0 + row, last_row) * ld + col, lds + lin);
  }
}

// Stage the NN B tile: 64 k-rows of BN columns starting at src
template <int BN, int THREADS>
DEV void gg_stage_rowmajor(const bf16* __restrict__ src, int64_t ld, char* lds,
                           int tid) {
  constexpr int ROWB = BN * 2;
  constexpr int NINST = GG_BK * ROWB / (THREADS * 16);
#pragma unroll
  for (int t = 0; t < NINST; ++t) {
    const int lin = (t * THREADS + tid) * 16;
    const int row = lin / ROWB;
    const int col = ((lin % ROWB) ^ (gg_f(row) << 5)) >> 1;
    fa_glds16(src + (int64_t)row * ld + col, lds + lin);
  }
}

// the four B fragments of one k-step from the NN image: 8 transposed reads
// under one lgkmcnt wait; a[j] is fragment j's address register
template <int OFF0, int OFF1>
DEV void gg_tr4(bf16x8 (&d)[4], const unsigned (&a)[4]) {
  u32x2 x[8];
  asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%12\n\t"
               "ds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
               "ds_read_b64_tr_b16 %2, %9 offset:%12\n\t"
               "ds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
               "ds_read_b64_tr_b16 %4, %10 offset:%12\n\t"
               "ds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
               "ds_read_b64_tr_b16 %6, %11 offset:%12\n\t"
               "ds_read_b64_tr_b16 %7, %11 offset:%13\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]),
                 "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7])
               : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "i"(OFF0),
                 "i"(OFF1)
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = fa_join(x[2 * j], x[2 * j + 1]);
}

// row r of a group is valid iff it is a filled slot (cnt == nullptr: all)
DEV bool gg_row_valid(const int* __restrict__ cnt, int r, int M, int seg) {
  if (r >= M) return false;
  if (cnt == nullptr) return true;
  const int s = r / seg;
  return r - s * seg < cnt[s];
}

template <bool TB, int BN>
__global__ __launch_bounds__(2 * BN) void grouped_gemm_bf16_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    bf16* __restrict__ C, const int* __restrict__ counts, int M, int N, int K,
    int P, int seg, int tiles_m, int tiles_n) {
  constexpr int THREADS = 2 * BN;
  constexpr int B_IMG = BN * GG_BK * 2;         // either layout
  constexpr int BUF = GG_A_IMG + B_IMG;
  constexpr int ROWB = BN * 2;                  // NN image row
  // loads one thread issues per K-tile
  constexpr int NLOAD = (GG_A_IMG + B_IMG) / (THREADS * 16);
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];

  // ---- block id -> (group, row tile, column tile) ----
  const int per_g = tiles_m * tiles_n;
  const int nwg = gridDim.x;
  const int orig = blockIdx.x;
  const int q8 = nwg / 8, r8 = nwg % 8;
  const int xcd = orig % 8, slot = orig / 8;
  const int wgid =
      (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  const int grp = wgid / per_g;
  const int rem = wgid - grp * per_g;
  const int band = rem / (tiles_m * GG_BAND);
  const int in_band = rem - band * (tiles_m * GG_BAND);
  const int band_w = min(GG_BAND, tiles_n - band * GG_BAND);
  const int tm = in_band / band_w;
  const int tn = band * GG_BAND + in_band - tm * band_w;
  const int bm = tm * GG_BM, bn = tn * BN;

  const int tid = threadIdx.x;
  const int* cnt = counts == nullptr ? nullptr : counts + (int64_t)grp * P;
  bf16* Cg = C + (int64_t)grp * M * N;

  // ---- all 128 rows invalid: zeros, and no load or barrier ----
  if (cnt != nullptr) {
    const int last = min(bm + GG_BM, M) - 1;
    bool any = false;
    for (int s = bm / seg; s <= last / seg; ++s)
      any = any || cnt[s] > max(bm - s * seg, 0);
    if (!any) {
      constexpr int CPR = BN / 8;               // 16-B chunks per tile row
      const uint4 z = {0u, 0u, 0u, 0u};
      for (int i = tid; i < GG_BM * CPR; i += THREADS) {
        const int row = bm + i / CPR;
        if (row < M)
          *reinterpret_cast<uint4*>(Cg + (int64_t)row * N + bn +
                                    (i % CPR) * 8) = z;
      }
      return;
    }
  }

  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid) >> 6;
  const int wr = (wid & 1) * 64;                // wave's rows in the tile
  const int wc = (wid >> 1) * 64;               // wave's columns in the tile
  const int fr = lane & 15;
  const int g = lane >> 4;

  const bf16* Ag = A + (int64_t)grp * M * K;
  const bf16* Bg = B + (int64_t)grp * N * K +
                   (TB ? (int64_t)bn * K : (int64_t)bn);

  auto stage = [&](int kt, int buf) {
    char* dst = smem + buf * BUF;
    gg_stage_kmajor<GG_BM, THREADS>(Ag + kt * GG_BK, K, bm, M - 1, dst, tid);
    if constexpr (TB)
      gg_stage_kmajor<BN, THREADS>(Bg + kt * GG_BK, K, 0, BN - 1,
                                   dst + GG_A_IMG, tid);
    else
      gg_stage_rowmajor<BN, THREADS>(Bg + (int64_t)kt * GG_BK * N, N,
                                     dst + GG_A_IMG, tid);
  };

  // NN: one address register per column fragment (buffer 0, k-step 0)
  unsigned baddr[4];
  if constexpr (!TB) {
    const int q = (lane >> 2) & 3, p = lane & 3;
    const int f = q | ((g & 1) << 2);
    const unsigned base = fa_lds_addr(smem) + GG_A_IMG + (8 * g + q) * ROWB;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      baddr[j] = base + ((2 * wc + 32 * j + 8 * p) ^ (f << 5));
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  const int ktiles = K / GG_BK;
  int cur = 0;
  for (int kt = 0; kt < ktiles; ++kt) {
    const bool last = kt + 1 == ktiles;
    if (!last) stage(kt + 1, cur ^ 1);
    fa_wait_tile<NLOAD>(last);
    __builtin_amdgcn_s_barrier();

    const char* abuf = smem + cur * BUF;
    const char* bbuf = abuf + GG_A_IMG;
    unsigned bcur[4];
    if constexpr (!TB) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bcur[j] = baddr[j] + cur * BUF;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr + 16 * i + fr;
        af[i] = *reinterpret_cast<const bf16x8*>(
            abuf + row * 128 + gg_swz(row, 64 * kk + 16 * g));
      }
      if constexpr (TB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = wc + 16 * j + fr;
          bfr[j] = *reinterpret_cast<const bf16x8*>(
              bbuf + row * 128 + gg_swz(row, 64 * kk + 16 * g));
        }
      } else {
        if (kk == 0)
          gg_tr4<0, 4 * ROWB>(bfr, bcur);
        else
          gg_tr4<32 * ROWB, 36 * ROWB>(bfr, bcur);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              bfr[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }

  // ---- epilogue ----
  // acc[i][j][reg] = out[row wr + 16 i + (lane & 15)][col wc + 16 j + 4 g +
  // reg] (first MFMA operand = B fragment): 4 columns per 8-byte store
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = bm + wr + 16 * i + fr;
    const bool ok = gg_row_valid(cnt, row, M, seg);
    if (row < M) {
      bf16* dst = Cg + (int64_t)row * N + bn + wc + 4 * g;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fa_store4_bf16(dst + 16 * j, ok ? acc[i][j][0] : 0.f,
                       ok ? acc[i][j][1] : 0.f, ok ? acc[i][j][2] : 0.f,
                       ok ? acc[i][j][3] : 0.f);
    }
  }
}

// counts[e] = number of entries >= 0 in pos[e, :]; one wave per expert
__global__ __launch_bounds__(64) void moe_slot_counts_kernel(
    const int64_t* __restrict__ pos, int* __restrict__ counts, int C) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int64_t* row = pos + (int64_t)e * C;
  int n = 0;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    const bool filled = c < C && row[min(c, C - 1)] >= 0;
    n += __popcll(__ballot(filled));
  }
  if (lane == 0) counts[e] = n;
}

template <bool TB, int BN>
void gg_launch(const torch::Tensor& a, const torch::Tensor& b,
               torch::Tensor& out, const int* counts, int G, int M, int N,
               int K, int P, int seg) {
  const int tiles_m = (M + GG_BM - 1) / GG_BM, tiles_n = N / BN;
  hipLaunchKernelGGL((grouped_gemm_bf16_kernel<TB, BN>),
                     dim3(tiles_m * tiles_n * G, 1, 1), dim3(2 * BN), 0,
                     hetu_current_stream(), (const bf16*)a.data_ptr(),
                     (const bf16*)b.data_ptr(), (bf16*)out.data_ptr(), counts,
                     M, N, K, P, seg, tiles_m, tiles_n);
}

void gg_check_operand(const char* fn, const char* name,
                      const torch::Tensor& t, const torch::Tensor& a) {
  TORCH_CHECK(t.is_cuda() && t.device() == a.device(), fn, ": ", name,
              " is on ", t.device(), ", a on ", a.device());
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 3, fn, ": ", name, " must be 3-D, got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, ": ",
              name, " must be 16-byte aligned");
}

}  // namespace

// out [G, M, N] = a [G, M, K] @ b [G, K, N]   (trans_b: b [G, N, K], a @ b^T)
// with the invalid rows (see the header) exactly zero.  n_tile: 128 or 256.
torch::Tensor grouped_gemm_bf16(torch::Tensor a, torch::Tensor b,
                                c10::optional<torch::Tensor> counts,
                                int64_t seg, bool trans_b, int64_t n_tile) {
  const char* fn = "grouped_gemm_bf16";
  TORCH_CHECK(a.is_cuda(), fn, ": a must be a GPU tensor");
  gg_check_operand(fn, "a", a, a);
  gg_check_operand(fn, "b", b, a);
  const int64_t G = a.size(0), M = a.size(1), K = a.size(2);
  const int64_t N = b.size(trans_b ? 1 : 2);
  TORCH_CHECK(b.size(0) == G && b.size(trans_b ? 2 : 1) == K, fn, ": b has "
              "shape ", b.sizes(), ", a ", a.sizes(), ", trans_b=", trans_b);
  TORCH_CHECK(n_tile == 128 || n_tile == 256, fn, ": n_tile must be 128 or "
              "256, got ", n_tile);
  TORCH_CHECK(G >= 1 && M >= 1 && K >= GG_BK && K % GG_BK == 0, fn,
              ": a has shape ", a.sizes(), ", K must be a positive multiple "
              "of ", GG_BK);
  TORCH_CHECK(N >= n_tile && N % n_tile == 0, fn, ": b has ", N,
              " output columns, must be a positive multiple of ", n_tile);
  const int64_t tiles = G * ((M + GG_BM - 1) / GG_BM) * (N / n_tile);
  TORCH_CHECK(M * K < (1ll << 31) && N * K < (1ll << 31) &&
              M * N < (1ll << 31) && tiles < (1ll << 31), fn,
              ": a group of ", M, " x ", N, " x ", K, " is too large");
  const int* cnt = nullptr;
  int64_t P = 1;
  if (counts.has_value()) {
    const torch::Tensor& c = *counts;
    TORCH_CHECK(c.is_cuda() && c.device() == a.device(), fn,
                ": counts is on ", c.device(), ", a on ", a.device());
    TORCH_CHECK(c.scalar_type() == at::kInt, fn,
                ": counts must be int32, got ", c.scalar_type());
    TORCH_CHECK(c.is_contiguous(), fn, ": counts must be contiguous");
    TORCH_CHECK(c.dim() == 2 && c.size(0) == G, fn, ": counts must be [G, P]"
                " with G = ", G, ", got ", c.sizes());
    P = c.size(1);
    TORCH_CHECK(seg >= 1 && P * seg == M, fn, ": counts has P = ", P,
                " segments of seg = ", seg, " rows, a has M = ", M, " rows");
    cnt = c.data_ptr<int>();
  } else {
    seg = M;
  }
  auto out = torch::empty({G, M, N}, a.options());
  if (trans_b) {
    if (n_tile == 128) gg_launch<true, 128>(a, b, out, cnt, G, M, N, K, P, seg);
    else gg_launch<true, 256>(a, b, out, cnt, G, M, N, K, P, seg);
  } else {
    if (n_tile == 128) gg_launch<false, 128>(a, b, out, cnt, G, M, N, K, P, seg);
    else gg_launch<false, 256>(a, b, out, cnt, G, M, N, K, P, seg);
  }
  return out;
}

// pos [E, C] int64 -> int32 [E]: filled slots (entries >= 0) per expert
torch::Tensor moe_slot_counts(torch::Tensor pos) {
  const char* fn = "moe_slot_counts";
  TORCH_CHECK(pos.is_cuda(), fn, ": pos must be a GPU tensor");
  TORCH_CHECK(pos.scalar_type() == at::kLong, fn, ": pos must be int64, got ",
              pos.scalar_type());
  TORCH_CHECK(pos.dim() == 2 && pos.is_contiguous(), fn,
              ": pos must be a contiguous [E, C], got ", pos.sizes());
  TORCH_CHECK(pos.size(0) < (1ll << 31) && pos.size(1) < (1ll << 31) - 64, fn,
              ": pos ", pos.sizes(), " is too large");
  TORCH_CHECK(pos.size(0) >= 1 && pos.size(1) >= 1, fn, ": pos ", pos.sizes(),
              " is empty");
  const int E = pos.size(0), C = pos.size(1);
  auto counts = torch::empty({E}, pos.options().dtype(at::kInt));
  hipLaunchKernelGGL(moe_slot_counts_kernel, dim3(E), dim3(64), 0,
                     hetu_current_stream(), pos.data_ptr<int64_t>(),
                     counts.data_ptr<int>(), C);
  return counts;
}
