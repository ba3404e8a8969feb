// Hand-written bf16 MFMA weight-gradient GEMM for gfx950:
//   dW[N, K] = gy[T, N]^T @ x[T, K]     (fp32 accumulate, one bf16 rounding)
//
// "NT over tokens" form: the contraction runs over the token index, which is
// the SLOW dimension of both operands, so no MFMA fragment is contiguous in
// memory.  Both operand tiles are staged as row-major [64 tokens][256
// columns] LDS images with global_load_lds width 16 and the fragments are
// read transposed in hardware with ds_read_b64_tr_b16 (two reads per
// 16x16x32 operand).
//
// Structure (CDNA HIP guide §5, the 256^2 8-phase template, adapted):
//   * 256x256 output tile, BK = 64 tokens, 8 waves as 2 (gy cols) x 4 (x
//     cols), per-wave output 128x64 = 8x4 accumulators of 16x16.
//   * ONE __shared__ object of 128 KiB: [A buf0 | A buf1 | B buf0 | B buf1],
//     each a 32 KiB [64][512 B] image; a "half-tile" is 32 token rows of one
//     operand (16 KiB, two global_load_lds per thread).
//   * 4 phases per K-tile, each {tr reads | stage one half-tile | s_barrier |
//     lgkmcnt(0) | 16 MFMA under s_setprio | s_barrier}; the two wave rows
//     run staggered by one barrier so one wave of every SIMD reads LDS while
//     the other issues MFMAs.
//   * counted s_waitcnt vmcnt(8) twice per K-tile, never 0 in the loop.
//   * bijective XCD-aware block remap; the 32 blocks an XCD runs at a time
//     form an 8x4 rectangle of output tiles.
//
// LDS image and bank derivation
// -----------------------------
// Row t of an image is 512 B (256 bf16), so every row starts on bank 0 of
// the 256-B bank row: unswizzled, the 4 rows x 32 B a 16-lane group touches
// in one ds_read_b64_tr_b16 would sit on the same 8 banks (4-way), and the
// second group of the 32-lane half (8 rows further) on them again (8-way).
// Swizzle: byte-in-row ^= f(t) << 5 with f(t) = (t & 3) | ((t >> 3) & 1) << 2,
// i.e. the 32-B slot index (bits 5..7) is XORed with a value that is
// distinct for the 8 rows {r..r+3, r+8..r+11} one half reads (r % 4 == 0).
// Lane 16g + 4q + p of a wave reads row 32s + 8g + q (+4 for the second
// read) at column bytes c0 + 8p, c0 % 32 == 0.  Within a half (g & 1 = 0, 1;
// q = 0..3) the address mod 256 is ((c0 + 8p) ^ (f << 5)) mod 256 with f
// taking all 8 values: 8 distinct 32-B slots x 4 distinct 8-B pieces = all
// 64 banks exactly once.  Every tr read is conflict-free.  f is unchanged
// by +4, +16 and +32 rows, so the second read (+2048 B), the second k-step
// (+16 KiB) and the second buffer (+32 KiB) are immediate offsets on one
// address register per fragment.
// global_load_lds writes lane-linear, so the swizzle is applied to the
// per-lane SOURCE column (guide rule 21); the XOR stays inside a 256-B
// segment and moves whole 16-B chunks, so the loads stay full-line.
//
// Pipeline order and the vmcnt arithmetic
// ---------------------------------------
// Half-tile (t, s, O): K-tile t, k-step s (token rows 32s..32s+31), operand
// O (B = x, A = gy); buffer = t & 1.  Phase p of tile t uses k-step p >> 1
// and the gy fragments 4(p&1)..4(p&1)+3; even phases also read the 4 x
// fragments of their k-step.  Stage issue order (2 loads each):
//   prologue: (0,0,B) (0,0,A) (0,1,B) (0,1,A) (1,0,B) (1,0,A)
//   tile t:   p0 (t+1,1,B)  p1 (t+1,1,A)  p2 (t+2,0,B)  p3 (t+2,0,A)
// WAR: a region is restaged two phases after its last read ((buf,0,B) read
// in p0 -> restaged p2; (buf,0,A) read p0,p1 -> p3; (buf,1,B) read p2 ->
// next tile's p0; (buf,1,A) read p2,p3 -> next p1).  Two, not one, because
// the staggered wave row retires its phase-j reads (lgkmcnt(0)) only after
// the barrier at which the other row already starts phase j+1.
// RAW: k-step 0 of tile t+1 is first read in (t+1, p0); its last load
// (t+1,0,A) was issued in (t-1, p3), and by the wait in (t, p3) four newer
// half-tiles have been issued: (t+1,1,B) (t+1,1,A) (t+2,0,B) (t+2,0,A) =
// 8 loads -> s_waitcnt vmcnt(8) before the first barrier of p3, read one
// phase later.  Likewise k-step 1 of tile t, first read in (t, p2): its
// last load (t,1,A) is followed by (t+1,0,B) (t+1,0,A) (t+1,1,B) (t+1,1,A)
// at the wait in (t, p1) -> vmcnt(8).  The prologue waits vmcnt(8) after
// its 6 half-tiles (4 newer than (0,0,A)).
// Tiles past the end are not skipped (that would change the counts): the
// tile index is clamped, so the tail re-loads the last K-tile into regions
// that are already dead ("pad, don't mask").  Every lane always holds a
// valid address and EXEC is full throughout, which the tr reads require;
// hence full tiles only.
//
// Bias variant (gemm_wgrad_bias_bf16_kernel)
// ------------------------------------------
// Also writes db[N] = sum_t gy[t, n], the bias gradient of the same Linear,
// which is gy^T @ ones: one more MFMA per phase whose x operand is a
// constant all-ones fragment.  Only the blocks with tk == 0 (one per tile
// row tn after the remap) do it; the choice is ONE block-uniform branch at
// the top of the kernel between two instantiations of the same body, so the
// other blocks run the plain instantiation, with no test in the loop.  In phase
// (S, H) the 4 waves of a wave row hold the same four gy fragments; wave wc
// takes fragment wc, so every wave issues 17 MFMAs and no operand is read
// twice.  To make that choice static the bias blocks keep their fragments
// rotated by wc (wg_frag): fragment wc is always gf[0].  With
// A = ones every row i of D[i][j] = sum_k A[i][k] gy[k][j] holds the 16
// column sums, so lanes 0..15 of one accumulator register carry them: two
// accumulators per wave (one per parity H), fp32 over all of T, rounded
// once.  Each db element has exactly one writer: no atomics, no workspace.
#include "attention_common.h"
#include "ext_stream.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WG_TILE_MN = 256;           // output tile edge
constexpr int WG_BK = 64;                 // tokens per K-tile
constexpr int WG_THREADS = 512;
constexpr int WG_ROW = WG_TILE_MN * 2;    // 512 B image row
constexpr int WG_HALF = 32 * WG_ROW;      // 16 KiB: one k-step of one operand
constexpr int WG_IMG = 2 * WG_HALF;       // 32 KiB: one operand tile
constexpr int WG_B_BASE = 2 * WG_IMG;     // x images start after both gy images
constexpr int WG_LDS = 4 * WG_IMG;        // 128 KiB

template <int OFF>
DEV u32x2 wg_tr_read(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}

// stage half-tile (tile tt, k-step S) of operand OP into buffer BUF; src is
// the thread's base pointer (row tid >> 5, swizzled column folded in)
template <int OP, int BUF, int S>
DEV void wg_stage(const bf16* src, int64_t ld, int tt, char* smem, int tid) {
  const bf16* p = src + ((int64_t)tt * WG_BK + 32 * S) * ld;
  char* dst = smem + OP * WG_B_BASE + BUF * WG_IMG + S * WG_HALF + tid * 16;
  fa_glds16(p, dst);
  fa_glds16(p + 16 * ld, dst + 8192);
}

// which 16-column gy fragment of the wave row's 8 a wave keeps in slot m
// (gf[m & 3] of parity m >> 2, acc[m][*]).  Plain blocks: fragment m.  Bias
// blocks rotate each parity's four by the wave's column wc, so that slot 0
// holds fragment wc, the one whose column sums wave wc owns; the rotation
// costs nothing in the loop (it only permutes the read addresses, set up
// once) and is undone by the epilogue's row offsets.  Every output element
// still sums its K-steps in the same order: dW is bit-identical.
template <bool BIAS>
DEV int wg_frag(int m, int wc) {
  return BIAS ? ((m & 4) | ((m + wc) & 3)) : m;
}

// all-ones bf16 MFMA operand (8 x 1.0)
DEV bf16x8 wg_ones() {
  const u32x2 v = {0x3F803F80u, 0x3F803F80u};
  return fa_join(v, v);
}

// one phase: reads, one half-tile staged, 16 MFMA between two barriers
// (17 with BIAS: the column-sum MFMA, see the header)
template <int BUF, int P, bool BIAS>
DEV void wg_phase(f32x4 (&acc)[8][4], f32x4 (&bacc)[2], bf16x8 (&xf)[4],
                  const unsigned (&aaddr)[8], const unsigned (&baddr)[4],
                  const bf16* pA, const bf16* pB, int64_t ldA, int64_t ldB,
                  int t, int nt, char* smem, int tid, const bf16x8& ones) {
  constexpr int S = P >> 1, H = P & 1;
  constexpr int OFF = BUF * WG_IMG + S * WG_HALF;
  bf16x8 gf[4];
  if constexpr (H == 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n)
      xf[n] = fa_join(wg_tr_read<OFF>(baddr[n]),
                      wg_tr_read<OFF + 4 * WG_ROW>(baddr[n]));
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
    gf[m] = fa_join(wg_tr_read<OFF>(aaddr[4 * H + m]),
                    wg_tr_read<OFF + 4 * WG_ROW>(aaddr[4 * H + m]));
  if constexpr (P == 0)
    wg_stage<1, BUF ^ 1, 1>(pB, ldB, min(t + 1, nt - 1), smem, tid);
  else if constexpr (P == 1)
    wg_stage<0, BUF ^ 1, 1>(pA, ldA, min(t + 1, nt - 1), smem, tid);
  else if constexpr (P == 2)
    wg_stage<1, BUF, 0>(pB, ldB, min(t + 2, nt - 1), smem, tid);
  else
    wg_stage<0, BUF, 0>(pA, ldA, min(t + 2, nt - 1), smem, tid);
  if constexpr (H == 1)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
      acc[4 * H + m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          xf[n], gf[m], acc[4 * H + m][n], 0, 0, 0);
  if constexpr (BIAS)
    // column sums of this wave's share of the phase's gy fragments: the
    // bias blocks read their fragments rotated by wc (wg_frag), so the
    // share is always gf[0]
    bacc[H] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, gf[0], bacc[H],
                                                      0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

template <int BUF, bool BIAS>
DEV void wg_tile(f32x4 (&acc)[8][4], f32x4 (&bacc)[2], bf16x8 (&xf)[4],
                 const unsigned (&aaddr)[8], const unsigned (&baddr)[4],
                 const bf16* pA, const bf16* pB, int64_t ldA, int64_t ldB,
                 int t, int nt, char* smem, int tid, const bf16x8& ones) {
  wg_phase<BUF, 0, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                         smem, tid, ones);
  wg_phase<BUF, 1, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                         smem, tid, ones);
  wg_phase<BUF, 2, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                         smem, tid, ones);
  wg_phase<BUF, 3, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                         smem, tid, ones);
}

// block id -> output tile (tn, tk)
DEV void wg_remap(int tiles_n, int tiles_k, int& tn, int& tk) {
  // ---- XCD-aware bijective remap (T1) ----
  // blocks b, b+8, b+16.. share an XCD; give each XCD a contiguous chunk of
  // work ids, then fold every aligned run of 32 ids (what one XCD's 32 CUs
  // hold at a time at 1 block/CU) into an 8x4 rectangle of output tiles:
  // 12 operand panels through that L2 instead of 64.  This assumes the
  // MI355X's 8 XCDs of 32 CUs.  A run stays on one XCD only when the chunk
  // nwg/8 is a multiple of 32: 32, 96, 128 ids at 256, 768, 1024 tiles.
  // Smaller or odd grids (32, 64, 128 tiles; anything that takes the
  // row-major branch) stay bijective, hence correct, but lose the L2
  // rectangle, which costs speed only; auto does not route them here.
  const int nwg = tiles_n * tiles_k;
  const int orig = blockIdx.x;
  const int q8 = nwg / 8, r8 = nwg % 8;
  const int xcd = orig % 8, slot = orig / 8;
  const int wgid =
      (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  if (tiles_n % 8 == 0 && tiles_k % 4 == 0) {
    const int rect = wgid >> 5, in = wgid & 31;
    const int rects_k = tiles_k >> 2;
    tn = (rect / rects_k) * 8 + (in & 7);
    tk = (rect % rects_k) * 4 + (in >> 3);
  } else {
    tn = wgid / tiles_k;
    tk = wgid % tiles_k;
  }
}

// the whole kernel for output tile (tn, tk); BIAS also writes this tile
// row's 256 elements of db
template <bool BIAS>
DEV void wg_body(const bf16* __restrict__ gy, const bf16* __restrict__ x,
                 bf16* __restrict__ dw, bf16* __restrict__ db, int T, int N,
                 int K, int tn, int tk, char* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid) >> 6;
  const int wr = wid >> 2;                  // gy-column half of the tile
  const int wc = wid & 3;                   // x-column quarter of the tile

  // staging: thread covers image row (tid >> 5) + 16 i, 16 B at linear
  // byte (tid & 31) * 16, which holds the source bytes at that ^ f << 5
  const int srow = tid >> 5;
  const int sf = (srow & 3) | (((srow >> 3) & 1) << 2);
  const int scol = (((tid & 31) * 16) ^ (sf << 5)) >> 1;
  const bf16* pA = gy + (int64_t)srow * N + (int64_t)tn * WG_TILE_MN + scol;
  const bf16* pB = x + (int64_t)srow * K + (int64_t)tk * WG_TILE_MN + scol;
  const int64_t ldA = N, ldB = K;
  const int nt = T / WG_BK;

  // tr-read addresses: lane 16g + 4q + p supplies row 8g + q, bytes c0 + 8p
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int f = q | ((g & 1) << 2);
  const unsigned lds0 = fa_lds_addr(smem);
  const unsigned rowb = (8 * g + q) * WG_ROW;
  unsigned aaddr[8], baddr[4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
    aaddr[m] = lds0 + rowb +
               ((256 * wr + 32 * wg_frag<BIAS>(m, wc) + 8 * p) ^ (f << 5));
#pragma unroll
  for (int n = 0; n < 4; ++n)
    baddr[n] = lds0 + WG_B_BASE + rowb +
               ((128 * wc + 32 * n + 8 * p) ^ (f << 5));

  f32x4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = {0.f, 0.f, 0.f, 0.f};
  // bias variant only (dead code otherwise): the column-sum accumulators,
  // the all-ones x operand
  f32x4 bacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const bf16x8 ones = wg_ones();
  bf16x8 xf[4];

  // ---- prologue: tile 0 and k-step 0 of tile 1 ----
  const int t1 = min(1, nt - 1);
  wg_stage<1, 0, 0>(pB, ldB, 0, smem, tid);
  wg_stage<0, 0, 0>(pA, ldA, 0, smem, tid);
  wg_stage<1, 0, 1>(pB, ldB, 0, smem, tid);
  wg_stage<0, 0, 1>(pA, ldA, 0, smem, tid);
  wg_stage<1, 1, 0>(pB, ldB, t1, smem, tid);
  wg_stage<0, 1, 0>(pA, ldA, t1, smem, tid);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  // stagger: the second wave row runs one barrier behind the first
  if (wr == 1) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int t = 0;
  for (; t + 1 < nt; t += 2) {
    wg_tile<0, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                     smem, tid, ones);
    wg_tile<1, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t + 1, nt,
                     smem, tid, ones);
  }
  if (t < nt)
    wg_tile<0, BIAS>(acc, bacc, xf, aaddr, baddr, pA, pB, ldA, ldB, t, nt,
                     smem, tid, ones);

  // drain the (dead) tail loads before the workgroup's LDS can be released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wr == 0) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue ----
  // acc[m][n] = D[i][j], i = x column 16n + 4g + reg (A operand = x
  // fragment), j = gy column 16m + (lane & 15): 4 consecutive dW columns
  // per lane -> one 8-byte store
  const int64_t row0 = (int64_t)tn * WG_TILE_MN + 128 * wr + (lane & 15);
  const int64_t col0 = (int64_t)tk * WG_TILE_MN + 64 * wc + 4 * g;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
      fa_store4_bf16(dw + (row0 + 16 * wg_frag<BIAS>(m, wc)) * K + col0 +
                         16 * n,
                     acc[m][n][0], acc[m][n][1], acc[m][n][2], acc[m][n][3]);
  if constexpr (BIAS) {
    // bacc[H][reg] = column sum of gy column 16 (4H + wc) + (lane & 15) of
    // this wave row's half, the same in every row 4g + reg: lanes 0..15
    // store register 0.  tn * 256 + 128 wr + 16 (4H + wc) + (lane & 15)
    // < N by the full-tile precondition.
    if (lane < 16) {
      unsigned short* d = reinterpret_cast<unsigned short*>(db) +
                          (int64_t)tn * WG_TILE_MN + 128 * wr + 16 * wc + lane;
      const unsigned w = fa_cvt_pk(bacc[0][0], bacc[1][0]);
      d[0] = (unsigned short)(w & 0xffffu);
      d[64] = (unsigned short)(w >> 16);
    }
  }
}

__global__ __launch_bounds__(WG_THREADS) void gemm_wgrad_bf16_kernel(
    const bf16* __restrict__ gy, const bf16* __restrict__ x,
    bf16* __restrict__ dw, int T, int N, int K, int tiles_n, int tiles_k) {
  __shared__ __attribute__((aligned(1024))) char smem[WG_LDS];
  int tn, tk;
  wg_remap(tiles_n, tiles_k, tn, tk);
  wg_body<false>(gy, x, dw, nullptr, T, N, K, tn, tk, smem);
}

// the same, plus db[N] = column sums of gy, written by the tk == 0 blocks
__global__ __launch_bounds__(WG_THREADS) void gemm_wgrad_bias_bf16_kernel(
    const bf16* __restrict__ gy, const bf16* __restrict__ x,
    bf16* __restrict__ dw, bf16* __restrict__ db, int T, int N, int K,
    int tiles_n, int tiles_k) {
  __shared__ __attribute__((aligned(1024))) char smem[WG_LDS];
  int tn, tk;
  wg_remap(tiles_n, tiles_k, tn, tk);
  if (tk == 0)
    wg_body<true>(gy, x, dw, db, T, N, K, tn, tk, smem);
  else
    wg_body<false>(gy, x, dw, db, T, N, K, tn, tk, smem);
}

// input check of the entry point; functional._wgrad_hip_eligible is the
// routing rule and must not admit more than this
bool wg_eligible(const torch::Tensor& gy, const torch::Tensor& x) {
  return gy.is_cuda() && x.is_cuda() && gy.device() == x.device() &&
         gy.dim() == 2 && x.dim() == 2 &&
         gy.scalar_type() == at::kBFloat16 &&
         x.scalar_type() == at::kBFloat16 && gy.is_contiguous() &&
         x.is_contiguous() && gy.size(0) == x.size(0) && gy.size(0) > 0 &&
         gy.size(0) % WG_BK == 0 && gy.size(1) > 0 && x.size(1) > 0 &&
         gy.size(1) % WG_TILE_MN == 0 && x.size(1) % WG_TILE_MN == 0 &&
         gy.size(0) < (1ll << 31) && gy.size(1) < (1ll << 31) &&
         x.size(1) < (1ll << 31);
}

}  // namespace

// dW[N, K] = gy[T, N]^T @ x[T, K]
torch::Tensor gemm_wgrad_bf16(torch::Tensor gy, torch::Tensor x) {
  TORCH_CHECK(wg_eligible(gy, x),
              "gemm_wgrad_bf16 requires contiguous 2-D bf16 operands on one "
              "GPU: "
              "gy [T, N], x [T, K] with N % 256 == 0, K % 256 == 0 and "
              "T % 64 == 0 (callers route everything else to the library)");
  const int T = gy.size(0), N = gy.size(1), K = x.size(1);
  auto dw = torch::empty({N, K}, x.options());
  const int tiles_n = N / WG_TILE_MN, tiles_k = K / WG_TILE_MN;
  hipLaunchKernelGGL(gemm_wgrad_bf16_kernel, dim3(tiles_n * tiles_k),
                     dim3(WG_THREADS), 0, hetu_current_stream(),
                     (const bf16*)gy.data_ptr(), (const bf16*)x.data_ptr(),
                     (bf16*)dw.data_ptr(), T, N, K, tiles_n, tiles_k);
  return dw;
}

// (dW[N, K] = gy^T @ x, db[N] = column sums of gy) from one launch
std::vector<torch::Tensor> gemm_wgrad_bias_bf16(torch::Tensor gy,
                                                torch::Tensor x) {
  TORCH_CHECK(wg_eligible(gy, x),
              "gemm_wgrad_bias_bf16 requires contiguous 2-D bf16 operands on "
              "one GPU: "
              "gy [T, N], x [T, K] with N % 256 == 0, K % 256 == 0 and "
              "T % 64 == 0 (callers route everything else to the library)");
  const int T = gy.size(0), N = gy.size(1), K = x.size(1);
  auto dw = torch::empty({N, K}, x.options());
  auto db = torch::empty({N}, gy.options());
  const int tiles_n = N / WG_TILE_MN, tiles_k = K / WG_TILE_MN;
  hipLaunchKernelGGL(gemm_wgrad_bias_bf16_kernel, dim3(tiles_n * tiles_k),
                     dim3(WG_THREADS), 0, hetu_current_stream(),
                     (const bf16*)gy.data_ptr(), (const bf16*)x.data_ptr(),
                     (bf16*)dw.data_ptr(), (bf16*)db.data_ptr(), T, N, K,
                     tiles_n, tiles_k);
  return {dw, db};
}
