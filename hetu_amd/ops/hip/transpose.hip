// Bandwidth-bound 2-D transpose of 2-byte elements for gfx950:
//   out[C, R] = in[R, C]^T        (bf16 / fp16; pure data movement)
//
// Feeds F.linear_dgrad(impl="transposed"): the weight W [N, K] is copied to
// Wt [K, N] so that dgrad dx = gy @ W runs in the forward's TN call form.
//
// Fast path (R % 8 == 0, C % 8 == 0, both base pointers 16-B aligned)
// -------------------------------------------------------------------
// One block of 256 threads moves one 64x64-element tile (8 KiB) through LDS.
//   * global read: thread t loads 16 B of tile row (t >> 3) + 32 i, 16-B
//     chunk t & 7 (i = 0, 1).  A wave instruction covers 8 whole rows of
//     128 B.
//   * LDS image: row r is 128 B = 8 chunks of 16 B; chunk k of row r is
//     stored at chunk slot k ^ (r >> 3).  The 8 lanes that write one row
//     (one 8-lane group of ds_write_b128) still fill the whole 128-B row,
//     i.e. all 32 banks once: conflict-free.
//   * LDS read: thread t = 8 p + l owns the column pair (2p, 2p+1) and the
//     8 tile rows 8 l .. 8 l + 7: eight ds_read_b32, read j taking the dword
//     of row 8 l + j that holds the pair.  Its bank is
//     ((p >> 2) ^ l) * 4 + (p & 3).  A 32-lane group of a wave has p >> 2
//     fixed, p & 3 = 0..3 and l = 0..7, so it touches all 32 banks exactly
//     once: conflict-free.
//   * the eight dwords are a 8x2 block; its low halves are 8 consecutive
//     elements of output row 2p, its high halves of output row 2p + 1:
//     two 16-B global stores.  A wave instruction covers 8 whole output
//     rows of 128 B.
// With R and C multiples of 8 every 16-B chunk lies wholly inside or wholly
// outside the tensor, so ragged edges are a per-chunk predicate.
//
// Element path (anything else): the same 64x64 tiling, one element per
// thread and access, LDS rows padded to 33 dwords.
//
// Block order: consecutive block ids walk along an INPUT row band (order 1,
// the default), so the blocks that run at the same time read whole
// neighbouring input rows and write 128-B pieces of neighbouring output
// columns.  Order 0 walks along an OUTPUT row band instead, so that
// concurrent blocks write whole neighbouring output rows; it measured equal
// or slower on every shape (docs/KERNELS.md, "Transpose / dgrad routing")
// and is kept as an argument for scripts/bench_dgrad.py.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include "common.h"
#include "ext_stream.h"

namespace {

constexpr int TR_TILE = 64;
constexpr int TR_THREADS = 256;
constexpr int TR_PITCH = 66;    // element path: 33 dwords per LDS row

typedef unsigned short u16;

DEV void tr_tile_origin(int64_t tiles_r, int64_t tiles_c, int order,
                        int64_t& r0, int64_t& c0) {
  const int64_t id = blockIdx.x;
  int64_t tr, tc;
  if (order == 0) {
    tc = id / tiles_r;
    tr = id % tiles_r;
  } else {
    tr = id / tiles_c;
    tc = id % tiles_c;
  }
  r0 = tr * TR_TILE;
  c0 = tc * TR_TILE;
}

__global__ __launch_bounds__(TR_THREADS) void transpose2d_vec_kernel(
    const u16* __restrict__ in, u16* __restrict__ out, int64_t R, int64_t C,
    int64_t tiles_r, int64_t tiles_c, int order) {
  __shared__ uint4 tile[TR_TILE * 8];
  int64_t r0, c0;
  tr_tile_origin(tiles_r, tiles_c, order, r0, c0);
  const int tid = threadIdx.x;

  // both loads in flight before the first LDS write waits on one
  const int k = tid & 7;
  const int64_t c = c0 + 8 * k;
  uint4 v[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t r = r0 + (tid >> 3) + 32 * i;
    v[i] = make_uint4(0u, 0u, 0u, 0u);
    if (r < R && c < C)
      v[i] = *reinterpret_cast<const uint4*>(in + r * C + c);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rr = (tid >> 3) + 32 * i;
    tile[rr * 8 + (k ^ ((rr >> 3) & 7))] = v[i];
  }
  __syncthreads();

  const int l = tid & 7, p = tid >> 3;
  const u32* t32 = reinterpret_cast<const u32*>(tile);
  u32 d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    d[j] = t32[(8 * l + j) * 32 + ((((p >> 2) ^ l) & 7) << 2) + (p & 3)];
  const int64_t oc = c0 + 2 * p;          // output row (input column)
  const int64_t orow = r0 + 8 * l;        // output column (input row)
  if (oc < C && orow < R) {
    uint4 lo, hi;
    lo.x = (d[0] & 0xffffu) | (d[1] << 16);
    lo.y = (d[2] & 0xffffu) | (d[3] << 16);
    lo.z = (d[4] & 0xffffu) | (d[5] << 16);
    lo.w = (d[6] & 0xffffu) | (d[7] << 16);
    hi.x = (d[0] >> 16) | (d[1] & 0xffff0000u);
    hi.y = (d[2] >> 16) | (d[3] & 0xffff0000u);
    hi.z = (d[4] >> 16) | (d[5] & 0xffff0000u);
    hi.w = (d[6] >> 16) | (d[7] & 0xffff0000u);
    // C % 8 == 0 and oc even: row oc + 1 exists whenever row oc does
    *reinterpret_cast<uint4*>(out + oc * R + orow) = lo;
    *reinterpret_cast<uint4*>(out + (oc + 1) * R + orow) = hi;
  }
}

__global__ __launch_bounds__(TR_THREADS) void transpose2d_elem_kernel(
    const u16* __restrict__ in, u16* __restrict__ out, int64_t R, int64_t C,
    int64_t tiles_r, int64_t tiles_c, int order) {
  __shared__ u16 tile[TR_TILE * TR_PITCH];
  int64_t r0, c0;
  tr_tile_origin(tiles_r, tiles_c, order, r0, c0);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < TR_TILE; rr += 4) {
    const int64_t r = r0 + rr, c = c0 + tx;
    if (r < R && c < C) tile[rr * TR_PITCH + tx] = in[r * C + c];
  }
  __syncthreads();
  for (int cc = ty; cc < TR_TILE; cc += 4) {
    const int64_t c = c0 + cc, r = r0 + tx;
    if (c < C && r < R) out[c * R + r] = tile[tx * TR_PITCH + cc];
  }
}

bool tr_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

// out [C, R] = w [R, C]^T.  `out`, if given, is a contiguous [C, R] tensor of
// w's dtype and device to write into (otherwise a new one is allocated).
torch::Tensor transpose2d(torch::Tensor w, c10::optional<torch::Tensor> out_,
                          int64_t order) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous() &&
                  w.element_size() == 2,
              "transpose2d requires a contiguous 2-D GPU tensor of a 2-byte "
              "element type");
  TORCH_CHECK(order == 0 || order == 1, "transpose2d: order is 0 or 1");
  const int64_t R = w.size(0), C = w.size(1);
  torch::Tensor out =
      out_.has_value() ? *out_ : torch::empty({C, R}, w.options());
  TORCH_CHECK(out.is_cuda() && out.device() == w.device() &&
                  out.scalar_type() == w.scalar_type() && out.dim() == 2 &&
                  out.size(0) == C && out.size(1) == R && out.is_contiguous(),
              "transpose2d: out must be a contiguous [C, R] tensor of the "
              "input's dtype and device");
  if (R == 0 || C == 0) return out;
  const int64_t tiles_r = (R + TR_TILE - 1) / TR_TILE;
  const int64_t tiles_c = (C + TR_TILE - 1) / TR_TILE;
  TORCH_CHECK(tiles_r * tiles_c < (1ll << 31), "transpose2d: too many tiles");
  const u16* src = reinterpret_cast<const u16*>(w.data_ptr());
  u16* dst = reinterpret_cast<u16*>(out.data_ptr());
  const bool vec = R % 8 == 0 && C % 8 == 0 && tr_aligned16(src) &&
                   tr_aligned16(dst);
  const dim3 grid((unsigned)(tiles_r * tiles_c)), block(TR_THREADS);
  if (vec)
    hipLaunchKernelGGL(transpose2d_vec_kernel, grid, block, 0,
                       hetu_current_stream(), src, dst, R, C, tiles_r,
                       tiles_c, (int)order);
  else
    hipLaunchKernelGGL(transpose2d_elem_kernel, grid, block, 0,
                       hetu_current_stream(), src, dst, R, C, tiles_r,
                       tiles_c, (int)order);
  return out;
}
