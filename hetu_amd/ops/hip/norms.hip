// RMSNorm / LayerNorm forward and backward for gfx950, with the optional
// fused residual add of the transformer pre-norm chain.
//
// Three kernels, all memory-bound, all on 16 B/lane vector I/O (VecIO:
// 8 bf16 or 4 fp32) with fp32 arithmetic and fp32 row statistics:
//   norm_fwd_kernel<T, LN, RES>   one 256-thread block per row (grid-stride),
//                                 block reductions for the row statistics
//   norm_bwd_dx_kernel<T, LN>     one wave per row, shuffle reductions only,
//                                 no LDS and no atomics
//   norm_bwd_dwdb_kernel<T, LN>   column sums over a [rows_chunk x 512-col]
//                                 tile per block, combined across row blocks
//                                 by one fp32 atomicAdd per column
// LN compiles in the mean and the bias; without it the kernels are RMSNorm.
// Two host entry points, norm_fwd and norm_bwd, pick the instantiation from
// which optional tensors are present and share one argument check.
// Capability parity: reference RMSNorm.cu / FusedLayerNorm.cu:455-760.
#include <torch/extension.h>

#include <climits>

#include "ext_stream.h"
#include "common.h"

namespace {

constexpr int BLOCK = 256;

// RES: fuse the transformer residual add into the norm — loads x+resid,
// writes the sum (feeds the next residual) alongside y, killing the
// standalone elementwise add kernel (the at::native tail).
template <typename T, bool LN, bool RES>
__global__ void norm_fwd_kernel(const T* __restrict__ x,
                                const T* __restrict__ resid,
                                const T* __restrict__ w,
                                const T* __restrict__ b,
                                T* __restrict__ y,
                                T* __restrict__ sum_out,
                                float* __restrict__ mean_out,
                                float* __restrict__ rstd_out,
                                int64_t rows, int D, float eps) {
  constexpr int V = VecIO<T>::VEC;
  __shared__ float smem[16];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * D;
    const T* rr = RES ? resid + row * D : nullptr;
    T* yr = y + row * D;
    T* sr = RES ? sum_out + row * D : nullptr;
    float s = 0.f, ss = 0.f;
    for (int i = threadIdx.x * V; i < D; i += BLOCK * V) {
      float v[VecIO<T>::VEC];
      VecIO<T>::load(xr + i, v);
      if (RES) {
        float rv[VecIO<T>::VEC];
        VecIO<T>::load(rr + i, rv);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] += rv[j];
        VecIO<T>::store(sr + i, v);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (LN) s += v[j];
        ss += v[j] * v[j];
      }
    }
    float mu = 0.f, rstd;
    if (LN) {
      s = block_sum(s, smem);
      ss = block_sum(ss, smem);
      mu = s / D;
      float var = ss / D - mu * mu;
      rstd = rsqrtf(var + eps);
      if (threadIdx.x == 0) { mean_out[row] = mu; rstd_out[row] = rstd; }
    } else {
      ss = block_sum(ss, smem);
      rstd = rsqrtf(ss / D + eps);
      if (threadIdx.x == 0) rstd_out[row] = rstd;
    }
    const T* sum_r = RES ? sr : xr;
    for (int i = threadIdx.x * V; i < D; i += BLOCK * V) {
      float v[VecIO<T>::VEC], wv[VecIO<T>::VEC], bv[VecIO<T>::VEC];
      VecIO<T>::load(sum_r + i, v);
      VecIO<T>::load(w + i, wv);
      if (LN) VecIO<T>::load(b + i, bv);
#pragma unroll
      for (int j = 0; j < V; ++j)
        v[j] = LN ? (v[j] - mu) * rstd * wv[j] + bv[j]
                  : v[j] * rstd * wv[j];
      VecIO<T>::store(yr + i, v);
    }
  }
}

// dx: a wave owns a row, so both row reductions are shuffles.  With dresid
// the residual-grad accumulation is fused in (the adjoint of add+norm):
// dx = dnorm/dsum + dresid, no standalone add kernel in the backward.
template <typename T, bool LN>
__global__ void norm_bwd_dx_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x,
                                   const T* __restrict__ w,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const T* __restrict__ dresid,
                                   T* __restrict__ dx,
                                   int64_t rows, int D) {
  constexpr int V = VecIO<T>::VEC;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int WV = 256 / 64;
  for (int64_t row = (int64_t)blockIdx.x * WV + wid; row < rows;
       row += (int64_t)gridDim.x * WV) {
    const T* dyr = dy + row * D;
    const T* xr = x + row * D;
    T* dxr = dx + row * D;
    const float mu = LN ? mean[row] : 0.f;
    const float r = rstd[row];
    float c1 = 0.f, c2 = 0.f;
    for (int i = lane * V; i < D; i += 64 * V) {
      float dv[VecIO<T>::VEC], xv[VecIO<T>::VEC], wv[VecIO<T>::VEC];
      VecIO<T>::load(dyr + i, dv);
      VecIO<T>::load(xr + i, xv);
      VecIO<T>::load(w + i, wv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float xhat = (xv[j] - mu) * r;
        float wdy = dv[j] * wv[j];
        c1 += wdy;
        c2 += wdy * xhat;
      }
    }
    c1 = wave_sum(c1) / D;
    c2 = wave_sum(c2) / D;
    for (int i = lane * V; i < D; i += 64 * V) {
      float dv[VecIO<T>::VEC], xv[VecIO<T>::VEC], wv[VecIO<T>::VEC];
      VecIO<T>::load(dyr + i, dv);
      VecIO<T>::load(xr + i, xv);
      VecIO<T>::load(w + i, wv);
      float o[VecIO<T>::VEC];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float xhat = (xv[j] - mu) * r;
        float wdy = dv[j] * wv[j];
        o[j] = LN ? (wdy - c1 - xhat * c2) * r : (wdy - xhat * c2) * r;
      }
      if (dresid != nullptr) {
        float rv[VecIO<T>::VEC];
        VecIO<T>::load(dresid + row * D + i, rv);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] += rv[j];
      }
      VecIO<T>::store(dxr + i, o);
    }
  }
}

// dw/db: column sums of dy*xhat / dy over a [rows_chunk x 512-col] tile
// per block; each thread owns 2 adjacent columns (one dword load per row
// per tensor), one atomicAdd pair per column at the end.
template <typename T, bool LN>
__global__ void norm_bwd_dwdb_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ dw_accum,
                                     float* __restrict__ db_accum,
                                     int64_t rows, int D, int rows_chunk) {
  const int c0 = blockIdx.x * 512 + threadIdx.x * 2;   // my column pair
  if (c0 >= D) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_chunk;
  const int64_t r1 = min((int64_t)rows, r0 + rows_chunk);
  float dw0 = 0.f, dw1 = 0.f, db0 = 0.f, db1 = 0.f;
  for (int64_t row = r0; row < r1; ++row) {
    const float mu = LN ? mean[row] : 0.f;
    const float r = rstd[row];
    float d0, d1, x0, x1;
    if (sizeof(T) == 2) {
      // bf16: one dword load covers the column pair
      union { unsigned u; T t[2]; } dv, xv;
      dv.u = *reinterpret_cast<const unsigned*>(dy + row * D + c0);
      xv.u = *reinterpret_cast<const unsigned*>(x + row * D + c0);
      d0 = (float)dv.t[0]; d1 = (float)dv.t[1];
      x0 = (float)xv.t[0]; x1 = (float)xv.t[1];
    } else {
      d0 = (float)dy[row * D + c0]; d1 = (float)dy[row * D + c0 + 1];
      x0 = (float)x[row * D + c0]; x1 = (float)x[row * D + c0 + 1];
    }
    dw0 += d0 * ((x0 - mu) * r);
    dw1 += d1 * ((x1 - mu) * r);
    if (LN) { db0 += d0; db1 += d1; }
  }
  atomicAdd(dw_accum + c0, dw0);
  atomicAdd(dw_accum + c0 + 1, dw1);
  if (LN) {
    atomicAdd(db_accum + c0, db0);
    atomicAdd(db_accum + c0 + 1, db1);
  }
}

inline int row_grid(int64_t rows) {
  // >> 256 workgroups to fill 256 CUs / 8 XCDs; cap and grid-stride
  int64_t g = rows < 8192 ? rows : 8192;
  return (int)(g > 0 ? g : 1);
}

inline int dx_grid(int64_t rows) {
  int64_t g = (rows + 3) / 4;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), 8192);
}

template <typename T, bool LN>
void norm_bwd_launch(const T* dy, const T* x, const T* w,
                     const float* mean, const float* rstd, const T* dresid,
                     T* dx, float* dw, float* db, int64_t rows, int D,
                     hipStream_t stream) {
  hipLaunchKernelGGL((norm_bwd_dx_kernel<T, LN>), dim3(dx_grid(rows)),
                     dim3(256), 0, stream, dy, x, w, mean, rstd,
                     dresid, dx, rows, D);
  // pick rows_chunk so the grid lands around ~2048 blocks
  int col_blocks = (D + 511) / 512;
  int target = (2048 + col_blocks - 1) / col_blocks;
  int rows_chunk = (int)std::max<int64_t>((rows + target - 1) / target, 64);
  int row_blocks = (int)((rows + rows_chunk - 1) / rows_chunk);
  hipLaunchKernelGGL((norm_bwd_dwdb_kernel<T, LN>),
                     dim3(col_blocks, row_blocks), dim3(256), 0, stream,
                     dy, x, mean, rstd, dw, db, rows, D, rows_chunk);
}

// ---- host side -----------------------------------------------------------

using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

// a named argument of an entry point; t == nullptr when it was not passed
struct NormArg {
  const char* name;
  const Tensor* t;
};
inline NormArg arg(const char* name, const Tensor& t) { return {name, &t}; }
inline NormArg arg(const char* name, const OptTensor& t) {
  return {name, t.has_value() ? &*t : nullptr};
}

template <typename T>
inline T* ptr(const Tensor& t) {
  return t.defined() ? static_cast<T*>(t.data_ptr()) : nullptr;
}
template <typename T>
inline T* ptr(const OptTensor& t) {
  return t.has_value() ? static_cast<T*>(t->data_ptr()) : nullptr;
}

// Everything the kernels take for granted, checked once for both entry
// points before anything is allocated or launched.  x fixes device, dtype
// and [rows, D]; like_x are full activations (dy, resid, dresid), per_col
// the [D] parameters (w, b), per_row the fp32 row statistics (mean, rstd).
// Returns rows.
int64_t check_norm_args(const char* fn, const Tensor& x,
                        std::initializer_list<NormArg> like_x,
                        std::initializer_list<NormArg> per_col,
                        std::initializer_list<NormArg> per_row) {
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kFloat,
              fn, ": x must be bf16 or fp32, got ", x.scalar_type());
  TORCH_CHECK(x.dim() >= 1, fn, ": x needs a last dim to normalize over");
  const int64_t D = x.size(-1);
  const int vec = x.scalar_type() == at::kBFloat16 ? VecIO<bf16>::VEC
                                                   : VecIO<float>::VEC;
  TORCH_CHECK(D > 0 && D <= INT_MAX, fn, ": last dim of x is ", D,
              ", must be in [1, INT_MAX]");
  TORCH_CHECK(D % vec == 0, fn, ": last dim of x is ", D,
              ", must be a multiple of ", vec, " (16 B vector I/O)");
  const int64_t rows = x.numel() / D;
  // vec_io: read or written 16 B at a time from its base pointer
  auto check = [&](const NormArg& a, at::ScalarType dtype, bool vec_io) {
    TORCH_CHECK(a.t->is_cuda() && a.t->device() == x.device(), fn, ": ",
                a.name, " is on ", a.t->device(), ", x on ", x.device());
    TORCH_CHECK(a.t->is_contiguous(), fn, ": ", a.name,
                " must be contiguous");
    TORCH_CHECK(a.t->scalar_type() == dtype, fn, ": ", a.name, " must be ",
                dtype, ", got ", a.t->scalar_type());
    TORCH_CHECK(!vec_io ||
                reinterpret_cast<uintptr_t>(a.t->data_ptr()) % 16 == 0,
                fn, ": ", a.name, " must be 16-byte aligned");
  };
  check(arg("x", x), x.scalar_type(), true);
  for (const NormArg& a : like_x) {
    if (a.t == nullptr) continue;
    check(a, x.scalar_type(), true);
    TORCH_CHECK(a.t->sizes() == x.sizes(), fn, ": ", a.name, " has shape ",
                a.t->sizes(), ", x has ", x.sizes());
  }
  for (const NormArg& a : per_col) {
    if (a.t == nullptr) continue;
    check(a, x.scalar_type(), true);
    TORCH_CHECK(a.t->numel() == D, fn, ": ", a.name, " has ",
                a.t->numel(), " elements, last dim of x is ", D);
  }
  for (const NormArg& a : per_row) {
    if (a.t == nullptr) continue;
    check(a, at::kFloat, false);
    TORCH_CHECK(a.t->numel() == rows, fn, ": ", a.name, " has ",
                a.t->numel(), " elements, x has ", rows, " rows");
  }
  return rows;
}

}  // namespace

// y = norm(x [+ resid]) * w [+ b]; LayerNorm when b is given, else RMSNorm.
// Returns {y, s = x + resid (if resid), mean (if b), rstd}; the statistics
// are fp32 of x's shape without the last dim.
std::vector<Tensor> norm_fwd(Tensor x, OptTensor resid, Tensor w,
                             OptTensor b, double eps) {
  const bool ln = b.has_value(), res = resid.has_value();
  const int64_t rows = check_norm_args(
      "norm_fwd", x, {arg("resid", resid)}, {arg("w", w), arg("b", b)}, {});
  const int D = (int)x.size(-1);
  const auto row_sizes = x.sizes().slice(0, x.dim() - 1);
  const auto stat_opts = x.options().dtype(at::kFloat);
  Tensor y = torch::empty_like(x), s, mean;
  if (res) s = torch::empty_like(x);
  if (ln) mean = torch::empty(row_sizes, stat_opts);
  Tensor rstd = torch::empty(row_sizes, stat_opts);
  if (rows > 0) {
    auto stream = hetu_current_stream();
    DISPATCH_FLOAT(x, "norm_fwd", [&] {
      using T = scalar_t;
      auto kernel =
          ln ? (res ? norm_fwd_kernel<T, true, true>
                    : norm_fwd_kernel<T, true, false>)
             : (res ? norm_fwd_kernel<T, false, true>
                    : norm_fwd_kernel<T, false, false>);
      hipLaunchKernelGGL(kernel, dim3(row_grid(rows)), dim3(BLOCK), 0,
                         stream, ptr<const T>(x), ptr<const T>(resid),
                         ptr<const T>(w), ptr<const T>(b), ptr<T>(y),
                         ptr<T>(s), ptr<float>(mean), ptr<float>(rstd),
                         rows, D, (float)eps);
    });
  }
  std::vector<Tensor> out{y};
  if (res) out.push_back(s);
  if (ln) out.push_back(mean);
  out.push_back(rstd);
  return out;
}

// Backward of norm_fwd over x (the sum s when a residual was fused);
// LayerNorm when mean is given.  dresid, the grad of s from its other
// consumers, is added into dx.  Returns {dx, dw, db (if mean)}: dx is the
// grad of both x and resid, dw/db are summed in fp32 and cast to w's dtype.
std::vector<Tensor> norm_bwd(Tensor dy, Tensor x, Tensor w, OptTensor mean,
                             Tensor rstd, OptTensor dresid) {
  const bool ln = mean.has_value();
  const int64_t rows = check_norm_args(
      "norm_bwd", x, {arg("dy", dy), arg("dresid", dresid)}, {arg("w", w)},
      {arg("mean", mean), arg("rstd", rstd)});
  const int D = (int)x.size(-1);
  const auto acc_opts = x.options().dtype(at::kFloat);
  Tensor dx = torch::empty_like(x), db32;
  Tensor dw32 = torch::zeros({D}, acc_opts);
  if (ln) db32 = torch::zeros({D}, acc_opts);
  if (rows > 0) {
    auto stream = hetu_current_stream();
    DISPATCH_FLOAT(x, "norm_bwd", [&] {
      using T = scalar_t;
      auto launch = ln ? norm_bwd_launch<T, true> : norm_bwd_launch<T, false>;
      launch(ptr<const T>(dy), ptr<const T>(x), ptr<const T>(w),
             ptr<const float>(mean), ptr<const float>(rstd),
             ptr<const T>(dresid), ptr<T>(dx), ptr<float>(dw32),
             ptr<float>(db32), rows, D, stream);
    });
  }
  std::vector<Tensor> out{dx, dw32.to(w.scalar_type())};
  if (ln) out.push_back(db32.to(w.scalar_type()));
  return out;
}
