// Candidate side of the mixed continuous / categorical GP (mixed_kernel.hip's kernel) on gfx950:
// what an acquisition chain needs beside evr_mixed_kernel_matrix to run on a mixed model.
//
// evr_mixed_split: raw transformed rows (continuous columns + one-hot blocks) -> normalised
// continuous columns Xc and category codes Cc ([upstream] Normalize + OneHotToNumeric).
// evr_mixed_kernel_cross_grad: the X-gradient of K(train, candidates), kcross_grad_kernel's
// pattern — a thread per candidate column, four row groups per workgroup, the training rows
// split over blockIdx.y into partials, then a fixed-order reduction that scatters the dc
// continuous columns into the d-wide dX (one-hot columns exactly 0).  No atomics.
#include <algorithm>

#include "common.hpp"
#include "../../include/everest_amd.h"

namespace evr {

constexpr int MX_MAXD = 32;   // continuous columns
constexpr int MX_MAXC = 8;    // categorical features

// thread per (row, slot): slots [0, dc) the continuous columns, [dc, dc + nc) the features.
// Column indices outside the row (a malformed map) read nothing: 0 / code 0.
__global__ __launch_bounds__(256) void mixed_split_kernel(int rows, int d, int dc, int nc,
                                                          const double* __restrict__ X,
                                                          const double* __restrict__ shift,
                                                          const double* __restrict__ scale,
                                                          const int* __restrict__ cont_idx,
                                                          const int* __restrict__ cat_start,
                                                          const int* __restrict__ cat_len, double* __restrict__ Xc,
                                                          int* __restrict__ Cc) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int slots = dc + nc;
  if (e >= (long long)rows * slots) return;
  const int r = (int)(e / slots), t = (int)(e - (long long)r * slots);
  const double* x = X + (size_t)r * d;
  if (t < dc) {
    const int col = cont_idx[t];
    double v = 0.0;
    if (col >= 0 && col < d) v = (x[col] - shift[col]) * scale[col];
    Xc[(size_t)r * dc + t] = v;
  } else {
    const int f = t - dc;
    const int c0 = cat_start[f], len = cat_len[f];
    int am = 0;
    if (c0 >= 0 && len >= 1 && c0 + len <= d) {
      double best = x[c0];
      for (int l = 1; l < len; ++l)
        if (x[c0 + l] > best) {   // strict: the first maximum wins a tie
          best = x[c0 + l];
          am = l;
        }
    }
    Cc[(size_t)r * nc + f] = am;
  }
}

// part[split][c][k] = sum_b sum_{i in split} G[b][i][c] (s_sum k_c'(r1^2) / ls1_k^2
//                                                  + s_prod h2 k_c'(r2^2) / ls2_k^2) (x2_ck - x1_ik)
// The candidate tile (64 rows of X2c, their codes) is staged in LDS once; a member's 1 / ls1,
// 1 / ls2, 1 / (nc lam2) and scales are staged per member.  The training row of a row group is
// wave-uniform (scalar loads).  acc[] is the only per-lane array: the differences are formed
// twice (as kcross_grad_kernel does above 16 columns) so that no instantiation spills.
template <int MAXD>
__global__ __launch_bounds__(256) void mixed_kcross_grad_kernel(int kind, int B, int n, int n2, int dc, int nc,
                                                                int rows_per, const double* __restrict__ Xc,
                                                                const int* __restrict__ C,
                                                                const double* __restrict__ X2c,
                                                                const int* __restrict__ C2,
                                                                const double* __restrict__ params,
                                                                const double* __restrict__ G,
                                                                double* __restrict__ part) {
  constexpr int LD = MAXD + 1;   // odd row stride: lane cx reads x2_s[cx * LD + k] without bank conflicts
  __shared__ double x2_s[64 * LD];
  __shared__ double red[64 * LD];
  __shared__ int c2_s[MX_MAXC * 64];   // [f][column]
  __shared__ double il1[MAXD], il2[MAXD], w2[MX_MAXC], sc_s[2];
  const int tid = threadIdx.x;
  const int cx = tid & 63;
  const int ry = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.x * 64, c = c0 + cx;
  const int split = blockIdx.y;
  const int i0 = split * rows_per, i1 = min(n, i0 + rows_per);
  const int P = 2 * dc + 2 * nc + 3;
  for (int e = tid; e < 64 * dc; e += 256) {
    const int r = e / dc, k = e - r * dc;
    x2_s[r * LD + k] = c0 + r < n2 ? X2c[(size_t)(c0 + r) * dc + k] : 0.0;
  }
  for (int e = tid; e < 64 * nc; e += 256) {
    const int r = e / nc, f = e - r * nc;
    c2_s[f * 64 + r] = c0 + r < n2 ? C2[(size_t)(c0 + r) * nc + f] : 0;
  }
  double acc[MAXD];
#pragma unroll
  for (int k = 0; k < MAXD; ++k) acc[k] = 0.0;
  const double* x2 = x2_s + cx * LD;
  for (int b = 0; b < B; ++b) {
    const double* pb = params + (size_t)b * P;
    __syncthreads();
    if (tid < MAXD) {
      il1[tid] = tid < dc ? 1.0 / pb[tid] : 0.0;
      il2[tid] = tid < dc ? 1.0 / pb[dc + tid] : 0.0;
    }
    if (tid >= 64 && tid < 64 + MX_MAXC) {
      const int f = tid - 64;
      w2[f] = f < nc ? 1.0 / ((double)nc * pb[2 * dc + nc + f]) : 0.0;
    }
    if (tid == 128) {
      sc_s[0] = pb[P - 3];
      sc_s[1] = pb[P - 1];
    }
    __syncthreads();
    if (c >= n2) continue;
    const double s_sum = sc_s[0], s_prod = sc_s[1];
    const double* Gc = G + (size_t)b * n * n2 + c;
#pragma unroll 1
    for (int i = i0 + ry; i < i1; i += 4) {
      const double g = Gc[(size_t)i * n2];
      const double* x1 = Xc + (size_t)i * dc;
      const int* c1 = C + (size_t)i * nc;
      double q1 = 0.0, q2 = 0.0;
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < dc) {
          const double df = x2[k] - x1[k];
          const double t1 = df * il1[k], t2 = df * il2[k];
          q1 = fma(t1, t1, q1);
          q2 = fma(t2, t2, q2);
        }
      double e2 = 0.0;
#pragma unroll
      for (int f = 0; f < MX_MAXC; ++f)
        if (f < nc && c2_s[f * 64 + cx] != c1[f]) e2 += w2[f];
      const double h2 = exp_k(-e2);
      const double u1 = g * s_sum * kernel_dscale(kind, q1);
      const double u2 = g * s_prod * h2 * kernel_dscale(kind, q2);
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < dc) {
          const double df = x2[k] - x1[k];
          const double a1 = il1[k], a2 = il2[k];
          acc[k] = fma(u1, (df * a1) * a1, acc[k]);   // (x2 - x1) / ls1^2
          acc[k] = fma(u2, (df * a2) * a2, acc[k]);   // (x2 - x1) / ls2^2
        }
    }
  }
  // the four row groups in order: ((g0 + g1) + g2) + g3
  for (int w = 1; w < 4; ++w) {
    __syncthreads();
    if (ry == w) {
#pragma unroll
      for (int k = 0; k < MAXD; ++k) red[cx * LD + k] = acc[k];
    }
    __syncthreads();
    if (ry == 0) {
#pragma unroll
      for (int k = 0; k < MAXD; ++k) acc[k] += red[cx * LD + k];
    }
  }
  if (ry == 0 && c < n2) {
#pragma unroll
    for (int k = 0; k < MAXD; ++k)
      if (k < dc) part[((size_t)split * n2 + c) * dc + k] = acc[k];
  }
}

// dX[j][t] (rows x d): the continuous column k with cont_idx[k] == t takes the partials in split
// order times scale[t]; every other column is 0.
__global__ __launch_bounds__(256) void mixed_kcross_grad_reduce(int nsplit, int n2, int d, int dc,
                                                                const double* __restrict__ part,
                                                                const double* __restrict__ scale,
                                                                const int* __restrict__ cont_idx,
                                                                double* __restrict__ dX) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)n2 * d) return;
  const int j = (int)(e / d), t = (int)(e - (long long)j * d);
  int k = -1;
  for (int kk = 0; kk < dc; ++kk)
    if (cont_idx[kk] == t) {
      k = kk;
      break;
    }
  if (k < 0) {
    dX[e] = 0.0;
    return;
  }
  double v = 0.0;
  for (int s = 0; s < nsplit; ++s) v += part[((size_t)s * n2 + j) * dc + k];
  dX[e] = v * scale[t];
}

// kcross_grad's row split: up to 2048 workgroups, at least 8 rows each
static int mixed_kcross_nsplit(int n, int n2) {
  const int ct = cdiv(n2, 64);
  return std::max(1, std::min(cdiv(2048, ct), cdiv(n, 8)));
}

bool mixed_model_sizes_ok(int kind, int B, int dc, int nc) {
  return kind >= 0 && kind <= 3 && B >= 1 && dc >= 1 && dc <= MX_MAXD && nc >= 1 && nc <= MX_MAXC;
}

size_t mixed_kcross_grad_ws_doubles(int n, int rows, int dc) {
  return (size_t)mixed_kcross_nsplit(n, rows) * rows * dc;
}

int mixed_kcross_grad_launch(hipStream_t s, int kind, int B, int n, int rows, int d, int dc, int nc, const double* Xc,
                             const int* C, const double* X2c, const int* C2, const double* params,
                             const double* scale, const int* cont_idx, const double* G, double* dX, double* work) {
  const int ns = mixed_kcross_nsplit(n, rows);
  const int rows_per = cdiv(n, ns);
  const dim3 grid(cdiv(rows, 64), ns);
#define LAUNCH(MD) \
  mixed_kcross_grad_kernel<MD><<<grid, 256, 0, s>>>(kind, B, n, rows, dc, nc, rows_per, Xc, C, X2c, C2, params, G, work)
  if (dc <= 8) LAUNCH(8);
  else if (dc <= 16) LAUNCH(16);
  else LAUNCH(32);
#undef LAUNCH
  EVR_LAUNCH_CHECK();
  mixed_kcross_grad_reduce<<<cdiv((long long)rows * d, 256), 256, 0, s>>>(ns, rows, d, dc, work, scale, cont_idx, dX);
  EVR_LAUNCH_CHECK();
  return 0;
}

int mixed_split_launch(hipStream_t s, int rows, int d, int dc, int nc, const double* X, const double* shift,
                       const double* scale, const int* cont_idx, const int* cat_start, const int* cat_len, double* Xc,
                       int* Cc) {
  mixed_split_kernel<<<cdiv((long long)rows * (dc + nc), 256), 256, 0, s>>>(rows, d, dc, nc, X, shift, scale, cont_idx,
                                                                          cat_start, cat_len, Xc, Cc);
  EVR_LAUNCH_CHECK();
  return 0;
}

}  // namespace evr

using namespace evr;

extern "C" {

int evr_mixed_split(void* stream, int rows, int d, int dc, int nc, const double* X, const double* shift,
                    const double* scale, const int* cont_idx, const int* cat_start, const int* cat_len, double* Xc,
                    int* Cc) {
  EVR_CHECK(mixed_model_sizes_ok(0, 1, dc, nc) && d >= dc + nc,
            "evr_mixed_split: unsupported d=%d dc=%d nc=%d (1 <= dc <= %d, 1 <= nc <= %d, d >= dc + nc)", d, dc, nc,
            MX_MAXD, MX_MAXC);
  EVR_CHECK(rows >= 0, "evr_mixed_split: rows=%d", rows);
  if (rows == 0) return 0;
  EVR_CHECK(X && shift && scale && cont_idx && cat_start && cat_len && Xc && Cc, "evr_mixed_split: null argument");
  return mixed_split_launch((hipStream_t)stream, rows, d, dc, nc, X, shift, scale, cont_idx, cat_start, cat_len, Xc,
                            Cc);
}

long long evr_mixed_kernel_cross_grad_workspace_doubles(int n, int rows, int dc) {
  return (n > 0 && rows > 0 && dc > 0) ? (long long)mixed_kcross_grad_ws_doubles(n, rows, dc) : 0;
}

int evr_mixed_kernel_cross_grad(void* stream, int kind, int B, int n, int rows, int d, int dc, int nc,
                                const double* Xc, const int* C, const double* X2c, const int* C2,
                                const double* params, const double* scale, const int* cont_idx, const double* G,
                                double* dX, double* work) {
  EVR_CHECK(mixed_model_sizes_ok(kind, B, dc, nc) && d >= dc + nc,
            "evr_mixed_kernel_cross_grad: unsupported kind=%d B=%d d=%d dc=%d nc=%d (one family 0..3, "
            "1 <= dc <= %d, 1 <= nc <= %d, d >= dc + nc)", kind, B, d, dc, nc, MX_MAXD, MX_MAXC);
  EVR_CHECK(n >= 1 && rows >= 0, "evr_mixed_kernel_cross_grad: bad sizes n=%d rows=%d", n, rows);
  if (rows == 0) return 0;
  EVR_CHECK(Xc && C && X2c && C2 && params && scale && cont_idx && G && dX,
            "evr_mixed_kernel_cross_grad: null argument");
  EVR_CHECK(cdiv(n, 8) <= 65535, "evr_mixed_kernel_cross_grad: n=%d too large", n);
  hipStream_t s = (hipStream_t)stream;
  const bool own = work == nullptr;
  if (own) EVR_HIP(hipMallocAsync((void**)&work, sizeof(double) * mixed_kcross_grad_ws_doubles(n, rows, dc), s));
  const int rc = mixed_kcross_grad_launch(s, kind, B, n, rows, d, dc, nc, Xc, C, X2c, C2, params, scale, cont_idx, G,
                                          dX, work);
  if (own) EVR_HIP(hipFreeAsync(work, s));
  return rc;
}

}  // extern "C"
