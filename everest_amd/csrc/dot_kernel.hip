// Dot-product GP kernels (gpytorch LinearKernel / PolynomialKernel behind the reference's
// LinearSurrogate / PolynomialSurrogate) on gfx950.  Everything is a function of the Gram matrix
// G = X1n X2n^T of the normalised inputs, which evr_gemm_f64 (transB) provides:
//
//   power = 0       k = theta g                      (theta = the variance v)
//   power = p >= 1  k = (g + theta)^p                (theta = the offset c)
//
// Integer powers are formed in one fixed order, with contraction off and never through pow():
//   t = g + theta,  r_1 = t,  r_{k+1} = r_k * t  (k = 1 .. p - 1),  k = r_p.
// The theta derivative is g (power 0), exactly 1 (p = 1), and (double)p * r_{p-1} (p >= 2).
//
// evr_dot_kernel_apply: element-wise map of G for B members (G is read once, every member's K is
// written from the same registers), double2 loads and stores when the element count is even.
// evr_dot_kernel_theta_grad: a wave per row of W, a fixed xor butterfly, per-row partials, then a
// fixed-order sum of the rows.  No atomics.
// evr_dot_gp_posterior: normalise the test rows, cross Gram, apply, R = M K*, finalise — the prior
// variance of each test point comes from its own normalised row.
#include "common.hpp"
#include "../../include/everest_amd.h"

namespace evr {

constexpr int DOT_MAX_POWER = 8;

// k(g; theta) in the documented order
__device__ __forceinline__ double dot_value(int power, double g, double theta) {
#pragma clang fp contract(off)
  if (power == 0) return theta * g;
  const double t = g + theta;
  double r = t;
  for (int k = 1; k < power; ++k) r = r * t;
  return r;
}

// dk / dtheta in the documented order
__device__ __forceinline__ double dot_dtheta(int power, double g, double theta) {
#pragma clang fp contract(off)
  if (power == 0) return g;
  if (power == 1) return 1.0;
  const double t = g + theta;
  double r = t;
  for (int k = 2; k < power; ++k) r = r * t;
  return (double)power * r;
}

// K[b][e] = f(G[e]; theta_b) (+ diag_add[b] where row == column), e the flat index into the
// n1 x n2 matrix.  VEC: a thread owns the elements 2 q and 2 q + 1 (N = n1 n2 even, so member
// b's matrix K + b N keeps G's 16-byte alignment); otherwise one element per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void dot_apply_kernel(int power, int B, unsigned n2, unsigned N,
                                                        const double* __restrict__ G,
                                                        const double* __restrict__ theta,
                                                        const double* __restrict__ dg, double* __restrict__ K) {
#pragma clang fp contract(off)
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if constexpr (VEC) {
    const unsigned e = 2u * q;
    if (e >= N) return;
    const double2 g = *reinterpret_cast<const double2*>(G + e);
    const unsigned i0 = e / n2, j0 = e - i0 * n2;
    // the second element: the next column, or the first column of the next row
    const unsigned i1 = j0 + 1 == n2 ? i0 + 1 : i0, j1 = j0 + 1 == n2 ? 0u : j0 + 1;
    for (int b = 0; b < B; ++b) {
      const double th = theta[b];
      double2 v;
      v.x = dot_value(power, g.x, th);
      v.y = dot_value(power, g.y, th);
      if (dg) {
        const double a = dg[b];
        if (i0 == j0) v.x += a;
        if (i1 == j1) v.y += a;
      }
      *reinterpret_cast<double2*>(K + (size_t)b * N + e) = v;
    }
  } else {
    if (q >= N) return;
    const double g = G[q];
    const unsigned i = q / n2, j = q - i * n2;
    for (int b = 0; b < B; ++b) {
      double v = dot_value(power, g, theta[b]);
      if (dg && i == j) v += dg[b];
      K[(size_t)b * N + q] = v;
    }
  }
}

// part[b][i] = sum_j W[b][i][j] df(G[i][j]; theta_b): a wave per row (four rows per workgroup),
// lane l sums its columns in ascending order (VEC: the pairs 2 l, 2 l + 1, then + 128, ...;
// otherwise l, l + 64, ...), then a fixed xor butterfly.
template <bool VEC>
__global__ __launch_bounds__(256) void dot_grad_rows_kernel(int power, int n, const double* __restrict__ G,
                                                            const double* __restrict__ theta,
                                                            const double* __restrict__ W,
                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;   // whole waves
  const double th = theta[b];
  const double* Gr = G + (size_t)i * n;
  const double* Wr = W + ((size_t)b * n + i) * n;
  double acc = 0.0;
  if constexpr (VEC) {
    for (int j = 2 * lane; j < n; j += 128) {   // n even: j + 1 < n
      const double2 g = *reinterpret_cast<const double2*>(Gr + j);
      const double2 w = *reinterpret_cast<const double2*>(Wr + j);
      acc = fma(w.x, dot_dtheta(power, g.x, th), acc);
      acc = fma(w.y, dot_dtheta(power, g.y, th), acc);
    }
  } else {
    for (int j = lane; j < n; j += 64) acc = fma(Wr[j], dot_dtheta(power, Gr[j], th), acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) part[(size_t)b * n + i] = acc;
}

// g[b] = sum_i part[b][i]: one workgroup per member, strided partials + a fixed LDS tree
// (mixed_colsum_kernel's order)
__global__ __launch_bounds__(256) void dot_grad_sum_kernel(int n, const double* __restrict__ part,
                                                           double* __restrict__ out) {
  const int b = blockIdx.x;
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[(size_t)b * n + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b] = red[0];
}

// Xt[r][k] = (X[r][k] - shift[k]) * scale[k]: exactly that subtraction and product
// (shift / scale NULL: the identity)
__global__ __launch_bounds__(256) void dot_normalize_kernel(long long total, int d, const double* __restrict__ X,
                                                            const double* __restrict__ shift,
                                                            const double* __restrict__ scale,
                                                            double* __restrict__ Xt) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % d);
  double v = X[e];
  if (shift) v = v - shift[k];
  if (scale) v = v * scale[k];
  Xt[e] = v;
}

// Moments of R[b] ((n + 1) x nt): 64 test points per workgroup, four row groups (rows
// i = g, g + 4, ... in ascending order), combined as (s0 + s1) + (s2 + s3).  The prior variance
// of test point t is formed from its own normalised row: q = sum_k xt_k^2 (k ascending, fma),
// k(x, x) = theta q or (q + theta)^p in dot_value's order.
__global__ __launch_bounds__(256) void dot_finalize_kernel(int power, int n, int nt, int d,
                                                           const double* __restrict__ R,
                                                           const double* __restrict__ Xt,
                                                           const double* __restrict__ theta,
                                                           const double* __restrict__ c,
                                                           const double* __restrict__ ym,
                                                           const double* __restrict__ ys,
                                                           const double* __restrict__ noise_add,
                                                           double* __restrict__ mean, double* __restrict__ var) {
#pragma clang fp contract(off)
  __shared__ double red[4][64];
  const int b = blockIdx.y;
  const int tx = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + tx;
  const double* Rb = R + (size_t)b * (n + 1) * nt;
  double s = 0.0;
  if (t < nt)
    for (int i = grp; i < n; i += 4) {
      const double r = Rb[(size_t)i * nt + t];
      s = fma(r, r, s);
    }
  red[grp][tx] = s;
  __syncthreads();
  if (grp != 0 || t >= nt) return;
  const double ss = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
  const double* x = Xt + (size_t)t * d;
  double q = 0.0;
  for (int k = 0; k < d; ++k) q = fma(x[k], x[k], q);
  const double kxx = dot_value(power, q, theta[b]);
  const double sd = ys[b];
  const double na = noise_add ? noise_add[b] : 0.0;
  mean[(size_t)b * nt + t] = ym[b] + sd * (c[b] + Rb[(size_t)n * nt + t]);
  var[(size_t)b * nt + t] = sd * sd * ((kxx - ss) + na);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int dot_apply_launch(hipStream_t s, int power, int B, int n1, int n2, const double* G, const double* theta,
                            const double* diag_add, double* K) {
  const unsigned N = (unsigned)n1 * (unsigned)n2;
  if (N % 2 == 0 && aligned16(G) && aligned16(K))
    dot_apply_kernel<true><<<cdiv(N / 2, 256), 256, 0, s>>>(power, B, (unsigned)n2, N, G, theta, diag_add, K);
  else
    dot_apply_kernel<false><<<cdiv(N, 256), 256, 0, s>>>(power, B, (unsigned)n2, N, G, theta, diag_add, K);
  EVR_LAUNCH_CHECK();
  return 0;
}

// doubles rounded up to an even count: every block of the workspace stays 16-byte aligned
static long long even_up(long long v) { return (v + 1) & ~1ll; }

}  // namespace evr

using namespace evr;

extern "C" {

int evr_dot_kernel_apply(void* stream, int power, int B, int n1, int n2, const double* G, const double* theta,
                         const double* diag_add, double* K) {
  EVR_CHECK(power >= 0 && power <= DOT_MAX_POWER,
            "evr_dot_kernel_apply: unsupported power=%d (0 = linear, 1 <= p <= %d = polynomial)", power,
            DOT_MAX_POWER);
  EVR_CHECK(B >= 1 && n1 >= 0 && n2 >= 0, "evr_dot_kernel_apply: bad sizes B=%d n1=%d n2=%d", B, n1, n2);
  if (n1 == 0 || n2 == 0) return 0;
  EVR_CHECK((long long)n1 * n2 < (1ll << 31), "evr_dot_kernel_apply: n1 * n2 = %lld too large",
            (long long)n1 * n2);
  EVR_CHECK(G && theta && K, "evr_dot_kernel_apply: null argument");
  EVR_CHECK(G != K, "evr_dot_kernel_apply: G and K must not alias (G is shared by the members)");
  return dot_apply_launch((hipStream_t)stream, power, B, n1, n2, G, theta, diag_add, K);
}

int evr_dot_kernel_theta_grad(void* stream, int power, int B, int n, const double* G, const double* theta,
                              const double* W, double* g, double* work) {
  EVR_CHECK(power >= 0 && power <= DOT_MAX_POWER,
            "evr_dot_kernel_theta_grad: unsupported power=%d (0 = linear, 1 <= p <= %d = polynomial)", power,
            DOT_MAX_POWER);
  EVR_CHECK(B >= 1 && B <= 65535 && n >= 1, "evr_dot_kernel_theta_grad: bad sizes B=%d n=%d", B, n);
  EVR_CHECK(G && theta && W && g, "evr_dot_kernel_theta_grad: null argument");
  EVR_CHECK(work != nullptr, "evr_dot_kernel_theta_grad: work (B*n doubles) required");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(n, 4), B);
  if (n % 2 == 0 && aligned16(G) && aligned16(W))
    dot_grad_rows_kernel<true><<<grid, 256, 0, s>>>(power, n, G, theta, W, work);
  else
    dot_grad_rows_kernel<false><<<grid, 256, 0, s>>>(power, n, G, theta, W, work);
  EVR_LAUNCH_CHECK();
  dot_grad_sum_kernel<<<B, 256, 0, s>>>(n, work, g);
  EVR_LAUNCH_CHECK();
  return 0;
}

long long evr_dot_gp_posterior_workspace_doubles(int B, int n, int nt, int d) {
  // the normalised test rows (nt x d), the cross Gram (n x nt), K* (B x n x nt) and R (B x (n + 1) x nt)
  if (B < 1 || n < 1 || nt < 1 || d < 1) return 0;
  return even_up((long long)nt * d) + even_up((long long)n * nt) + even_up((long long)B * n * nt) +
         even_up((long long)B * (n + 1) * nt);
}

int evr_dot_gp_posterior(void* stream, int power, int B, int n, int nt, int d, const double* Xn, const double* X,
                         const double* shift, const double* scale, const double* theta, const double* M,
                         const double* c, const double* ym, const double* ys, const double* noise_add, double* mean,
                         double* var, double* work) {
  EVR_CHECK(power >= 0 && power <= DOT_MAX_POWER,
            "evr_dot_gp_posterior: unsupported power=%d (0 = linear, 1 <= p <= %d = polynomial)", power,
            DOT_MAX_POWER);
  EVR_CHECK(B >= 1 && B <= 65535 && n >= 1 && d >= 1 && nt >= 0, "evr_dot_gp_posterior: bad sizes B=%d n=%d nt=%d d=%d",
            B, n, nt, d);
  if (nt == 0) return 0;
  EVR_CHECK((long long)n * nt < (1ll << 31), "evr_dot_gp_posterior: n * nt = %lld too large", (long long)n * nt);
  EVR_CHECK(Xn && X && theta && M && c && ym && ys && mean && var && work, "evr_dot_gp_posterior: null argument");
  hipStream_t s = (hipStream_t)stream;
  double* Xt = work;                                        // nt x d
  double* Gx = Xt + even_up((long long)nt * d);             // n x nt
  double* Kx = Gx + even_up((long long)n * nt);             // B x n x nt
  double* R = Kx + even_up((long long)B * n * nt);          // B x (n + 1) x nt
  const long long total = (long long)nt * d;
  dot_normalize_kernel<<<cdiv(total, 256), 256, 0, s>>>(total, d, X, shift, scale, Xt);
  EVR_LAUNCH_CHECK();
  if (int rc = evr_gemm_f64(stream, 0, 1, n, nt, d, 1.0, Xn, d, 0, Xt, d, 0, 0.0, Gx, nt, 0, 1)) return rc;
  if (int rc = dot_apply_launch(s, power, B, n, nt, Gx, theta, nullptr, Kx)) return rc;
  if (int rc = evr_gemm_f64(stream, 0, 0, n + 1, nt, n, 1.0, M, n, (long long)(n + 1) * n, Kx, nt, (long long)n * nt,
                            0.0, R, nt, (long long)(n + 1) * nt, B))
    return rc;
  dot_finalize_kernel<<<dim3(cdiv(nt, 64), B), 256, 0, s>>>(power, n, nt, d, R, Xt, theta, c, ym, ys, noise_add, mean,
                                                           var);
  EVR_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
