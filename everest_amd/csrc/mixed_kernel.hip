// Mixed continuous / categorical GP kernel ([upstream] BoTorch MixedSingleTaskGP) on gfx950:
//
//   K(x, x') = s_sum (k_c(r1) + s_cat h1) + s_prod k_c(r2) h2
//   r_t^2 = sum_k ((xc_k - xc'_k) / ls_t,k)^2,   h_t = exp(-(1 / nc) sum_f [c_f != c'_f] / lam_t,f)
//
// with k_c one of the four stationary families of common.hpp.  Member b reads the P = 2 dc + 2 nc + 3
// parameters params + b P = [ls1 (dc) | ls2 (dc) | lam1 (nc) | lam2 (nc) | s_sum | s_cat | s_prod].
// Inputs are shared by the members: Xc (n x dc, normalised) and the category codes C (n x nc, int32).
//
// evr_mixed_kernel_matrix: kmat_kernel's VALU form — a 64 x 64 tile per 256-thread workgroup, both
// point tiles staged in LDS, a 4 x 4 micro-tile per thread (rows ty + 16 a, columns tx + 16 c: a
// store instruction writes 16 consecutive doubles of a row), explicit differences.
// evr_mixed_kernel_param_grad: kls_grad_kernel's pattern — per-row partial sums of all P parameters
// in one pass over W, then a fixed-order column sum.
#include "common.hpp"
#include "../../include/everest_amd.h"

namespace evr {

constexpr int MK_T = 64;       // tile edge of the matrix kernel
constexpr int MK_MAXD = 32;    // continuous columns
constexpr int MK_MAXC = 8;     // categorical features

// Every entry is a function of (x_i, x_j) that does not depend on their order: the difference
// a - b and its negation have the same square, the sums run over k and f in index order, and the
// final expression is spelled out with contraction off (explicit fma only), so the 16 unrolled
// copies of the epilogue round alike.  K(X, X) is therefore bitwise symmetric, and bitwise the
// cross call's result with X2 = X (the same kernel).
template <int KIND>
__global__ __launch_bounds__(256) void mixed_kmat_kernel(int n1, int n2, int dc, int nc,
                                                         const double* __restrict__ X1, const int* __restrict__ C1,
                                                         const double* __restrict__ X2, const int* __restrict__ C2,
                                                         const double* __restrict__ params,
                                                         const double* __restrict__ dg, double* __restrict__ K) {
#pragma clang fp contract(off)
  __shared__ double A[MK_T * (MK_MAXD + 1)], Bt[MK_T * (MK_MAXD + 1)];
  __shared__ int CA[MK_MAXC * MK_T], CB[MK_MAXC * MK_T];   // [f][row]
  __shared__ double il1[MK_MAXD], il2[MK_MAXD], w1[MK_MAXC], w2[MK_MAXC];
  __shared__ double kexp[64];
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * MK_T, j0 = blockIdx.x * MK_T;
  const int tid = threadIdx.x;
  const int P = 2 * dc + 2 * nc + 3;
  const double* pb = params + (size_t)b * P;
  const int ld = dc | 1;   // odd row stride: the column-tile reads (stride ld) spread over the banks
  for (int e = tid; e < MK_T * dc; e += 256) {
    const int r = e / dc, k = e - r * dc;
    A[r * ld + k] = i0 + r < n1 ? X1[(size_t)(i0 + r) * dc + k] : 0.0;
    Bt[r * ld + k] = j0 + r < n2 ? X2[(size_t)(j0 + r) * dc + k] : 0.0;
  }
  for (int e = tid; e < MK_T * nc; e += 256) {
    const int r = e / nc, f = e - r * nc;
    CA[f * MK_T + r] = i0 + r < n1 ? C1[(size_t)(i0 + r) * nc + f] : 0;
    CB[f * MK_T + r] = j0 + r < n2 ? C2[(size_t)(j0 + r) * nc + f] : 0;
  }
  if (tid < dc) {
    il1[tid] = 1.0 / pb[tid];
    il2[tid] = 1.0 / pb[dc + tid];
  }
  if (tid >= 64 && tid < 64 + nc) {
    const int f = tid - 64;
    w1[f] = 1.0 / ((double)nc * pb[2 * dc + f]);
    w2[f] = 1.0 / ((double)nc * pb[2 * dc + nc + f]);
  }
  kexp_stage(kexp, tid, 256);
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  double d1[4][4], d2[4][4], g1[4][4], g2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) d1[a][c] = d2[a][c] = g1[a][c] = g2[a][c] = 0.0;
  for (int k = 0; k < dc; ++k) {
    double av[4], bv[4];
    const double s1 = il1[k], s2 = il2[k];
#pragma unroll
    for (int a = 0; a < 4; ++a) av[a] = A[(ty + 16 * a) * ld + k];
#pragma unroll
    for (int c = 0; c < 4; ++c) bv[c] = Bt[(tx + 16 * c) * ld + k];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double df = av[a] - bv[c];
        const double t1 = df * s1, t2 = df * s2;
        d1[a][c] = fma(t1, t1, d1[a][c]);
        d2[a][c] = fma(t2, t2, d2[a][c]);
      }
  }
  for (int f = 0; f < nc; ++f) {
    int ca[4], cb[4];
    const double u1 = w1[f], u2 = w2[f];
#pragma unroll
    for (int a = 0; a < 4; ++a) ca[a] = CA[f * MK_T + ty + 16 * a];
#pragma unroll
    for (int c = 0; c < 4; ++c) cb[c] = CB[f * MK_T + tx + 16 * c];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool ne = ca[a] != cb[c];
        g1[a][c] += ne ? u1 : 0.0;
        g2[a][c] += ne ? u2 : 0.0;
      }
  }
  const double s_sum = pb[P - 3], s_cat = pb[P - 2], s_prod = pb[P - 1];
  const double dadd = dg ? dg[b] : 0.0;
  double* Kb = K + (size_t)b * n1 * n2;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ty + 16 * a;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tx + 16 * c;
      const double k1 = kernel_value_r(KIND, d1[a][c], kexp), k2 = kernel_value_r(KIND, d2[a][c], kexp);
      const double h1 = exp_k_t(-g1[a][c], kexp), h2 = exp_k_t(-g2[a][c], kexp);
      double v = fma(s_prod * k2, h2, s_sum * fma(s_cat, h1, k1));
      if (i == j) v += dadd;
      if (i < n1 && j < n2) Kb[(size_t)i * n2 + j] = v;
    }
  }
}

// part[b][i][p] = sum_j W[b][i][j] dK_b[i][j] / dparams_p.  ROWS rows per 256-thread workgroup,
// 4 / ROWS waves per row: a wave per row up to 16 continuous columns (ROWS = 4), the four waves
// of a workgroup on one row above (ROWS = 1) — the P = 2 dc + 2 nc + 3 accumulators per lane
// are the register budget.  Lane l of a row's waves sums j = l, l + 64 (4 / ROWS), ...; what
// is constant along a row (the parameter's own factor: s_sum / ls1_k, s_prod / ls2_k,
// s_sum s_cat / (nc lam1_f^2), s_prod / (nc lam2_f^2), s_sum) multiplies the row's sum once.
// A fixed xor butterfly per wave, then the row's waves in wave order: no atomics, the result
// is the same bits on every run.  The row's point, the reciprocal lengthscales and the
// category weights 1 / (nc lam) sit in LDS (broadcast reads), not in per-lane registers.
template <int MAXD>
__host__ __device__ constexpr int mixed_pmax() { return 2 * MAXD + 2 * MK_MAXC + 3; }

template <int MAXD, int ROWS>
__global__ __launch_bounds__(256) void mixed_grad_kernel(int kind, int n, int dc, int nc,
                                                         const double* __restrict__ X, const int* __restrict__ C,
                                                         const double* __restrict__ params,
                                                         const double* __restrict__ W, double* __restrict__ part) {
  constexpr int WPR = 4 / ROWS;            // waves per row
  constexpr int PMAX = mixed_pmax<MAXD>();
  __shared__ double xi_s[ROWS][MAXD], il1[MAXD], il2[MAXD], w1[MK_MAXC], w2[MK_MAXC];
  __shared__ int ci_s[ROWS][MK_MAXC];
  __shared__ double red[4][PMAX];
  const int b = blockIdx.y;
  const int ib = blockIdx.x * ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = 2 * dc + 2 * nc + 3;
  const double* pb = params + (size_t)b * P;
  for (int t = tid; t < ROWS * MAXD; t += 256) {
    const int r = t / MAXD, k = t - r * MAXD;
    xi_s[r][k] = (k < dc && ib + r < n) ? X[(size_t)(ib + r) * dc + k] : 0.0;
  }
  for (int t = tid; t < ROWS * MK_MAXC; t += 256) {
    const int r = t / MK_MAXC, f = t - r * MK_MAXC;
    ci_s[r][f] = (f < nc && ib + r < n) ? C[(size_t)(ib + r) * nc + f] : 0;
  }
  if (tid < MAXD) {
    il1[tid] = tid < dc ? 1.0 / pb[tid] : 0.0;
    il2[tid] = tid < dc ? 1.0 / pb[dc + tid] : 0.0;
  }
  if (tid >= 64 && tid < 64 + MK_MAXC) {
    const int f = tid - 64;
    w1[f] = f < nc ? 1.0 / ((double)nc * pb[2 * dc + f]) : 0.0;
    w2[f] = f < nc ? 1.0 / ((double)nc * pb[2 * dc + nc + f]) : 0.0;
  }
  __syncthreads();
  const double s_sum = pb[P - 3], s_cat = pb[P - 2], s_prod = pb[P - 1];
  const int row = wave / WPR, sub = wave % WPR;
  const int i = ib + row;
  double a1[MAXD], a2[MAXD], l1[MK_MAXC], l2[MK_MAXC], sc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < MAXD; ++k) a1[k] = a2[k] = 0.0;
#pragma unroll
  for (int f = 0; f < MK_MAXC; ++f) l1[f] = l2[f] = 0.0;
  if (i < n) {   // whole waves
    const double* Wr = W + ((size_t)b * n + i) * n;
    const double* xi = xi_s[row];
    const int* ci = ci_s[row];
    for (int j = sub * 64 + lane; j < n; j += 64 * WPR) {
      const double w = Wr[j];
      const double* xj = X + (size_t)j * dc;
      const int* cj = C + (size_t)j * nc;
      double q1 = 0.0, q2 = 0.0;
      // up to 16 columns the differences stay in registers; above, the second pass forms them again
      double df[MAXD <= 16 ? MAXD : 1];
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < dc) {
          const double e = xi[k] - xj[k];
          if constexpr (MAXD <= 16) df[k] = e;
          const double t1 = e * il1[k], t2 = e * il2[k];
          q1 = fma(t1, t1, q1);
          q2 = fma(t2, t2, q2);
        }
      unsigned ne = 0;
      double e1 = 0.0, e2 = 0.0;
#pragma unroll
      for (int f = 0; f < MK_MAXC; ++f)
        if (f < nc && ci[f] != cj[f]) {
          ne |= 1u << f;
          e1 += w1[f];
          e2 += w2[f];
        }
      const double h1 = exp_k(-e1), h2 = exp_k(-e2);
      const double k1 = kernel_value(kind, q1), k2 = kernel_value(kind, q2);
      const double wh1 = w * h1, wkh2 = w * k2 * h2;
      const double u1 = -w * kernel_dscale(kind, q1), u2 = -w * h2 * kernel_dscale(kind, q2);
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < dc) {
          double e;
          if constexpr (MAXD <= 16) e = df[k];
          else e = xi[k] - xj[k];
          const double t1 = e * il1[k], t2 = e * il2[k];
          a1[k] = fma(u1, t1 * t1, a1[k]);
          a2[k] = fma(u2, t2 * t2, a2[k]);
        }
#pragma unroll
      for (int f = 0; f < MK_MAXC; ++f)
        if (ne >> f & 1) {
          l1[f] += wh1;
          l2[f] += wkh2;
        }
      sc[0] += w * fma(s_cat, h1, k1);
      sc[1] += wh1;
      sc[2] += wkh2;
    }
  }
  // the wave's sums of every parameter: a fixed xor butterfly, lane 0 posts them
#define MIXED_POST(val, p)                                        \
  do {                                                            \
    double v_ = (val);                                            \
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) v_ += __shfl_xor(v_, o, 64); \
    if (lane == 0) red[wave][p] = v_;                             \
  } while (0)
#pragma unroll
  for (int k = 0; k < MAXD; ++k)
    if (k < dc) {
      MIXED_POST(a1[k], k);
      MIXED_POST(a2[k], dc + k);
    }
#pragma unroll
  for (int f = 0; f < MK_MAXC; ++f)
    if (f < nc) {
      MIXED_POST(l1[f], 2 * dc + f);
      MIXED_POST(l2[f], 2 * dc + nc + f);
    }
  MIXED_POST(sc[0], P - 3);
  MIXED_POST(sc[1], P - 2);
  MIXED_POST(sc[2], P - 1);
#undef MIXED_POST
  __syncthreads();
  for (int t = tid; t < ROWS * P; t += 256) {
    const int r = t / P, p = t - r * P;
    if (ib + r >= n) continue;
    double v = red[r * WPR][p];
#pragma unroll
    for (int s = 1; s < WPR; ++s) v += red[r * WPR + s][p];
    double f;   // the parameter's own factor
    if (p < dc) f = s_sum * il1[p];
    else if (p < 2 * dc) f = s_prod * il2[p - dc];
    else if (p < 2 * dc + nc) f = s_sum * s_cat * ((double)nc * w1[p - 2 * dc] * w1[p - 2 * dc]);
    else if (p < 2 * dc + 2 * nc) f = s_prod * ((double)nc * w2[p - 2 * dc - nc] * w2[p - 2 * dc - nc]);
    else f = p == P - 2 ? s_sum : 1.0;
    part[((size_t)b * n + ib + r) * P + p] = v * f;
  }
}

// out[b][p] = sum_i part[b][i][p]: one block per (b, p), strided partials + fixed LDS tree
// (colsum_kernel's order)
__global__ __launch_bounds__(256) void mixed_colsum_kernel(int n, int P, const double* __restrict__ part,
                                                           double* __restrict__ out) {
  const int b = blockIdx.x / P, p = blockIdx.x % P;
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[((size_t)b * n + i) * P + p];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)b * P + p] = red[0];
}

static bool mixed_sizes_ok(int kind, int B, int dc, int nc) {
  return kind >= 0 && kind <= 3 && B >= 1 && B <= 65535 && dc >= 1 && dc <= MK_MAXD && nc >= 1 && nc <= MK_MAXC;
}

}  // namespace evr

using namespace evr;

extern "C" {

int evr_mixed_kernel_matrix(void* stream, int kind, int B, int n1, int n2, int dc, int nc, const double* X1c,
                            const int* C1, const double* X2c, const int* C2, const double* params,
                            const double* diag_add, double* K) {
  EVR_CHECK(mixed_sizes_ok(kind, B, dc, nc),
            "evr_mixed_kernel_matrix: unsupported kind=%d B=%d dc=%d nc=%d (one family 0..3, 1 <= dc <= %d, "
            "1 <= nc <= %d)", kind, B, dc, nc, MK_MAXD, MK_MAXC);
  EVR_CHECK(n1 >= 0 && n2 >= 0, "evr_mixed_kernel_matrix: bad sizes n1=%d n2=%d", n1, n2);
  if (n1 == 0 || n2 == 0) return 0;
  EVR_CHECK(X1c && C1 && X2c && C2 && params && K, "evr_mixed_kernel_matrix: null argument");
  EVR_CHECK(cdiv(n1, MK_T) <= 65535, "evr_mixed_kernel_matrix: n1=%d too large", n1);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(cdiv(n2, MK_T), cdiv(n1, MK_T), B);
#define LAUNCH(KD) \
  mixed_kmat_kernel<KD><<<grid, 256, 0, s>>>(n1, n2, dc, nc, X1c, C1, X2c, C2, params, diag_add, K)
  switch (kind) {
    case RBF: LAUNCH(RBF); break;
    case MATERN05: LAUNCH(MATERN05); break;
    case MATERN15: LAUNCH(MATERN15); break;
    default: LAUNCH(MATERN25); break;
  }
#undef LAUNCH
  EVR_LAUNCH_CHECK();
  return 0;
}

int evr_mixed_kernel_param_grad(void* stream, int kind, int B, int n, int dc, int nc, const double* Xc, const int* C,
                                const double* params, const double* W, double* g, double* work) {
  EVR_CHECK(mixed_sizes_ok(kind, B, dc, nc),
            "evr_mixed_kernel_param_grad: unsupported kind=%d B=%d dc=%d nc=%d (one family 0..3, 1 <= dc <= %d, "
            "1 <= nc <= %d)", kind, B, dc, nc, MK_MAXD, MK_MAXC);
  EVR_CHECK(n >= 1 && Xc && C && params && W && g, "evr_mixed_kernel_param_grad: bad arguments n=%d", n);
  EVR_CHECK(work != nullptr, "evr_mixed_kernel_param_grad: work (B*n*(2 dc + 2 nc + 3) doubles) required");
  hipStream_t s = (hipStream_t)stream;
  const int P = 2 * dc + 2 * nc + 3;
  if (dc <= 8) mixed_grad_kernel<8, 4><<<dim3(cdiv(n, 4), B), 256, 0, s>>>(kind, n, dc, nc, Xc, C, params, W, work);
  else if (dc <= 16)
    mixed_grad_kernel<16, 4><<<dim3(cdiv(n, 4), B), 256, 0, s>>>(kind, n, dc, nc, Xc, C, params, W, work);
  else mixed_grad_kernel<32, 1><<<dim3(n, B), 256, 0, s>>>(kind, n, dc, nc, Xc, C, params, W, work);
  EVR_LAUNCH_CHECK();
  mixed_colsum_kernel<<<B * P, 256, 0, s>>>(n, P, work, g);
  EVR_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
