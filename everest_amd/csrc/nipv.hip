// Negative integrated posterior variance on gfx950: the per-candidate step of
// ActiveLearningStrategy's acquisition ([upstream] qNegIntegratedPosteriorVariance, restated
// from memory; bofire/strategies/predictives/active_learning.py:16-66).
//
// Per output j (standardised units, k_j(x, x) = 1) and candidate X_c of q joint points, from
//       C_j  = k_j(P, X_c) - Vp_j^T Vx_j     N x q   posterior cross-covariance to the N points
//       Vx_j = Linv_j k_j(Xn, X_c)           n x q
// the kernel forms
//       G_j = C_j^T C_j,   A_j = k_j(X_c, X_c) - Vx_j^T Vx_j + noise_j I,
//       acq(X_c) = - sum_j coef_j ( v0_j - tr(A_j^-1 G_j) / N )
// and, for the backward, the slopes of acq with respect to C, Vx and (through the self block
// k_j(X_c, X_c)) the raw candidate points:
//       dC = s C A^-1,   dVx = s Vx (A^-1 G A^-1),   s = coef_j gout_c 2 / N,
//       dX_i (self) = - s sum_{k != i} (A^-1 G A^-1)_ik  dk/dx_i (x_i, x_k).
//
// MI355X layout: one 256-thread workgroup per candidate, the outputs in turn inside it.  The two
// tall reductions (over N rows of C, over n rows of Vx) keep the q (q + 1) / 2 products of a row
// in registers per thread (78 doubles at q = 12), then combine lanes by shuffle-down and the
// four waves through LDS in wave order.  The q x q state (G, A and its Cholesky factor L, L^-1,
// the whitened Gram H = L^-1 G L^-T, A^-1 G A^-1, the self block's slopes) lives in LDS; the
// factorisation runs on thread 0, the q x q products on q^2 threads.  A second walk over the rows
// writes the slopes.  No atomics; a candidate's result depends neither on b nor on its place in
// the batch; bitwise reproducible.
#include "sb_common.hpp"

namespace evr {

constexpr int NV_THREADS = 256;
constexpr int NV_WAVES = NV_THREADS / 64;

__host__ __device__ constexpr int nv_idx(int i, int k) { return i >= k ? i * (i + 1) / 2 + k : k * (k + 1) / 2 + i; }

struct NvArgs {
  int B, n, N, b, d, kind, ldv;
  const double *C, *Vx, *X, *lo, *ir, *ls, *noise, *coef, *v0, *gout;
  double* acq;
  int* flags;
  double *dC, *dVx, *dXs;
};

// dst[packed lower] = A^T A for the `rows` x Q block at A (rows `stride` doubles apart)
template <int Q>
__device__ __forceinline__ void nv_gram(const double* __restrict__ A, int rows, size_t stride,
                                        double (*red)[Q * (Q + 1) / 2], double* dst, int tid) {
  constexpr int T = Q * (Q + 1) / 2;
  double acc[T];
#pragma unroll
  for (int e = 0; e < T; ++e) acc[e] = 0.0;
  for (int p = tid; p < rows; p += NV_THREADS) {
    const double* r = A + (size_t)p * stride;
    double v[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) v[i] = r[i];
#pragma unroll
    for (int i = 0; i < Q; ++i)
#pragma unroll
      for (int k = 0; k <= i; ++k) acc[nv_idx(i, k)] = fma(v[i], v[k], acc[nv_idx(i, k)]);
  }
#pragma unroll
  for (int e = 0; e < T; ++e) {
    double v = acc[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6][e] = v;
  }
  __syncthreads();
  if (tid < T) {
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < NV_WAVES; ++w) v += red[w][tid];
    dst[tid] = v;
  }
  __syncthreads();
}

// out rows = s * (rows of A) * Mq  (Mq: Q x Q, row-major, LDS)
template <int Q>
__device__ __forceinline__ void nv_apply(const double* __restrict__ A, double* __restrict__ out, int rows,
                                         size_t stride, const double* Mq, double s, int tid) {
  for (int p = tid; p < rows; p += NV_THREADS) {
    const double* r = A + (size_t)p * stride;
    double* w = out + (size_t)p * stride;
    double v[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) v[i] = r[i];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      double o = 0.0;
#pragma unroll
      for (int k = 0; k < Q; ++k) o = fma(v[k], Mq[k * Q + i], o);
      w[i] = s * o;
    }
  }
}

// out rows = s * (rows of A) * Li^T Li = s * (rows of A) * A^-1  (Li: the factor's inverse, lower,
// packed, LDS): the row is whitened first, y = Li r, then out = Li^T y
template <int Q>
__device__ __forceinline__ void nv_apply_tri(const double* __restrict__ A, double* __restrict__ out, int rows,
                                             size_t stride, const double* Li, double s, int tid) {
  for (int p = tid; p < rows; p += NV_THREADS) {
    const double* r = A + (size_t)p * stride;
    double* w = out + (size_t)p * stride;
    double v[Q], y[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) v[i] = r[i];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      double o = 0.0;
#pragma unroll
      for (int m = 0; m <= i; ++m) o = fma(Li[nv_idx(i, m)], v[m], o);
      y[i] = o;
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      double o = 0.0;
#pragma unroll
      for (int m = i; m < Q; ++m) o = fma(Li[nv_idx(m, i)], y[m], o);
      w[i] = s * o;
    }
  }
}

template <int Q, bool BWD>
__global__ __launch_bounds__(NV_THREADS) void nipv_reduce_kernel(NvArgs a) {
  constexpr int T = Q * (Q + 1) / 2;
  __shared__ double red[NV_WAVES][T];
  __shared__ double Gs[T], Ws[T], Ls[T], Li[T];
  __shared__ double Hs[Q * Q], Tm[Q * Q], Ms[Q * Q], Kd[Q * Q];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  if (c >= a.b) return;   // whole workgroups (the grid is b)
  const int d = a.d;
  const size_t bq = (size_t)a.b * Q;
  const double* Xc = a.X + (size_t)c * Q * d;
  const double go = (BWD && a.gout) ? a.gout[c] : 1.0;
  double total = 0.0;   // thread 0
  int bad = 0;          // thread 0
  for (int j = 0; j < a.B; ++j) {
    const double* Cj = a.C + (size_t)j * a.N * bq + (size_t)c * Q;
    const double* Vj = a.Vx + (size_t)j * a.ldv * bq + (size_t)c * Q;
    nv_gram<Q>(Cj, a.N, bq, red, Gs, tid);
    nv_gram<Q>(Vj, a.n, bq, red, Ws, tid);
    // A = k_j(X_c, X_c) - Vx^T Vx + noise I (lower, packed, into Ls); Kd: the kernel's slope
    // factor per pair (kernel_cross_grad's convention at r = 0 is kernel_dscale's)
    if (tid < Q * Q) {
      const int i = tid / Q, k = tid - i * Q;
      if (k < i) {
        const int kj = kind_of(a.kind, j);
        const double* lsj = a.ls + (size_t)j * d;
        double d2 = 0.0;
        for (int t = 0; t < d; ++t) {
          const double df = (Xc[(size_t)i * d + t] - Xc[(size_t)k * d + t]) * a.ir[t] / lsj[t];
          d2 = fma(df, df, d2);
        }
        Ls[nv_idx(i, k)] = kernel_value(kj, d2) - Ws[nv_idx(i, k)];
        const double ds = kernel_dscale(kj, d2);
        Kd[i * Q + k] = ds;
        Kd[k * Q + i] = ds;
      } else if (k == i) {
        Ls[nv_idx(i, i)] = (1.0 - Ws[nv_idx(i, i)]) + a.noise[j];
        Kd[i * Q + i] = 0.0;
      }
    }
    __syncthreads();
    if (tid == 0) {
      // Cholesky in place, then the inverse of the factor
#pragma unroll 1
      for (int i = 0; i < Q; ++i) {
#pragma unroll 1
        for (int k = 0; k <= i; ++k) {
          double s = Ls[nv_idx(i, k)];
#pragma unroll 1
          for (int m = 0; m < k; ++m) s -= Ls[nv_idx(i, m)] * Ls[nv_idx(k, m)];
          if (k == i) {
            if (!(s > 0.0)) bad = 1;
            Ls[nv_idx(i, i)] = sqrt(s);
          } else {
            Ls[nv_idx(i, k)] = s / Ls[nv_idx(k, k)];
          }
        }
      }
#pragma unroll 1
      for (int k = 0; k < Q; ++k) {
        Li[nv_idx(k, k)] = 1.0 / Ls[nv_idx(k, k)];
#pragma unroll 1
        for (int i = k + 1; i < Q; ++i) {
          double s = 0.0;
#pragma unroll 1
          for (int m = k; m < i; ++m) s -= Ls[nv_idx(i, m)] * Li[nv_idx(m, k)];
          Li[nv_idx(i, k)] = s / Ls[nv_idx(i, i)];
        }
      }
    }
    __syncthreads();
    // whitened: H = Li G Li^T (symmetric, H_ii >= 0, so tr(A^-1 G) = tr(H) sums without
    // cancellation), A^-1 G A^-1 = Li^T H Li.  A^-1 itself is never formed: with nearly coincident
    // points its entries are ~1 / noise while C A^-1 stays moderate.
    const int qi = tid / Q, qk = tid - qi * Q;   // used below tid < Q * Q only
    if (tid < Q * Q) {   // Li G
      double s = 0.0;
      for (int m = 0; m <= qi; ++m) s = fma(Li[nv_idx(qi, m)], Gs[nv_idx(m, qk)], s);
      Tm[qi * Q + qk] = s;
    }
    __syncthreads();
    if (tid < Q * Q) {   // H = (Li G) Li^T
      double s = 0.0;
      for (int m = 0; m <= qk; ++m) s = fma(Tm[qi * Q + m], Li[nv_idx(qk, m)], s);
      Hs[qi * Q + qk] = s;
    }
    __syncthreads();
    if (tid < Q * Q) {   // Li^T H
      double s = 0.0;
      for (int m = qi; m < Q; ++m) s = fma(Li[nv_idx(m, qi)], Hs[m * Q + qk], s);
      Tm[qi * Q + qk] = s;
    }
    if (tid == 0) {
      double tr = 0.0;
      for (int i = 0; i < Q; ++i) tr += Hs[i * Q + i];
      total -= a.coef[j] * (a.v0[j] - tr / (double)a.N);
    }
    __syncthreads();
    if (tid < Q * Q) {   // A^-1 G A^-1 = (Li^T H) Li
      double s = 0.0;
      for (int m = qk; m < Q; ++m) s = fma(Tm[qi * Q + m], Li[nv_idx(m, qk)], s);
      Ms[qi * Q + qk] = s;
    }
    __syncthreads();
    if (BWD) {
      const double s = a.coef[j] * go * 2.0 / (double)a.N;
      nv_apply_tri<Q>(Cj, a.dC + (size_t)j * a.N * bq + (size_t)c * Q, a.N, bq, Li, s, tid);
      nv_apply<Q>(Vj, a.dVx + (size_t)j * a.n * bq + (size_t)c * Q, a.n, bq, Ms, s, tid);
      // the self block: outputs added in order j = 0, 1, ... by the element's own thread
      const double* lsj = a.ls + (size_t)j * d;
      double* dXc = a.dXs + (size_t)c * Q * d;
      for (int t = tid; t < Q * d; t += NV_THREADS) {
        const int i = t / d, dd = t - i * d;
        const double xi = Xc[(size_t)i * d + dd];
        double g = 0.0;
        for (int k = 0; k < Q; ++k)
          if (k != i) g = fma(Ms[i * Q + k] * Kd[i * Q + k], xi - Xc[(size_t)k * d + dd], g);
        const double il = a.ir[dd] / lsj[dd];
        g *= -s * il * il;
        dXc[t] = j == 0 ? g : dXc[t] + g;
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    a.acq[c] = total;
    a.flags[c] = bad;
  }
}

int nipv_reduce_launch(hipStream_t s, int q, const NvArgs& a) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "nipv_reduce: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  EVR_CHECK(a.B >= 1 && a.n >= 1 && a.N >= 1 && a.b >= 0 && a.d >= 1,
            "nipv_reduce: bad sizes (B = %d, n = %d, N = %d, b = %d, d = %d)", a.B, a.n, a.N, a.b, a.d);
  EVR_CHECK(kind_code_ok(a.kind, a.B), "nipv_reduce: kind code %d does not describe %d outputs", a.kind, a.B);
  EVR_CHECK(a.ldv >= a.n, "nipv_reduce: Vx leading dimension %d < n = %d", a.ldv, a.n);
  if (a.b == 0) return 0;
  EVR_CHECK(a.C && a.Vx && a.X && a.lo && a.ir && a.ls && a.noise && a.coef && a.v0 && a.acq && a.flags,
            "nipv_reduce: null argument");
  const bool bwd = a.dC != nullptr;
  EVR_CHECK(bwd == (a.dVx != nullptr) && bwd == (a.dXs != nullptr),
            "nipv_reduce: the backward needs dC, dVx and dXself together");
  EVR_CHECK(bwd || !a.gout, "nipv_reduce: gout without a backward");
#define GO(QQ)                                                                   \
  if (bwd) nipv_reduce_kernel<QQ, true><<<a.b, NV_THREADS, 0, s>>>(a);           \
  else nipv_reduce_kernel<QQ, false><<<a.b, NV_THREADS, 0, s>>>(a);              \
  EVR_LAUNCH_CHECK()
  SB_SWITCH(q, GO, "nipv_reduce");
#undef GO
  return 0;
}

}  // namespace evr

extern "C" int evr_nipv_reduce(void* stream, int q, int B, int n, int N, int b, int d, int kind, const double* C,
                               const double* Vx, int ldv, const double* X, const double* lo,
                               const double* inv_range, const double* ls, const double* noise, const double* coef,
                               const double* v0, const double* gout, double* acq, int* flags, double* dC,
                               double* dVx, double* dXself) {
  evr::NvArgs a;
  a.B = B; a.n = n; a.N = N; a.b = b; a.d = d; a.kind = kind; a.ldv = ldv;
  a.C = C; a.Vx = Vx; a.X = X; a.lo = lo; a.ir = inv_range; a.ls = ls; a.noise = noise; a.coef = coef; a.v0 = v0;
  a.gout = gout; a.acq = acq; a.flags = flags; a.dC = dC; a.dVx = dVx; a.dXs = dXself;
  return evr::nipv_reduce_launch((hipStream_t)stream, q, a);
}
