// Augmented Chebyshev scalarisation scan with output constraints on gfx950: the step between the
// joint samples Y of q-point candidates (several model outputs) and dY for QparegoStrategy.
//
// Restates, for the utility
//       t_k(y) = A_k g_k(y[out_k]) + B_k,   u(y) = min_k t_k(y) + alpha sum_k t_k(y)
// ([upstream] botorch.utils.multi_objective.scalarization.get_chebyshev_scalarization, with the
// weights, the normalisation bounds and the signs folded into A_k > 0 and B_k on the host) and
// constraints c(y) = sign*(y[out] - thr), the reductions of sobo_scan.hip:
//       plain: acq = mean_s max_i [ (u(y_si) - best_s)_+ * exp(sum_c logsigmoid(-c(y_si) / eta_c)) ]
//       log:   acq = logmeanexp_s fatmax_i [ log fatplus(u(y_si) - best_s; tau_relu)
//                                            + sum_c log_fatmoid(-c(y_si) / eta_c) ; tau_max ]
// as called from bofire/strategies/predictives/qparego.py:30-140.  The utility is not a sum over
// terms: the slope of u with respect to t_k is alpha + [k == k*], k* the FIRST arg-min (lowest
// term index on ties, torch.min).
//
// MI355X layout: that of sobo_scan.hip / nei_scan.hip.  A 256-thread workgroup owns a tile of 16
// candidates; thread = (column lane cl = tid & 15, sample lane sl = tid >> 4); the 16 sample
// lanes of a column are combined in the fixed order of ns_reduce.hpp (shuffle-down by 32 and 16,
// then waves 0..3 through LDS).  The per-thread state is O(Q): running minimum, running sum and
// arg-min index per point.  The term / constraint table travels by value in the launch
// arguments; its loops are wave-uniform and the OUTER ones with the q points unrolled inside, so
// the table is read through scalar loads and never copied to scratch (see sobo_scan.hip).  No
// atomics; run-to-run bitwise reproducible.  One launch per evaluation, forward and backward.
#include "sb_common.hpp"

namespace evr {

// terms (QgObj's objective slots, affine / close-to-target only, plus scale A and shift B),
// constraints and the augmentation weight, by value
struct PgTab {
  QgObj o;
  double A[QG_MAXM], B[QG_MAXM];
  double alpha;
};

// the Q points of one (sample, candidate): utilities, first arg-min term (ks, nullable) and
// summed log feasibilities
template <int Q, bool LOG>
__device__ __forceinline__ void pg_points(const PgTab& t, const double* __restrict__ Ys, size_t st, double* u,
                                          int* ks, double* lw) {
  double sm[Q];
  {
    const double* Y0 = Ys + (size_t)t.o.oo[0] * st;
    const double A0 = t.A[0], B0 = t.B[0];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      u[i] = sm[i] = A0 * qg_obj(t.o, 0, Y0[i]) + B0;
      if (ks) ks[i] = 0;
      lw[i] = 0.0;
    }
  }
  for (int k = 1; k < t.o.mo; ++k) {
    const double* Yk = Ys + (size_t)t.o.oo[k] * st;
    const double Ak = t.A[k], Bk = t.B[k];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double tk = Ak * qg_obj(t.o, k, Yk[i]) + Bk;
      sm[i] += tk;
      if (tk < u[i]) {   // strict: the first arg-min stays on ties
        u[i] = tk;
        if (ks) ks[i] = k;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < Q; ++i) u[i] += t.alpha * sm[i];
  sb_feas<Q, LOG>(t.o, Ys, st, lw);
}

template <int Q, bool LOG>
__device__ __forceinline__ double pg_sample(const PgTab& t, const double* __restrict__ Ys, size_t st, double best,
                                            double tr, double tm, int* ks, double* du, double* dl) {
  double u[Q], lw[Q];
  pg_points<Q, LOG>(t, Ys, st, u, ks, lw);
  return sb_reduce<Q, LOG>(u, lw, t.o.nc != 0, best, tr, tm, du, dl);
}

template <int Q, bool LOG, bool BWD>
__global__ __launch_bounds__(NS_THREADS) void parego_scan(int S, int b, PgTab t, const double* __restrict__ Y,
                                                          const double* __restrict__ best, int best_stride,
                                                          double tr, double tm, const int* __restrict__ flags,
                                                          const double* __restrict__ gout, double* __restrict__ acq,
                                                          double* __restrict__ dY) {
  __shared__ double red_m[NS_THREADS / 64][NS_CL];
  __shared__ double red_s[NS_THREADS / 64][NS_CL];
  const int tid = threadIdx.x, cl = tid & (NS_CL - 1), sl = tid >> 4;
  const int c = blockIdx.x * NS_CL + cl;
  const bool live = c < b;
  const int mm = t.o.m;
  const size_t bq = (size_t)b * Q, sbq = (size_t)mm * bq;
  const double* Yc = Y + (size_t)c * Q;   // dereferenced only when live
  double m = -INFINITY, sum = 0.0;
  if (live) {
    for (int s = sl; s < S; s += NS_SL) {
      const double v = pg_sample<Q, LOG>(t, Yc + (size_t)s * sbq, bq, best[(size_t)s * best_stride], tr, tm, nullptr,
                                         nullptr, nullptr);
      if (LOG) {
        if (v > -INFINITY) ns_merge(m, sum, v, 1.0);
      } else {
        sum += v;
      }
    }
  }
  // sample lanes of one column: lanes cl + 16 k of the wave (k = 0..3), then the four waves
#pragma unroll
  for (int o = 32; o >= NS_CL; o >>= 1) {
    const double s2 = __shfl_down(sum, o, 64);
    if (LOG) {
      const double m2 = __shfl_down(m, o, 64);
      ns_merge(m, sum, m2, s2);
    } else {
      sum += s2;
    }
  }
  if ((tid & 63) < NS_CL) {
    red_m[tid >> 6][cl] = m;
    red_s[tid >> 6][cl] = sum;
  }
  __syncthreads();
  m = red_m[0][cl];
  sum = red_s[0][cl];
#pragma unroll
  for (int w = 1; w < NS_THREADS / 64; ++w) {
    if (LOG) ns_merge(m, sum, red_m[w][cl], red_s[w][cl]);
    else sum += red_s[w][cl];
  }
  if (!live) return;
  const double lse = LOG ? (sum > 0.0 ? m + log(sum) : -INFINITY) : 0.0;
  if (sl == 0) {
    const double val = LOG ? lse - log((double)S) : sum / (double)S;
    bool bad = false;
    if (flags)
      for (int j = 0; j < mm; ++j) bad |= flags[(size_t)j * b + c] != 0;
    acq[c] = bad ? nan("") : val;
  }
  if (!BWD) return;
  const double go = gout ? gout[c] : 1.0;
  double* dYc = dY + (size_t)c * Q;
  for (int s = sl; s < S; s += NS_SL) {
    const double* Ys = Yc + (size_t)s * sbq;
    double* dYs = dYc + (size_t)s * sbq;
    double du[Q], dl[Q];
    int ks[Q];
    const double v = pg_sample<Q, LOG>(t, Ys, bq, best[(size_t)s * best_stride], tr, tm, ks, du, dl);
    // d acq / d v_s: softmax weight over the samples (log), 1 / S (plain)
    double w;
    if (LOG) w = (v > -INFINITY && lse > -INFINITY) ? go * exp(v - lse) : 0.0;
    else w = go / (double)S;
    // every output row is written: the slopes of the terms / constraints reading output j
    for (int j = 0; j < mm; ++j) {
      const double* Yj = Ys + (size_t)j * bq;
      double acc[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) acc[i] = 0.0;
      for (int k = 0; k < t.o.mo; ++k) {
        if (t.o.oo[k] != j) continue;
        const double Ak = t.A[k], al = t.alpha;
#pragma unroll
        for (int i = 0; i < Q; ++i)   // d u / d t_k = alpha + [k == k*]
          acc[i] += du[i] * ((ks[i] == k ? al + 1.0 : al) * (Ak * qg_dobj(t.o, k, Yj[i])));
      }
      sb_dfeas<Q, LOG>(t.o, j, Yj, dl, acc);
#pragma unroll
      for (int i = 0; i < Q; ++i) dYs[(size_t)j * bq + i] = w == 0.0 ? 0.0 : w * acc[i];
    }
  }
}

static int pg_params(const evr_parego* pg, int m_model, PgTab* t) {
  std::memset(t, 0, sizeof(*t));
  if (int rc = sb_fill("parego_scan", pg, pg && pg->term_a && pg->term_b, m_model, 2, false, &t->o)) return rc;
  EVR_CHECK(pg->alpha >= 0.0, "parego_scan: alpha = %g is negative", pg->alpha);
  t->alpha = pg->alpha;
  for (int k = 0; k < pg->n_term; ++k) {
    EVR_CHECK(pg->term_a[k] > 0.0, "parego_scan: term %d has scale A = %g (must be positive)", k, pg->term_a[k]);
    t->A[k] = pg->term_a[k];
    t->B[k] = pg->term_b[k];
  }
  return 0;
}

int parego_scan_launch(hipStream_t s, int q, int m_model, int S, int b, const evr_parego* pg, const double* Y,
                       const int* flags, const double* gout, double* acq, double* dY) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "parego_scan: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  PgTab t;
  if (int rc = pg_params(pg, m_model, &t)) return rc;
  EVR_CHECK(S >= 1 && b >= 0 && Y && pg->best && acq && (pg->best_stride == 0 || pg->best_stride == 1),
            "parego_scan: bad arguments (S >= 1, best_stride 0 or 1)");
  const bool log_mode = pg->log != 0;
  const double tr = pg->tau_relu, tm = pg->tau_max;
  EVR_CHECK(!log_mode || (tr > 0.0 && tm > 0.0), "parego_scan: tau_relu / tau_max must be positive");
  if (b == 0) return 0;
  const int grid = cdiv(b, NS_CL);
  const double* best = pg->best;
  const int bs = pg->best_stride;
#define GO(QQ)                                                                                                        \
  if (log_mode) {                                                                                                     \
    if (dY) parego_scan<QQ, true, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,   \
                                                                    dY);                                              \
    else parego_scan<QQ, true, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,     \
                                                                  dY);                                                \
  } else {                                                                                                            \
    if (dY) parego_scan<QQ, false, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,  \
                                                                     dY);                                             \
    else parego_scan<QQ, false, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,    \
                                                                   dY);                                               \
  }                                                                                                                   \
  EVR_LAUNCH_CHECK()
  SB_SWITCH(q, GO, "parego_scan");
#undef GO
  return 0;
}

}  // namespace evr

extern "C" int evr_parego_scan(void* stream, int q, int m_model, int S, int b, const evr_parego* pg, const double* Y,
                               const int* flags, const double* gout, double* acq, double* dY) {
  return evr::parego_scan_launch((hipStream_t)stream, q, m_model, S, b, pg, Y, flags, gout, acq, dY);
}
