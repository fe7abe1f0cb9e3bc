// Multiplicative / multiplicative-additive utility scan on gfx950: the step between the joint
// samples Y of q-point candidates (several model outputs) and dY for MultiplicativeSoboStrategy
// and MultiplicativeAdditiveSoboStrategy.
//
// Restates, for the utility
//       u(y) = [ prod_{k factor} g_k(y[out_k]) ** w_k ] * [ 1 + sum_{a addend} w_a g_a(y[out_a]) ]
// (bofire/utils/torch_tools.py:662-675 get_multiplicative_botorch_objective, no addends, and
// :730-806 get_multiplicative_additive_objective; ** is C pow: a negative base is real with an
// integer-valued exponent and NaN with any other), the reductions of sobo_scan.hip without
// output constraints:
//       plain: acq = mean_s max_i (u(y_si) - best_s)_+
//       log:   acq = logmeanexp_s fatmax_i log fatplus(u(y_si) - best_s; tau_relu)
// as called from bofire/strategies/predictives/sobo.py:225-284.  The utility is not a sum over
// terms.  With P the product and A the additive bracket its slopes are
//       d u / d g_k = w_k pow(g_k, w_k - 1) * prod_{s != k} g_s ** w_s * A,    d u / d g_a = w_a P.
// The product of the OTHER factors is multiplied up from the others, never divided out of P, so
// an exactly zero factor has the slope of the rest and gives the rest slope 0, as autograd does.
// A weight of exactly 1 skips pow in both places (pow(x, 1) = x, and the slope 1 * pow(x, 0) = 1).
//
// NaN: a comparison drops a NaN utility from the plain maximum, where the reference's mean keeps
// it.  Each thread therefore carries a flag "some utility of this candidate was NaN" through the
// same fixed-order reduction as the sums; a flagged candidate's acq is NaN (its dY columns are
// unspecified), every other candidate is untouched.
//
// MI355X layout: that of parego_scan.hip / sobo_scan.hip.  A 256-thread workgroup owns a tile of
// 16 candidates; thread = (column lane cl = tid & 15, sample lane sl = tid >> 4); the 16 sample
// lanes of a column are combined in the fixed order of ns_reduce.hpp (shuffle-down by 32 and 16,
// then waves 0..3 through LDS).  The per-thread state is O(Q): product, bracket, slope
// accumulator and the product of the others per point; the backward recomputes the factors in
// table loops instead of keeping a terms x Q array.  The table travels by value in the launch
// arguments; its loops are wave-uniform and the OUTER ones with the q points unrolled inside, so
// the table is read through scalar loads and never copied to scratch.  No atomics; run-to-run
// bitwise reproducible.  One launch per evaluation, forward and backward; the forward-only launch
// runs the same forward code and gives the same bits.
#include "sb_common.hpp"

#include <cmath>

namespace evr {

// terms 0 .. nf-1 are the factors, nf .. s.o.mo-1 the addends (SbTab's slots, no constraints)
struct MtTab {
  SbTab s;
  int nf;
};

// g ** w of one factor; one: w == 1 exactly (wave-uniform)
__device__ __forceinline__ double mt_pow(double g, double w, bool one) { return one ? g : pow(g, w); }

// product P and additive bracket A of the Q points of one (sample, candidate), in the
// reference's order: 1 * g_0 ** w_0 * g_1 ** w_1 ..., 1 + g_a w_a + ...
template <int Q>
__device__ __forceinline__ void mt_points(const MtTab& t, const double* __restrict__ Ys, size_t st, double* P,
                                          double* A) {
#pragma unroll
  for (int i = 0; i < Q; ++i) P[i] = A[i] = 1.0;
  for (int k = 0; k < t.nf; ++k) {
    const double* Yk = Ys + (size_t)t.s.o.oo[k] * st;
    const double wk = t.s.w[k];
    const bool one = wk == 1.0;
#pragma unroll
    for (int i = 0; i < Q; ++i) P[i] *= mt_pow(sb_term(t.s, k, Yk[i]), wk, one);
  }
  for (int k = t.nf; k < t.s.o.mo; ++k) {
    const double* Yk = Ys + (size_t)t.s.o.oo[k] * st;
    const double wk = t.s.w[k];
#pragma unroll
    for (int i = 0; i < Q; ++i) A[i] += sb_term(t.s, k, Yk[i]) * wk;
  }
}

// value of one (sample, candidate) entering the sample reduction; P, A kept for the backward;
// bad: set when a utility is NaN
template <int Q, bool LOG>
__device__ __forceinline__ double mt_sample(const MtTab& t, const double* __restrict__ Ys, size_t st, double best,
                                            double tr, double tm, double* P, double* A, double* du, bool& bad) {
  double u[Q], lw[Q], dl[Q];
  mt_points<Q>(t, Ys, st, P, A);
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    u[i] = P[i] * A[i];
    bad |= u[i] != u[i];
    lw[i] = 0.0;
  }
  return sb_reduce<Q, LOG>(u, lw, false, best, tr, tm, du, dl);
}

template <int Q, bool LOG, bool BWD>
__global__ __launch_bounds__(NS_THREADS) void mult_scan(int S, int b, MtTab t, const double* __restrict__ Y,
                                                        const double* __restrict__ best, int best_stride, double tr,
                                                        double tm, const int* __restrict__ flags,
                                                        const double* __restrict__ gout, double* __restrict__ acq,
                                                        double* __restrict__ dY) {
  __shared__ double red_m[NS_THREADS / 64][NS_CL];
  __shared__ double red_s[NS_THREADS / 64][NS_CL];
  __shared__ int red_b[NS_THREADS / 64][NS_CL];
  const int tid = threadIdx.x, cl = tid & (NS_CL - 1), sl = tid >> 4;
  const int c = blockIdx.x * NS_CL + cl;
  const bool live = c < b;
  const int mm = t.s.o.m;
  const size_t bq = (size_t)b * Q, sbq = (size_t)mm * bq;
  const double* Yc = Y + (size_t)c * Q;   // dereferenced only when live
  double m = -INFINITY, sum = 0.0;
  bool bad = false;
  if (live) {
    for (int s = sl; s < S; s += NS_SL) {
      double P[Q], A[Q];
      const double v =
          mt_sample<Q, LOG>(t, Yc + (size_t)s * sbq, bq, best[(size_t)s * best_stride], tr, tm, P, A, nullptr, bad);
      if (LOG) {
        if (v > -INFINITY) ns_merge(m, sum, v, 1.0);
      } else {
        sum += v;
      }
    }
  }
  // sample lanes of one column: lanes cl + 16 k of the wave (k = 0..3), then the four waves;
  // the NaN flag takes the same route
  int nb = bad ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= NS_CL; o >>= 1) {
    const double s2 = __shfl_down(sum, o, 64);
    nb |= __shfl_down(nb, o, 64);
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
    red_b[tid >> 6][cl] = nb;
  }
  __syncthreads();
  m = red_m[0][cl];
  sum = red_s[0][cl];
  nb = red_b[0][cl];
#pragma unroll
  for (int w = 1; w < NS_THREADS / 64; ++w) {
    if (LOG) ns_merge(m, sum, red_m[w][cl], red_s[w][cl]);
    else sum += red_s[w][cl];
    nb |= red_b[w][cl];
  }
  if (!live) return;
  const double lse = LOG ? (sum > 0.0 ? m + log(sum) : -INFINITY) : 0.0;
  if (sl == 0) {
    const double val = LOG ? lse - log((double)S) : sum / (double)S;
    bool off = nb != 0;
    if (flags)
      for (int j = 0; j < mm; ++j) off |= flags[(size_t)j * b + c] != 0;
    acq[c] = off ? nan("") : val;
  }
  if (!BWD) return;
  const double go = gout ? gout[c] : 1.0;
  const int nf = t.nf, nt = t.s.o.mo;
  double* dYc = dY + (size_t)c * Q;
  for (int s = sl; s < S; s += NS_SL) {
    const double* Ys = Yc + (size_t)s * sbq;
    double* dYs = dYc + (size_t)s * sbq;
    double P[Q], A[Q], du[Q];
    bool unused = false;
    const double v = mt_sample<Q, LOG>(t, Ys, bq, best[(size_t)s * best_stride], tr, tm, P, A, du, unused);
    // d acq / d v_s: softmax weight over the samples (log), 1 / S (plain)
    double w;
    if (LOG) w = (v > -INFINITY && lse > -INFINITY) ? go * exp(v - lse) : 0.0;
    else w = go / (double)S;
    // every output row is written: the slopes of the terms reading output j
    for (int j = 0; j < mm; ++j) {
      const double* Yj = Ys + (size_t)j * bq;
      double acc[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) acc[i] = 0.0;
      for (int k = 0; k < nt; ++k) {
        if (t.s.o.oo[k] != j) continue;
        const double wk = t.s.w[k];
        if (k >= nf) {   // addend: d u / d g_a = w_a P
#pragma unroll
          for (int i = 0; i < Q; ++i) acc[i] += du[i] * ((wk * P[i]) * sb_dterm(t.s, k, Yj[i]));
          continue;
        }
        // factor: the product of the others, from the others
        double oth[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) oth[i] = 1.0;
        for (int r = 0; r < nf; ++r) {
          if (r == k) continue;
          const double* Yr = Ys + (size_t)t.s.o.oo[r] * bq;
          const double wr = t.s.w[r];
          const bool oner = wr == 1.0;
#pragma unroll
          for (int i = 0; i < Q; ++i) oth[i] *= mt_pow(sb_term(t.s, r, Yr[i]), wr, oner);
        }
        const bool one = wk == 1.0;
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const double sl_k = one ? 1.0 : wk * pow(sb_term(t.s, k, Yj[i]), wk - 1.0);
          acc[i] += du[i] * (((sl_k * oth[i]) * A[i]) * sb_dterm(t.s, k, Yj[i]));
        }
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) dYs[(size_t)j * bq + i] = w == 0.0 ? 0.0 : w * acc[i];
    }
  }
}

static int mt_params(const evr_mult* mt, int m_model, MtTab* t) {
  std::memset(t, 0, sizeof(*t));
  EVR_CHECK(mt && m_model >= 1 && m_model <= QG_MAXM && mt->n_fac >= 0 && mt->n_add >= 0 &&
                mt->n_fac + mt->n_add >= 1 && mt->n_fac + mt->n_add <= EVR_SOBO_MAX_TERMS,
            "mult_scan: bad table sizes (factors >= 0, addends >= 0, 1..%d terms in all, outputs 1..%d)",
            EVR_SOBO_MAX_TERMS, QG_MAXM);
  EVR_CHECK(mt->n_fac == 0 || (mt->fac_out && mt->fac_kind && mt->fac_w && mt->fac_p0 && mt->fac_p1 && mt->fac_p2),
            "mult_scan: null factor column");
  EVR_CHECK(mt->n_add == 0 || (mt->add_out && mt->add_kind && mt->add_w && mt->add_p0 && mt->add_p1 && mt->add_p2),
            "mult_scan: null addend column");
  t->nf = mt->n_fac;
  t->s.o.m = m_model;
  t->s.o.mo = mt->n_fac + mt->n_add;
  t->s.o.nc = 0;
  for (int k = 0; k < t->s.o.mo; ++k) {
    const bool fac = k < mt->n_fac;
    const int e = fac ? k : k - mt->n_fac;
    const char* what = fac ? "factor" : "addend";
    const int out = fac ? mt->fac_out[e] : mt->add_out[e], kind = fac ? mt->fac_kind[e] : mt->add_kind[e];
    const double w = fac ? mt->fac_w[e] : mt->add_w[e];
    EVR_CHECK(out >= 0 && out < m_model, "mult_scan: %s %d reads output %d of %d", what, e, out, m_model);
    EVR_CHECK(kind == EVR_OBJ_AFFINE || kind == EVR_OBJ_CLOSE_TO_TARGET || kind == EVR_OBJ_SIGMOID ||
                  kind == EVR_OBJ_TARGET,
              "mult_scan: %s %d has kind %d", what, e, kind);
    EVR_CHECK(std::isfinite(w) && (!fac || w >= 1.0), "mult_scan: %s %d has weight %g (finite%s)", what, e, w,
              fac ? ", >= 1 after normalisation" : "");
    t->s.o.oo[k] = out;
    t->s.o.ok[k] = kind;
    t->s.w[k] = w;
    t->s.o.p0[k] = fac ? mt->fac_p0[e] : mt->add_p0[e];
    t->s.o.p1[k] = fac ? mt->fac_p1[e] : mt->add_p1[e];
    t->s.p2[k] = fac ? mt->fac_p2[e] : mt->add_p2[e];
  }
  return 0;
}

int mult_scan_launch(hipStream_t s, int q, int m_model, int S, int b, const evr_mult* mt, const double* Y,
                     const int* flags, const double* gout, double* acq, double* dY) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "mult_scan: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  MtTab t;
  if (int rc = mt_params(mt, m_model, &t)) return rc;
  EVR_CHECK(S >= 1 && b >= 0 && Y && mt->best && acq && (mt->best_stride == 0 || mt->best_stride == 1),
            "mult_scan: bad arguments (S >= 1, best_stride 0 or 1)");
  const bool log_mode = mt->log != 0;
  const double tr = mt->tau_relu, tm = mt->tau_max;
  EVR_CHECK(!log_mode || (tr > 0.0 && tm > 0.0), "mult_scan: tau_relu / tau_max must be positive");
  if (b == 0) return 0;
  const int grid = cdiv(b, NS_CL);
  const double* best = mt->best;
  const int bs = mt->best_stride;
#define GO(QQ)                                                                                                      \
  if (log_mode) {                                                                                                   \
    if (dY) mult_scan<QQ, true, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,   \
                                                                  dY);                                              \
    else mult_scan<QQ, true, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,     \
                                                                dY);                                                \
  } else {                                                                                                          \
    if (dY) mult_scan<QQ, false, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,  \
                                                                   dY);                                             \
    else mult_scan<QQ, false, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,    \
                                                                 dY);                                               \
  }                                                                                                                 \
  EVR_LAUNCH_CHECK()
  SB_SWITCH(q, GO, "mult_scan");
#undef GO
  return 0;
}

}  // namespace evr

extern "C" int evr_mult_scan(void* stream, int q, int m_model, int S, int b, const evr_mult* mt, const double* Y,
                             const int* flags, const double* gout, double* acq, double* dY) {
  return evr::mult_scan_launch((hipStream_t)stream, q, m_model, S, b, mt, Y, flags, gout, acq, dY);
}
