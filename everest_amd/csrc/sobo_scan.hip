// Scalarised single-objective scan with output constraints on gfx950: the step between the
// joint samples Y of q-point candidates (several model outputs) and dY for SoboStrategy with
// constrained objectives and for AdditiveSoboStrategy.
//
// Restates, for the utility u(y) = sum_t w_t g_t(y[out_t]) and constraints c(y) = sign*(y[out] - thr),
//   [upstream] SampleReducingMCAcquisitionFunction._apply_constraints as used by
//   qNoisyExpectedImprovement / qExpectedImprovement:
//       acq = mean_s max_i [ (u(y_si) - best_s)_+ * exp(sum_c logsigmoid(-c(y_si) / eta_c)) ]
//   and by qLogNoisyExpectedImprovement / qLogExpectedImprovement (fat = True):
//       acq = logmeanexp_s fatmax_i [ log fatplus(u(y_si) - best_s; tau_relu)
//                                     + sum_c log_fatmoid(-c(y_si) / eta_c) ; tau_max ]
// as called from bofire/strategies/predictives/sobo.py:42-222 with the objective callables of
// bofire/utils/torch_tools.py:384-450 and the constraints of get_output_constraints (:258-381).
// The feasibility weighs every (sample, point) BEFORE the reduction over the q points — unlike
// the hypervolume chain, which weighs q-subsets (qnehvi_general.hip).
//
// MI355X layout: that of nei_scan.hip.  A 256-thread workgroup owns a tile of 16 candidates;
// thread = (column lane cl = tid & 15, sample lane sl = tid >> 4); the 16 sample lanes of a
// column are combined in the same fixed order (shuffle-down by 32 and 16, then waves 0..3 through
// LDS).  The q points of a (sample, candidate) are evaluated from direct loads of the outputs
// their terms / constraints read (Y[s][j][c*q + i]: 16 q consecutive doubles per output row and
// wave quarter), so the per-thread state is O(Q) and never O(Q m); the backward walks Y a second
// time and re-reads y when it distributes the slopes to the outputs.  The term / constraint
// tables travel by value in the launch arguments; their loops are wave-uniform and the OUTER
// ones (one set of scalar table reads per term, the q points unrolled inside): with the point
// loop outside, the by-value table was copied to scratch at Q = 12.  No atomics; run-to-run
// bitwise reproducible.  One launch per evaluation, forward and backward.
//
// With m = 1, one affine term of weight 1 and no constraints every operation added here is exact
// (0.0 + 1.0 g, a + 0.0, x * 1.0), so the results equal nei_scan's bit for bit.
#include "sb_common.hpp"

namespace evr {

// the Q points of one (sample, candidate) (Ys: the output-0 sample of point 0, outputs `st`
// doubles apart): utilities and summed log feasibilities (log-sigmoid in plain mode, log-fatmoid
// in log mode).  The table loops are the outer ones: one set of scalar table reads per term /
// constraint, whatever Q.
template <int Q, bool LOG>
__device__ __forceinline__ void sb_points(const SbTab& t, const double* __restrict__ Ys, size_t st, double* u,
                                          double* lw) {
#pragma unroll
  for (int i = 0; i < Q; ++i) u[i] = lw[i] = 0.0;
  for (int k = 0; k < t.o.mo; ++k) {
    const double* Yk = Ys + (size_t)t.o.oo[k] * st;
    const double wk = t.w[k];
#pragma unroll
    for (int i = 0; i < Q; ++i) u[i] += wk * sb_term(t, k, Yk[i]);
  }
  for (int e = 0; e < t.o.nc; ++e) {
    const double* Ye = Ys + (size_t)t.o.co[e] * st;
    const double cs = t.o.cs[e], ct = t.o.ct[e], ce = t.o.ce[e];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double cval = cs * (Ye[i] - ct);
      lw[i] += LOG ? qg_log_fatmoid(-cval / ce) : qg_logsig(-cval / ce);
    }
  }
}

// per (sample, candidate): the value entering the sample reduction and, with `du`, its slopes
// with respect to the Q utilities (du) and the Q summed log feasibilities (dl)
template <int Q, bool LOG>
__device__ __forceinline__ double sb_sample(const SbTab& t, const double* __restrict__ Ys, size_t st, double best,
                                            double tr, double tm, double* du, double* dl) {
  if (!LOG) {
    double val[Q], W[Q];
    sb_points<Q, false>(t, Ys, st, val, W);
    const bool con = t.o.nc != 0;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double v = val[i] - best;
      W[i] = con ? exp(W[i]) : 1.0;
      val[i] = (v > 0.0 ? v : 0.0) * W[i];
    }
    double mx = val[0];
    int am = 0;
#pragma unroll
    for (int i = 1; i < Q; ++i)
      if (val[i] > mx) {   // first arg-max (torch.max)
        mx = val[i];
        am = i;
      }
    const bool on = mx > 0.0;
    if (du)
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        du[i] = (on && i == am) ? W[i] : 0.0;       // d [(u - best)_+ W] / d u
        dl[i] = (on && i == am) ? val[i] : 0.0;     // d [(u - best)_+ exp(lw)] / d lw
      }
    return on ? mx : 0.0;
  }
  double a[Q], da[Q], lw[Q];
  sb_points<Q, true>(t, Ys, st, a, lw);
#pragma unroll
  for (int i = 0; i < Q; ++i) a[i] = log_fatplus(a[i] - best, tr, du ? &da[i] : nullptr) + lw[i];
  const double v = ns_fatmax<Q>(a, tm, du ? dl : nullptr);
  if (du)
#pragma unroll
    for (int i = 0; i < Q; ++i) du[i] = dl[i] * da[i];
  return v;
}

template <int Q, bool LOG, bool BWD>
__global__ __launch_bounds__(NS_THREADS) void sobo_scan(int S, int b, SbTab t, const double* __restrict__ Y,
                                                        const double* __restrict__ best, int best_stride, double tr,
                                                        double tm, const int* __restrict__ flags,
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
      const double v = sb_sample<Q, LOG>(t, Yc + (size_t)s * sbq, bq, best[(size_t)s * best_stride], tr, tm, nullptr,
                                         nullptr);
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
    const double v = sb_sample<Q, LOG>(t, Ys, bq, best[(size_t)s * best_stride], tr, tm, du, dl);
    // d acq / d v_s: softmax weight over the samples (log), 1 / S (plain)
    double w;
    if (LOG) w = (v > -INFINITY && lse > -INFINITY) ? go * exp(v - lse) : 0.0;
    else w = go / (double)S;
    // every output row is written: the slopes of the terms / constraints reading output j
    for (int j = 0; j < mm; ++j) {
      double acc[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) acc[i] = 0.0;
      for (int k = 0; k < t.o.mo; ++k) {
        if (t.o.oo[k] != j) continue;
        const double wk = t.w[k];
#pragma unroll
        for (int i = 0; i < Q; ++i) acc[i] += du[i] * (wk * sb_dterm(t, k, Ys[(size_t)j * bq + i]));
      }
      for (int e = 0; e < t.o.nc; ++e) {
        if (t.o.co[e] != j) continue;
        const double cs = t.o.cs[e], ct = t.o.ct[e], ce = t.o.ce[e];
        const double sc = -cs / ce;   // d (-c / eta) / d y
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const double x = -(cs * (Ys[(size_t)j * bq + i] - ct)) / ce;
          acc[i] += dl[i] * (LOG ? qg_dlog_fatmoid(x) : qg_sig(-x)) * sc;
        }
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) dYs[(size_t)j * bq + i] = w == 0.0 ? 0.0 : w * acc[i];
    }
  }
}

int sobo_scan_launch(hipStream_t s, int q, int m_model, int S, int b, const evr_sobo* sb, const double* Y,
                     const int* flags, const double* gout, double* acq, double* dY) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "sobo_scan: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  SbTab t;
  if (int rc = sb_tab("sobo_scan", sb, m_model, &t)) return rc;
  EVR_CHECK(S >= 1 && b >= 0 && Y && sb->best && acq && (sb->best_stride == 0 || sb->best_stride == 1),
            "sobo_scan: bad arguments (S >= 1, best_stride 0 or 1)");
  const bool log_mode = sb->log != 0;
  const double tr = sb->tau_relu, tm = sb->tau_max;
  EVR_CHECK(!log_mode || (tr > 0.0 && tm > 0.0), "sobo_scan: tau_relu / tau_max must be positive");
  if (b == 0) return 0;
  const int grid = cdiv(b, NS_CL);
  const double* best = sb->best;
  const int bs = sb->best_stride;
#define GO(QQ)                                                                                                      \
  if (log_mode) {                                                                                                   \
    if (dY) sobo_scan<QQ, true, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq, dY); \
    else sobo_scan<QQ, true, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq, dY); \
  } else {                                                                                                          \
    if (dY) sobo_scan<QQ, false, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,  \
                                                                   dY);                                             \
    else sobo_scan<QQ, false, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, Y, best, bs, tr, tm, flags, gout, acq,    \
                                                                 dY);                                               \
  }                                                                                                                 \
  EVR_LAUNCH_CHECK()
  SB_SWITCH(q, GO, "sobo_scan");
#undef GO
  return 0;
}

}  // namespace evr

extern "C" int evr_sobo_scan(void* stream, int q, int m_model, int S, int b, const evr_sobo* sb, const double* Y,
                             const int* flags, const double* gout, double* acq, double* dY) {
  return evr::sobo_scan_launch((hipStream_t)stream, q, m_model, S, b, sb, Y, flags, gout, acq, dY);
}
