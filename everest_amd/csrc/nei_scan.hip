// Single-objective improvement scan on gfx950: the step between the joint samples Y of
// q-point candidates and dY for qNEI / qLogNEI / qLogEI (and qEI over joint batches).
//
// Restates, for one model output with the affine objective g = a y + b,
//   [upstream] qNoisyExpectedImprovement:     acq = mean_s max_i (g(y_si) - best_s)_+
//   [upstream] qLogNoisyExpectedImprovement / qLogExpectedImprovement (fat = True):
//       acq = logmeanexp_s fatmax_i(log fatplus(g(y_si) - best_s; tau_relu); tau_max)
// as called from bofire/strategies/predictives/sobo.py:51-90; best_s is the per-sample
// incumbent max_k g(Y_base[s, k]) of the noisy variants or the scalar best_f (stride 0).
// fatplus / fatmax are botorch.utils.safe_math's (alpha = 2: pareto(u) = 2 / (2 + 2u + u^2)),
// log_fatplus and its slope are the ones of the log hypervolume scans (common.hpp).
//
// MI355X layout: a 256-thread workgroup owns a tile of 16 candidates; thread = (column lane
// cl = tid & 15, sample lane sl = tid >> 4), so a wave covers 16 candidates x 4 sample rows
// and its loads / stores of Y / dY walk the contiguous c*q + i axis (16 q consecutive doubles
// per row).  Each thread folds the samples sl, sl + 16, ... into a running sum (plain) or an
// online (max, sum) pair (log); the 16 sample lanes of a column are combined in a fixed order:
// shuffle-down by 32 and 16 inside the wave, then waves 0..3 through LDS, every thread
// repeating the same four merges.  The backward needs the candidate's logsumexp first, so it
// walks Y a second time (S x 16 q doubles per tile: cache resident) instead of keeping
// per-sample values.  No atomics; run-to-run bitwise reproducible.  One launch per
// evaluation, forward and backward.
#include "common.hpp"
#include "ns_reduce.hpp"
#include "../../include/everest_amd.h"

namespace evr {

// per (sample, candidate): the value entering the sample reduction and, with `d`, its
// gradient with respect to the Q sample values y
template <int Q, bool LOG>
__device__ __forceinline__ double ns_point(const double* y, double best, double oa, double ob, double tr, double tm,
                                           double* d) {
  if (!LOG) {
    double mx = fma(oa, y[0], ob) - best;
    int am = 0;
#pragma unroll
    for (int i = 1; i < Q; ++i) {
      const double v = fma(oa, y[i], ob) - best;
      if (v > mx) {   // first arg-max (torch.max)
        mx = v;
        am = i;
      }
    }
    const bool on = mx > 0.0;
    if (d)
#pragma unroll
      for (int i = 0; i < Q; ++i) d[i] = (on && i == am) ? oa : 0.0;
    return on ? mx : 0.0;
  }
  double a[Q], da[Q], dz[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) a[i] = log_fatplus(fma(oa, y[i], ob) - best, tr, d ? &da[i] : nullptr);
  const double v = ns_fatmax<Q>(a, tm, d ? dz : nullptr);
  if (d)
#pragma unroll
    for (int i = 0; i < Q; ++i) d[i] = dz[i] * da[i] * oa;
  return v;
}

template <int Q, bool LOG, bool BWD>
__global__ __launch_bounds__(NS_THREADS) void nei_scan(int S, int b, const double* __restrict__ Y,
                                                       const double* __restrict__ best, int best_stride, double oa,
                                                       double ob, double tr, double tm,
                                                       const int* __restrict__ flags, const double* __restrict__ gout,
                                                       double* __restrict__ acq, double* __restrict__ dY) {
  __shared__ double red_m[NS_THREADS / 64][NS_CL];
  __shared__ double red_s[NS_THREADS / 64][NS_CL];
  const int tid = threadIdx.x, cl = tid & (NS_CL - 1), sl = tid >> 4;
  const int c = blockIdx.x * NS_CL + cl;
  const bool live = c < b;
  const size_t bq = (size_t)b * Q;
  const double* Yc = Y + (size_t)c * Q;   // dereferenced only when live
  double m = -INFINITY, sum = 0.0;
  if (live) {
    for (int s = sl; s < S; s += NS_SL) {
      double y[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) y[i] = Yc[(size_t)s * bq + i];
      const double v = ns_point<Q, LOG>(y, best[(size_t)s * best_stride], oa, ob, tr, tm, nullptr);
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
    acq[c] = (flags && flags[c] != 0) ? nan("") : val;
  }
  if (!BWD) return;
  const double go = gout ? gout[c] : 1.0;
  double* dYc = dY + (size_t)c * Q;
  for (int s = sl; s < S; s += NS_SL) {
    double y[Q], d[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) y[i] = Yc[(size_t)s * bq + i];
    const double v = ns_point<Q, LOG>(y, best[(size_t)s * best_stride], oa, ob, tr, tm, d);
    // d acq / d v_s: softmax weight over the samples (log), 1 / S (plain)
    double w;
    if (LOG) w = (v > -INFINITY && lse > -INFINITY) ? go * exp(v - lse) : 0.0;
    else w = go / (double)S;
#pragma unroll
    for (int i = 0; i < Q; ++i) dYc[(size_t)s * bq + i] = w == 0.0 ? 0.0 : w * d[i];
  }
}

#define NS_SWITCH(q, MACRO)                                                 \
  switch (q) {                                                              \
    case 1: MACRO(1); break;                                                \
    case 2: MACRO(2); break;                                                \
    case 3: MACRO(3); break;                                                \
    case 4: MACRO(4); break;                                                \
    case 5: MACRO(5); break;                                                \
    case 6: MACRO(6); break;                                                \
    case 7: MACRO(7); break;                                                \
    case 8: MACRO(8); break;                                                \
    case 9: MACRO(9); break;                                                \
    case 10: MACRO(10); break;                                              \
    case 11: MACRO(11); break;                                              \
    case 12: MACRO(12); break;                                              \
    default: EVR_CHECK(false, "nei_scan: q = %d not supported", q);         \
  }

int nei_scan_launch(hipStream_t s, int q, bool log_mode, int S, int b, const double* Y, const double* best,
                    int best_stride, double oa, double ob, double tr, double tm, const int* flags,
                    const double* gout, double* acq, double* dY) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "nei_scan: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  EVR_CHECK(S >= 1 && b >= 0 && Y && best && acq && (best_stride == 0 || best_stride == 1),
            "nei_scan: bad arguments (S >= 1, best_stride 0 or 1)");
  EVR_CHECK(!log_mode || (tr > 0.0 && tm > 0.0), "nei_scan: tau_relu / tau_max must be positive");
  if (b == 0) return 0;
  const int grid = cdiv(b, NS_CL);
#define GO(QQ)                                                                                                     \
  if (log_mode) {                                                                                                  \
    if (dY) nei_scan<QQ, true, true><<<grid, NS_THREADS, 0, s>>>(S, b, Y, best, best_stride, oa, ob, tr, tm, flags, \
                                                                 gout, acq, dY);                                   \
    else nei_scan<QQ, true, false><<<grid, NS_THREADS, 0, s>>>(S, b, Y, best, best_stride, oa, ob, tr, tm, flags,   \
                                                               gout, acq, dY);                                     \
  } else {                                                                                                         \
    if (dY) nei_scan<QQ, false, true><<<grid, NS_THREADS, 0, s>>>(S, b, Y, best, best_stride, oa, ob, tr, tm,       \
                                                                  flags, gout, acq, dY);                           \
    else nei_scan<QQ, false, false><<<grid, NS_THREADS, 0, s>>>(S, b, Y, best, best_stride, oa, ob, tr, tm, flags,  \
                                                                gout, acq, dY);                                    \
  }                                                                                                                \
  EVR_LAUNCH_CHECK()
  NS_SWITCH(q, GO);
#undef GO
  return 0;
}

}  // namespace evr

extern "C" int evr_nei_scan(void* stream, int q, int log, int S, int b, const double* Y, const double* best,
                            int best_stride, double obj_a, double obj_b, double tau_relu, double tau_max,
                            const int* flags, const double* gout, double* acq, double* dY) {
  return evr::nei_scan_launch((hipStream_t)stream, q, log != 0, S, b, Y, best, best_stride, obj_a, obj_b, tau_relu,
                              tau_max, flags, gout, acq, dY);
}
