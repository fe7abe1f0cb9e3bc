// Objective / output-constraint tables passed by value to the kernels, and the per-point device
// functions over them (objective callables, log-sigmoid, log-fatmoid), shared by the general
// hypervolume chain (qnehvi_general.hip) and the single-objective scan (sobo_scan.hip).
#pragma once
#include "common.hpp"
#include "../../include/everest_amd.h"

namespace evr {

constexpr int QG_MAXM = 8, QG_MAXC = 16;

// objectives / constraints by value (kernel argument)
struct QgObj {
  int m, mo, nc;
  int oo[QG_MAXM], ok[QG_MAXM];
  double p0[QG_MAXM], p1[QG_MAXM];
  int co[QG_MAXC];
  double cs[QG_MAXC], ct[QG_MAXC], ce[QG_MAXC];
};

__device__ __forceinline__ double qg_obj(const QgObj& o, int k, double y) {
  if (o.ok[k] == EVR_OBJ_AFFINE) return fma(o.p0[k], y, o.p1[k]);
  return -pow(fabs(y - o.p0[k]), o.p1[k]);   // CloseToTarget: -|y - t|^e
}

__device__ __forceinline__ double qg_dobj(const QgObj& o, int k, double y) {
  if (o.ok[k] == EVR_OBJ_AFFINE) return o.p0[k];
  const double u = y - o.p0[k], e = o.p1[k];
  if (u == 0.0) return 0.0;                  // torch: sign(0) = 0 in abs' backward
  return -e * pow(fabs(u), e - 1.0) * (u > 0.0 ? 1.0 : -1.0);
}

// log-sigmoid, stable: min(x, 0) - log1p(exp(-|x|))
__device__ __forceinline__ double qg_logsig(double x) { return fmin(x, 0.0) - log1p(exp(-fabs(x))); }
__device__ __forceinline__ double qg_sig(double x) {
  return x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
}

// [upstream] botorch.utils.safe_math.log_fatmoid — the fat-tailed (Cauchy, O(1/x^2) for
// x -> -inf) smooth Heaviside that compute_smoothed_feasibility_indicator(log=True, fat=True)
// uses in qLogNEHVI / qLogEHVI:  fatmoid(x) = 2/3 cauchy(x - m) for x < 0,
// 1 - 2/3 cauchy(x + m) otherwise, cauchy(x) = 1 / (1 + x^2), m = sqrt(1/3) (continuous, = 1/2
// at 0).  Log evaluated without cancellation on both branches; qg_dlog_fatmoid is its slope.
constexpr double QG_FATMOID_M = 0.57735026918962576;
__device__ __forceinline__ double qg_log_fatmoid(double x) {
  if (x < 0.0) {
    const double u = x - QG_FATMOID_M;
    return -0.40546510810816438 - log1p(u * u);   // log(2/3) - log(1 + u^2)
  }
  const double u = x + QG_FATMOID_M;
  return log1p(-(2.0 / 3.0) / (1.0 + u * u));
}
__device__ __forceinline__ double qg_dlog_fatmoid(double x) {
  if (x < 0.0) {
    const double u = x - QG_FATMOID_M;
    return -2.0 * u / (1.0 + u * u);
  }
  const double u = x + QG_FATMOID_M, w = 1.0 + u * u, c = (2.0 / 3.0) / w;
  return 2.0 * u * c / (w * (1.0 - c));
}

}  // namespace evr
