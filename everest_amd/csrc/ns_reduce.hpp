// Pieces shared by the single-objective scans (nei_scan.hip, sobo_scan.hip): the workgroup
// shape, the online log-sum-exp merge of the fixed-order sample reduction, and the fat-max over
// the q points of a candidate.
#pragma once
#include "common.hpp"

namespace evr {

constexpr int NS_CL = 16, NS_SL = 16, NS_THREADS = NS_CL * NS_SL;

// online log-sum-exp pair: (m, s) <- (m, s) (+) (m2, s2); empty = (-inf, 0)
__device__ __forceinline__ void ns_merge(double& m, double& s, double m2, double s2) {
  if (s2 == 0.0) return;
  if (s == 0.0) {
    m = m2;
    s = s2;
    return;
  }
  if (m2 > m) {
    s = fma(s, exp(m - m2), s2);
    m = m2;
  } else {
    s = fma(s2, exp(m2 - m), s);
  }
}

// fat-max over a[0..Q) (tau t) and its partials dz (nullable)
template <int Q>
__device__ __forceinline__ double ns_fatmax(const double* a, double t, double* dz) {
  double M = a[0];
  int am = 0;
#pragma unroll
  for (int i = 1; i < Q; ++i)
    if (a[i] > M) {
      M = a[i];
      am = i;
    }
  if (Q == 1 || M == -INFINITY) {   // one element: exactly the element
    if (dz)
#pragma unroll
      for (int i = 0; i < Q; ++i) dz[i] = i == am ? 1.0 : 0.0;
    return M;
  }
  double Ssum = 0.0, sp = 0.0, pp[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const double u = (M - a[i]) / t;
    const double p = u < INFINITY ? 2.0 / (2.0 + u * (2.0 + u)) : 0.0;
    Ssum += p;
    pp[i] = p > 0.0 ? (1.0 + u) * p * p : 0.0;   // -pareto'(u)
    if (i != am) sp += pp[i];
  }
  if (dz)
#pragma unroll
    for (int i = 0; i < Q; ++i) dz[i] = i == am ? 1.0 - sp / Ssum : pp[i] / Ssum;
  return M + t * log(Ssum);
}

}  // namespace evr
