// Pieces shared by the utility scans over several model outputs (sobo_scan.hip: sum of terms;
// parego_scan.hip: augmented Chebyshev): the by-value term / constraint table, the per-term
// callables, and the same steps sobo_scan's sb_points / sb_sample / backward take around the
// utility, as functions of their own: the summed log feasibilities of the q points, the reduction
// over the q points of a (sample, candidate), and the constraint slopes of one output row.
// sobo_scan.hip keeps its own fused copies of those three: its device code is unchanged.
// Host side: the table check and copy of the three scans (sb_fill, sb_tab), reward_scan.hip's too.
#pragma once
#include "common.hpp"
#include "ns_reduce.hpp"
#include "qg_obj.hpp"
#include "../../include/everest_amd.h"

namespace evr {

static_assert(EVR_SOBO_MAX_TERMS == QG_MAXM, "the term table reuses QgObj's objective slots");

// terms (QgObj's objective slots plus weight and third parameter) and constraints, by value
struct SbTab {
  QgObj o;
  double w[QG_MAXM], p2[QG_MAXM];
};

__device__ __forceinline__ double sb_term(const SbTab& t, int k, double y) {
  const int kind = t.o.ok[k];
  if (kind == EVR_OBJ_AFFINE || kind == EVR_OBJ_CLOSE_TO_TARGET) return qg_obj(t.o, k, y);
  const double st = t.o.p0[k];
  if (kind == EVR_OBJ_SIGMOID) return qg_sig(st * (y - t.o.p1[k]));
  // target: sig(st (y - (tv - tol))) * (1 - sig(st (y - (tv + tol))))
  return qg_sig(st * (y - (t.o.p1[k] - t.p2[k]))) * qg_sig(-st * (y - (t.o.p1[k] + t.p2[k])));
}

__device__ __forceinline__ double sb_dterm(const SbTab& t, int k, double y) {
  const int kind = t.o.ok[k];
  if (kind == EVR_OBJ_AFFINE || kind == EVR_OBJ_CLOSE_TO_TARGET) return qg_dobj(t.o, k, y);
  const double st = t.o.p0[k];
  if (kind == EVR_OBJ_SIGMOID) {
    const double x = st * (y - t.o.p1[k]);
    return st * qg_sig(x) * qg_sig(-x);
  }
  const double x1 = st * (y - (t.o.p1[k] - t.p2[k])), x2 = st * (y - (t.o.p1[k] + t.p2[k]));
  return st * qg_sig(x1) * qg_sig(-x2) * (qg_sig(-x1) - qg_sig(x2));
}

// utilities u(y) = sum_t w_t g_t(y[out_t]) of the Q points of one (sample, candidate) (Ys, st as
// in sb_feas below).  The term loop is the outer one, as in sobo_scan.hip's sb_points.
template <int Q>
__device__ __forceinline__ void sb_util(const SbTab& t, const double* __restrict__ Ys, size_t st, double* u) {
#pragma unroll
  for (int i = 0; i < Q; ++i) u[i] = 0.0;
  for (int k = 0; k < t.o.mo; ++k) {
    const double* Yk = Ys + (size_t)t.o.oo[k] * st;
    const double wk = t.w[k];
#pragma unroll
    for (int i = 0; i < Q; ++i) u[i] += wk * sb_term(t, k, Yk[i]);
  }
}

// summed log feasibilities of the Q points of one (sample, candidate), added to lw (log-sigmoid
// in plain mode, log-fatmoid in log mode).  Ys: the output-0 sample of point 0, outputs `st`
// doubles apart.  The constraint loop is the outer one: one set of scalar table reads per
// constraint, whatever Q.
template <int Q, bool LOG>
__device__ __forceinline__ void sb_feas(const QgObj& o, const double* __restrict__ Ys, size_t st, double* lw) {
  for (int e = 0; e < o.nc; ++e) {
    const double* Ye = Ys + (size_t)o.co[e] * st;
    const double cs = o.cs[e], ct = o.ct[e], ce = o.ce[e];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double cval = cs * (Ye[i] - ct);
      lw[i] += LOG ? qg_log_fatmoid(-cval / ce) : qg_logsig(-cval / ce);
    }
  }
}

// per (sample, candidate), from the Q utilities u and summed log feasibilities lw (both
// overwritten): the value entering the sample reduction and, with `du`, its slopes with respect
// to the utilities (du) and the log feasibilities (dl).  con: whether any constraint exists.
template <int Q, bool LOG>
__device__ __forceinline__ double sb_reduce(double* u, double* lw, bool con, double best, double tr, double tm,
                                            double* du, double* dl) {
  if (!LOG) {
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double v = u[i] - best;
      lw[i] = con ? exp(lw[i]) : 1.0;
      u[i] = (v > 0.0 ? v : 0.0) * lw[i];
    }
    double mx = u[0];
    int am = 0;
#pragma unroll
    for (int i = 1; i < Q; ++i)
      if (u[i] > mx) {   // first arg-max (torch.max)
        mx = u[i];
        am = i;
      }
    const bool on = mx > 0.0;
    if (du)
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        du[i] = (on && i == am) ? lw[i] : 0.0;     // d [(u - best)_+ W] / d u
        dl[i] = (on && i == am) ? u[i] : 0.0;      // d [(u - best)_+ exp(lw)] / d lw
      }
    return on ? mx : 0.0;
  }
  double da[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) u[i] = log_fatplus(u[i] - best, tr, du ? &da[i] : nullptr) + lw[i];
  const double v = ns_fatmax<Q>(u, tm, du ? dl : nullptr);
  if (du)
#pragma unroll
    for (int i = 0; i < Q; ++i) du[i] = dl[i] * da[i];
  return v;
}

// backward: the slopes of the constraints reading output j, added to acc (Yj: the output-j
// sample of point 0; dl: the slopes with respect to the summed log feasibilities)
template <int Q, bool LOG>
__device__ __forceinline__ void sb_dfeas(const QgObj& o, int j, const double* __restrict__ Yj, const double* dl,
                                         double* acc) {
  for (int e = 0; e < o.nc; ++e) {
    if (o.co[e] != j) continue;
    const double cs = o.cs[e], ct = o.ct[e], ce = o.ce[e];
    const double sc = -cs / ce;   // d (-c / eta) / d y
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const double x = -(cs * (Yj[i] - ct)) / ce;
      acc[i] += dl[i] * (LOG ? qg_dlog_fatmoid(x) : qg_sig(-x)) * sc;
    }
  }
}

// host: what the three scans' table builders share.  Checks the description p (evr_sobo,
// evr_parego or evr_reward: the fields read here carry the same names) and copies m, the term
// headers (out, kind, p0, p1) and the constraints into o; the caller adds its own term columns.
// who: the caller's name for the messages; cols: whether the caller's own term columns are
// there; min_terms: 1 (sum of terms) or 2 (Chebyshev); sig_kinds: whether the sigmoid and target
// kinds are allowed beside affine and close-to-target.
template <class P>
static int sb_fill(const char* who, const P* p, bool cols, int m_model, int min_terms, bool sig_kinds, QgObj* o) {
  EVR_CHECK(p && cols && m_model >= 1 && m_model <= QG_MAXM && p->n_term >= min_terms &&
                p->n_term <= EVR_SOBO_MAX_TERMS && p->n_con >= 0 && p->n_con <= QG_MAXC && p->term_out &&
                p->term_kind && p->term_p0 && p->term_p1 &&
                (p->n_con == 0 || (p->con_out && p->con_sign && p->con_thr && p->con_eta)),
            "%s: bad term / constraint description (terms %d..%d, constraints 0..%d, outputs 1..%d)", who, min_terms,
            EVR_SOBO_MAX_TERMS, QG_MAXC, QG_MAXM);
  o->m = m_model;
  o->mo = p->n_term;
  o->nc = p->n_con;
  for (int k = 0; k < p->n_term; ++k) {
    const int kind = p->term_kind[k];
    EVR_CHECK(p->term_out[k] >= 0 && p->term_out[k] < m_model, "%s: term %d reads output %d of %d", who, k,
              p->term_out[k], m_model);
    EVR_CHECK(kind == EVR_OBJ_AFFINE || kind == EVR_OBJ_CLOSE_TO_TARGET ||
                  (sig_kinds && (kind == EVR_OBJ_SIGMOID || kind == EVR_OBJ_TARGET)),
              "%s: term kind %d%s", who, kind, sig_kinds ? "" : " (affine and close-to-target only)");
    o->oo[k] = p->term_out[k];
    o->ok[k] = kind;
    o->p0[k] = p->term_p0[k];
    o->p1[k] = p->term_p1[k];
  }
  for (int e = 0; e < p->n_con; ++e) {
    EVR_CHECK(p->con_out[e] >= 0 && p->con_out[e] < m_model && p->con_eta[e] > 0.0,
              "%s: constraint %d (output %d, eta %g)", who, e, p->con_out[e], p->con_eta[e]);
    o->co[e] = p->con_out[e];
    o->cs[e] = p->con_sign[e];
    o->ct[e] = p->con_thr[e];
    o->ce[e] = p->con_eta[e];
  }
  return 0;
}

// host: the table of a sum of terms (evr_sobo, evr_reward) — sb_fill plus the weights and the
// third parameters
template <class P>
static int sb_tab(const char* who, const P* p, int m_model, SbTab* t) {
  std::memset(t, 0, sizeof(*t));
  if (int rc = sb_fill(who, p, p && p->term_w && p->term_p2, m_model, 1, true, &t->o)) return rc;
  for (int k = 0; k < p->n_term; ++k) {
    t->w[k] = p->term_w[k];
    t->p2[k] = p->term_p2[k];
  }
  return 0;
}

// shared by the launchers: the q switch over the compiled instantiations
#define SB_SWITCH(q, MACRO, NAME)                                           \
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
    default: EVR_CHECK(false, NAME ": q = %d not supported", q);            \
  }

}  // namespace evr
