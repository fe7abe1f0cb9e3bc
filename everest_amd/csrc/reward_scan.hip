// Reward scans qSR / qUCB / qPI with output constraints on gfx950: the step between the joint
// samples Y of q-point candidates (several model outputs) and dY for the three single-objective
// acquisitions of SoboStrategy / AdditiveSoboStrategy that are no improvement over an incumbent
// per sample.
//
// Restates (from memory of BoTorch, parity-unpinned), for the utility u(y) = sum_t w_t g_t(y[out_t]),
// the constraints c_e(y) = sign_e (y[out_e] - thr_e) and W = exp(sum_e logsigmoid(-c_e / eta_e))
// (plain sigmoid; W = 1 without constraints):
//   [upstream] ConstrainedMCObjective / apply_constraints with infeasible cost M >= 0 — the reward
//       r = (u + M) W - M   (constraints exist),   r = u   (none)
//   as bofire/strategies/predictives/sobo.py:130-145, 192-205 builds it for qSR and qUCB;
//   [upstream] qSimpleRegret:            acq = mean_s max_i r_si
//   [upstream] qUpperConfidenceBound:    acq = mean_s max_i ( rbar_i + k |r_si - rbar_i| ),
//       rbar_i = mean_s r_si,  k = sqrt(beta pi / 2)
//   [upstream] qProbabilityOfImprovement with SampleReducingMCAcquisitionFunction._apply_constraints:
//       acq = mean_s max_i [ sigmoid((u_si - best_f) / tau) W_si ]
// All maxima take the FIRST arg-max (torch.max).  Adjoints, with i*_s the arg-max of sample s:
//   qSR:  d acq / d r_ti = [i*_t = i] / S
//   qUCB: d acq / d r_ti = ( [i*_t = i] k sgn(r_ti - rbar_i) + G_i / S ) / S,
//         G_i = sum_s [i*_s = i] (1 - k sgn(r_si - rbar_i)),  sgn(0) = 0 (torch.abs)
//   qPI:  x = (u - best_f) / tau, v = sigmoid(x) W: dv/du = sigmoid(x) sigmoid(-x) W / tau, dv/dlw = v
//   reward: dr/du = W, dr/dlw = (u + M) W.
//
// MI355X layout: that of sobo_scan.hip.  A 256-thread workgroup owns a tile of 16 candidates;
// thread = (column lane cl = tid & 15, sample lane sl = tid >> 4); the 16 sample lanes of a
// column are combined in the fixed order of the sibling scans (shuffle-down by 32 and 16, then
// waves 0..3 read back from LDS by every thread, which is also the broadcast).  The term /
// constraint table travels by value; its loops are the OUTER ones with the q points unrolled
// inside (see sobo_scan.hip on scratch).  No atomics; run-to-run bitwise reproducible.
//
// qSR and qPI are one pass over Y forward and one more backward.  qUCB needs the sample mean of
// every point's reward before any sample can be reduced, and its adjoint couples all samples of a
// column; because the workgroup owns all S samples of its 16 columns it still is ONE launch:
//   pass 1: per-point reward sums over the thread's samples, combined -> the Q means;
//   pass 2: per-sample arg-max and value; backward also the per-point sums G_i, combined;
//   pass 3 (backward): dY from the per-sample term plus G_i / S.
// Per-thread state is O(Q) doubles (means, G, reward, weight); the rewards are recomputed from Y
// in every pass, never stored.
#include "sb_common.hpp"

namespace evr {

// everything but the table and the pointers, by value
struct RwPar {
  double ks;     // qUCB: k = sqrt(beta pi / 2)
  double tau;    // qPI: temperature
  double M;      // qSR / qUCB: infeasible cost
};

// sums v[0..N) over the 16 sample lanes of each column, in the fixed order; every thread of the
// column gets the result.  All 256 threads must call it.
template <int N, int NR>
__device__ __forceinline__ void rw_combine(double* v, double (&red)[NS_THREADS / 64][NR][NS_CL], int tid, int cl) {
  static_assert(N <= NR, "reduction buffer too small");
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int o = 32; o >= NS_CL; o >>= 1) v[i] += __shfl_down(v[i], o, 64);
    if ((tid & 63) < NS_CL) red[tid >> 6][i][cl] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double a = red[0][i][cl];
#pragma unroll
    for (int w = 1; w < NS_THREADS / 64; ++w) a += red[w][i][cl];
    v[i] = a;
  }
}

// the Q points of one (sample, candidate): rewards r, and for the backward uw = (u + M) W and W
// (1 and unused 0 without constraints)
template <int Q>
__device__ __forceinline__ void rw_rewards(const SbTab& t, double M, const double* __restrict__ Ys, size_t st,
                                           double* r, double* uw, double* W) {
  sb_util<Q>(t, Ys, st, r);
#pragma unroll
  for (int i = 0; i < Q; ++i) W[i] = 0.0;
  sb_feas<Q, false>(t.o, Ys, st, W);
  const bool con = t.o.nc != 0;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    if (con) {
      W[i] = exp(W[i]);
      uw[i] = (r[i] + M) * W[i];
      r[i] = uw[i] - M;
    } else {
      W[i] = 1.0;
      uw[i] = 0.0;
    }
  }
}

// qPI: the Q weighted probabilities v = sigmoid(x) W, and for the backward the slopes dv/du
template <int Q>
__device__ __forceinline__ void rw_pi(const SbTab& t, double best, double tau, const double* __restrict__ Ys,
                                      size_t st, double* v, double* dvu) {
  double W[Q];
  sb_util<Q>(t, Ys, st, v);
#pragma unroll
  for (int i = 0; i < Q; ++i) W[i] = 0.0;
  sb_feas<Q, false>(t.o, Ys, st, W);
  const bool con = t.o.nc != 0;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const double x = (v[i] - best) / tau, w = con ? exp(W[i]) : 1.0, sg = qg_sig(x);
    v[i] = sg * w;
    dvu[i] = sg * qg_sig(-x) * w / tau;
  }
}

// first arg-max (torch.max)
template <int Q>
__device__ __forceinline__ int rw_argmax(const double* v, double& mx) {
  mx = v[0];
  int am = 0;
#pragma unroll
  for (int i = 1; i < Q; ++i)
    if (v[i] > mx) {
      mx = v[i];
      am = i;
    }
  return am;
}

__device__ __forceinline__ double rw_sgn(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// one sample's rows of dY from the slopes with respect to the Q utilities (du) and summed log
// feasibilities (dl), times w.  Every output row is written; outputs nothing reads get zeros.
template <int Q>
__device__ __forceinline__ void rw_write(const SbTab& t, const double* __restrict__ Ys, double* __restrict__ dYs,
                                         size_t bq, const double* du, const double* dl, double w) {
  for (int j = 0; j < t.o.m; ++j) {
    const double* Yj = Ys + (size_t)j * bq;
    double acc[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) acc[i] = 0.0;
    for (int k = 0; k < t.o.mo; ++k) {
      if (t.o.oo[k] != j) continue;
      const double wk = t.w[k];
#pragma unroll
      for (int i = 0; i < Q; ++i) acc[i] += du[i] * (wk * sb_dterm(t, k, Yj[i]));
    }
    sb_dfeas<Q, false>(t.o, j, Yj, dl, acc);
#pragma unroll
    for (int i = 0; i < Q; ++i) dYs[(size_t)j * bq + i] = w == 0.0 ? 0.0 : w * acc[i];
  }
}

template <int Q, int MODE, bool BWD>
__global__ __launch_bounds__(NS_THREADS) void reward_scan(int S, int b, SbTab t, RwPar p,
                                                          const double* __restrict__ Y,
                                                          const double* __restrict__ best,
                                                          const int* __restrict__ flags,
                                                          const double* __restrict__ gout, double* __restrict__ acq,
                                                          double* __restrict__ dY) {
  constexpr bool UCB = MODE == EVR_REWARD_UCB, PI = MODE == EVR_REWARD_PI;
  constexpr int NA = UCB ? Q : 1, NB = (UCB && BWD) ? Q + 1 : 1;
  __shared__ double red_a[NS_THREADS / 64][NA][NS_CL];   // qUCB pass 1: the Q reward sums
  __shared__ double red_b[NS_THREADS / 64][NB][NS_CL];   // the value sum (slot 0) and qUCB's G (1..Q)
  const int tid = threadIdx.x, cl = tid & (NS_CL - 1), sl = tid >> 4;
  const int c = blockIdx.x * NS_CL + cl;
  const bool live = c < b;
  const size_t bq = (size_t)b * Q, sbq = (size_t)t.o.m * bq;
  const double* Yc = Y + (size_t)c * Q;   // dereferenced only when live
  const double bf = PI ? best[0] : 0.0;
  const double dS = (double)S;

  double mean[UCB ? Q : 1];
  if constexpr (UCB) {
    // pass 1: the sample mean of every point's reward
#pragma unroll
    for (int i = 0; i < Q; ++i) mean[i] = 0.0;
    if (live)
      for (int s = sl; s < S; s += NS_SL) {
        double r[Q], uw[Q], W[Q];
        rw_rewards<Q>(t, p.M, Yc + (size_t)s * sbq, bq, r, uw, W);
#pragma unroll
        for (int i = 0; i < Q; ++i) mean[i] += r[i];
      }
    rw_combine<NA, NA>(mean, red_a, tid, cl);
#pragma unroll
    for (int i = 0; i < Q; ++i) mean[i] /= dS;
  }

  // the value sum (ga[0]) and, in qUCB's backward, G_i (ga[1 + i])
  double ga[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) ga[i] = 0.0;
  if (live)
    for (int s = sl; s < S; s += NS_SL) {
      const double* Ys = Yc + (size_t)s * sbq;
      double v[Q], mx;
      if constexpr (PI) {
        double dvu[Q];
        rw_pi<Q>(t, bf, p.tau, Ys, bq, v, dvu);
        rw_argmax<Q>(v, mx);
      } else {
        double uw[Q], W[Q];
        rw_rewards<Q>(t, p.M, Ys, bq, v, uw, W);
        if constexpr (UCB) {
          double sg[Q];
#pragma unroll
          for (int i = 0; i < Q; ++i) {
            const double dlt = v[i] - mean[i];
            sg[i] = rw_sgn(dlt);
            v[i] = mean[i] + p.ks * fabs(dlt);
          }
          const int am = rw_argmax<Q>(v, mx);
          if constexpr (BWD) {
#pragma unroll
            for (int i = 0; i < Q; ++i)
              if (i == am) ga[1 + i] += 1.0 - p.ks * sg[i];
          }
        } else {
          rw_argmax<Q>(v, mx);
        }
      }
      ga[0] += mx;
    }
  rw_combine<NB, NB>(ga, red_b, tid, cl);
  if (!live) return;
  if (sl == 0) {
    bool bad = false;
    if (flags)
      for (int j = 0; j < t.o.m; ++j) bad |= flags[(size_t)j * b + c] != 0;
    acq[c] = bad ? nan("") : ga[0] / dS;
  }
  if constexpr (BWD) {
    const double w = (gout ? gout[c] : 1.0) / dS;
    double* dYc = dY + (size_t)c * Q;
#pragma unroll
    for (int i = 1; i < NB; ++i) ga[i] /= dS;   // qUCB: G_i / S
    // backward pass over Y: the arg-max again, the slopes with respect to u and lw, dY
    for (int s = sl; s < S; s += NS_SL) {
      const double* Ys = Yc + (size_t)s * sbq;
      double du[Q], dl[Q], mx;
      if constexpr (PI) {
        rw_pi<Q>(t, bf, p.tau, Ys, bq, dl, du);
        const int am = rw_argmax<Q>(dl, mx);
#pragma unroll
        for (int i = 0; i < Q; ++i)
          if (i != am) du[i] = dl[i] = 0.0;
      } else {
        double v[Q];
        rw_rewards<Q>(t, p.M, Ys, bq, v, dl, du);   // dl = (u + M) W, du = W
        if constexpr (UCB) {
          double sg[Q];
#pragma unroll
          for (int i = 0; i < Q; ++i) {
            const double dlt = v[i] - mean[i];
            sg[i] = rw_sgn(dlt);
            v[i] = mean[i] + p.ks * fabs(dlt);
          }
          const int am = rw_argmax<Q>(v, mx);
#pragma unroll
          for (int i = 0; i < Q; ++i) {
            const double dr = (i == am ? p.ks * sg[i] : 0.0) + ga[1 + i];
            du[i] *= dr;
            dl[i] *= dr;
          }
        } else {
          const int am = rw_argmax<Q>(v, mx);
#pragma unroll
          for (int i = 0; i < Q; ++i)
            if (i != am) du[i] = dl[i] = 0.0;
        }
      }
      rw_write<Q>(t, Ys, dYc + (size_t)s * sbq, bq, du, dl, w);
    }
  }
}

int reward_scan_launch(hipStream_t s, int q, int m_model, int S, int b, const evr_reward* rw, const double* Y,
                       const int* flags, const double* gout, double* acq, double* dY) {
  EVR_CHECK(q >= 1 && q <= EVR_QNG_MAX_Q, "reward_scan: q = %d outside 1..%d", q, EVR_QNG_MAX_Q);
  SbTab t;
  if (int rc = sb_tab("reward_scan", rw, m_model, &t)) return rc;
  const int mode = rw->mode;
  EVR_CHECK(mode == EVR_REWARD_SR || mode == EVR_REWARD_UCB || mode == EVR_REWARD_PI, "reward_scan: mode %d", mode);
  EVR_CHECK(S >= 1 && b >= 0 && Y && acq, "reward_scan: bad arguments (S >= 1)");
  RwPar p{0.0, 1.0, 0.0};
  if (mode == EVR_REWARD_UCB) {
    EVR_CHECK(rw->ucb_scale >= 0.0 && rw->ucb_scale < INFINITY,
              "reward_scan: ucb_scale = %g (sqrt(beta pi / 2), beta >= 0) is negative or not finite", rw->ucb_scale);
    p.ks = rw->ucb_scale;
  }
  if (mode == EVR_REWARD_PI) {
    EVR_CHECK(rw->tau > 0.0 && rw->tau < INFINITY, "reward_scan: tau = %g must be positive", rw->tau);
    EVR_CHECK(rw->best, "reward_scan: qPI needs the incumbent");
    p.tau = rw->tau;
  } else {
    EVR_CHECK(rw->infeasible_cost >= 0.0 && rw->infeasible_cost < INFINITY,
              "reward_scan: infeasible cost M = %g is negative or not finite", rw->infeasible_cost);
    p.M = rw->infeasible_cost;
  }
  if (b == 0) return 0;
  const int grid = cdiv(b, NS_CL);
  const double* best = rw->best;
#define GO_MODE(QQ, MM)                                                                                      \
  if (dY) reward_scan<QQ, MM, true><<<grid, NS_THREADS, 0, s>>>(S, b, t, p, Y, best, flags, gout, acq, dY);  \
  else reward_scan<QQ, MM, false><<<grid, NS_THREADS, 0, s>>>(S, b, t, p, Y, best, flags, gout, acq, dY)
#define GO(QQ)                                          \
  if (mode == EVR_REWARD_SR) {                          \
    GO_MODE(QQ, EVR_REWARD_SR);                         \
  } else if (mode == EVR_REWARD_UCB) {                  \
    GO_MODE(QQ, EVR_REWARD_UCB);                        \
  } else {                                              \
    GO_MODE(QQ, EVR_REWARD_PI);                         \
  }                                                     \
  EVR_LAUNCH_CHECK()
  SB_SWITCH(q, GO, "reward_scan");
#undef GO
#undef GO_MODE
  return 0;
}

}  // namespace evr

extern "C" int evr_reward_scan(void* stream, int q, int m_model, int S, int b, const evr_reward* rw, const double* Y,
                               const int* flags, const double* gout, double* acq, double* dY) {
  return evr::reward_scan_launch((hipStream_t)stream, q, m_model, S, b, rw, Y, flags, gout, acq, dY);
}
