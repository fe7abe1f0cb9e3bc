"""Timing of the scalarised, output-constrained single-objective scan on the MI355X
(evr_sobo_scan, sobo_scan.hip) and of the full chain evr_qsobo_eval.  Nothing here is a target.

  scan:        S = 512, q = 1, m = 3 (affine + close-to-target terms), 2 constraints, b = 20 and
               b = 512, forward and forward + backward;
  degenerate:  m = 1, one affine term of weight 1, no constraints, beside evr_nei_scan at the same
               shape and inputs (the existing kernel is the yardstick);
  chain:       QSoboLogNEI.forward_backward per evaluation at b = 20 (n = 512, d = 6, m = 2 outputs,
               S = 512, one constraint).

The paths alternate inside one process, warm; each round times a window of ``--calls`` launches
between device events; reported per launch: the median over ``--rounds`` (>= 20) rounds and the
spread.  Prints one JSON line.

    python tools/bench_sobo.py [--rounds 25] [--calls 20] [--warmup 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from everest_amd import ops
from everest_amd.acquisition import QSoboLogNEI
from everest_amd.gp import GPBatch, GPHyper, standardize_params


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


def stats(v):
    v = np.asarray(v)
    q25, q50, q75 = np.percentile(v, [25, 50, 75])
    return dict(median_us=round(float(q50), 2), iqr_us=round(float(q75 - q25), 2), min_us=round(float(v.min()), 2),
                max_us=round(float(v.max()), 2))


def run(paths, args):
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.rounds):              # alternate the paths round by round
        for k, fn in paths.items():
            times[k].append(window_us(fn, args.calls))
    return {k: stats(v) for k, v in times.items()}


def make_gp(n, d, m, seed, dev):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X + j).sum(1) + 0.5 * ((X - 0.4) ** 2).sum(1) + 0.01 * rng.normal(size=n)
                  for j in range(m)], 1)
    hyp = []
    for j in range(m):
        ym, ys = standardize_params(Y[:, j])
        hyp.append(GPHyper(lengthscale=rng.uniform(0.4, 1.2, d), noise=1e-3, constant=0.0, y_mean=ym, y_std=ys))
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    return X, Y, GPBatch(t(X), t(Y), hyp, 3, t(np.zeros(d)), t(np.ones(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("bench_sobo reports the median of at least 20 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sobo needs the MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    S, q = 512, 1
    out = dict(S=S, q=q, rounds=args.rounds, calls=args.calls, scan=[], degenerate=[])
    gen = torch.Generator(device="cpu").manual_seed(0)
    spec3 = ops.SoboSpec(3, [(0, ops.OBJ_AFFINE, 0.3, -1.0, 0.3, 0.0), (1, ops.OBJ_CLOSE_TO_TARGET, 1.0, 0.4, 2.0, 0.0)],
                         [(1, 1.0, 0.2, 0.5), (2, -1.0, 0.1, 1.0)])
    spec1 = ops.SoboSpec(1, [(0, ops.OBJ_AFFINE, 1.0, -1.0, 0.3, 0.0)])
    for b in (20, 512):
        Y3 = torch.randn(S, 3, b * q, generator=gen, dtype=torch.float64).to(dev)
        Y1 = Y3[:, 0].contiguous()
        best = torch.randn(S, generator=gen, dtype=torch.float64).to(dev)
        for log in (False, True):
            st = run(dict(
                sobo_fwd=lambda: ops.sobo_scan(Y3, q, best, spec3, log=log),
                sobo_fwd_bwd=lambda: ops.sobo_scan(Y3, q, best, spec3, log=log, backward=True)), args)
            out["scan"].append(dict(b=b, m=3, constraints=2, log=log, **st))
            st = run(dict(
                nei_fwd=lambda: ops.nei_scan(Y1, q, best, -1.0, 0.3, log=log),
                sobo_fwd=lambda: ops.sobo_scan(Y1.unsqueeze(1), q, best, spec1, log=log),
                nei_fwd_bwd=lambda: ops.nei_scan(Y1, q, best, -1.0, 0.3, log=log, backward=True),
                sobo_fwd_bwd=lambda: ops.sobo_scan(Y1.unsqueeze(1), q, best, spec1, log=log, backward=True)), args)
            a0, d0 = ops.nei_scan(Y1, q, best, -1.0, 0.3, log=log, backward=True)
            a1, d1 = ops.sobo_scan(Y1.unsqueeze(1), q, best, spec1, log=log, backward=True)
            out["degenerate"].append(dict(b=b, log=log, bitwise_equal=bool(torch.equal(a0, a1) and
                                                                           torch.equal(d0, d1.reshape_as(d0))), **st))
    n, d = 512, 6
    X, Y, gp = make_gp(n, d, 2, 0, dev)
    spec2 = ops.SoboSpec(2, [(0, ops.OBJ_AFFINE, 1.0, -1.0, 0.0, 0.0)], [(1, 1.0, float(np.median(Y[:, 1])), 0.25)])
    acqf = QSoboLogNEI(gp, X, X, spec2, S=S, sampler_seed=7, prune_baseline=True, prune_seed=3)
    Xc = torch.as_tensor(np.random.default_rng(1).uniform(size=(20, 1, d)), device=dev)
    st = run(dict(qsobo_fwd=lambda: acqf.forward(Xc), qsobo_fwd_bwd=lambda: acqf.forward_backward(Xc)), args)
    out["chain"] = dict(b=20, n=n, d=d, m=2, n_base=int(acqf.nb), **st)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
