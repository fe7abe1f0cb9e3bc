"""Single-objective acquisition timing on the MI355X: one forward + backward of the joint qEI
integrand through evr_qnei_eval (plain mode, scalar incumbent, no H^T rows: QLogEI(log=False))
against QEIJoint's general chain (evr_qng_eval at m = 1: subset expansion + HVI scan +
combine; its graph-captured q = 1 plan is reported beside it), at identical (n = 512, d = 6,
S = 512) states and base samples, and the log mode (QLogEI).  The paths alternate inside one process; each round times a window of ``--calls``
evaluations between device events; reported per evaluation: median over the rounds and the
spread (interquartile range, min .. max).  Pass: the new path's median does not exceed the
parent path's median by more than the parent's interquartile range.  Prints one JSON line.

    python tools/bench_nei.py [--rounds 15] [--calls 20] [--warmup 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from everest_amd.acquisition import QEIJoint, QLogEI
from everest_amd.gp import GPBatch, GPHyper, standardize_params


def make_gp(n, d, seed, dev):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X).sum(1) + 0.5 * ((X - 0.4) ** 2).sum(1) + 0.01 * rng.normal(size=n)
    ym, ys = standardize_params(y)
    hyp = GPHyper(lengthscale=rng.uniform(0.4, 1.2, d), noise=1e-3, constant=0.0, y_mean=ym, y_std=ys)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    return X, GPBatch(t(X), t(y[:, None]), [hyp], 3, t(np.zeros(d)), t(np.ones(d)))


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(v):
    v = np.asarray(v)
    q25, q50, q75 = np.percentile(v, [25, 50, 75])
    return dict(median_ms=round(float(q50), 4), iqr_ms=round(float(q75 - q25), 4), min_ms=round(float(v.min()), 4),
                max_ms=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nei needs the MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    n, d, S = 512, 6, 512
    X, gp = make_gp(n, d, 0, dev)
    out = dict(n=n, d=d, S=S, rounds=args.rounds, calls=args.calls, cases=[])
    ok = True
    for b, q in ((20, 1), (20, 3), (512, 1)):
        parent = QEIJoint(gp, X, -1.0, 0.0, S=S, seed=7)
        plain = QLogEI(gp, X, -1.0, 0.0, S=S, seed=7, log=False)
        logm = QLogEI(gp, X, -1.0, 0.0, S=S, seed=7)
        Xc = torch.as_tensor(np.random.default_rng(b + q).uniform(size=(b, q, d)), device=dev)
        # QEIJoint.forward_backward takes the graph-captured q = 1 plan when it applies; the
        # like-for-like reference is its general chain (evr_qng_eval), timed for every case
        paths = dict(parent_qng=lambda: parent._general(Xc, True), nei_plain=lambda: plain.forward_backward(Xc),
                     nei_log=lambda: logm.forward_backward(Xc))
        if q == 1:
            paths["parent_plan_q1"] = lambda: parent.forward_backward(Xc)
        a0, g0 = paths["parent_qng"]()
        a1, g1 = paths["nei_plain"]()
        diff = dict(acq=float((a0 - a1).abs().max()), grad=float((g0 - g1).abs().max()),
                    acq_max=float(a0.abs().max()), grad_max=float(g0.abs().max()))
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(args.rounds):          # alternate the paths round by round
            for k, fn in paths.items():
                times[k].append(window_ms(fn, args.calls))
        st = {k: stats(v) for k, v in times.items()}
        passed = st["nei_plain"]["median_ms"] <= st["parent_qng"]["median_ms"] + st["parent_qng"]["iqr_ms"]
        ok &= passed
        out["cases"].append(dict(b=b, q=q, **st, plain_vs_parent_max_abs_diff=diff, passed=bool(passed)))
    out["passed"] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
