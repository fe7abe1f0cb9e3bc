"""Timing of the negative integrated posterior variance on the MI355X: one
QNegIntPosVar.forward_backward (kernel assembly, GEMMs, evr_nipv_reduce of nipv.hip,
kernel_cross_grad) and the fused reduction alone, at B = 5 outputs, n = 512 training rows,
N = 512 integration points, d = 6, q = 1, for b = 20 and b = 512 candidates.  Nothing here is a
target.

The paths alternate inside one process, warm; each round times a window of ``--calls`` launches
between device events; reported per launch: the median over ``--rounds`` (>= 20) rounds and the
spread, beside the algorithmic bytes of the reduction (C and Vx read twice — the reduction and the
second walk — dC and dVx written once) and the rate they imply.  Prints one JSON line.

    python tools/bench_nipv.py [--rounds 25] [--calls 20] [--warmup 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from everest_amd import ops
from everest_amd.acquisition import QNegIntPosVar
from everest_amd.gp import GPBatch, GPHyper


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("bench_nipv reports the median of at least 20 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_nipv needs the MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    B, n, N, d, q = 5, 512, 512, 6, 1
    rng = np.random.default_rng(0)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    hyp = [GPHyper(lengthscale=rng.uniform(0.4, 1.2, d), noise=1e-3, constant=0.0, y_mean=0.0, y_std=1.0 + 0.1 * j)
           for j in range(B)]
    gp = GPBatch(t(rng.uniform(size=(n, d))), t(rng.normal(size=(n, B))), hyp, 3, t(np.zeros(d)), t(np.ones(d)))
    acqf = QNegIntPosVar(gp, rng.uniform(size=(N, d)))
    out = dict(B=B, n=n, N=N, d=d, q=q, rounds=args.rounds, calls=args.calls, cases=[])
    for b in (20, 512):
        X = t(rng.uniform(size=(b, q, d)))
        X2 = X.view(b * q, d)
        R = ops.gemm(gp.M, gp.cross(X2))
        C = ops.kernel_matrix(acqf.Pn, X2, gp.ls, gp.kind, shift2=acqf._lo, scale2=acqf._ir)
        C -= torch.matmul(acqf.Vp.transpose(1, 2), R[:, :n])

        def reduce(backward):
            return ops.nipv_reduce(C, R, X, acqf._lo, acqf._ir, gp.ls, gp.kind, gp.noise, acqf.coef, acqf.v0, n=n,
                                   backward=backward)

        st = run(dict(forward=lambda: acqf.forward(X), forward_backward=lambda: acqf.forward_backward(X),
                      reduce_fwd=lambda: reduce(False), reduce_fwd_bwd=lambda: reduce(True)), args)
        words = B * (N + n) * b * q
        by = dict(reduce_fwd=8 * words, reduce_fwd_bwd=8 * 3 * words)      # C, Vx read (twice), dC, dVx written
        case = dict(b=b, bytes=by, **st)
        for k, v in by.items():
            case[k]["GBps"] = round(v / (case[k]["median_us"] * 1e-6) / 1e9, 2)
        out["cases"].append(case)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
