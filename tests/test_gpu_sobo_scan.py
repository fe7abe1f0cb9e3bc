"""The scalarised, output-constrained single-objective scan on the MI355X (evr_sobo_scan,
sobo_scan.hip) alone, against the torch restatement with autograd (tests/sobo_reference.py),
against evr_nei_scan in the degenerate case, and for determinism.

Tolerances are the project's bars for this chain (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10 and gradients rtol 1e-5 / atol 1e-8; log variants 5e-6 absolute in log space
and 1e-3 relative gradients per candidate.  Every candidate is held.

Inputs.  Term sets with an affine term get prescribed improvements u - best = +-10^e, e uniform
in [-9, 3] (test_gpu_nei._scan_inputs): the affine term's output is solved for them after the
other outputs are drawn.  The sigmoid + target set has no free term (its utility is bounded),
so its outputs are drawn so that steepness * (y - tp) spans +-40 and ``best`` lies inside the
utility's range.  Constraint outputs are drawn so that c / eta spans +-40 (with m = 1 the
constraints read the solved output, eta = 25 puts +-1e3 at +-40).  All values are continuous
random numbers: arg-max ties have probability zero."""
import numpy as np
import pytest
import torch

from everest_amd import ops
from tests import sobo_reference as sr

pytestmark = pytest.mark.gpu

TERM_SETS = {
    # name: m -> [(out, kind, w, p0, p1, p2)]
    "affine": {1: [(0, sr.AFFINE, 1.0, -1.0, 0.3, 0.0)], 3: [(0, sr.AFFINE, 1.0, -1.0, 0.3, 0.0)]},
    "affine_ctt": {3: [(0, sr.AFFINE, 0.3, -1.0, 0.3, 0.0), (1, sr.CLOSE_TO_TARGET, 1.0, 0.4, 2.0, 0.0)]},
    "sig_tgt": {1: [(0, sr.SIGMOID, 1.0, -2.0, 0.1, 0.0), (0, sr.TARGET, 0.5, 1.5, -0.2, 3.0)],
                3: [(0, sr.SIGMOID, 1.0, -2.0, 0.1, 0.0), (1, sr.TARGET, 0.5, 1.5, -0.2, 3.0),
                    (1, sr.SIGMOID, 0.7, 3.0, 0.5, 0.0)]},
}


def _constraints(m, n):
    """0, 1, or 3 constraints (two on one output, as a TargetObjective gives)."""
    eta = 25.0 if m == 1 else 0.5
    o1, o2 = min(1, m - 1), m - 1
    return {0: [], 1: [(o1, 1.0, 0.2, eta)],
            3: [(o1, -1.0, -1.0, eta), (o1, 1.0, 1.5, eta), (o2, -1.0, 0.1, 2.0 * eta)]}[n]


def _inputs(S, b, q, m, terms, cons, seed):
    """Y (S x b x q x m, numpy) and the S per-sample incumbents."""
    rng = np.random.default_rng(seed)
    Y = np.empty((S, b, q, m))
    for j in range(m):
        # c / eta of the constraints on j spans about +-40; sigmoid / target arguments likewise
        etas = [c[3] for c in cons if c[0] == j]
        span = 40.0 * min(etas) if etas else 15.0
        Y[..., j] = rng.uniform(-span, span, size=(S, b, q))
    if terms[0][1] != sr.AFFINE:
        Y[..., 0] = rng.uniform(-15.0, 15.0, size=(S, b, q))
        lo, hi = 0.0, sum(t[2] for t in terms)
        return Y, torch.tensor(rng.uniform(lo + 0.05 * hi, 0.8 * hi, size=S))
    best = torch.tensor(rng.normal(size=S))
    imp = rng.choice([-1.0, 1.0], size=(S, b, q)) * 10.0 ** rng.uniform(-9.0, 3.0, size=(S, b, q))
    imp[0, 0, 0], imp[S - 1, b - 1, q - 1] = -1e3, 1e3
    return (Y, imp), best


def _solve_affine(Yimp, best, terms):
    """Output 0 such that u - best = imp (the first term is affine on output 0, alone there)."""
    Y, imp = Yimp
    _, _, w, a, c, _ = terms[0]
    assert all(t[0] != 0 for t in terms[1:])
    rest = sr.Utility(terms[1:])(torch.tensor(Y)).numpy() if len(terms) > 1 else 0.0
    Y = Y.copy()
    Y[..., 0] = ((imp + best.reshape(-1, 1, 1).numpy() - rest) / w - c) / a
    return Y


def _dev_layout(Y):
    """S x b x q x m -> the kernel's S x m x (b*q)."""
    S, b, q, m = Y.shape
    return Y.permute(0, 3, 1, 2).reshape(S, m, b * q).contiguous()


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("q", [1, 2, 4])
@pytest.mark.parametrize("S", [8, 24, 64])
def test_sobo_scan_matches_restatement(S, q, m, log):
    worst = dict(v=0.0, g=0.0)
    for b in (1, 3, 17, 65):
        for ncon in (0, 1, 3):
            cons = _constraints(m, ncon)
            for tname, by_m in TERM_SETS.items():
                if m not in by_m:
                    continue
                terms = by_m[m]
                raw, best_s = _inputs(S, b, q, m, terms, cons, 100000 * S + 1000 * b + 100 * q + 10 * m + ncon)
                spec = ops.SoboSpec(m, terms, cons)
                util, oc = sr.Utility(terms), sr.constraints_of(cons)
                used = {t[0] for t in terms} | {c[0] for c in cons}
                for scalar, with_gout in ((False, False), (True, True), (False, True), (True, False)):
                    best = best_s[:1].clone() if scalar else best_s
                    Y = torch.tensor(raw if terms[0][1] != sr.AFFINE else _solve_affine(raw, best, terms))
                    gout = torch.tensor(np.random.default_rng(b).uniform(0.5, 2.0, size=b)) if with_gout else None
                    y = Y.clone().requires_grad_(True)
                    ref = sr.scan(y, util, oc, best, log)
                    (ref if gout is None else ref * gout).sum().backward()
                    flags = torch.zeros(m, b, dtype=torch.int32)
                    flags[m - 1, b // 2] = 1
                    kw = dict(log=log, tau_relu=sr.TAU_RELU, tau_max=sr.TAU_MAX, flags=flags.cuda())
                    Yd = _dev_layout(Y).cuda()
                    acq, dY = ops.sobo_scan(Yd, q, best.cuda(), spec, gout=None if gout is None else gout.cuda(),
                                            backward=True, **kw)
                    fwd, none = ops.sobo_scan(Yd, q, best.cuda(), spec, **kw)
                    acq, fwd = acq.cpu(), fwd.cpu()
                    dY = dY.cpu().reshape(S, m, b, q).permute(0, 2, 3, 1)          # S x b x q x m
                    ok = flags.sum(0) == 0
                    tag = (b, ncon, tname, scalar, with_gout)
                    assert none is None and torch.isnan(acq[~ok]).all() and torch.isfinite(acq[ok]).all(), tag
                    assert torch.equal(fwd[ok], acq[ok]), tag        # forward-only kernel: the same values
                    assert torch.isfinite(dY).all(), tag
                    for j in set(range(m)) - used:                   # outputs nothing reads: exact zeros
                        assert (dY[..., j] == 0.0).all(), tag
                    r, gr = ref.detach(), y.grad
                    if log:
                        ev = (acq[ok] - r[ok]).abs().max().item() if ok.any() else 0.0
                        eg = ((dY - gr).abs().amax((0, 2, 3)) /
                              gr.abs().amax((0, 2, 3)).clamp_min(1e-300)).max().item()
                        worst["v"], worst["g"] = max(worst["v"], ev), max(worst["g"], eg)
                        assert ev <= 5e-6, (tag, ev)
                        assert eg <= 1e-3, (tag, eg)
                    else:
                        if ok.any():
                            worst["v"] = max(worst["v"], ((acq[ok] - r[ok]).abs() /
                                                          r[ok].abs().clamp_min(1e-300)).max().item())
                        worst["g"] = max(worst["g"], (dY - gr).abs().max().item())
                        assert torch.allclose(acq[ok], r[ok], rtol=1e-6, atol=1e-10), tag
                        assert torch.allclose(dY, gr, rtol=1e-5, atol=1e-8), tag
    print(f"sobo_scan S={S} q={q} m={m} log={log}: worst value error {worst['v']:.3e}, "
          f"gradient error {worst['g']:.3e}")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("q", [1, 2, 4])
def test_degenerate_case_equals_nei_scan_bitwise(q, log):
    """m = 1, one affine term with w = 1, no constraints: 0.0 + 1.0 g, a + 0.0 and x * 1.0 are
    exact and the reduction tree is nei_scan's, so acq and dY are the same bits."""
    oa, ob = -1.0, 0.3
    terms = [(0, sr.AFFINE, 1.0, oa, ob, 0.0)]
    spec = ops.SoboSpec(1, terms)
    for S in (8, 24, 64):
        for b in (1, 3, 17, 65):
            raw, best_s = _inputs(S, b, q, 1, terms, [], 7 * S + b + q)
            for best in (best_s, best_s[:1].clone()):
                Y = torch.tensor(_solve_affine(raw, best, terms))
                gout = torch.tensor(np.random.default_rng(b).uniform(0.5, 2.0, size=b)).cuda()
                Yd = _dev_layout(Y).cuda()
                flags = torch.zeros(1, b, dtype=torch.int32)
                flags[0, b // 2] = 1
                kw = dict(log=log, tau_relu=sr.TAU_RELU, tau_max=sr.TAU_MAX, gout=gout, backward=True)
                a1, d1 = ops.sobo_scan(Yd, q, best.cuda(), spec, flags=flags.cuda(), **kw)
                a2, d2 = ops.nei_scan(Yd.reshape(S, b * q), q, best.cuda(), oa, ob, flags=flags[0].cuda(), **kw)
                ok = (flags[0] == 0).cuda()
                assert torch.equal(a1[ok], a2[ok]) and torch.isnan(a1[~ok]).all() and torch.isnan(a2[~ok]).all()
                assert torch.equal(d1.reshape(S, b * q), d2), (S, b, best.numel())


def test_sobo_scan_is_bitwise_reproducible():
    S, b, q, m = 24, 65, 4, 3
    terms, cons = TERM_SETS["affine_ctt"][3], _constraints(3, 3)
    raw, best = _inputs(S, b, q, m, terms, cons, 5)
    Yd = _dev_layout(torch.tensor(_solve_affine(raw, best, terms))).cuda()
    spec = ops.SoboSpec(m, terms, cons)
    for log in (False, True):
        a1, d1 = ops.sobo_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        a2, d2 = ops.sobo_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        assert torch.equal(a1, a2) and torch.equal(d1, d2), log


def test_sobo_scan_refuses_bad_tables():
    Y = torch.zeros(8, 2, 3, device="cuda", dtype=torch.float64)
    best = torch.zeros(8, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.SoboSpec(2, [(2, sr.AFFINE, 1.0, 1.0, 0.0, 0.0)])
    with pytest.raises(ValueError):
        ops.SoboSpec(2, [(0, 7, 1.0, 1.0, 0.0, 0.0)])
    spec = ops.SoboSpec(2, [(0, sr.AFFINE, 1.0, 1.0, 0.0, 0.0)], [(1, 1.0, 0.0, 1.0)])
    spec._carrs[3][0] = 0.0                                # eta = 0 must be refused by the library
    with pytest.raises(RuntimeError):
        ops.sobo_scan(Y, 1, best, spec)
    with pytest.raises(ValueError):
        ops.sobo_scan(Y, 2, best, ops.SoboSpec(2, [(0, sr.AFFINE, 1.0, 1.0, 0.0, 0.0)]))


def test_general_chain_keeps_refusing_the_new_kinds():
    """evr_qng_eval / evr_qlog_eval / evr_objective_* share one table check: the sigmoid and
    target kinds exist for the scan only."""
    Y = torch.zeros(2, 5, device="cuda", dtype=torch.float64)
    for kind in (ops.OBJ_SIGMOID, ops.OBJ_TARGET):
        with pytest.raises(RuntimeError, match="objective kind"):
            ops.objective_weights(Y, ops.GeneralSpec(2, [(0, kind, 1.0, 0.0)]))
