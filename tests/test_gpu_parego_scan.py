"""The augmented Chebyshev scan on the MI355X (evr_parego_scan, parego_scan.hip) alone, against
the torch restatement with autograd (tests/sobo_reference.scan with tests/parego_reference.
Chebyshev), against evr_sobo_scan where one term is the arg-min everywhere, and for determinism.

Tolerances are the project's bars for this chain (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10 and gradients rtol 1e-5 / atol 1e-8; log variants 5e-6 absolute in log space
and 1e-3 relative gradients per candidate.  Every candidate is held.

Inputs.  Improvements are prescribed as in test_gpu_sobo_scan: u - best = +-10^e, e uniform in
[-9, 3].  Term 0 is affine on output 0 and alone there; u is continuous, strictly increasing and
piecewise linear in t_0 (slope 1 + alpha while t_0 is the minimum, alpha above), so output 0 is
solved in closed form after the other outputs are drawn: the branch t_0 <= min_{k>0} t_k first,
else the other one.  Constraint outputs are drawn so that c / eta spans +-40.  All values are
continuous random numbers: arg-min and arg-max ties have probability zero (the exact tie has a
test of its own)."""
import numpy as np
import pytest
import torch

from everest_amd import ops
from tests import parego_reference as pr
from tests import sobo_reference as sr
from tests.test_gpu_sobo_scan import _constraints, _dev_layout

pytestmark = pytest.mark.gpu

ALPHA = 0.05
A, C = sr.AFFINE, sr.CLOSE_TO_TARGET
# name -> the model sizes it runs at and [(out, kind, p0, p1, A, B)]
TERM_SETS = {
    "two_affine": ((2, 3, 8), [(0, A, -1.0, 0.3, 0.6, 0.1), (1, A, 0.7, -0.2, 0.25, 0.4)]),
    # affine + close-to-target; at m = 3 output 2 is read by nothing (unless a constraint does)
    "affine_ctt": ((2, 3, 8), [(0, A, 1.5, 0.3, 0.3, -0.2), (1, C, 0.4, 2.0, 0.02, 1.0)]),
    # eight terms on eight outputs: the limit
    "eight": ((8,), [(0, A, -1.0, 0.3, 0.6, 0.1)] + [(k, A if k % 3 else C, 0.3 * k - 1.0 if k % 3 else 0.4,
                                                      0.1 * k if k % 3 else 2.0, 0.1 + 0.05 * k, 0.2 * k - 0.5)
                                                     for k in range(1, 8)]),
}


def _inputs(S, b, q, m, cons, seed):
    """Outputs 1.. (S x b x q x m, output 0 still to solve), the prescribed improvements and S
    per-sample incumbents."""
    rng = np.random.default_rng(seed)
    Y = np.empty((S, b, q, m))
    for j in range(m):
        etas = [c[3] for c in cons if c[0] == j]
        span = 40.0 * min(etas) if etas else 15.0
        Y[..., j] = rng.uniform(-span, span, size=(S, b, q))
    best = torch.tensor(rng.normal(size=S))
    imp = rng.choice([-1.0, 1.0], size=(S, b, q)) * 10.0 ** rng.uniform(-9.0, 3.0, size=(S, b, q))
    imp[0, 0, 0], imp[S - 1, b - 1, q - 1] = -1e3, 1e3
    return (Y, imp), best


def _solve(Yimp, best, terms, alpha=ALPHA):
    """Output 0 such that u - best = imp."""
    Y, imp = Yimp
    _, kind, a, c, A0, B0 = terms[0]
    assert kind == sr.AFFINE and all(t[0] != 0 for t in terms[1:])
    rest = pr.Chebyshev(terms[1:], alpha).term_values(torch.tensor(Y)).numpy()
    rmin, rsum = rest.min(-1), rest.sum(-1)
    U = imp + best.reshape(-1, 1, 1).numpy()
    t0 = (U - alpha * rsum) / (1.0 + alpha)                 # t_0 is the minimum
    t0 = np.where(t0 <= rmin, t0, (U - rmin - alpha * rsum) / alpha)
    Y = Y.copy()
    Y[..., 0] = ((t0 - B0) / A0 - c) / a
    return Y


def _compare(S, b, q, m, terms, cons, log, seed, variants, worst):
    raw, best_s = _inputs(S, b, q, m, cons, seed)
    spec = ops.ParegoSpec(m, terms, ALPHA, cons)
    util, oc = pr.Chebyshev(terms, ALPHA), sr.constraints_of(cons)
    used = {t[0] for t in terms} | {c[0] for c in cons}
    for scalar, with_gout in variants:
        best = best_s[:1].clone() if scalar else best_s
        Y = torch.tensor(_solve(raw, best, terms))
        gout = torch.tensor(np.random.default_rng(b).uniform(0.5, 2.0, size=b)) if with_gout else None
        y = Y.clone().requires_grad_(True)
        ref = sr.scan(y, util, oc, best, log)
        (ref if gout is None else ref * gout).sum().backward()
        flags = torch.zeros(m, b, dtype=torch.int32)
        flags[m - 1, b // 2] = 1                                   # one flagged candidate
        kw = dict(log=log, tau_relu=sr.TAU_RELU, tau_max=sr.TAU_MAX, flags=flags.cuda())
        Yd = _dev_layout(Y).cuda()
        acq, dY = ops.parego_scan(Yd, q, best.cuda(), spec, gout=None if gout is None else gout.cuda(),
                                  backward=True, **kw)
        fwd, none = ops.parego_scan(Yd, q, best.cuda(), spec, **kw)
        acq, fwd = acq.cpu(), fwd.cpu()
        dY = dY.cpu().reshape(S, m, b, q).permute(0, 2, 3, 1)      # S x b x q x m
        ok = flags.sum(0) == 0
        tag = (b, len(cons), len(terms), scalar, with_gout)
        assert none is None and torch.isnan(acq[~ok]).all() and torch.isfinite(acq[ok]).all(), tag
        assert torch.equal(fwd[ok], acq[ok]), tag                  # forward-only kernel: the same bits
        assert torch.isfinite(dY).all(), tag
        for j in set(range(m)) - used:                             # outputs nothing reads: exact zeros
            assert (dY[..., j] == 0.0).all(), tag
        r, gr = ref.detach(), y.grad
        if log:
            ev = (acq[ok] - r[ok]).abs().max().item() if ok.any() else 0.0
            eg = ((dY - gr).abs().amax((0, 2, 3)) / gr.abs().amax((0, 2, 3)).clamp_min(1e-300)).max().item()
            worst["v"], worst["g"] = max(worst["v"], ev), max(worst["g"], eg)
            assert ev <= 5e-6, (tag, ev)
            assert eg <= 1e-3, (tag, eg)
        else:
            if ok.any():
                worst["v"] = max(worst["v"], ((acq[ok] - r[ok]).abs() / r[ok].abs().clamp_min(1e-300)).max().item())
            worst["g"] = max(worst["g"], (dY - gr).abs().max().item())
            assert torch.allclose(acq[ok], r[ok], rtol=1e-6, atol=1e-10), tag
            assert torch.allclose(dY, gr, rtol=1e-5, atol=1e-8), tag


ALL_VARIANTS = ((False, False), (True, True), (False, True), (True, False))     # (scalar best, gout)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("q", [1, 2, 4])
@pytest.mark.parametrize("S", [8, 24, 64])
def test_parego_scan_matches_restatement(S, q, m, log):
    worst = dict(v=0.0, g=0.0)
    for b in (1, 3, 17, 65):
        for ncon in (0, 1, 3):
            cons = _constraints(m, ncon)
            for tname, (sizes, terms) in TERM_SETS.items():
                if m not in sizes:
                    continue
                _compare(S, b, q, m, terms, cons, log, 100000 * S + 1000 * b + 100 * q + 10 * m + ncon, ALL_VARIANTS,
                         worst)
    print(f"parego_scan S={S} q={q} m={m} log={log}: worst value error {worst['v']:.3e}, "
          f"gradient error {worst['g']:.3e}")


@pytest.mark.parametrize("log", [False, True])
def test_parego_scan_q12(log):
    """The widest instantiation (the one a by-value table copy to scratch would show in)."""
    worst = dict(v=0.0, g=0.0)
    for m, tname, ncon in ((3, "affine_ctt", 3), (8, "eight", 1)):
        _compare(24, 17, 12, m, TERM_SETS[tname][1], _constraints(m, ncon), log, 12 + m, ALL_VARIANTS[:2], worst)
    print(f"parego_scan q=12 log={log}: worst value error {worst['v']:.3e}, gradient error {worst['g']:.3e}")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("k0", [0, 2])
def test_matches_sobo_scan_where_one_term_is_the_minimum(k0, log):
    """With term k0 the arg-min everywhere, u = (1 + alpha) t_k0 + alpha sum_{k != k0} t_k is a sum:
    evr_sobo_scan with weights alpha A_k, a second copy of term k0 with weight A_k0 and
    best - (1 + alpha) B_k0 - alpha sum_{k != k0} B_k computes the same acquisition."""
    S, b, q, m = 24, 17, 3, 3
    rng = np.random.default_rng(31 + k0)
    terms = [(0, A, -1.0, 0.3, 0.6, 0.1), (1, A, 0.7, -0.2, 0.25, 0.4), (2, C, 0.4, 2.0, 0.02, 1.0)]
    o, kind, p0, p1, Ak, _ = terms[k0]
    terms[k0] = (o, kind, p0, p1, Ak, -1e3)                        # far below every other term
    cons = _constraints(m, 1)
    Y = torch.tensor(rng.uniform(-15.0, 15.0, size=(S, b, q, m)))
    cheb = pr.Chebyshev(terms, ALPHA)
    tv = cheb.term_values(Y)
    assert bool((tv.argmin(-1) == k0).all())
    u = cheb(Y)
    # a good part of the points improve; 0.41 * (b q - 1) = 20.5: the incumbent lies half way between
    # two utilities, never on one (a zero improvement would leave its sign to the rounding)
    best = torch.quantile(u.reshape(S, -1), 0.41, dim=1)
    Bs = [t[5] for t in terms]
    shift = (1.0 + ALPHA) * Bs[k0] + ALPHA * sum(B for k, B in enumerate(Bs) if k != k0)
    sterms = [(o, kd, ALPHA * Ak, p0, p1, 0.0) for o, kd, p0, p1, Ak, _ in terms] + [(o, kind, Ak, p0, p1, 0.0)]
    gout = torch.tensor(rng.uniform(0.5, 2.0, size=b)).cuda()
    Yd = _dev_layout(Y).cuda()
    kw = dict(log=log, tau_relu=sr.TAU_RELU, tau_max=sr.TAU_MAX, gout=gout, backward=True)
    a1, d1 = ops.parego_scan(Yd, q, best.cuda(), ops.ParegoSpec(m, terms, ALPHA, cons), **kw)
    a2, d2 = ops.sobo_scan(Yd, q, (best - shift).cuda(), ops.SoboSpec(m, sterms, cons), **kw)
    a1, d1, a2, d2 = a1.cpu(), d1.cpu(), a2.cpu(), d2.cpu()
    assert torch.isfinite(a1).all() and (log or bool((a1 > 0).all()))
    if log:
        ev = (a1 - a2).abs().max().item()
        eg = ((d1 - d2).abs().reshape(S, m, b, q).amax((0, 1, 3)) /
              d2.abs().reshape(S, m, b, q).amax((0, 1, 3)).clamp_min(1e-300)).max().item()
        print(f"parego vs sobo scan k0={k0} log: value {ev:.3e}, gradient {eg:.3e}")
        assert ev <= 5e-6 and eg <= 1e-3
    else:
        print(f"parego vs sobo scan k0={k0} plain: value {(a1 - a2).abs().max():.3e}, "
              f"gradient {(d1 - d2).abs().max():.3e}")
        assert torch.allclose(a1, a2, rtol=1e-6, atol=1e-10)
        assert torch.allclose(d1, d2, rtol=1e-5, atol=1e-8)


def test_exact_tie_flows_through_the_first_term():
    """t_0 == t_1 exactly (powers of two): dY follows the lowest term index."""
    S, b = 8, 3
    spec = ops.ParegoSpec(3, [(2, A, 2.0, 0.0, 0.25, 0.25), (0, A, 1.0, 0.0, 0.5, 0.25), (1, A, 1.0, 0.0, 1.0, 0.0)],
                          0.125)
    Y = torch.tensor([1.0, 4.0, 1.0]).double().reshape(1, 3, 1).repeat(S, 1, b).contiguous().cuda()   # t = (.75, .75, 4)
    best = torch.full((S,), -1.0, dtype=torch.float64).cuda()
    acq, dY = ops.parego_scan(Y, 1, best, spec, backward=True)
    u = 0.75 + 0.125 * 5.5
    assert torch.equal(acq.cpu(), torch.full((b,), u + 1.0, dtype=torch.float64))
    want = torch.tensor([0.125 * 0.5 * 1.0, 0.125 * 1.0 * 1.0, 1.125 * 0.25 * 2.0]).double() / S   # outputs 0, 1, 2
    assert torch.equal(dY.cpu(), want.reshape(1, 3, 1).expand(S, 3, b))


def test_parego_scan_is_bitwise_reproducible():
    S, b, q, m = 24, 65, 4, 3
    terms, cons = TERM_SETS["affine_ctt"][1], _constraints(3, 3)
    raw, best = _inputs(S, b, q, m, cons, 5)
    Yd = _dev_layout(torch.tensor(_solve(raw, best, terms))).cuda()
    spec = ops.ParegoSpec(m, terms, ALPHA, cons)
    for log in (False, True):
        a1, d1 = ops.parego_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        a2, d2 = ops.parego_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        assert torch.equal(a1, a2) and torch.equal(d1, d2), log


def test_parego_scan_refuses_bad_tables():
    """The library's own checks (the spec's host checks are bypassed by editing its arrays)."""
    Y = torch.zeros(8, 2, 3, device="cuda", dtype=torch.float64)
    best = torch.zeros(8, device="cuda", dtype=torch.float64)
    two = [(0, A, 1.0, 0.0, 1.0, 0.0), (1, A, 1.0, 0.0, 1.0, 0.0)]

    def spec():
        return ops.ParegoSpec(2, two, ALPHA, [(1, 1.0, 0.0, 1.0)])

    ops.parego_scan(Y, 1, best, spec())                    # the unedited table runs
    one = spec()
    one.terms = one.terms[:1]                              # one term
    with pytest.raises(RuntimeError):
        ops.parego_scan(Y, 1, best, one)
    sig = spec()
    sig._tarrs[1][1] = ops.OBJ_SIGMOID                     # a sigmoid kind
    with pytest.raises(RuntimeError, match="kind"):
        ops.parego_scan(Y, 1, best, sig)
    for bad in (0.0, -1.0):                                # A <= 0
        neg = spec()
        neg._tarrs[4][0] = bad
        with pytest.raises(RuntimeError, match="scale"):
            ops.parego_scan(Y, 1, best, neg)
    eta = spec()
    eta._carrs[3][0] = 0.0                                 # eta = 0
    with pytest.raises(RuntimeError):
        ops.parego_scan(Y, 1, best, eta)
    al = spec()
    al.alpha = -0.1
    with pytest.raises(RuntimeError, match="alpha"):
        ops.parego_scan(Y, 1, best, al)
    out = spec()
    out._tarrs[0][1] = 2                                   # an output index outside the model
    with pytest.raises(RuntimeError):
        ops.parego_scan(Y, 1, best, out)
    with pytest.raises(ValueError):
        ops.parego_scan(Y, 2, best, spec())                # 3 columns are no multiple of q = 2
