"""The multiplicative / multiplicative-additive scan on the MI355X (evr_mult_scan, mult_scan.hip)
alone, against the torch restatement with autograd (tests/sobo_reference.scan with
tests/mult_reference.Product), at exactly zero factors, at negative bases, for NaN utilities and
for determinism.

Tolerances are the project's bars for this chain (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10 and gradients rtol 1e-5 / atol 1e-8; log variants 5e-6 absolute in log space
and 1e-3 relative gradients per candidate.  Every candidate is held.

Inputs.  Improvements are prescribed as in test_gpu_parego_scan: u - best = +-10^e, e uniform in
[-9, 3].  Term 0 is affine with weight 1 and alone on output 0; u is linear in it (u = g_0 R with
R the product of the other factors times the bracket, or u = 1 + g_0 + the other addends when
there are no factors), so output 0 is solved in closed form after the other outputs are drawn.
The other factors g ** w are kept in [0.05, 3] so that the division by R is well conditioned: a
sigmoid factor's argument in [-0.8, 8], a target factor within one 1 / steepness of its window,
affine and close-to-target factors with |g| in [0.4, 1.4] (the close-to-target one is negative and
carries an even weight).  Addends see the whole range, sigmoid and target arguments within +-40.
All values are continuous random numbers: arg-max ties have probability zero."""
import numpy as np
import pytest
import torch

from everest_amd import ops
from tests import mult_reference as mr
from tests import sobo_reference as sr
from tests.mult_reference import dev_layout

pytestmark = pytest.mark.gpu

A, C, G, T = sr.AFFINE, sr.CLOSE_TO_TARGET, sr.SIGMOID, sr.TARGET
T0 = (0, A, 1.0, -1.25, 0.3, 0.0)          # term 0 of every table: affine, weight 1, alone on output 0
# name -> the model sizes it runs at, factors, addends; rows (out, kind, w, p0, p1, p2)
TABLES = {
    "two_factors": ((2, 3, 8), [T0, (1, G, 2.5, 1.5, 0.2, 0.0)], []),
    # at m = 3 output 2 is read by nothing
    "factor_addend": ((2, 3, 8), [T0], [(1, T, 0.5, 2.0, 0.4, 1.5)]),
    "addends_only": ((2, 3, 8), [], [T0, (1, G, 0.75, -0.8, 0.1, 0.0)]),
    # two terms reading output 1: a factor and an addend
    "same_output": ((2, 3, 8), [T0, (1, G, 2.0, 1.2, -0.3, 0.0)], [(1, T, 0.5, 1.5, 0.0, 2.0)]),
    # eight terms on eight outputs, all four kinds on both sides: the limit
    "eight": ((8,), [T0, (1, G, 2.5, 1.5, 0.2, 0.0), (2, T, 1.5, 2.0, 0.4, 1.5), (3, C, 2.0, 0.4, 1.5, 0.0),
                     (4, A, 3.0, 0.7, 0.1, 0.0)],
              [(5, G, 0.5, -2.0, 0.3, 0.0), (6, A, 0.25, 1.1, -0.2, 0.0), (7, C, 0.125, -0.3, 2.0, 0.0)]),
}


def _draw(rng, shape, term, factor):
    """Model-output values for one term (not term 0): see the module docstring."""
    _, kind, w, p0, p1, p2 = term
    if kind == G:
        x = rng.uniform(-0.8, 8.0, size=shape) if factor else rng.uniform(-40.0, 40.0, size=shape)
        return p1 + x / p0
    if kind == T:
        half = p2 + 1.0 / p0 if factor else 40.0 / p0 - p2
        assert half > 0
        return p1 + rng.uniform(-half, half, size=shape)
    mag = rng.uniform(0.4, 1.4, size=shape) if factor else rng.uniform(0.05, 2.0, size=shape)
    if kind == A:
        g = mag if factor else mag * rng.choice([-1.0, 1.0], size=shape)
        return (g - p1) / p0
    assert not factor or w % 2 == 0                 # a negative base needs an integer weight
    return p0 + rng.choice([-1.0, 1.0], size=shape) * mag ** (1.0 / p1)


def _inputs(S, b, q, m, factors, addends, seed):
    """Outputs 1.. (S x b x q x m, output 0 still to solve), the prescribed improvements and S
    per-sample incumbents."""
    rng = np.random.default_rng(seed)
    Y = rng.uniform(-15.0, 15.0, size=(S, b, q, m))
    first = {}
    for t, fac in [(t, True) for t in factors] + [(t, False) for t in addends]:
        if t is T0:
            continue
        assert t[0] != 0
        if t[0] not in first:                       # a shared output is drawn for its first reader
            first[t[0]] = (t, fac)
            Y[..., t[0]] = _draw(rng, (S, b, q), t, fac)
    best = torch.tensor(rng.normal(size=S))
    imp = rng.choice([-1.0, 1.0], size=(S, b, q)) * 10.0 ** rng.uniform(-9.0, 3.0, size=(S, b, q))
    imp[0, 0, 0], imp[S - 1, b - 1, q - 1] = -1e3, 1e3
    return (Y, imp), best


def _solve(Yimp, best, factors, addends):
    """Output 0 such that u - best = imp."""
    Y, imp = Yimp
    U = imp + best.reshape(-1, 1, 1).numpy()
    Yt = torch.tensor(Y)
    if factors:
        assert factors[0] is T0
        R = mr.Product(factors[1:], addends)(Yt).numpy()
        assert (np.abs(R) > 1e-6).all()
        g0 = U / R
    else:
        assert addends[0] is T0
        g0 = U - mr.Product([], addends[1:])(Yt).numpy()          # u = 1 + g_0 + the rest
    Y = Y.copy()
    Y[..., 0] = (g0 - T0[4]) / T0[3]
    return Y


def _check(Y, q, best, factors, addends, log, gout=None, flags=None, skip=(), worst=None, tag=None):
    """Device scan (backward and forward-only launch) against sr.scan with autograd on
    Y (S x b x q x m).  A flag only turns acq into NaN: the flagged candidate's dY is compared like
    every other.  skip: candidates with a NaN utility, whose acq must be NaN and whose dY is
    unspecified."""
    S, b, _, m = Y.shape
    spec, util = ops.MultSpec(m, factors, addends), mr.Product(factors, addends)
    used = {t[0] for t in list(factors) + list(addends)}
    y = Y.clone().requires_grad_(True)
    ref = sr.scan(y, util, None, best, log)
    held = torch.ones(b, dtype=torch.bool)                         # candidates whose dY is compared
    for c in skip:
        held[c] = False
    ok = held.clone()                                              # candidates whose acq is a number
    if flags is not None:
        ok &= flags.sum(0) == 0
    (ref if gout is None else ref * gout)[held].sum().backward()
    kw = dict(log=log, tau_relu=sr.TAU_RELU, tau_max=sr.TAU_MAX, flags=None if flags is None else flags.cuda())
    Yd = dev_layout(Y).cuda()
    acq, dY = ops.mult_scan(Yd, q, best.cuda(), spec, gout=None if gout is None else gout.cuda(), backward=True, **kw)
    fwd, none = ops.mult_scan(Yd, q, best.cuda(), spec, **kw)
    acq, fwd = acq.cpu(), fwd.cpu()
    dY = dY.cpu().reshape(S, m, b, q).permute(0, 2, 3, 1)          # S x b x q x m
    assert none is None and torch.isnan(acq[~ok]).all() and torch.isfinite(acq[ok]).all(), tag
    assert torch.isnan(fwd[~ok]).all() and torch.equal(fwd[ok], acq[ok]), tag    # forward-only: the same bits
    dY, gr = dY[:, held], y.grad[:, held]
    assert torch.isfinite(dY).all(), tag
    for j in set(range(m)) - used:                                 # outputs nothing reads: exact zeros
        assert (dY[..., j] == 0.0).all(), tag
    r = ref.detach()
    if log:
        ev = (acq[ok] - r[ok]).abs().max().item() if ok.any() else 0.0
        eg = ((dY - gr).abs().amax((0, 2, 3)) / gr.abs().amax((0, 2, 3)).clamp_min(1e-300)).max().item()
    else:
        ev = ((acq[ok] - r[ok]).abs() / r[ok].abs().clamp_min(1e-300)).max().item() if ok.any() else 0.0
        eg = (dY - gr).abs().max().item()
    if worst is not None:
        worst["v"], worst["g"] = max(worst["v"], ev), max(worst["g"], eg)
    if log:
        assert ev <= 5e-6, (tag, ev)
        assert eg <= 1e-3, (tag, eg)
    else:
        assert torch.allclose(acq[ok], r[ok], rtol=1e-6, atol=1e-10), (tag, ev)
        assert torch.allclose(dY, gr, rtol=1e-5, atol=1e-8), (tag, eg)
    return acq, dY


ALL_VARIANTS = ((False, False), (True, True), (False, True), (True, False))     # (scalar best, gout)


def _compare(S, b, q, m, factors, addends, log, seed, variants, worst):
    raw, best_s = _inputs(S, b, q, m, factors, addends, seed)
    for scalar, with_gout in variants:
        best = best_s[:1].clone() if scalar else best_s
        Y = torch.tensor(_solve(raw, best, factors, addends))
        gout = torch.tensor(np.random.default_rng(b).uniform(0.5, 2.0, size=b)) if with_gout else None
        flags = torch.zeros(m, b, dtype=torch.int32)
        if b > 1:
            flags[m - 1, b // 2] = 1                               # one flagged candidate; b = 1 keeps its value
        _check(Y, q, best, factors, addends, log, gout, flags, worst=worst,
               tag=(b, len(factors), len(addends), scalar, with_gout))


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("q", [1, 2, 4])
@pytest.mark.parametrize("S", [8, 24, 64])
def test_mult_scan_matches_restatement(S, q, m, log):
    worst = dict(v=0.0, g=0.0)
    for b in (1, 3, 17, 65):
        for i, (sizes, factors, addends) in enumerate(TABLES.values()):
            if m in sizes:
                _compare(S, b, q, m, factors, addends, log, 100000 * S + 1000 * b + 100 * q + 10 * m + i,
                         ALL_VARIANTS, worst)
    print(f"mult_scan S={S} q={q} m={m} log={log}: worst value error {worst['v']:.3e}, "
          f"gradient error {worst['g']:.3e}")


@pytest.mark.parametrize("log", [False, True])
def test_mult_scan_q12(log):
    """The widest instantiation (the one a by-value table copy to scratch would show in)."""
    worst = dict(v=0.0, g=0.0)
    for m, name in ((3, "same_output"), (8, "eight")):
        _, factors, addends = TABLES[name]
        _compare(24, 17, 12, m, factors, addends, log, 12 + m, ALL_VARIANTS[:2], worst)
    print(f"mult_scan q=12 log={log}: worst value error {worst['v']:.3e}, gradient error {worst['g']:.3e}")


ZERO_FACTORS = [(0, A, 1.0, 2.0, -1.0, 0.0), (1, A, 2.0, 1.0, 0.0, 0.0)]   # (2 y0 - 1) ** 1 * y1 ** 2
ZERO_ADDENDS = [(2, A, 0.5, 1.0, 0.0, 0.0)]                                # 1 + 0.5 y2


def test_exact_zero_factor_known_slopes():
    """0 ** 1 * 3 ** 2 * (1 + 0.5 * 3) = 0: the slope with respect to the zero factor is the product
    of the others, 9 * 2.5 = 22.5, and every other slope is exactly 0."""
    S, b = 8, 3
    Y = torch.tensor([0.5, 3.0, 3.0]).double().reshape(1, 3, 1).repeat(S, 1, b).contiguous().cuda()
    best = torch.full((S,), -1.0, dtype=torch.float64).cuda()
    acq, dY = ops.mult_scan(Y, 1, best, ops.MultSpec(3, ZERO_FACTORS, ZERO_ADDENDS), backward=True)
    assert torch.equal(acq.cpu(), torch.full((b,), 1.0, dtype=torch.float64))
    dY = dY.cpu()
    want = torch.full((S, b), 22.5 * 2.0 / S, dtype=torch.float64)             # d g_0 / d y_0 = 2
    assert torch.allclose(dY[:, 0], want, rtol=1e-14, atol=0.0)                # 3 ** 2 goes through pow
    assert bool((dY[:, 1:] == 0.0).all())


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("q", [1, 2])
def test_exact_zero_factors_match_autograd(q, log):
    """Exactly zero factors of weight 1 (slope: the rest) and of weight 2 (slope 0, and 0 for the
    rest) in some (sample, point)s; a * y + c == 0.0 exactly at y = 0.5 and at y = 0."""
    S, b, m = 8, 5, 3
    rng = np.random.default_rng(77 + q)
    Y = rng.uniform(0.5, 2.0, size=(S, b, q, m))
    Y[::2, 1, 0, 0] = 0.5                          # the weight-1 factor is zero ...
    Y[::2, 1, 1:, 0] = 0.25                        # ... and the best point: the others have u < 0
    Y[1::2, 2, q - 1, 1] = 0.0                     # the weight-2 factor is zero
    Y[:, 3, :, 0], Y[:, 3, :, 1] = 0.5, 0.0        # both, everywhere
    Yt = torch.tensor(Y)
    assert bool((sr.Utility.term(A, 2.0, -1.0, 0.0, Yt[::2, 1, 0, 0]) == 0.0).all())
    best = torch.tensor(rng.uniform(-1.0, -0.5, size=S))          # u = 0 improves
    _, dY = _check(Yt, q, best, ZERO_FACTORS, ZERO_ADDENDS, log, tag=("zero", q, log))
    assert bool((dY[::2, 1, 0, 0] != 0.0).any())                  # the zero factor itself has a slope
    assert bool((dY[1::2, 2, q - 1] == 0.0).all()) and bool((dY[:, 3] == 0.0).all())


@pytest.mark.parametrize("log", [False, True])
def test_negative_base_integer_weight(log):
    """(-g) ** 3 is real: finite, and it matches."""
    S, b, q, m = 24, 17, 2, 2
    rng = np.random.default_rng(3)
    Y = torch.tensor(rng.uniform(-2.0, 2.0, size=(S, b, q, m)))
    factors = [(0, A, 1.0, 0.8, 0.1, 0.0), (1, A, 3.0, 1.0, 0.0, 0.0)]
    assert bool((Y[..., 1] < 0).any())
    best = torch.quantile(mr.Product(factors)(Y).reshape(S, -1), 0.41, dim=1)
    _check(Y, q, best, factors, [], log, tag=("neg3", log))
    assert float(mr.Product([(0, A, 3.0, 1.0, 0.0, 0.0)])(torch.tensor([[-2.0]]).double())) == -8.0


@pytest.mark.parametrize("log", [False, True])
def test_nan_utility_marks_its_candidate_only(log):
    """A negative base with weight 1.5 in one sample of one candidate: that acq is NaN (the plain
    maximum's comparisons would drop it), all others are finite and match."""
    S, b, q, m = 24, 17, 2, 2
    rng = np.random.default_rng(4)
    Y = rng.uniform(0.2, 2.0, size=(S, b, q, m))
    Y[5, 11, 1, 1] = -2.0
    Y = torch.tensor(Y)
    factors = [(0, A, 1.0, 0.8, 0.1, 0.0), (1, A, 1.5, 1.0, 0.0, 0.0)]
    u = mr.Product(factors)(Y)
    assert int(torch.isnan(u).sum()) == 1 and bool(torch.isnan(u[5, 11, 1]))
    best = torch.quantile(torch.nan_to_num(u, nan=1.0).reshape(S, -1), 0.41, dim=1)
    acq, _ = _check(Y, q, best, factors, [], log, skip=(11,), tag=("nan", log))
    assert bool(torch.isnan(acq[11])) and int(torch.isnan(acq).sum()) == 1


def test_mult_scan_is_bitwise_reproducible():
    S, b, q, m = 24, 65, 4, 8
    _, factors, addends = TABLES["eight"]
    raw, best = _inputs(S, b, q, m, factors, addends, 5)
    Yd = dev_layout(torch.tensor(_solve(raw, best, factors, addends))).cuda()
    spec = ops.MultSpec(m, factors, addends)
    for log in (False, True):
        a1, d1 = ops.mult_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        a2, d2 = ops.mult_scan(Yd, q, best.cuda(), spec, log=log, backward=True)
        assert torch.equal(a1, a2) and torch.equal(d1, d2), log


def test_mult_scan_refuses_bad_tables():
    """The library's own checks (the spec's host checks are bypassed by editing its arrays)."""
    Y = torch.zeros(8, 2, 3, device="cuda", dtype=torch.float64)
    best = torch.zeros(8, device="cuda", dtype=torch.float64)

    def spec():
        return ops.MultSpec(2, [(0, A, 1.0, 1.0, 0.0, 0.0)], [(1, A, 0.5, 1.0, 0.0, 0.0)])

    ops.mult_scan(Y, 1, best, spec())                      # the unedited table runs
    none = spec()
    none.factors, none.addends = [], []                    # no term at all
    with pytest.raises(RuntimeError, match="sizes"):
        ops.mult_scan(Y, 1, best, none)
    many = spec()
    many.factors = many.factors * 8                        # nine terms
    with pytest.raises(RuntimeError, match="sizes"):
        ops.mult_scan(Y, 1, best, many)
    kind = spec()
    kind._aarrs[1][0] = 7                                  # an unknown kind
    with pytest.raises(RuntimeError, match="kind"):
        ops.mult_scan(Y, 1, best, kind)
    for bad in (0.5, float("nan"), float("inf")):          # a factor's weight below 1 or not finite
        w = spec()
        w._farrs[2][0] = bad
        with pytest.raises(RuntimeError, match="weight"):
            ops.mult_scan(Y, 1, best, w)
    w = spec()
    w._aarrs[2][0] = float("inf")                          # an addend's weight not finite
    with pytest.raises(RuntimeError, match="weight"):
        ops.mult_scan(Y, 1, best, w)
    w = spec()
    w._aarrs[2][0] = -0.5                                  # ... but any finite one passes
    ops.mult_scan(Y, 1, best, w)
    out = spec()
    out._farrs[0][0] = 2                                   # an output index outside the model
    with pytest.raises(RuntimeError, match="output"):
        ops.mult_scan(Y, 1, best, out)
    with pytest.raises(RuntimeError, match="tau"):
        ops.mult_scan(Y, 1, best, spec(), log=True, tau_relu=0.0)
    with pytest.raises(ValueError):
        ops.mult_scan(Y, 2, best, spec())                  # 3 columns are no multiple of q = 2
