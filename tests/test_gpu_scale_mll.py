"""GPU: the MLL of the scaled kernel k = sigma^2 k_base (value and full gradient of MLL / n with
the hyperpriors, x = [noise, constant, raw lengthscales, raw sigma^2]) and its fit.

* Value and gradient against CPU torch autograd over ``oracle.gp.kernel_matrix``
  (tests/scale_kernel_reference.mll_value: oracle.gp.mll_value restated with sigma^2), with a Gamma
  and a LogNormal prior on sigma^2 and with none; through the op chain (MLLEvaluator, MLLBatch
  without the plan) and through the plan, shared inputs and member form.  Bars (tests/
  test_gpu_mll_chain.py): value 1e-9 max(1, |ref|), gradient rtol 1e-7 / atol 1e-9; plan against op
  chain 1e-10 max(1, |.|).  Sizes: gp_kernel_reference.MLL_PLAN_CASES.  One case has
  sigma^2 = 1e-3 noise, where (r.alpha - n - noise (sum alpha^2 - tr K^-1)) / sigma^2 would lose
  digits: the sigma^2 gradient comes from the direct sum.
* Fit: the native lock-step rounds against the Python loop (bitwise, tests/test_gpu_fit.py); the
  loss at the device optimum against scipy L-BFGS-B on the CPU restatement from the same start
  (n = 40, d = 2; slack 10 x the distance of two CPU fits from starts 1e-8 apart, floor 1e-9, the
  method of tests/test_gpu_dot_gp.py); the data are y = 5 f(x), standardised by hand to unit
  scale times 5, so sigma^2 must come out above 1.
"""
import math

import numpy as np
import pytest
import torch

from oracle import gp as ogp
from tests import gp_kernel_reference as ref
from tests import scale_kernel_reference as sref

pytestmark = pytest.mark.gpu
NOISE_PRIOR = ("lognormal", -4.0, 1.0)
OS_PRIORS = {"gamma": ("gamma", 2.0, 0.15), "lognormal": ("lognormal", 0.3, 0.8), "none": None}
WORST = {}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _lsp(d):
    return ("lognormal",) + tuple(ogp.dim_scaled_lognormal(d))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"max error  {k}: value {WORST[k][0]:.3e} (of 1e-9), gradient {WORST[k][1]:.3e} (of 1)")


def _check(label, got, want):
    (v, g), (rv, rg) = got, want
    ev = abs(v - rv) / max(1.0, abs(rv))
    eg = float((np.abs(g - rg) / (1e-9 + 1e-7 * np.abs(rg))).max())
    w = WORST.get(label, (0.0, 0.0))
    WORST[label] = (max(w[0], ev), max(w[1], eg))
    print(f"{label}: value error {ev:.3e} (bar 1e-9), gradient error / bar {eg:.3e}")
    assert ev <= 1e-9, (v, rv)
    assert g.shape == rg.shape and np.allclose(g, rg, rtol=1e-7, atol=1e-9), (g, rg)


def _oracle(X, y, x, d, kind, osp):
    return sref.mll_value_and_grad(X, y, x, d, kind, _lsp(d), NOISE_PRIOR, osp)


def _spy(ev, monkeypatch):
    taken, plan = [], ev._eval_plan

    def spy(*a):
        out = plan(*a)
        taken.append(out is not None)
        return out

    monkeypatch.setattr(ev, "_eval_plan", spy)
    return taken


CASES = [(n, d, kind, tuple(OS_PRIORS)[(i + kind) % 3]) for i, (n, d) in enumerate(ref.MLL_PLAN_CASES)
         for kind in ref.MLL_PLAN_KINDS]


def test_cases_cover_the_priors():
    assert {c[3] for c in CASES} == set(OS_PRIORS)
    for n, d in ref.MLL_PLAN_CASES:
        assert {c[3] for c in CASES if c[:2] == (n, d)} == set(OS_PRIORS)


@pytest.mark.parametrize("n,d,kind,prior", CASES)
def test_scaled_mll_matches_autograd(n, d, kind, prior, monkeypatch):
    """Shared inputs: MLLEvaluator (op chain), MLLBatch through the plan and without it."""
    from everest_amd.gp import MLLBatch, MLLEvaluator

    B = 3
    osp = OS_PRIORS[prior]
    X, Ys, xs = sref.scaled_case(n, d, B)
    want = [_oracle(X, Ys[b], xs[b], d, kind, osp) for b in range(B)]
    b0 = (n + kind) % 3
    one = MLLEvaluator(_t(X), Ys[b0], kind, _lsp(d), NOISE_PRIOR, outputscale_prior=osp, scaled=True)
    _check(f"MLLEvaluator scaled d={d}", one(xs[b0]), want[b0])
    ev = MLLBatch(_t(X), Ys, kind, _lsp(d), NOISE_PRIOR, outputscale_prior=osp, scaled=True)
    assert ev.use_plan and ev.scaled and ev.nx == d + 3
    taken = _spy(ev, monkeypatch)
    chain = MLLBatch(_t(X), Ys, kind, _lsp(d), NOISE_PRIOR, outputscale_prior=osp, scaled=True)
    chain.use_plan = False
    for idx in ([0, 1, 2], [1], [2, 0]):
        got = ev(idx, [xs[b] for b in idx])
        assert taken and taken[-1], "the plan handed the evaluation to the op-by-op chain"
        via = chain(idx, [xs[b] for b in idx])
        for k, b in enumerate(idx):
            assert got[k] is not None and via[k] is not None
            _check(f"MLLBatch scaled plan n={n} d={d}", got[k], want[b])
            _check(f"MLLBatch scaled chain n={n} d={d}", via[k], want[b])
            assert abs(got[k][0] - via[k][0]) <= 1e-10 * max(1.0, abs(via[k][0]))
            assert np.all(np.abs(got[k][1] - via[k][1]) <= 1e-10 * np.maximum(1.0, np.abs(via[k][1])))
    # a second evaluation of the plan is bitwise the first
    a, b = ev([0, 1, 2], list(xs)), ev([0, 1, 2], list(xs))
    assert all(p[0] == q[0] and np.array_equal(p[1], q[1]) for p, q in zip(a, b))


@pytest.mark.parametrize("n,d", ref.MLL_PLAN_CASES)
def test_scaled_member_mll_matches_autograd(n, d, monkeypatch):
    """Member form: each member against autograd on its own rows, plan and op chain; member 0 has
    no padding.  Three padded rows would move gos / 2 by -1.5 if the padding entered."""
    from everest_amd.gp import MLLBatch

    B = 3
    X, Ys, xs = sref.scaled_case(n, d, B)
    pads = (0, 3, min(7, n - 2))
    rows = [np.arange(n), np.r_[np.arange(4), np.arange(7, n)], np.arange(pads[2], n)]
    nvalid = np.array([len(r) for r in rows], dtype=np.int32)
    assert list(n - nvalid) == list(pads)
    Xb, Yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b, r in enumerate(rows):
        Xb[b, :len(r)], Yb[b, :len(r)] = X[r], Ys[b, r]
    for kind, prior in ((0, "gamma"), (3, "lognormal"), (2 if d in (8, 17) else 1, "none")):
        osp = OS_PRIORS[prior]
        ev = MLLBatch(_t(Xb), Yb, kind, _lsp(d), NOISE_PRIOR, nvalid=nvalid, outputscale_prior=osp, scaled=True)
        taken = _spy(ev, monkeypatch)
        chain = MLLBatch(_t(Xb), Yb, kind, _lsp(d), NOISE_PRIOR, nvalid=nvalid, outputscale_prior=osp, scaled=True)
        chain.use_plan = False
        want = [_oracle(X[r], Ys[b, r], xs[b], d, kind, osp) for b, r in enumerate(rows)]
        for idx in ([0, 1, 2], [2, 0]):
            got = ev(idx, [xs[b] for b in idx])
            assert taken and taken[-1], "the plan handed the evaluation to the op-by-op chain"
            via = chain(idx, [xs[b] for b in idx])
            for k, b in enumerate(idx):
                _check(f"member scaled plan n={n} d={d} pad={pads[b]}", got[k], want[b])
                _check(f"member scaled chain n={n} d={d} pad={pads[b]}", via[k], want[b])
                assert abs(got[k][0] - via[k][0]) <= 1e-10 * max(1.0, abs(via[k][0]))
                assert np.all(np.abs(got[k][1] - via[k][1]) <= 1e-10 * np.maximum(1.0, np.abs(via[k][1])))


@pytest.mark.parametrize("kind", [0, 3])
def test_outputscale_far_below_the_noise(kind, monkeypatch):
    """sigma^2 = 1e-3 noise (the optimiser visits such points): plan and chain against autograd."""
    from everest_amd.gp import MLLBatch

    n, d, B = 97, 8, 3
    X, Ys, xs = sref.scaled_case(n, d, B)
    xs[:, 2 + d] = ref.inv_softplus(1e-3 * xs[:, 0])
    assert np.allclose(np.logaddexp(0.0, xs[:, 2 + d]), 1e-3 * xs[:, 0], rtol=1e-12)
    osp = OS_PRIORS["gamma"]
    want = [_oracle(X, Ys[b], xs[b], d, kind, osp) for b in range(B)]
    ev = MLLBatch(_t(X), Ys, kind, _lsp(d), NOISE_PRIOR, outputscale_prior=osp)
    taken = _spy(ev, monkeypatch)
    got = ev([0, 1, 2], list(xs))
    assert taken == [True]
    chain = MLLBatch(_t(X), Ys, kind, _lsp(d), NOISE_PRIOR, outputscale_prior=osp)
    chain.use_plan = False
    via = chain([0, 1, 2], list(xs))
    for b in range(B):
        print(f"sigma^2 = {np.logaddexp(0.0, xs[b, 2 + d]):.3e}: d/d raw sigma^2 device {got[b][1][-1]:.12e} "
              f"autograd {want[b][1][-1]:.12e}")
        _check(f"scaled plan sigma^2 << noise kind={kind}", got[b], want[b])
        _check(f"scaled chain sigma^2 << noise kind={kind}", via[b], want[b])
        # the sigma^2 entry on its own, relatively: the five-term identity would not hold this
        assert abs(got[b][1][-1] - want[b][1][-1]) <= 1e-7 * abs(want[b][1][-1]) + 1e-9


# ---------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------
def _fit_data(n, d, m, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    F = np.stack([np.sin(3.0 * X[:, 0] + 0.7 * j) + (X ** 2).sum(1) * (0.5 + 0.2 * j) for j in range(m)], 1)
    F = (F - F.mean(0)) / F.std(0, ddof=1)
    return X, 5.0 * F + 0.05 * rng.normal(size=(n, m))           # y = 5 f(x): unit-scale f


@pytest.mark.parametrize("dup", [False, True])
def test_native_scaled_fit_rounds_match_python_loop(dup, monkeypatch):
    """test_gpu_fit.test_native_fit_rounds_match_python_loop over a scaled plan: bitwise."""
    from everest_amd.gp import LAST_FIT_STATS, fit_batch

    X, Y = _fit_data(90, 4, 3, 21)
    if dup:
        X[60:75] = X[:15]
        Y[60:75] = Y[:15]
    prior = (math.sqrt(2) + 0.5 * math.log(4), math.sqrt(3))
    out, counts = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("EVR_FIT_NATIVE", mode)
        out[mode] = fit_batch(_t(X), Y, 3, prior, (-4.0, 1.0), outputscale_prior=("gamma", 2.0, 0.15))
        counts[mode] = (LAST_FIT_STATS.get("driver"), LAST_FIT_STATS.get("nfev"))
    assert counts["1"][0] == "native" and counts["0"][0] == "python"
    assert counts["1"][1] == counts["0"][1], counts
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a.lengthscale, b.lengthscale), (a.lengthscale, b.lengthscale)
        assert a.noise == b.noise and a.constant == b.constant
        assert a.outputscale is not None and a.outputscale == b.outputscale


def _cpu_fit(X, y, d, kind, lsp, nzp, osp, x0):
    from scipy.optimize import minimize

    def f(x):
        v, g = sref.mll_value_and_grad(X, y, x, d, kind, lsp, nzp, osp)
        return -v, -g

    return minimize(f, x0, jac=True, method="L-BFGS-B", bounds=[(1e-4, None)] + [(None, None)] * (d + 2)).x


@pytest.mark.parametrize("driver", ["fit_single", "fit_batch"])
def test_scaled_fit_reaches_the_cpu_optimum(driver):
    from everest_amd.gp import fit_batch, fit_single, noise_start

    n, d, kind = 40, 2, 3
    X, Y = _fit_data(n, d, 1, 5)
    y = Y[:, 0]                                                   # not standardised again: scale 5
    lsp, nzp, osp = ("gamma", 3.0, 6.0), ("gamma", 1.1, 0.05), ("gamma", 2.0, 0.15)
    if driver == "fit_single":
        h = fit_single(_t(X), y, kind, lsp, nzp, standardize=False, outputscale_prior=osp)
    else:
        (h,) = fit_batch(_t(X), y[:, None], kind, lsp, nzp, standardize=False, outputscale_prior=osp)
    assert h.y_mean == 0.0 and h.y_std == 1.0 and h.outputscale is not None
    x_dev = np.r_[h.noise, h.constant, ref.inv_softplus(h.lengthscale), ref.inv_softplus(h.outputscale)]
    start = np.r_[noise_start(nzp), 0.0, np.zeros(d + 1)]
    x_a = _cpu_fit(X, y, d, kind, lsp, nzp, osp, start)
    x_b = _cpu_fit(X, y, d, kind, lsp, nzp, osp, start + 1e-8)
    nll = lambda x: -sref.mll_value_and_grad(X, y, x, d, kind, lsp, nzp, osp)[0]  # noqa: E731
    l_dev, l_a, l_b = nll(x_dev), nll(x_a), nll(x_b)
    slack = max(10 * abs(l_a - l_b), 1e-9)
    print(f"scaled fit {driver}: loss device {l_dev:.12f}, CPU {l_a:.12f} / {l_b:.12f}; |device - CPU| = "
          f"{abs(l_dev - l_a):.3e}, slack {slack:.3e}; sigma^2 device {h.outputscale:.6f}, CPU "
          f"{np.logaddexp(0.0, x_a[-1]):.6f}; x device {x_dev.tolist()}, x CPU {x_a.tolist()}")
    assert h.outputscale > 1.0, "y = 5 f(x) needs an outputscale above 1"
    assert abs(l_dev - l_a) <= slack


def test_unscaled_fit_keeps_its_layout():
    """Without the flag nothing of the scaled form runs: d + 2 entries, no outputscale."""
    from everest_amd.gp import MLLBatch, fit_batch

    X, Y = _fit_data(40, 2, 2, 7)
    ev = MLLBatch(_t(X), (Y / 5.0).T.copy(), 0, None, (-4.0, 1.0))
    assert not ev.scaled and ev.nx == 4 and ev.prior_spec().shape == (6,)
    hs = fit_batch(_t(X), Y, 0, None, (-4.0, 1.0))
    assert all(h.outputscale is None for h in hs)
