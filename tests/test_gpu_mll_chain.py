"""GPU: the whole MLL evaluation (value and gradient of MLL / n with the hyperpriors) against
``oracle.gp.mll_value`` with autograd, float64 on the CPU — the op-by-op chain (MLLEvaluator) at
every lengthscale-gradient and kernel-matrix dispatch (d = 1 .. 64), and the native plan
(evr_mll_plan: one graph launch) at odd and even n (both mll_w_kernel instantiations), n below, at
and above one 32-tile, d >= 16 (kmat_mfma_sym), for index subsets, and at B = 52 outputs.

Bars (those of test_mll_value_and_grad at n = 80): value 1e-9 * max(1, |ref|); gradient
rtol 1e-7, atol 1e-9.  The inputs' conditioning (Cholesky succeeds, cond <= 1e6, so the oracle's own
float64 error is two orders inside these bars) is asserted by tests/test_gp_kernel_reference.py.
"""
import numpy as np
import pytest
import torch

from oracle import gp as ogp
from tests import gp_kernel_reference as ref

pytestmark = pytest.mark.gpu
NOISE_PRIOR = (-4.0, 1.0)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"max error  {k}: value {WORST[k][0]:.3e} (of 1e-9), gradient {WORST[k][1]:.3e} (of 1)")


def _oracle(X, y, x, kind, d):
    t = torch.tensor(x, requires_grad=True)
    v = ogp.mll_value(torch.tensor(X), torch.tensor(y), t[2:], t[0], t[1], kind, ogp.dim_scaled_lognormal(d),
                      NOISE_PRIOR)
    v.backward()
    return v.item(), t.grad.numpy().copy()


def _check(label, got, want):
    (v, g), (rv, rg) = got, want
    ev = abs(v - rv) / max(1.0, abs(rv))
    eg = float((np.abs(g - rg) / (1e-9 + 1e-7 * np.abs(rg))).max())     # <= 1: np.allclose(rtol 1e-7, atol 1e-9)
    w = WORST.get(label, (0.0, 0.0))
    WORST[label] = (max(w[0], ev), max(w[1], eg))
    print(f"{label}: value error {ev:.3e} (bar 1e-9), gradient error / bar {eg:.3e}")
    assert ev <= 1e-9, (v, rv)
    assert np.allclose(g, rg, rtol=1e-7, atol=1e-9), (g, rg)


# the member of the B = 3 inputs cycles over the cases, so that the chain meets every noise and a
# nonzero constant (r = Y - c) against the oracle
@pytest.mark.parametrize("n,d,kind,b", [(n, d, k, i % 3) for i, (n, d, k) in enumerate(
    (n, d, k) for n, d, kinds in ref.MLL_CHAIN_CASES for k in kinds)])
def test_mll_evaluator_matches_oracle(n, d, kind, b):
    from everest_amd.gp import MLLEvaluator

    X, Ys, xs = ref.mll_case(n, d, 3)
    assert xs[b, 0] == ref.NOISES[b] and xs[b, 1] == ref.CONSTANTS[b]
    ev = MLLEvaluator(torch.tensor(X, device="cuda"), Ys[b], kind, ogp.dim_scaled_lognormal(d), NOISE_PRIOR)
    _check(f"MLLEvaluator d={d}", ev(xs[b]), _oracle(X, Ys[b], xs[b], kind, d))


@pytest.mark.parametrize("kind", ref.MLL_PLAN_KINDS)
@pytest.mark.parametrize("n,d", ref.MLL_PLAN_CASES)
def test_mll_plan_matches_oracle(n, d, kind, monkeypatch):
    from everest_amd.gp import MLLBatch

    B = 3
    X, Ys, xs = ref.mll_case(n, d, B)
    ev = MLLBatch(torch.tensor(X, device="cuda"), Ys, kind, ogp.dim_scaled_lognormal(d), NOISE_PRIOR)
    assert ev.use_plan
    taken = []
    plan = ev._eval_plan

    def spy(*a):
        out = plan(*a)
        taken.append(out is not None)
        return out

    monkeypatch.setattr(ev, "_eval_plan", spy)
    want = [_oracle(X, Ys[b], xs[b], kind, d) for b in range(B)]
    for idx in ([0, 1, 2], [1], [2, 0]):
        got = ev(idx, [xs[b] for b in idx])
        # the plan was the path taken: the ladder fallback would pass without running it
        assert taken and taken[-1], "the plan handed the evaluation to the op-by-op chain"
        for k, b in enumerate(idx):
            assert got[k] is not None
            _check(f"MLLBatch plan n={n} d={d}", got[k], want[b])
    assert len(taken) == 3 and all(taken)


def test_mll_plan_many_outputs():
    """B = 52 outputs (5 B = 260 terms: more than one thread each of the 256-thread copy-out
    block): every member's five terms and lengthscale-gradient pieces from the plan equal the
    op-by-op chain's to 1e-10 (relative to max(1, |.|)), its Cholesky info is 0, and member 51
    equals the oracle."""
    from everest_amd.gp import MLLBatch, _softplus_libm

    n, d, B = ref.MLL_MANY
    X, Ys, xs = ref.mll_case(n, d, B)
    prior = ogp.dim_scaled_lognormal(d)
    ev = MLLBatch(torch.tensor(X, device="cuda"), Ys, 0, prior, NOISE_PRIOR)
    idx = list(range(B))
    ls = np.array([[_softplus_libm(v) for v in row] for row in xs[:, 2:]])
    host = ev._eval_plan(idx, ls, xs[:, 0].copy(), xs[:, 1].copy())
    assert host is not None, "the plan handed the evaluation to the op-by-op chain"
    want = ev._eval_ops(idx, ls, xs[:, 0].copy(), xs[:, 1].copy())
    assert host.shape == want.shape == (B * (5 + d + 1),)
    terms, terms_w = host[:5 * B].reshape(B, 5), want[:5 * B].reshape(B, 5)
    gls, gls_w = host[5 * B:5 * B + B * d], want[5 * B:5 * B + B * d]
    assert np.all(want[5 * B + B * d:] == 0) and np.all(host[5 * B + B * d:] == 0)
    close = np.abs(terms - terms_w) <= 1e-10 * np.maximum(1.0, np.abs(terms_w))
    bad = [b for b in range(B) if not close[b].all()]
    assert not bad, f"members {bad}: plan terms {terms[bad[0]]} vs chain {terms_w[bad[0]]}"
    assert np.all(np.abs(gls - gls_w) <= 1e-10 * np.maximum(1.0, np.abs(gls_w)))
    got = ev(idx, list(xs))
    chain = MLLBatch(torch.tensor(X, device="cuda"), Ys, 0, prior, NOISE_PRIOR)
    chain.use_plan = False
    for (v1, g1), (v2, g2) in zip(got, chain(idx, list(xs))):
        assert abs(v1 - v2) <= 1e-10 * max(1.0, abs(v2))
        assert np.all(np.abs(g1 - g2) <= 1e-10 * np.maximum(1.0, np.abs(g2)))
    _check("MLLBatch plan B=52 member 51", got[51], _oracle(X, Ys[51], xs[51], 0, d))
