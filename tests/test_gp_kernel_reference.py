"""CPU: the plain reference of the GP gradient kernels (tests/gp_kernel_reference.py) checked
before the GPU tests trust it — against float64 torch autograd through the oracle's kernel
matrix, against 40-digit mpmath, and the MLL-chain inputs' conditioning (what keeps the oracle's
own float64 error, about cond * 1e-16, two orders inside the bars of tests/test_gpu_mll_chain.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import gp as ogp
from tests import gp_kernel_reference as ref

KINDS = [0, 1, 2, 3, "mixed"]
MIXED = [0, 3, 1, 2, 3]


def _kinds(kind, B):
    return MIXED[:B] if kind == "mixed" else [kind] * B


def _inputs(n1, n2, d, B, seed, dup=True):
    rng = np.random.default_rng(seed)
    X1 = rng.uniform(-1, 2, (n1, d))
    X2 = rng.uniform(-1, 2, (n2, d))
    if dup:
        k = min(3, n1, n2)
        X2[:k] = X1[n1 - k:]                     # exact duplicates: the Matern clamp kills the gradient
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    G = rng.normal(size=(B, n1, n2))
    os_ = rng.uniform(0.5, 2.0, B)
    return X1, X2, ls, G, os_


@pytest.mark.parametrize("norm", ["none", "side2", "both"])
@pytest.mark.parametrize("n1,n2,d", [(1, 1, 1), (7, 5, 6), (40, 23, 17), (40, 23, 1), (12, 23, 6)])
@pytest.mark.parametrize("kind", KINDS)
def test_cross_grad_matches_autograd(kind, n1, n2, d, norm):
    B = 5 if kind == "mixed" else 2
    kinds = _kinds(kind, B)
    X1, X2, ls, G, os_ = _inputs(n1, n2, d, B, 7 * n1 + n2 + d)
    use_os = norm != "side2"
    shift, scale = -np.ones(d), np.full(d, 1.0 / 3.0)
    s1 = (shift, scale) if norm == "both" else (None, None)
    s2 = (shift, scale) if norm != "none" else (None, None)
    if norm == "side2":                            # X1 already normalised, as the product calls it
        X1 = (X1 - shift) * scale
    got, S = ref.cross_grad(X1, X2, ls, G, kinds, *s1, *s2, os_ if use_os else None)
    x2 = torch.tensor(X2, requires_grad=True)
    u1 = torch.tensor(X1) if s1[0] is None else (torch.tensor(X1) - torch.tensor(shift)) * torch.tensor(scale)
    u2 = x2 if s2[0] is None else (x2 - torch.tensor(shift)) * torch.tensor(scale)
    tot = 0.0
    for b in range(B):
        K = ogp.kernel_matrix(u1, u2, torch.tensor(ls[b]), kinds[b], os_[b] if use_os else 1.0)
        tot = tot + (torch.tensor(G[b]) * K).sum()
    tot.backward()
    err = np.abs(got.astype(np.float64) - x2.grad.numpy())
    assert np.all(err <= 1e-12 * S.astype(np.float64)), (err / np.maximum(S.astype(np.float64), 1e-300)).max()
    if kind in (1, 2, 3) and n1 == 1 and n2 == 1:  # the single pair is a duplicate: gradient exactly 0
        assert np.all(got == 0)


@pytest.mark.parametrize("n,d", [(1, 1), (9, 6), (40, 17), (23, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_lengthscale_grad_matches_autograd(kind, n, d):
    B = 5 if kind == "mixed" else 2
    kinds = _kinds(kind, B)
    rng = np.random.default_rng(n + 10 * d)
    X = rng.uniform(-1, 2, (n, d))
    if n >= 9:
        X[n - 2:] = X[:2]
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    W = rng.normal(size=(B, n, n))                 # not symmetric
    got, S = ref.lengthscale_grad(X, ls, W, kinds)
    lt = torch.tensor(ls, requires_grad=True)
    tot = 0.0
    for b in range(B):
        tot = tot + (torch.tensor(W[b]) * ogp.kernel_matrix(torch.tensor(X), torch.tensor(X), lt[b], kinds[b])).sum()
    tot.backward()
    err = np.abs(got.astype(np.float64) - lt.grad.numpy())
    assert np.all(err <= 1e-12 * S.astype(np.float64))


def _mp_kernel(mp, kind, d2):
    if kind == 0:
        return mp.exp(-d2 / 2)
    r = mp.sqrt(max(d2, mp.mpf("1e-30")))
    if kind == 1:
        return mp.exp(-r)
    if kind == 2:
        return (1 + mp.sqrt(3) * r) * mp.exp(-mp.sqrt(3) * r)
    return (1 + mp.sqrt(5) * r + mp.mpf(5) / 3 * d2) * mp.exp(-mp.sqrt(5) * r)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_reference_matches_mpmath(kind):
    """One 5 x 4, d = 3 case per family at 40 digits: the gradients by mpmath's own numerical
    differentiation of the kernel VALUE (mp.diff), so that no derivative formula is shared."""
    import mpmath as mp
    mp.mp.dps = 40
    n1, n2, d = 5, 4, 3
    X1, X2, ls, G, os_ = _inputs(n1, n2, d, 1, 99 + kind, dup=False)
    shift, scale = -np.ones(d), np.full(d, 1.0 / 3.0)
    got, S = ref.cross_grad(X1, X2, ls, G, [kind], shift, scale, shift, scale, os_)
    M = lambda a: [[mp.mpf(float(v)) for v in row] for row in a]  # noqa: E731
    x1, x2, l, sh, sc = M(X1), M(X2), [mp.mpf(float(v)) for v in ls[0]], mp.mpf(-1), mp.mpf(float(scale[0]))

    def kval(i, c, k, xck, lk=None):
        d2 = mp.mpf(0)
        for q in range(d):
            a = (x1[i][q] - sh) * sc
            b = ((xck if q == k else x2[c][q]) - sh) * sc
            lq = lk if (lk is not None and q == k) else l[q]
            d2 += ((b - a) / lq) ** 2
        return mp.mpf(float(os_[0])) * _mp_kernel(mp, kind, d2)

    for c in range(n2):
        for k in range(d):
            want = sum(mp.mpf(float(G[0, i, c])) * mp.diff(lambda t, i=i: kval(i, c, k, t), x2[c][k])
                       for i in range(n1))
            assert abs(mp.mpf(float(got[c, k])) - want) <= mp.mpf("1e-14") * mp.mpf(float(S[c, k])), (c, k)

    # lengthscale gradient on X1 (5 rows), W non-symmetric
    W = np.random.default_rng(5 + kind).normal(size=(1, n1, n1))
    g, Sg = ref.lengthscale_grad(X1, ls, W, [kind])

    def kls(i, j, k, lk):
        d2 = mp.mpf(0)
        for q in range(d):
            d2 += ((x1[j][q] - x1[i][q]) / (lk if q == k else l[q])) ** 2
        return _mp_kernel(mp, kind, d2)

    for k in range(d):
        want = sum(mp.mpf(float(W[0, i, j])) * mp.diff(lambda t, i=i, j=j: kls(i, j, k, t), l[k])
                   for i in range(n1) for j in range(n1) if i != j)
        assert abs(mp.mpf(float(g[0, k])) - want) <= mp.mpf("1e-14") * mp.mpf(float(Sg[0, k])), k


def test_mll_terms_and_finalize_reference():
    """The two small references against float64 numpy on well-scaled inputs."""
    rng = np.random.default_rng(3)
    B, n, nt = 2, 7, 5
    L = np.tril(rng.normal(size=(B, n, n)) * 0.1) + np.eye(n) * rng.uniform(0.5, 2.0, (B, n, 1))
    Linv = np.linalg.inv(L)
    r, a = rng.normal(size=(B, n)), rng.normal(size=(B, n))
    out, S = ref.mll_terms(L, Linv, r, a)
    want = np.stack([2 * np.log(np.einsum("bii->bi", L)).sum(1), (r * a).sum(1), (Linv ** 2).sum((1, 2)), a.sum(1),
                     (a * a).sum(1)], 1)
    assert np.allclose(out.astype(np.float64), want, rtol=1e-13, atol=1e-13)
    assert np.all(S >= np.abs(out))
    R = rng.normal(size=(B, n + 1, nt)) * 0.2
    c, ym, ys, kxx, nz = rng.normal(size=B), rng.normal(size=B), rng.uniform(0.5, 2, B), np.ones(B), np.array([.1, .2])
    mean, var, ss = ref.posterior_finalize(R, c, ym, ys, kxx, nz)
    assert np.allclose(mean.astype(np.float64), ym[:, None] + ys[:, None] * (c[:, None] + R[:, n]), rtol=1e-14)
    assert np.allclose(var.astype(np.float64), ys[:, None] ** 2 * (1 - (R[:, :n] ** 2).sum(1) + nz[:, None]),
                       rtol=1e-13, atol=1e-14)
    _, var0, _ = ref.posterior_finalize(R, c, ym, ys, kxx)
    assert np.allclose((var - var0).astype(np.float64), (ys ** 2 * nz)[:, None], rtol=1e-13)


def _mll_inputs():
    cases = [(n, d, 3, k) for n, d, kinds in ref.MLL_CHAIN_CASES for k in kinds]
    cases += [(n, d, 3, k) for n, d in ref.MLL_PLAN_CASES for k in ref.MLL_PLAN_KINDS]
    n, d, B = ref.MLL_MANY
    return list(dict.fromkeys(cases + [(n, d, B, 0)]))     # (97, 8) and (129, 17) are in both lists


@pytest.mark.parametrize("n,d,B,kind", _mll_inputs())
def test_mll_inputs_are_well_conditioned(n, d, B, kind):
    """A condition on the inputs of tests/test_gpu_mll_chain.py, not a measurement: the plain
    Cholesky of K + noise I succeeds and cond <= 1e6 for every member."""
    X, Ys, xs = ref.mll_case(n, d, B)
    assert Ys.shape == (B, n) and np.allclose(Ys.mean(1), 0, atol=1e-12) and np.allclose(Ys.std(1, ddof=1), 1)
    for b in range(B):
        ls = np.logaddexp(0.0, xs[b, 2:])
        assert np.all(ls >= 0.3 * math.sqrt(d) * (1 - 1e-12)) and np.all(ls <= 1.2 * math.sqrt(d) * (1 + 1e-12))
        assert xs[b, 0] in ref.NOISES and xs[b, 1] in ref.CONSTANTS
        K = ref.train_matrix(X, ls, xs[b, 0], kind)
        np.linalg.cholesky(K)                       # raises LinAlgError when not p.d.
        assert np.linalg.cond(K) <= 1e6


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_oracle_mll_gradient_central_differences(kind):
    """oracle.gp.mll_value's autograd gradient for the Matern families (tests/test_oracle.py has
    RBF): central differences, step 1e-6, at n = 30, d = 3."""
    X, Ys, xs = ref.mll_case(30, 3, 1)
    Xt, yt = torch.tensor(X), torch.tensor(Ys[0])
    prior = ogp.dim_scaled_lognormal(3)
    x0 = torch.tensor(xs[0], requires_grad=True)
    ogp.mll_value(Xt, yt, x0[2:], x0[0], x0[1], kind, prior).backward()
    h = 1e-6
    for k in range(5):
        e = torch.zeros(5, dtype=torch.float64)
        e[k] = h
        xp, xm = x0.detach() + e, x0.detach() - e
        fp = ogp.mll_value(Xt, yt, xp[2:], xp[0], xp[1], kind, prior).item()
        fm = ogp.mll_value(Xt, yt, xm[2:], xm[0], xm[1], kind, prior).item()
        g = x0.grad[k].item()
        assert abs((fp - fm) / (2 * h) - g) <= 1e-6 * abs(g), (k, (fp - fm) / (2 * h), g)
