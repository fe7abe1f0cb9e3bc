"""CPU: the long-double restatement of the dot-product GP (tests/dot_kernel_reference.py) checked
against two independent derivations, so that the GPU tests can lean on it.

* Ridge identity: a GP with k = v <x, x'> and noise s2 is Bayesian linear regression with weights
  ~ N(0, v I), so the n x n posterior equals the d x d ridge formulas
      mean = c + x*^T (X^T X + (s2 / v) I)^-1 X^T (y - c),   var = s2 x*^T (X^T X + (s2 / v) I)^-1 x*
  (push-through identity).  Held to 1e-15 relative in long double: n = 12, d = 3, s2 = 0.05 keep
  k(x, x) / var near 50, so the subtraction in the n x n form loses about two of the 19 digits.
* Gradient: loss_grad equals central differences of loss in long double, step 1e-6, to 1e-9
  relative.  The points keep the noise at 0.2 and above: the truncation term h^2 f''' / 6 is about
  1e-12 / noise^2 of the noise derivative, three orders inside the bar; the rounding term
  eps |f| / h is 1e-13.
"""
import numpy as np
import pytest

from tests import dot_kernel_reference as ref

LD = ref.LD


@pytest.mark.parametrize("v,s2,const", [(np.log(2.0), 0.05, 0.0), (1.7, 0.05, 0.3), (0.4, 0.2, -0.6)])
def test_linear_posterior_is_ridge_regression(v, s2, const):
    n, d = 12, 3
    Xn, y = ref.train_case(n, d, seed=1)
    Xt = np.random.default_rng(3).uniform(-0.3, 1.3, size=(7, d))
    mean, var, kxx = ref.posterior(Xn, y, Xt, 0, v, s2, const, 0.0, 1.0, False, LD)
    X, xs = Xn.astype(LD), Xt.astype(LD)
    A = X.T @ X + (LD(s2) / LD(v)) * np.eye(d, dtype=LD)
    La = ref.cholesky(A)
    solve = lambda b: ref.solve_lower_t(La, ref.solve_lower(La, b))  # noqa: E731
    want_mean = LD(const) + xs @ solve(X.T @ (y.astype(LD) - LD(const)))
    want_var = LD(s2) * (xs * solve(xs.T).T).sum(1)
    r_mean = float(np.max(np.abs(mean - want_mean) / np.abs(want_mean)))
    r_var = float(np.max(np.abs(var - want_var) / np.abs(want_var)))
    print(f"ridge identity v={v:.3g} s2={s2}: mean {r_mean:.2e}, var {r_var:.2e} (bar 1e-15); "
          f"k(x,x)/var up to {float(np.max(kxx / var)):.1f}")
    assert r_mean <= 1e-15 and r_var <= 1e-15
    # with observation noise the variance gains exactly s2
    _, var_n, _ = ref.posterior(Xn, y, Xt, 0, v, s2, const, 0.0, 1.0, True, LD)
    assert float(np.max(np.abs(var_n - (want_var + LD(s2))) / np.abs(var_n))) <= 1e-15


@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("power", [0, 1, 2, 4])
def test_loss_gradient_matches_central_differences(power, priors):
    n, d = 12, 3
    Xn, y = ref.train_case(n, d, seed=2)
    thp = ("gamma", 2.0, 0.5) if priors else None
    nzp = ("gamma", 1.1, 0.05) if priors else None
    h = LD(1e-6)
    for x in (np.array([0.2, 0.3, 0.0]), np.array([0.5, -0.4, 1.1]), np.array([1.5, 0.2, -0.8])):
        g = ref.loss_grad(x, Xn, y, power, thp, nzp, LD)
        for i in range(3):
            xp, xm = x.astype(LD), x.astype(LD)
            xp[i] += h
            xm[i] -= h
            fd = (ref.loss(xp, Xn, y, power, thp, nzp, LD) - ref.loss(xm, Xn, y, power, thp, nzp, LD)) / (2 * h)
            r = float(abs(fd - g[i]) / abs(g[i]))
            print(f"power={power} priors={priors} x={x.tolist()} d/dx{i}: rel. diff {r:.2e} (bar 1e-9)")
            assert r <= 1e-9


@pytest.mark.parametrize("power", ref.POWERS)
def test_power_order_and_derivative(power):
    """apply multiplies left to right; dtheta is its exact derivative (p = 1: exactly 1)."""
    G = np.array([[-0.75, 0.0], [0.3, 2.5]])
    th = 0.37
    K = ref.apply(G, th, power, LD)
    want = LD(th) * G.astype(LD) if power == 0 else (G.astype(LD) + LD(th)) ** power
    assert float(np.max(np.abs(K - want))) <= 1e-17 * float(np.max(np.abs(want)))
    D = ref.dtheta(G, th, power, LD)
    if power == 1:
        assert np.all(D == 1)
    h = LD(1e-6)
    fd = (ref.apply(G, LD(th) + h, power, LD) - ref.apply(G, LD(th) - h, power, LD)) / (2 * h)
    assert float(np.max(np.abs(fd - D))) <= 1e-9 * max(1.0, float(np.max(np.abs(D))))


def test_float64_restatement_is_close():
    """The same code in float64 (what the GPU bars are measured with) agrees to working precision."""
    Xn, y = ref.train_case(20, 3)
    Xt = np.random.default_rng(0).uniform(size=(5, 3))
    for power in (0, 2):
        a = ref.posterior(Xn, y, Xt, power, 0.69, 1e-2, 0.1, -1.0, 2.5, True, LD)
        b = ref.posterior(Xn, y, Xt, power, 0.69, 1e-2, 0.1, -1.0, 2.5, True, np.float64)
        assert b[0].dtype == np.float64
        assert np.allclose(np.asarray(a[0], dtype=np.float64), b[0], rtol=1e-9, atol=0)
        assert np.allclose(np.asarray(a[1], dtype=np.float64), b[1], rtol=1e-7, atol=0)
