"""Plain numpy restatement of the dot-product GP (LinearKernel / PolynomialKernel surrogates),
written from the formulas alone.  Every function takes ``dtype``: ``np.longdouble`` (the
reference; 64-bit mantissa where the platform has x87 extended) or ``np.float64`` (the same
code in the device's number format, so that the restatement's own rounding error can be measured
and a device bar taken from it).  It imports nothing of everest_amd.

    power = 0        k(x, x') = theta <x, x'>             theta = the variance v
    power = p >= 1   k(x, x') = (<x, x'> + theta)^p       theta = the offset c

Integer powers are formed as the device documents them: t = g + theta, r_1 = t, r_{k+1} = r_k t.
The theta derivative is g (power 0), exactly 1 (p = 1), p r_{p-1} (p >= 2).

Model: constant mean c, Gaussian noise s2, K = k(Xn, Xn) + s2 I = L L^T (unblocked Cholesky),
alpha = K^-1 (y - c) by two triangular solves, posterior

    mean = y_mean + y_std (c + k_*^T alpha)
    var  = y_std^2 (k(x_*, x_*) - |L^-1 k_*|^2 + noise_add)

and the loss (MLL + sum log prior) / n in x = [noise, constant, raw_theta], theta = softplus(raw).

The module also holds the inputs of the dot-product tests (``kernel_case``, ``posterior_case``,
``mll_case``, ``fit_case``).
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
POWERS = (0, 1, 2, 3, 8)


# ---- kernel ---------------------------------------------------------------------------------
def gram(X1, X2, dtype=LD):
    """(G, S): G = X1 X2^T and S = sum_k |x_k x'_k|, the sum of the absolute values of G's terms."""
    a, b = np.asarray(X1, dtype=np.float64).astype(dtype), np.asarray(X2, dtype=np.float64).astype(dtype)
    G = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    S = np.zeros_like(G)
    for k in range(a.shape[1]):
        t = a[:, k, None] * b[None, :, k]
        G += t
        S += np.abs(t)
    return G, S


def apply(G, theta, power: int, dtype=LD):
    """f(G; theta) elementwise, theta a scalar."""
    G, theta = np.asarray(G, dtype=dtype), dtype(theta)
    if power == 0:
        return theta * G
    t = G + theta
    r = t
    for _ in range(1, power):
        r = r * t
    return r


def dtheta(G, theta, power: int, dtype=LD):
    """df / dtheta elementwise."""
    G, theta = np.asarray(G, dtype=dtype), dtype(theta)
    if power == 0:
        return G.copy()
    if power == 1:
        return np.ones_like(G)
    t = G + theta
    r = t
    for _ in range(2, power):
        r = r * t
    return dtype(power) * r


def kdiag(X, theta, power: int, dtype=LD):
    """k(x, x) per row of X."""
    x = np.asarray(X, dtype=np.float64).astype(dtype)
    return apply((x * x).sum(1), theta, power, dtype)


def theta_grad(G, thetas, W, power: int, dtype=LD):
    """(g, S) per member: g[b] = sum_ij W[b] df(G; theta_b), S[b] the sum of the absolute values."""
    W = np.asarray(W, dtype=np.float64).astype(dtype)
    g, S = np.zeros(len(thetas), dtype=dtype), np.zeros(len(thetas), dtype=dtype)
    for b, th in enumerate(thetas):
        t = W[b] * dtheta(G, th, power, dtype)
        g[b], S[b] = t.sum(), np.abs(t).sum()
    return g, S


# ---- dense linear algebra, unblocked ---------------------------------------------------------
def cholesky(A):
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not s > 0:
            raise np.linalg.LinAlgError(f"pivot {j} not positive")
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, Bm):
    """L^-1 B by forward substitution (B: n or n x m)."""
    X = np.array(Bm)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_lower_t(L, Bm):
    """L^-T B by back substitution."""
    X = np.array(Bm)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


# ---- model ----------------------------------------------------------------------------------
def softplus(x, dtype=LD):
    x = dtype(x)
    return np.logaddexp(dtype(0), x)


def sigmoid(x, dtype=LD):
    x = dtype(x)
    return 1 / (1 + np.exp(-x))


def _factor(Xn, y, power, theta, noise, const, dtype):
    G, _ = gram(Xn, Xn, dtype)
    K = apply(G, theta, power, dtype)
    K[np.diag_indices_from(K)] += dtype(noise)
    L = cholesky(K)
    r = np.asarray(y, dtype=np.float64).astype(dtype) - dtype(const)
    alpha = solve_lower_t(L, solve_lower(L, r))
    return G, L, r, alpha


def posterior(Xn, y, Xtn, power: int, theta, noise, const, y_mean, y_std, observation_noise: bool, dtype=LD):
    """(mean, var, kxx) at the normalised test rows Xtn; y the standardised targets."""
    _, L, _, alpha = _factor(Xn, y, power, theta, noise, const, dtype)
    Gx, _ = gram(Xn, Xtn, dtype)
    Kx = apply(Gx, theta, power, dtype)
    V = solve_lower(L, Kx)
    kxx = kdiag(Xtn, theta, power, dtype)
    ym, ys = dtype(y_mean), dtype(y_std)
    mean = ym + ys * (dtype(const) + Kx.T @ alpha)
    var = ys * ys * (kxx - (V * V).sum(0) + (dtype(noise) if observation_noise else dtype(0)))
    return mean, var, kxx


def prior_logpdf(p, x, dtype=LD):
    fam, a, b = p[0], dtype(p[1]), dtype(p[2])
    x = dtype(x)
    if fam == "gamma":
        return a * np.log(b) - dtype(math.lgamma(float(a))) + (a - 1) * np.log(x) - b * x
    if fam == "normal":
        return -np.log(2 * dtype(np.pi) * b * b) / 2 - ((x - a) / b) ** 2 / 2
    if fam == "lognormal":
        lx = np.log(x)
        return -lx - np.log(b) - np.log(2 * dtype(np.pi)) / 2 - ((lx - a) / b) ** 2 / 2
    raise ValueError(fam)


def prior_dlogpdf(p, x, dtype=LD):
    fam, a, b = p[0], dtype(p[1]), dtype(p[2])
    x = dtype(x)
    if fam == "gamma":
        return (a - 1) / x - b
    if fam == "normal":
        return -(x - a) / (b * b)
    if fam == "lognormal":
        return (-1 - (np.log(x) - a) / (b * b)) / x
    raise ValueError(fam)


def loss(x, Xn, y, power: int, theta_prior=None, noise_prior=None, dtype=LD):
    """(MLL + sum log prior) / n at x = [noise, constant, raw_theta]."""
    noise, const, raw = dtype(x[0]), dtype(x[1]), dtype(x[2])
    theta = softplus(raw, dtype)
    n = len(y)
    _, L, r, alpha = _factor(Xn, y, power, theta, noise, const, dtype)
    ll = -(r @ alpha) / 2 - np.log(np.diag(L)).sum() - dtype(n) * np.log(2 * dtype(np.pi)) / 2
    if theta_prior is not None:
        ll = ll + prior_logpdf(theta_prior, theta, dtype)
    if noise_prior is not None:
        ll = ll + prior_logpdf(noise_prior, noise, dtype)
    return ll / n


def loss_grad(x, Xn, y, power: int, theta_prior=None, noise_prior=None, dtype=LD):
    """Gradient of ``loss`` in x, analytically: W = alpha alpha^T - K^-1,
    d/dnoise = tr(W) / 2, d/dconst = sum alpha, d/dtheta = sum W dK/dtheta / 2."""
    noise, const, raw = dtype(x[0]), dtype(x[1]), dtype(x[2])
    theta = softplus(raw, dtype)
    n = len(y)
    G, L, _, alpha = _factor(Xn, y, power, theta, noise, const, dtype)
    Li = solve_lower(L, np.eye(n, dtype=dtype))
    W = np.outer(alpha, alpha) - Li.T @ Li
    d_noise = np.trace(W) / 2
    d_const = alpha.sum()
    d_theta = (W * dtheta(G, theta, power, dtype)).sum() / 2
    if theta_prior is not None:
        d_theta = d_theta + prior_dlogpdf(theta_prior, theta, dtype)
    if noise_prior is not None:
        d_noise = d_noise + prior_dlogpdf(noise_prior, noise, dtype)
    return np.array([d_noise, d_const, d_theta * sigmoid(raw, dtype)], dtype=dtype) / n


# ---- inputs of the tests ----------------------------------------------------------------------
def kernel_case(n1: int, n2: int, d: int, B: int):
    """(X1, X2, thetas): rows in [-1, 1]^d, so that the terms of <x, x'> cancel; X2 repeats rows of
    X1 (a test point equal to a training point) and X1 holds a duplicated row."""
    rng = np.random.default_rng(7919 * n1 + 104729 * n2 + 31 * d + B)
    X1 = rng.uniform(-1.0, 1.0, size=(n1, d))
    X2 = rng.uniform(-1.0, 1.0, size=(n2, d))
    if n1 > 1:
        X1[-1] = X1[0]
    X2[::3] = X1[np.arange(0, n2, 3) % n1]
    thetas = np.array([math.log(2.0), 0.37, 2.5])[:B]
    return np.ascontiguousarray(X1), np.ascontiguousarray(X2), thetas


def train_case(n: int, d: int, seed: int = 0):
    """Normalised training rows in [0, 1]^d and standardised targets of a noisy quadratic."""
    rng = np.random.default_rng(1009 * n + 17 * d + seed)
    Xn = rng.uniform(size=(n, d))
    w = rng.normal(size=d)
    y = Xn @ w + 0.5 * (Xn[:, 0] - 0.4) ** 2 + 0.1 * rng.normal(size=n)
    y = (y - y.mean()) / (y.std(ddof=1) if n > 1 else 1.0)
    return np.ascontiguousarray(Xn), y


def posterior_case(n: int, nt: int, d: int):
    """(Xn, y, Xraw, lo, hi): raw test rows with Normalize bounds lo / hi; a third of them lie
    outside the box."""
    Xn, y = train_case(n, d, seed=nt)
    rng = np.random.default_rng(13 * n + 7 * nt + d)
    lo, hi = rng.uniform(-3.0, 1.0, size=d), rng.uniform(2.0, 30.0, size=d)
    U = rng.uniform(size=(nt, d))
    U[::3] = rng.uniform(-0.4, 1.4, size=U[::3].shape)
    return Xn, y, np.ascontiguousarray(lo + U * (hi - lo)), lo, hi


def mll_case():
    return train_case(40, 3, seed=5)


MLL_POINTS = [np.array([0.05, 0.1, 0.0]), np.array([0.6, -0.3, 1.2]), np.array([2.0, 0.0, -1.5])]


def fit_case():
    """n = 40, d = 2 raw inputs a in [0, 40], b in [20, 60]; y = 2.2 a + 0.95 b + noise."""
    rng = np.random.default_rng(11)
    a, b = rng.uniform(0.0, 40.0, size=40), rng.uniform(20.0, 60.0, size=40)
    y = 2.2 * a + 0.95 * b + rng.normal(0.0, 5.0, size=40)
    return a, b, y
