"""GPU: the dot-product kernel entry points alone, through everest_amd.ops, against the plain
long-double reference (tests/dot_kernel_reference.py, itself checked on the CPU by
tests/test_dot_kernel_reference.py).

* evr_dot_kernel_apply: shapes below a workgroup, ragged, odd and even element counts (the scalar
  and the double2 path), more than one workgroup (1 x 1, 5 x 3, 33 x 65, 257 x 130); d = 1, 6, 17, 64
  (the Gram comes from evr_gemm_f64 as the product path takes it); powers 0, 1, 2, 3, 8; B = 1, 3 with
  their own theta; duplicated rows and rows in [-1, 1]^d, so that the terms of <x, x'> cancel.
  Bar, element-wise against long double: the project's kernel-assembly bar stated on the absolute
  terms S = sum_k |x_k x'_k| — 1e-12 theta S (linear), 1e-12 (S + theta)^p (polynomial) — plus
  1e-13 max k(x, x).  The Gram's own rounding is at most d 1.1e-16 S = 7e-15 S, and p multiplications
  carry it to at most p (S + theta)^(p-1) 7e-15 S <= 6e-14 (S + theta)^p.
* evr_dot_kernel_theta_grad: n = 1, 5 (one partial workgroup of rows, odd: the scalar path), 64
  (the double2 path, one round), 65, 257 (a wave's further rounds); W random and not symmetric.
  Bar: |got - ref| <= 1e-12 S, S the reference's sum of the absolute values of the same terms.
"""
import numpy as np
import pytest
import torch

from tests import dot_kernel_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = ref.LD
SHAPES = [(1, 1), (5, 3), (33, 65), (257, 130)]
DS = [1, 6, 17, 64]
GRAD_N = [1, 5, 64, 65, 257]
MAXRATIO = {}


def _t(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXRATIO):
        print(f"max error / bar  {k}: {MAXRATIO[k]:.3e}")


def _note(label, r):
    MAXRATIO[label] = max(MAXRATIO.get(label, 0.0), r)


def _gram(X1, X2):
    from everest_amd import ops

    return ops.gemm(_t(X1), _t(X2), transB=True)


@pytest.mark.parametrize("power", ref.POWERS)
@pytest.mark.parametrize("d", DS)
def test_apply_matches_reference(d, power):
    from everest_amd import ops

    for k, (n1, n2) in enumerate(SHAPES):
        B = 3 if (k + d + power) % 2 == 0 else 1
        X1, X2, thetas = ref.kernel_case(n1, n2, d, B)
        G = _gram(X1, X2)
        K = ops.dot_kernel_apply(G, _t(thetas), power)
        assert K.shape == (B, n1, n2)
        Gl, S = ref.gram(X1, X2, LD)
        got = K.cpu().numpy().astype(LD)
        for b, th in enumerate(thetas):
            want = ref.apply(Gl, th, power, LD)
            kmax = max(float(np.abs(ref.kdiag(X1, th, power, LD)).max()), float(np.abs(ref.kdiag(X2, th, power, LD)).max()))
            bar = 1e-12 * (LD(th) * S if power == 0 else (S + LD(th)) ** power) + 1e-13 * kmax
            r = float((np.abs(got[b] - want) / bar).max())
            _note(f"apply power {power}", r)
            print(f"apply d={d} power={power} B={B} b={b} {n1}x{n2}: max error / bar = {r:.3e}")
            assert r <= 1.0


@pytest.mark.parametrize("power", ref.POWERS)
@pytest.mark.parametrize("n,d", [(1, 1), (5, 6), (33, 17), (64, 6), (257, 64), (130, 17)])
def test_train_matrix_symmetric_and_diag_add(n, d, power):
    """K(X, X) is bitwise symmetric, and diag_add lands on the diagonal alone."""
    from everest_amd import ops

    B = 3
    X, _, thetas = ref.kernel_case(n, n, d, B)
    G, th = _gram(X, X), _t(thetas)
    K = ops.dot_kernel_apply(G, th, power)
    assert torch.equal(K, K.transpose(1, 2))
    dg = _t([0.25, 1e-3, 7.0])
    Kd = ops.dot_kernel_apply(G, th, power, diag_add=dg)
    eye = torch.eye(n, dtype=torch.bool, device=DEV)
    assert torch.equal(Kd[:, ~eye], K[:, ~eye])
    assert torch.equal(Kd[:, eye], K[:, eye] + dg[:, None])


def test_diag_add_on_a_rectangle():
    """i == j, not the flat index: a 5 x 3 and a 4 x 6 matrix (the double2 path crossing row ends)."""
    from everest_amd import ops

    for n1, n2 in ((5, 3), (4, 6), (3, 5)):
        X1, X2, thetas = ref.kernel_case(n1, n2, 6, 1)
        G, th = _gram(X1, X2), _t(thetas)
        K = ops.dot_kernel_apply(G, th, 2)
        Kd = ops.dot_kernel_apply(G, th, 2, diag_add=_t([3.0]))
        want = K.clone()
        for i in range(min(n1, n2)):
            want[0, i, i] += 3.0
        assert torch.equal(Kd, want)


@pytest.mark.parametrize("power", ref.POWERS)
@pytest.mark.parametrize("n", GRAD_N)
def test_theta_grad_matches_reference(n, power):
    from everest_amd import ops

    for B in (1, 3):
        d = {1: 1, 5: 6, 64: 17, 65: 6, 257: 64}[n]
        X, _, thetas = ref.kernel_case(n, n, d, B)
        W = np.random.default_rng(1000 * n + power + B).normal(size=(B, n, n))
        G = _gram(X, X)
        args = (G, _t(thetas), _t(W), power)
        g = ops.dot_kernel_theta_grad(*args)
        assert g.shape == (B,)
        assert torch.equal(g, ops.dot_kernel_theta_grad(*args))       # bitwise reproducible
        # the reference on the device's own Gram (its rounding is the apply test's subject)
        want, S = ref.theta_grad(G.cpu().numpy().astype(LD), thetas, W, power, LD)
        err = np.abs(g.cpu().numpy().astype(LD) - want)
        r = float((err / S).max())
        _note(f"theta_grad power {power}", r / 1e-12)
        print(f"theta_grad n={n} d={d} power={power} B={B}: max |err| / S = {r:.3e}")
        assert np.all(err <= 1e-12 * S)
        if power == 1:      # df / dtheta = 1 exactly: the sum of W
            sw = W.astype(LD).sum((1, 2))
            assert np.all(np.abs(g.cpu().numpy().astype(LD) - sw) <= 1e-12 * np.abs(W).astype(LD).sum((1, 2)))


@pytest.mark.parametrize("power", [-1, 9])
def test_power_limits_raise(power):
    from everest_amd import ops

    n = 4
    G = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    th = torch.ones(1, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="unsupported power"):
        ops.dot_kernel_apply(G, th, power)
    with pytest.raises(NotImplementedError, match="unsupported power"):
        ops.dot_kernel_theta_grad(G, th, torch.zeros(1, n, n, dtype=torch.float64, device=DEV), power)
    M = torch.zeros(1, n + 1, n, dtype=torch.float64, device=DEV)
    one = torch.ones(1, dtype=torch.float64, device=DEV)
    col = torch.ones(2, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="unsupported power"):
        ops.dot_gp_posterior(torch.zeros(n, 2, dtype=torch.float64, device=DEV),
                             torch.zeros(3, 2, dtype=torch.float64, device=DEV), col, col, th, M, power, one, one, one)


def test_mismatched_shapes_raise():
    from everest_amd import ops

    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)  # noqa: E731
    with pytest.raises(ValueError):
        ops.dot_kernel_apply(z(4, 4), z(2), 0, diag_add=z(3))
    with pytest.raises(ValueError):
        ops.dot_kernel_apply(z(2, 4, 4), z(2), 0)
    with pytest.raises(ValueError):
        ops.dot_kernel_theta_grad(z(4, 5), z(1), z(1, 4, 4), 2)
    with pytest.raises(ValueError):
        ops.dot_kernel_theta_grad(z(4, 4), z(2), z(1, 4, 4), 2)
    with pytest.raises(ValueError):
        ops.dot_gp_posterior(z(4, 2), z(3, 3), z(2), z(2), z(1), z(1, 5, 4), 0, z(1), z(1), z(1))
    with pytest.raises(ValueError):
        ops.dot_gp_posterior(z(4, 2), z(3, 2), z(2), z(2), z(1), z(1, 4, 4), 0, z(1), z(1), z(1))
    with pytest.raises(ValueError):
        ops.dot_kernel_apply(z(4, 4), z(1), 2.5)


def test_empty_side_returns_empty():
    from everest_amd import ops

    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)  # noqa: E731
    assert ops.dot_kernel_apply(z(0, 5), z(2), 2).shape == (2, 0, 5)
    assert ops.dot_kernel_apply(z(5, 0), z(1), 0).shape == (1, 5, 0)
    mean, var = ops.dot_gp_posterior(z(4, 2), z(0, 2), z(2), z(2), z(1), z(1, 5, 4), 0, z(1), z(1), z(1))
    assert mean.shape == (1, 0) and var.shape == (1, 0)
