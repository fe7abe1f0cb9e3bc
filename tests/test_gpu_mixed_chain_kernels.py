"""GPU: the candidate side of the mixed GP — evr_mixed_split and evr_mixed_kernel_cross_grad
(mixed_chain.hip) against tests/mixed_acq_reference.cross_grad (numpy long double, the explicit
sum) and plain torch.

Bar of the X-gradient, the form the parameter gradient's test uses: |err| <= 1e-12 S, S the sum of
the absolute values of the summed terms (a float64 sum of N terms of either sign is good to about
N eps S' with S' <= S; N <= 2 * 2 * 70 terms per entry here).  One-hot columns are exactly 0 and
two runs are bitwise equal (fixed-order reduction, no atomics)."""
import numpy as np
import pytest
import torch

from everest_amd import ops
from tests import mixed_acq_reference as mar
from tests import mixed_kernel_reference as mkr

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _layout(rng, dc, nc):
    """A d-wide row: the one-hot blocks first (2..5 levels), then the continuous columns in
    reversed order.  Returns (d, cont_idx, cat_start, cat_len, scale)."""
    card = mkr.cardinalities(nc)
    start = np.concatenate([[0], np.cumsum(card)[:-1]])
    d = int(card.sum()) + dc
    cont = np.arange(d - 1, d - 1 - dc, -1)
    scale = np.ones(d)
    scale[cont] = rng.uniform(0.5, 2.0, dc)
    return d, cont.astype(np.int32), start.astype(np.int32), card.astype(np.int32), scale


def _run(Xc, C, X2c, C2, params, G, scale, cont, kind):
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)  # noqa: E731
    return ops.mixed_kernel_cross_grad(t(Xc), t(C, torch.int32), t(X2c), t(C2, torch.int32), t(params), t(G), t(scale),
                                       t(cont, torch.int32), kind)


# dc at both edges of every dispatch bin (<= 8, <= 16, <= 32)
@pytest.mark.parametrize("dc", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("kind", mkr.FAMILIES)
def test_cross_grad_matches_explicit_sum(kind, dc):
    worst = 0.0
    for n in (5, 70):                   # 70: a ragged second 64-row tile of the row split
        for rows in (1, 65):            # 65: a second candidate tile with one column
            for nc in (1, 8):
                for B in (1, 2):
                    Xc, C, X2c, C2, params = mkr.kernel_case(n, rows, dc, nc, B)
                    rng = np.random.default_rng(7 * n + rows + dc + nc + B)
                    d, cont, _, _, scale = _layout(rng, dc, nc)
                    G = rng.normal(size=(B, n, rows))
                    dX = _run(Xc, C, X2c, C2, params, G, scale, cont, kind)
                    again = _run(Xc, C, X2c, C2, params, G, scale, cont, kind)
                    assert torch.equal(dX, again), "two runs differ"
                    dX = dX.cpu().numpy()
                    assert dX.shape == (rows, d)
                    onehot = np.setdiff1d(np.arange(d), cont)
                    assert np.all(dX[:, onehot] == 0.0) and not np.signbit(dX[:, onehot]).any()
                    g, S = mar.cross_grad(Xc, C, X2c, C2, params, G, kind)
                    g, S = g * scale[cont], S * scale[cont]
                    err = np.abs(dX[:, cont].astype(mar.LD) - g)
                    assert np.all(S > 0)
                    ratio = float((err / S).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1e-12, (n, rows, nc, B, ratio)
    print(f"mixed cross grad kind={kind} dc={dc}: worst |err| / S = {worst:.3e}")


@pytest.mark.parametrize("kind", mkr.FAMILIES)
def test_coincident_pair_contributes_zero(kind):
    """Candidate 0 is training row 0 with equal codes, candidate 1 the same point with every code
    changed (kernel_case).  With dK supported on those two pairs only, the gradient is exactly 0:
    the difference is 0 and k_c' is finite — 0 where r^2 < 1e-30 for the Matern families (the
    convention kcross_grad has: autograd through clamp_min(1e-30).sqrt() gives 0 there)."""
    for dc, nc in ((2, 2), (9, 1), (32, 8)):
        Xc, C, X2c, C2, params = mkr.kernel_case(5, 3, dc, nc, 2)
        assert np.array_equal(X2c[0], Xc[0]) and np.array_equal(C2[0], C[0])
        assert np.array_equal(X2c[1], Xc[0]) and (C2[1] != C[0]).all()
        rng = np.random.default_rng(dc)
        d, cont, _, _, scale = _layout(rng, dc, nc)
        G = np.zeros((2, 5, 3))
        G[:, 0, 0], G[:, 0, 1] = 1.5, -2.5
        dX = _run(Xc, C, X2c, C2, params, G, scale, cont, kind).cpu().numpy()
        assert np.all(dX == 0.0)
        # and inside a full dK those pairs add nothing: the result is the sum without them
        G = rng.normal(size=(2, 5, 3))
        full = _run(Xc, C, X2c, C2, params, G, scale, cont, kind)
        G[:, 0, 0] = G[:, 0, 1] = 0.0
        assert torch.equal(full, _run(Xc, C, X2c, C2, params, G, scale, cont, kind))


def test_split_codes_and_normalisation():
    rng = np.random.default_rng(3)
    dc, nc = 3, 2
    # row: [c0 (3 levels) | x0 | c1 (2 levels) | x1 x2]
    cont = np.array([3, 6, 7], dtype=np.int32)
    start, length = np.array([0, 4], dtype=np.int32), np.array([3, 2], dtype=np.int32)
    d = 8
    rows = 70
    X = np.zeros((rows, d))
    X[:, cont] = rng.uniform(-3.0, 5.0, size=(rows, dc))
    c0, c1 = rng.integers(0, 3, rows), rng.integers(0, 2, rows)
    X[np.arange(rows), c0] = 1.0
    X[np.arange(rows), 4 + c1] = 1.0
    # relaxed rows: a tie takes the first maximum, as does an all-zero block
    X[0, :3], c0[0] = [0.5, 0.5, 0.0], 0
    X[1, :3], c0[1] = [0.2, 0.4, 0.4], 1
    X[2, :3], c0[2] = [0.0, 0.0, 0.0], 0
    X[3, 4:6], c1[3] = [0.5, 0.5], 0
    X[4, :3], c0[4] = [0.1, 0.3, 0.6], 2
    lo = np.zeros(d)
    hi = np.ones(d)
    lo[cont], hi[cont] = [-3.0, -4.0, 0.1], [5.5, 5.0, 7.3]
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=DEV)  # noqa: E731
    Xd, lod = t(X), t(lo)
    ir = 1.0 / (t(hi) - lod)
    Xc, Cc = ops.mixed_split(Xd, lod, ir, t(cont, torch.int32), t(start, torch.int32), t(length, torch.int32))
    assert Xc.shape == (rows, dc) and Cc.shape == (rows, nc) and Cc.dtype == torch.int32
    assert np.array_equal(Cc.cpu().numpy(), np.stack([c0, c1], 1))
    idx = t(cont, torch.long)
    assert torch.equal(Xc, (Xd[:, idx] - lod[idx]) * ir[idx])          # bitwise torch's own expression


def test_sizes_outside_the_kernels_are_errors():
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=DEV)  # noqa: E731
    dc, nc = 33, 1
    with pytest.raises(NotImplementedError):
        ops.mixed_kernel_cross_grad(t(np.zeros((4, dc))), t(np.zeros((4, nc)), torch.int32), t(np.zeros((2, dc))),
                                    t(np.zeros((2, nc)), torch.int32), t(np.ones((1, 2 * dc + 2 * nc + 3))),
                                    t(np.zeros((1, 4, 2))), t(np.ones(dc + 2)), t(np.arange(dc), torch.int32), 3)
