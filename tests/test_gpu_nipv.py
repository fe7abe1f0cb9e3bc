"""Negative integrated posterior variance on the MI355X: the fused reduction of nipv.hip
(ops.nipv_reduce) and the acquisition around it (acquisition.QNegIntPosVar) against the independent
``direct`` route of tests/nipv_reference.py (one dense (n + q) Cholesky per output and candidate,
gradients by autograd).

States: GPBatch built from given hypers, no fit; inputs in a box that is not the unit cube;
lengthscales in [0.3, 1] on the normalised inputs, noise in [1e-4, 1e-2], three different kernel
families at B = 3.  The grid covers q in {1, 2, 3, 12}, b in {1, 15, 16, 17, 33},
N in {1, 63, 64, 65, 130}, n in {5, 64, 70}, d in {1, 6}, B in {1, 3}: every (q, b) pair, the other
factors cycled so that each of their values meets each q.

Tolerances are measured, not fixed: per state, e is the CPU error of ``schur_route`` (the device's
own algebra in torch) against ``direct`` — relative for values, row-relative for gradients — and
the device is held to max(8 e, 64 * 2.2e-16 * sum_j coef_j) (``nipv_reference.bounds``).  Every test
prints its figures before it asserts.

Measured over the grid states (this file's CASES, seeds as below; e moves a little with the
host's thread count):
    e       values <= 3.9e-12 relative, gradients <= 1.1e-10 row-relative (largest at d = 1, where
            the training rows crowd; at d = 6 e is 1e-16..3e-15 and the floor of 64 ulp decides)
    device  values <= 2.2e-12, gradients <= 9.7e-11 (one run); per state within 4.0 e (values) and
            4.4 e (gradients: q = 12, n = 5, d = 1 — twelve points on a line — 6.1e-11 against
            e = 1.4e-11, bound 1.1e-10), elsewhere at or below e.  DESIGN.md section 4.8 has the rest."""
import functools

import numpy as np
import pytest
import torch

from everest_amd import ops
from everest_amd.acquisition import QNegIntPosVar
from everest_amd.gp import GPBatch, GPHyper
from everest_amd.optim import host_values
from tests import nipv_reference as nr

pytestmark = pytest.mark.gpu

KINDS = {1: [nr.MATERN25], 3: [nr.RBF, nr.MATERN25, nr.MATERN15]}
QS, BS, NS, NTR, DS, NOUT = (1, 2, 3, 12), (1, 15, 16, 17, 33), (1, 63, 64, 65, 130), (5, 64, 70), (1, 6), (1, 3)
CASES = [(q, b, NS[(iq + ib) % 5], NTR[(iq + 2 * ib) % 3], DS[(iq + ib) % 2], NOUT[(iq + ib // 2) % 2])
         for iq, q in enumerate(QS) for ib, b in enumerate(BS)]


@functools.lru_cache(maxsize=None)
def _host_state(n, N, d, B, seed=0):
    """Host arrays of a model state."""
    rng = np.random.default_rng(1000 * n + 10 * N + d + 7 * B + seed)
    lo, hi = rng.uniform(-2.0, 0.0, size=d), rng.uniform(1.0, 3.0, size=d)
    Xn = rng.uniform(size=(n, d))
    ls = rng.uniform(0.3, 1.0, size=(B, d))
    noise = 10.0 ** rng.uniform(-4.0, -2.0, size=B)
    ys = rng.uniform(0.5, 2.0, size=B)
    w = np.ones(1) if B == 1 else rng.uniform(0.2, 1.5, size=B)
    P = lo + (hi - lo) * rng.uniform(size=(N, d))
    Y = rng.normal(size=(n, B))
    return dict(Xn=Xn, P=P, Y=Y, ls=ls, noise=noise, ys=ys, kinds=KINDS[B], coef=(w * ys) ** 2, w=w, lo=lo, hi=hi, d=d,
                B=B)


@functools.lru_cache(maxsize=None)
def _state(n, N, d, B, seed=0):
    """The host state with its GPBatch on the device (given hypers, no fit)."""
    s = dict(_host_state(n, N, d, B, seed))
    hyp = [GPHyper(lengthscale=s["ls"][j], noise=float(s["noise"][j]), constant=0.1 * j, y_mean=0.3,
                   y_std=float(s["ys"][j])) for j in range(B)]
    s["gp"] = GPBatch(_dev(s["Xn"]), _dev(s["Y"]), hyp, KINDS[B], _dev(s["lo"]), _dev(s["hi"]))
    return s


def _ref_args(s):
    return s["Xn"], s["P"], s["ls"], s["noise"], s["kinds"], s["coef"], s["lo"], s["hi"]


@functools.lru_cache(maxsize=None)
def _host_case(q, b, N, n, d, B):
    """The candidates, gout and both CPU routes of one grid case (computed once, never changed)."""
    s = _host_state(n, N, d, B)
    rng = np.random.default_rng(q * 100 + b)
    X = s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(b, q, d))
    gout = rng.uniform(0.5, 2.0, size=b) * rng.choice([-1.0, 1.0], size=b)
    Xn, P, *rest = _ref_args(s)
    v_d, g_d = nr.batch(nr.direct, Xn, P, X, *rest, gout=gout)
    v_s, g_s = nr.batch(nr.schur_route, Xn, P, X, *rest, gout=gout)
    e = (nr.value_error(v_s, v_d), nr.row_error(g_s, g_d))
    return X, gout, v_d, g_d, e


def _case(q, b, N, n, d, B):
    return (_state(n, N, d, B),) + _host_case(q, b, N, n, d, B)


def _acqf(s, **kw):
    return QNegIntPosVar(s["gp"], s["P"], weights=None if s["B"] == 1 else s["w"], **kw)


def _dev(a):
    return torch.as_tensor(a, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("q,b,N,n,d,B", CASES)
def test_forward_matches_direct(q, b, N, n, d, B):
    s, X, _, v_d, _, e = _case(q, b, N, n, d, B)
    tol_v, _ = nr.bounds(*e, s["coef"])
    acq = host_values(_acqf(s).forward(_dev(X if q > 1 else X[:, 0])))
    err = nr.value_error(acq, v_d)
    print(f"NIPV fwd q={q} b={b} N={N} n={n} d={d} B={B}: e_val={e[0]:.3e} dev_val={err:.3e} bound={tol_v:.3e}")
    assert err <= tol_v


@pytest.mark.parametrize("q,b,N,n,d,B", CASES)
def test_forward_backward_matches_direct(q, b, N, n, d, B):
    s, X, gout, v_d, g_d, e = _case(q, b, N, n, d, B)
    tol_v, tol_g = nr.bounds(*e, s["coef"])
    Xd = _dev(X if q > 1 else X[:, 0])
    acq, dX = _acqf(s).forward_backward(Xd, _dev(gout))
    assert tuple(dX.shape) == tuple(Xd.shape)
    ev, eg = nr.value_error(host_values(acq), v_d), nr.row_error(dX.cpu().reshape(b, q, d), g_d)
    print(f"NIPV fwd+bwd q={q} b={b} N={N} n={n} d={d} B={B}: e_val={e[0]:.3e} dev_val={ev:.3e} "
          f"bound={tol_v:.3e} | e_grad={e[1]:.3e} dev_grad={eg:.3e} bound={tol_g:.3e}")
    assert ev <= tol_v
    assert eg <= tol_g


def test_gout_defaults_to_ones():
    s, X, gout, *_ = _case(3, 17, 64, 5, 1, 3)
    a = _acqf(s)
    Xd = _dev(X)
    acq1, g1 = a.forward_backward(Xd)
    acq2, g2 = a.forward_backward(Xd, torch.ones(17, dtype=torch.float64, device="cuda"))
    acq3, _ = a.forward_backward(Xd, _dev(gout))
    assert torch.equal(acq1, acq2) and torch.equal(g1, g2)
    assert torch.equal(acq1, acq3)                          # gout weights the backward only


@pytest.mark.parametrize("q,npend", [(1, 2), (2, 1)])
def test_pending_points_join_every_candidate(q, npend):
    s = _state(64, 65, 6, 3)
    rng = np.random.default_rng(q)
    b, d = 15, 6
    X = s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(b, q, d))
    Xp = s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(npend, d))
    joint = np.concatenate([X, np.broadcast_to(Xp, (b, npend, d))], 1)
    a_p, a_j = _acqf(s, X_pending_raw=Xp), _acqf(s)
    assert a_p.n_pending == npend
    acq_p, g_p = a_p.forward_backward(_dev(X))
    acq_j, g_j = a_j.forward_backward(_dev(joint))
    assert torch.equal(a_p.forward(_dev(X)), acq_p)
    assert torch.equal(acq_p, acq_j)                       # the value is the joint batch's
    assert tuple(g_p.shape) == (b, q, d)                   # the pending points' rows are dropped
    assert torch.equal(g_p, g_j[:, :q])
    Xn, P, *rest = _ref_args(s)
    v_d, g_d = nr.batch(nr.direct, Xn, P, joint, *rest)
    v_s, g_s = nr.batch(nr.schur_route, Xn, P, joint, *rest)
    tol_v, tol_g = nr.bounds(nr.value_error(v_s, v_d), nr.row_error(g_s[:, :q], g_d[:, :q]), s["coef"])
    ev, eg = nr.value_error(host_values(acq_p), v_d), nr.row_error(g_p.cpu(), g_d[:, :q])
    print(f"NIPV pending q={q}+{npend}: dev_val={ev:.3e} bound={tol_v:.3e} dev_grad={eg:.3e} bound={tol_g:.3e}")
    assert ev <= tol_v and eg <= tol_g


def _chain(s, X3):
    """C, R (rows 0..n-1 = Vx) of the acquisition's chain for the candidates X3 (b x q x d)."""
    a, gp = _acqf(s), s["gp"]
    X2 = X3.reshape(-1, X3.shape[-1]).contiguous()
    R = ops.gemm(gp.M, gp.cross(X2))
    C = ops.kernel_matrix(a.Pn, X2, gp.ls, gp.kind, shift2=a._lo, scale2=a._ir)
    C -= torch.matmul(a.Vp.transpose(1, 2), R[:, :gp.n])
    return a, C.contiguous(), R.contiguous()


def _reduce(a, s, C, R, X3, backward=True, gout=None):
    gp = s["gp"]
    return ops.nipv_reduce(C, R, X3, a._lo, a._ir, gp.ls, gp.kind, gp.noise, a.coef, a.v0, n=gp.n, backward=backward,
                           gout=gout)


def test_two_runs_are_bitwise_equal():
    s, X, gout, *_ = _case(12, 33, 65, 64, 6, 3)
    a, Xd = _acqf(s), _dev(X)
    r1, r2 = a.forward_backward(Xd, _dev(gout)), a.forward_backward(Xd, _dev(gout))
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    assert torch.equal(a.forward(Xd), r1[0])


@pytest.mark.parametrize("q", [1, 3, 12])
def test_a_candidate_does_not_depend_on_its_batch(q):
    """b = 33 in one call against calls of 16 + 17 on the same columns of C and Vx: bit for bit."""
    s = _state(70, 130, 6, 3)
    rng = np.random.default_rng(q)
    X3 = _dev(s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(33, q, 6)))
    gout = _dev(rng.uniform(0.5, 2.0, size=33))
    a, C, R = _chain(s, X3)
    full = _reduce(a, s, C, R, X3, gout=gout)
    for c0, c1 in ((0, 16), (16, 33)):
        cols = slice(c0 * q, c1 * q)
        part = _reduce(a, s, C[:, :, cols].contiguous(), R[:, :, cols].contiguous(), X3[c0:c1].contiguous(),
                       gout=gout[c0:c1].contiguous())
        assert torch.equal(part[0], full[0][c0:c1]) and torch.equal(part[1], full[1][c0:c1])
        assert torch.equal(part[2], full[2][:, :, cols]) and torch.equal(part[3], full[3][:, :, cols])
        assert torch.equal(part[4], full[4][c0:c1])
    # and through the whole acquisition
    af, ab = a.forward_backward(X3, gout)
    for c0, c1 in ((0, 16), (16, 33)):
        pf, pb = a.forward_backward(X3[c0:c1].contiguous(), gout[c0:c1].contiguous())
        assert torch.equal(pf, af[c0:c1]) and torch.equal(pb, ab[c0:c1])


def test_identical_points_stay_finite():
    """Two identical points in a candidate: noise > 0 keeps A positive definite."""
    s = _state(64, 64, 6, 3)
    rng = np.random.default_rng(3)
    X = s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(5, 3, 6))
    X[:, 2] = X[:, 0]
    X[4, 1] = s["lo"] + (s["hi"] - s["lo"]) * s["Xn"][7]          # and one on a training row
    acq, dX = _acqf(s).forward_backward(_dev(X))
    assert torch.isfinite(acq).all() and torch.isfinite(dX).all()
    Xn, P, *rest = _ref_args(s)
    v_d, _ = nr.batch(nr.direct, Xn, P, X, *rest, grad=False)
    v_s, _ = nr.batch(nr.schur_route, Xn, P, X, *rest, grad=False)
    tol_v, _ = nr.bounds(nr.value_error(v_s, v_d), 0.0, s["coef"])
    ev = nr.value_error(host_values(acq), v_d)
    print(f"NIPV identical points: e_val={nr.value_error(v_s, v_d):.3e} dev_val={ev:.3e} bound={tol_v:.3e}")
    assert ev <= tol_v


def test_negative_pivot_sets_the_flag_and_nan():
    """|Vx|^2 > 1 + noise makes A's pivot negative: a numeric flag on that candidate alone, NaN in
    the acquisition's values and NotPSDError from optim.host_values."""
    s = _state(5, 63, 6, 3)
    rng = np.random.default_rng(4)
    X3 = _dev(s["lo"] + (s["hi"] - s["lo"]) * rng.uniform(size=(4, 2, 6)))
    a, C, R = _chain(s, X3)
    R[1, 0, 2 * 2 + 1] = 1.5            # output 1, candidate 2, point 1
    acq, flags, *_ = _reduce(a, s, C, R, X3, backward=False)
    assert flags.dtype == torch.int32 and flags.cpu().tolist() == [0, 0, 1, 0]
    assert torch.isfinite(acq[[0, 1, 3]]).all()
    ok = _reduce(a, s, *_chain(s, X3)[1:], X3, backward=False)
    assert torch.equal(ok[0][[0, 1, 3]], acq[[0, 1, 3]]) and ok[1].cpu().tolist() == [0, 0, 0, 0]
    # through the acquisition: the same state with an inflated projection
    gp = s["gp"]
    M = gp.M
    try:
        gp.M = (M * 3.0).contiguous()
        Xt = _dev(s["lo"] + (s["hi"] - s["lo"]) * s["Xn"][:3])
        vals = _acqf(s).forward(Xt)
        assert torch.isnan(vals).all()
        with pytest.raises(ops.NotPSDError):
            host_values(vals)
    finally:
        gp.M = M


def test_argument_checks():
    s = _state(5, 63, 6, 3)
    X3 = _dev(s["lo"] + (s["hi"] - s["lo"]) * np.random.default_rng(5).uniform(size=(2, 13, 6)))
    a = _acqf(s)
    with pytest.raises(ValueError, match="12"):
        a.forward(X3)
    gp = s["gp"]
    C = torch.zeros(3, 63, 26, dtype=torch.float64, device="cuda")
    R = torch.zeros(3, 6, 26, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="q = 13"):
        ops.nipv_reduce(C, R, X3, a._lo, a._ir, gp.ls, gp.kind, gp.noise, a.coef, a.v0, n=5)
    with pytest.raises(RuntimeError, match="kind"):
        ops.nipv_reduce(C[:, :, :24].contiguous(), R[:, :, :24].contiguous(), X3[:, :12].contiguous(), a._lo, a._ir,
                        gp.ls, 7, gp.noise, a.coef, a.v0, n=5)
    empty = a.forward(torch.zeros(0, 6, dtype=torch.float64, device="cuda"))
    assert tuple(empty.shape) == (0,)
    e = ops.nipv_reduce(C[:, :, :0].contiguous(), R[:, :, :0].contiguous(), X3[:0, :12].contiguous(), a._lo, a._ir,
                        gp.ls, gp.kind, gp.noise, a.coef, a.v0, n=5)
    assert e[0].numel() == 0 and e[1].numel() == 0
