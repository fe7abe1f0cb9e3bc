"""GPU: the member form of the MLL chain (B GPs on their own rows, the folds of a cross-validation:
evr_kernel_matrix_members, evr_kernel_lengthscale_grad_members, evr_mll_plan_create_members,
MLLBatch(nvalid=...)) against references on each member's own rows.

Inputs: ``tests.gp_kernel_reference.mll_case(n, d, B)``; member b keeps all n rows but a
contiguous block (pads 0, 1 and 7 in one batch of B = 3: member 0 keeps everything), its rows
compacted to the front of Xb[b] and zeros behind.  A principal submatrix of an s.p.d. matrix is no
worse conditioned than the matrix, so the conditioning tests/test_gp_kernel_reference.py asserts
for mll_case carries over to every member.

Shapes: n in {5, 63, 64, 65, 97, 129} (one 64-tile, its edge, two tiles; nmax = n odd and even: both
mll_w_kernel instantiations), d in {1, 8, 9, 16, 17, 33, 64} (kmat_kernel; kmat_mfma_sym<16|32|64>;
kls_grad_kernel<8|16>, kls_grad_block_kernel<32|64>), families 0-3 at d in {8, 17} and 0, 3
elsewhere, and B = 53 at n = 8, d = 1 (more than 256 terms in the copy-out block).

Bars: kernel matrix 1e-12 absolute (entries O(1)) and ``==`` on the padding; lengthscale gradient
1e-12 S (tests/test_gpu_kernel_grads.py); plan against the oracle value 1e-9 max(1, |ref|),
gradient rtol 1e-7 atol 1e-9 (tests/test_gpu_mll_chain.py); plan against the shared-X chain on the
member's rows alone 1e-10 max(1, |.|) (test_mll_plan_many_outputs).
"""
import math

import numpy as np
import pytest
import torch

from oracle import gp as ogp
from tests import gp_kernel_reference as ref

pytestmark = pytest.mark.gpu
NOISE_PRIOR = (-4.0, 1.0)
NS = (5, 63, 64, 65, 97, 129)
DS = (1, 8, 9, 16, 17, 33, 64)


def _kinds(d):
    return (0, 1, 2, 3) if d in (8, 17) else (0, 3)


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _members(n, d, B=3, pads=None):
    """mll_case(n, d, B) split into members: rows[b] the kept row indices (member 0: all), Xb and
    Yb zero-padded to nmax = n, nvalid, and the raw parameter vectors."""
    X, Ys, xs = ref.mll_case(n, d, B)
    pads = pads if pads is not None else (0, 1, min(7, n - 2))
    rows = []
    for b in range(B):
        p = pads[b % len(pads)]
        start = ((b * n) // (B + 1)) % (n - p + 1)          # a different block per member
        rows.append(np.r_[np.arange(start), np.arange(start + p, n)])
    nvalid = np.array([len(r) for r in rows], dtype=np.int32)
    assert nvalid[0] == n and nvalid.min() >= 1
    Xb, Yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b, r in enumerate(rows):
        Xb[b, :len(r)], Yb[b, :len(r)] = X[r], Ys[b, r]
    return X, Ys, xs, rows, Xb, Yb, nvalid


def test_member_case_pads():
    for n in NS:
        nvalid = _members(n, 1)[6]
        assert sorted(n - nvalid) == sorted((0, 1, min(7, n - 2)))


# ---------------------------------------------------------------------------------------
# evr_kernel_matrix_members
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_kernel_matrix_members(n, d):
    from everest_amd import ops

    X, _, xs, rows, Xb, _, nvalid = _members(n, d)
    ls = np.logaddexp(0.0, xs[:, 2:])
    noise = xs[:, 0].copy()
    for kind in _kinds(d):
        K = ops.kernel_matrix_members(_t(Xb), _t(nvalid, torch.int32), _t(ls), kind, diag_add=_t(noise)).cpu().numpy()
        for b, r in enumerate(rows):
            nv = len(r)
            want = ref.train_matrix(X[r], ls[b], noise[b], kind)
            err = np.abs(K[b, :nv, :nv] - want).max()
            assert err <= 1e-12, (kind, b, err)
            assert np.array_equal(K[b, :nv, :nv], K[b, :nv, :nv].T)
            eye = np.eye(n)
            assert np.all(K[b, nv:, :] == eye[nv:, :]) and np.all(K[b, :, nv:] == eye[:, nv:]), (kind, b)


def test_kernel_matrix_members_equals_shared_kernel():
    """An unpadded member is the shared-X train matrix, bit for bit (the same tile code)."""
    from everest_amd import ops

    for n, d in ((65, 8), (129, 17)):
        X, _, xs, _, _, _, _ = _members(n, d)
        ls, noise = np.logaddexp(0.0, xs[:1, 2:]), xs[:1, 0].copy()
        for kind in (0, 3):
            Km = ops.kernel_matrix_members(_t(X[None]), _t([n], torch.int32), _t(ls), kind, diag_add=_t(noise))
            Ks = ops.kernel_matrix(_t(X), _t(X), _t(ls), kind, diag_add=_t(noise))
            assert torch.equal(Km, Ks)


# ---------------------------------------------------------------------------------------
# evr_kernel_lengthscale_grad_members
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", (5, 65, 129))
def test_kernel_lengthscale_grad_members(n, d):
    from everest_amd import ops

    X, _, xs, rows, Xb, _, nvalid = _members(n, d)
    ls = np.logaddexp(0.0, xs[:, 2:])
    rng = np.random.default_rng(17 * n + d)
    B = len(rows)
    W = np.zeros((B, n, n))
    Wm = []
    for b, r in enumerate(rows):
        nv = len(r)
        A = rng.normal(size=(nv, nv))
        Wm.append(A + A.T)
        W[b, :nv, :nv] = Wm[b]
        W[b, nv:, nv:] = -np.eye(n - nv)          # alpha alpha^T - K^-1 on the padding: -I
    other = Xb.copy()
    for b, r in enumerate(rows):
        other[b, len(r):] = rng.uniform(-3.0, 3.0, size=(n - len(r), d))
    for kind in _kinds(d):
        got = ops.kernel_lengthscale_grad_members(_t(Xb), _t(ls), _t(W), kind)
        moved = ops.kernel_lengthscale_grad_members(_t(other), _t(ls), _t(W), kind)
        assert torch.equal(got, moved), "padded rows of Xb leak into the gradient"
        g = got.cpu().numpy()
        for b, r in enumerate(rows):
            want, S = ref.lengthscale_grad(X[r], ls[b:b + 1], Wm[b][None], kind)
            err = np.abs(g[b].astype(ref.LD) - want[0])
            assert np.all(err <= ref.LD(1e-12) * S[0]), (kind, b, float((err / S[0]).max()))


# ---------------------------------------------------------------------------------------
# the member plan
# ---------------------------------------------------------------------------------------
def _oracle(X, y, x, kind, d):
    t = torch.tensor(x, requires_grad=True)
    v = ogp.mll_value(torch.tensor(X), torch.tensor(y), t[2:], t[0], t[1], kind, ogp.dim_scaled_lognormal(d),
                      NOISE_PRIOR)
    v.backward()
    return v.item(), t.grad.numpy().copy()


def _check_oracle(label, got, want):
    (v, g), (rv, rg) = got, want
    ev = abs(v - rv) / max(1.0, abs(rv))
    eg = float((np.abs(g - rg) / (1e-9 + 1e-7 * np.abs(rg))).max())
    print(f"{label}: value error {ev:.3e} (bar 1e-9), gradient error / bar {eg:.3e}")
    assert ev <= 1e-9, (label, v, rv)
    assert np.allclose(g, rg, rtol=1e-7, atol=1e-9), (label, g, rg)


def _spy(ev, monkeypatch):
    taken, plan = [], ev._eval_plan

    def spy(*a):
        out = plan(*a)
        taken.append(out is not None)
        return out

    monkeypatch.setattr(ev, "_eval_plan", spy)
    return taken


def _raw(xs):
    """(ls, noise, constant) host arrays of raw parameter vectors, with the fit drivers' softplus."""
    from everest_amd.gp import _softplus_libm

    ls = np.array([[_softplus_libm(v) for v in row] for row in xs[:, 2:]])
    return ls, xs[:, 0].copy(), xs[:, 1].copy()


PLAN_CASES = [(5, 1), (63, 8), (64, 16), (65, 9), (97, 17), (129, 33), (65, 64)]


@pytest.mark.parametrize("n,d", PLAN_CASES)
def test_member_plan(n, d, monkeypatch):
    """MLLBatch over a member plan: against the oracle on each member's rows, and its raw terms
    and gradient pieces against today's shared-X MLLBatch on those rows alone (B = 1).  Member 0
    has no padding in a batch with padded members: subtracting a pad count it does not have
    would show."""
    from everest_amd.gp import MLLBatch

    X, Ys, xs, rows, Xb, Yb, nvalid = _members(n, d)
    prior = ogp.dim_scaled_lognormal(d)
    B = len(rows)
    for kind in _kinds(d):
        ev = MLLBatch(_t(Xb), Yb, kind, prior, NOISE_PRIOR, nvalid=nvalid)
        assert ev.use_plan
        taken = _spy(ev, monkeypatch)
        want = [_oracle(X[r], Ys[b, r], xs[b], kind, d) for b, r in enumerate(rows)]
        for idx in ([0, 1, 2], [1], [2, 0]):
            got = ev(idx, [xs[b] for b in idx])
            assert taken and taken[-1], "the plan handed the evaluation to the op-by-op chain"
            for k, b in enumerate(idx):
                assert got[k] is not None
                _check_oracle(f"member plan n={n} d={d} kind={kind} pad={n - nvalid[b]}", got[k], want[b])
        # the five terms and the gradient pieces against the shared-X plan on the member's rows
        idx = list(range(B))
        host = ev._eval_plan(idx, *_raw(xs))
        assert host is not None and np.all(host[5 * B + B * d:] == 0)
        for b, r in enumerate(rows):
            one = MLLBatch(_t(X[r]), Ys[b:b + 1, r], kind, prior, NOISE_PRIOR)
            w = one._eval_plan([0], *_raw(xs[b:b + 1]))
            assert w is not None
            t, tw = host[5 * b:5 * b + 5], w[:5]
            g, gw = host[5 * B + b * d:5 * B + (b + 1) * d], w[5:5 + d]
            assert np.all(np.abs(t - tw) <= 1e-10 * np.maximum(1.0, np.abs(tw))), (kind, b, t, tw)
            assert np.all(np.abs(g - gw) <= 1e-10 * np.maximum(1.0, np.abs(gw))), (kind, b, g, gw)
            # the op chain's member form (the jitter ladder's path) meets the same bar
        chain = ev._eval_ops(idx, *_raw(xs))
        ok = np.abs(chain - host) <= 1e-10 * np.maximum(1.0, np.abs(host))
        assert ok.all(), (kind, chain[~ok], host[~ok])


def test_member_plan_many_members():
    """B = 53 members at n = 8, d = 1: 265 terms through the 256-thread copy-out block, pads
    0 / 1 / 6 cycling."""
    from everest_amd.gp import MLLBatch

    n, d, B = 8, 1, 53
    X, Ys, xs, rows, Xb, Yb, nvalid = _members(n, d, B)
    prior = ogp.dim_scaled_lognormal(d)
    ev = MLLBatch(_t(Xb), Yb, 0, prior, NOISE_PRIOR, nvalid=nvalid)
    got = ev(list(range(B)), list(xs))
    host = ev._eval_plan(list(range(B)), *_raw(xs))
    assert host is not None, "the plan handed the evaluation to the op-by-op chain"
    for b, r in enumerate(rows):
        assert got[b] is not None
        _check_oracle(f"member plan B=53 member {b}", got[b], _oracle(X[r], Ys[b, r], xs[b], 0, d))


@pytest.mark.parametrize("noise", [1e-13, 1e-18])
def test_member_ladder_fallback(noise, monkeypatch):
    """Members with duplicated rows (test_mll_plan_matches_op_chain's inputs).  At noise 1e-13, that
    test's value, every member — padded or not — agrees with the op-by-op shared-X chain on its own
    rows under that test's rule, whichever path the round takes (measured on the MI355X: the
    attempt-0 factor succeeds there, the duplicates' pivots of about 2e-13 being far above the
    factor's rounding, so the plan keeps the round).  At noise 1e-18 the diagonal 1 + 1e-18 rounds to
    1: the matrix is exactly singular, the attempt-0 factor fails, the round goes through the op
    chain with the jitter ladder — asserted — and the same rule holds (the values are finite: the
    padded block's jitter is taken out of log det and tr K^-1)."""
    from everest_amd.gp import MLLBatch
    from tests.helpers import dtlz2

    rng = np.random.default_rng(5)
    n, d, B = 150, 4, 3
    X = rng.uniform(size=(n, d))
    X[100:110] = X[:10]                                   # duplicates: singular without noise
    Y = dtlz2(X, B)
    Ys = ((Y - Y.mean(0)) / Y.std(0)).T.copy()
    rows = [np.arange(n), np.r_[np.arange(50), np.arange(51, n)], np.r_[np.arange(60), np.arange(67, n)]]
    nvalid = np.array([len(r) for r in rows], dtype=np.int32)
    Xb, Yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b, r in enumerate(rows):
        Xb[b, :len(r)], Yb[b, :len(r)] = X[r], Ys[b, r]
    prior = (math.sqrt(2) + 0.5 * math.log(d), math.sqrt(3))
    for kind in (0, 3):
        ev = MLLBatch(_t(Xb), Yb, kind, prior, NOISE_PRIOR, nvalid=nvalid)
        taken = _spy(ev, monkeypatch)
        bad = [np.r_[noise, 0.0, rng.normal(size=d)] for _ in range(B)]
        got = ev([0, 1, 2], bad)
        print(f"kind {kind} noise {noise}: the plan kept the round: {taken}")
        if noise < 1e-16:
            assert taken == [False], "the failed attempt-0 factor did not hand the round to the op chain"
        for b, r in enumerate(rows):
            one = MLLBatch(_t(X[r]), Ys[b:b + 1, r], kind, prior, NOISE_PRIOR)
            one.use_plan = False
            (want,) = one([0], [bad[b]])
            assert (got[b] is None) == (want is None), b
            if want is not None:
                a, w = got[b][0], want[0]
                print(f"kind {kind} noise {noise} member {b} (pad {n - nvalid[b]}): {a!r} vs {w!r}")
                assert (np.isnan(a) and np.isnan(w)) or abs(a - w) <= 1e-6 * max(1.0, abs(w))
