"""GPU: the device pieces of the scaled kernel k = sigma^2 k_base alone, through everest_amd.ops.

* evr_kernel_hyper_grad ([gls | gos] in one pass over W) against long double:
  tests/gp_kernel_reference.lengthscale_grad times sigma^2 and tests/scale_kernel_reference.
  outputscale_grad, each with the absolute sum S of its own terms.  Bar 1e-12 S
  (tests/test_gpu_kernel_grads.py).  d = 1, 8 (kls_grad_kernel<8>), 9, 16 (<16>), 17
  (kls_grad_block_kernel<32>), 33, 64 (<64>: the value column's own LDS partials); n = 5 (less
  than a wave), 65 (one lane into the second column round), 97, 130; the four families; B = 1 and
  3 and sigma^2 = 0.05, ln 2, 7 cycling over the cases so that every instantiation meets each.
  A second run is bitwise equal (no atomics).  On a NaN-filled workspace (the C entry points
  called directly) every row partial is written.
* evr_kernel_hyper_grad_members (n = 97, nvalid = 97, 61, 5): each member against the long-double
  reference on its own rows, to the same bar, and the padding contributes exactly nothing: other
  padded inputs and other padded entries of W leave every bit as it was.
* evr_kernel_matrix_members_scaled: 1e-12 absolute on the real block, ``==`` on the padding
  (tests/test_gpu_cv_members.py).
"""
import math

import numpy as np
import pytest
import torch

from tests import gp_kernel_reference as ref
from tests import scale_kernel_reference as sref

pytestmark = pytest.mark.gpu
DS = (1, 8, 9, 16, 17, 33, 64)
NS = (5, 65, 97, 130)
MAXRATIO = {}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _label(d):
    return ("kls_grad_kernel<8>" if d <= 8 else "kls_grad_kernel<16>" if d <= 16 else
            "kls_grad_block_kernel<32>" if d <= 32 else "kls_grad_block_kernel<64>") + " scaled"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXRATIO):
        print(f"max |err| / S  {k}: {MAXRATIO[k]:.3e}")


def _note(label, r):
    MAXRATIO[label] = max(MAXRATIO.get(label, 0.0), r)


def _cases():
    out, i = [], 0
    for d in DS:
        for n in NS:
            for kind in (0, 1, 2, 3):
                # B flips with the kind and again from one (d, n) to the next, so that every family
                # meets B = 1 and B = 3 within each instantiation
                B = (1, 3)[(i + i // 4) % 2]
                out.append(pytest.param(d, n, kind, B, (i // 2) % 3, id=f"d{d}-n{n}-kind{kind}-B{B}-os{(i // 2) % 3}"))
                i += 1
    return out


def test_case_list_covers_every_option():
    seen, by_kind = {}, {}
    for p in _cases():
        d, n, kind, B, io = p.values
        s = seen.setdefault(_label(d), dict(B=set(), os=set(), kind=set(), n=set()))
        s["B"].add(B), s["os"].add(io), s["kind"].add(kind), s["n"].add(n)
        k = by_kind.setdefault((_label(d), kind), dict(B=set(), os=set()))
        k["B"].add(B), k["os"].add(io)
    assert len(seen) == 4 and len(by_kind) == 16
    for s in seen.values():
        assert s["B"] == {1, 3} and s["os"] == {0, 1, 2} and s["kind"] == {0, 1, 2, 3} and s["n"] == set(NS)
    for key, k in by_kind.items():               # jointly: each family of each instantiation at both B, every sigma^2
        assert k["B"] == {1, 3} and k["os"] == {0, 1, 2}, key


def _check(label, g, gos, X, ls, os_, W, kinds):
    want_ls, S_ls = ref.lengthscale_grad(X, ls, W, kinds)
    want_os, S_os = sref.outputscale_grad(X, ls, W, kinds)
    osl = np.asarray(os_, dtype=ref.LD)[:, None]
    e_ls = np.abs(g.astype(ref.LD) - want_ls * osl)
    e_os = np.abs(gos.astype(ref.LD) - want_os)
    r_ls = float((e_ls / (S_ls * osl)).max())
    r_os = float((e_os / S_os).max())
    print(f"{label}: max |err| / S  gls {r_ls:.3e}  gos {r_os:.3e}")
    _note(label + " gls", r_ls), _note(label + " gos", r_os)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gos))
    assert np.all(e_ls <= ref.LD(1e-12) * S_ls * osl), r_ls
    assert np.all(e_os <= ref.LD(1e-12) * S_os), r_os


@pytest.mark.parametrize("d,n,kind,B,io", _cases())
def test_kernel_hyper_grad(d, n, kind, B, io):
    from everest_amd import ops

    rng = np.random.default_rng(7919 * d + 31 * n + 5 * kind + B)
    X = rng.uniform(-1, 2, (n, d))
    if n >= 65:
        X[[n - 1, n - 2, 40, 33]] = X[[0, 1, 2, 3]]              # zero distances off the diagonal
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    os_ = np.array([sref.OUTPUTSCALES[(io + b) % 3] for b in range(B)])
    W = rng.normal(size=(B, n, n))                               # not symmetric
    args = (_t(X), _t(ls), _t(os_), _t(W), kind)
    gls, gos = ops.kernel_hyper_grad(*args)
    gls2, gos2 = ops.kernel_hyper_grad(*args)
    torch.cuda.synchronize()
    assert torch.equal(gls, gls2) and torch.equal(gos, gos2)     # fixed-order sums: bitwise reproducible
    _check(_label(d), gls.cpu().numpy(), gos.cpu().numpy(), X, ls, os_, W, kind)


@pytest.mark.parametrize("d", (8, 16, 32, 64))
def test_every_row_partial_is_written(d):
    """The C entry points on a workspace full of NaN: a partial left unwritten (a padded row's, the
    value column's) would reach the column sums.  Shared form and members, bitwise the ops results."""
    from everest_amd import ops

    n, B = 97, 3
    rng = np.random.default_rng(d)
    nvalid = _t(NVALID, torch.int32)
    Xb = _t(rng.uniform(size=(B, n, d)))
    ls, os_, W = _t(rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)), _t(sref.OUTPUTSCALES), _t(rng.normal(size=(B, n, n)))
    for members in (False, True):
        out = torch.full((B * (d + 1),), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.full((B * n * (d + 1),), float("nan"), dtype=torch.float64, device="cuda")
        if members:
            ops.call("evr_kernel_hyper_grad_members", ops._stream(), 3, B, n, d, Xb.data_ptr(), nvalid.data_ptr(),
                     ls.data_ptr(), os_.data_ptr(), W.data_ptr(), out.data_ptr(), work.data_ptr())
            gls, gos = ops.kernel_hyper_grad_members(Xb, nvalid, ls, os_, W, 3)
        else:
            ops.call("evr_kernel_hyper_grad", ops._stream(), 3, B, n, d, Xb[0].data_ptr(), ls.data_ptr(),
                     os_.data_ptr(), W.data_ptr(), out.data_ptr(), work.data_ptr())
            gls, gos = ops.kernel_hyper_grad(Xb[0].contiguous(), ls, os_, W, 3)
        torch.cuda.synchronize()
        assert torch.isfinite(work).all() and torch.isfinite(out).all(), members
        assert torch.equal(out[:B * d].reshape(B, d), gls) and torch.equal(out[B * d:], gos)
        if members:                               # padded rows: exact zeros in every column
            wk = work.reshape(B, n, d + 1)
            for b, nv in enumerate(NVALID):
                assert torch.all(wk[b, nv:] == 0.0)


def test_hyper_grad_of_a_unit_scale_agrees_with_the_lengthscale_entry_point():
    """sigma^2 = 1: the lengthscale pieces are the unscaled kernel's to rounding of the one-exponential
    form (1e-12 S), so the two entry points cannot drift apart unnoticed."""
    from everest_amd import ops

    for d, n in ((8, 97), (16, 65), (33, 97)):
        rng = np.random.default_rng(d + n)
        X, ls, W = rng.uniform(size=(n, d)), rng.uniform(0.3, 1.2, (2, d)) * math.sqrt(d), rng.normal(size=(2, n, n))
        for kind in (0, 3):
            a = ops.kernel_lengthscale_grad(_t(X), _t(ls), _t(W), kind).cpu().numpy()
            b, _ = ops.kernel_hyper_grad(_t(X), _t(ls), _t(np.ones(2)), _t(W), kind)
            _, S = ref.lengthscale_grad(X, ls, W, kind)
            assert np.all(np.abs(a - b.cpu().numpy()) <= 2e-12 * S.astype(np.float64))


NVALID = (97, 61, 5)


@pytest.mark.parametrize("d", DS)
def test_kernel_hyper_grad_members(d):
    from everest_amd import ops

    n, B = 97, 3
    rng = np.random.default_rng(1000 + d)
    nvalid = np.array(NVALID, dtype=np.int32)
    Xb, W = np.zeros((B, n, d)), np.zeros((B, n, n))
    for b, nv in enumerate(NVALID):
        Xb[b, :nv] = rng.uniform(-1, 2, (nv, d))
        A = rng.normal(size=(nv, nv))
        W[b, :nv, :nv] = A + A.T
        W[b, nv:, nv:] = -np.eye(n - nv)          # alpha alpha^T - K^-1 on the padding: -I
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    os_ = np.array(sref.OUTPUTSCALES)
    other_X, other_W = Xb.copy(), W.copy()
    for b, nv in enumerate(NVALID):
        other_X[b, nv:] = rng.uniform(-3.0, 3.0, size=(n - nv, d))
        other_W[b, nv:, :] = rng.normal(size=(n - nv, n))
        other_W[b, :, nv:] = rng.normal(size=(n, n - nv))
    for kind in ((0, 1, 2, 3) if d in (8, 17) else (0, 3)):
        gls, gos = ops.kernel_hyper_grad_members(_t(Xb), _t(nvalid, torch.int32), _t(ls), _t(os_), _t(W), kind)
        g2, o2 = ops.kernel_hyper_grad_members(_t(other_X), _t(nvalid, torch.int32), _t(ls), _t(os_), _t(other_W), kind)
        assert torch.equal(gls, g2) and torch.equal(gos, o2), "the padding leaks into the gradient pieces"
        gls, gos = gls.cpu().numpy(), gos.cpu().numpy()
        for b, nv in enumerate(NVALID):
            _check(_label(d) + " members", gls[b:b + 1], gos[b:b + 1], Xb[b, :nv], ls[b:b + 1], os_[b:b + 1],
                   W[b:b + 1, :nv, :nv], kind)
            # the shared form on the member's own rows: the same lane order over the same columns
            sg, so = ops.kernel_hyper_grad(_t(Xb[b, :nv]), _t(ls[b:b + 1]), _t(os_[b:b + 1]),
                                           _t(W[b:b + 1, :nv, :nv]), kind)
            _, S_ls = ref.lengthscale_grad(Xb[b, :nv], ls[b:b + 1], W[b:b + 1, :nv, :nv], kind)
            _, S_os = sref.outputscale_grad(Xb[b, :nv], ls[b:b + 1], W[b:b + 1, :nv, :nv], kind)
            assert np.all(np.abs(sg.cpu().numpy() - gls[b]) <= 2e-12 * os_[b] * S_ls.astype(np.float64))
            assert abs(float(so.cpu().numpy()[0]) - gos[b]) <= 2e-12 * float(S_os[0])


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", (5, 64, 97, 129))
def test_kernel_matrix_members_scaled(n, d):
    from everest_amd import ops

    B = 3
    rng = np.random.default_rng(50 * n + d)
    pads = (0, 1, min(7, n - 2))
    nvalid = np.array([n - p for p in pads], dtype=np.int32)
    Xb = np.zeros((B, n, d))
    for b in range(B):
        Xb[b, :nvalid[b]] = rng.uniform(size=(nvalid[b], d))
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    noise, os_ = np.array([1e-2, 5e-2, 0.2]), np.array(sref.OUTPUTSCALES)
    eye = np.eye(n)
    for kind in ((0, 1, 2, 3) if d in (8, 17) else (0, 3)):
        K = ops.kernel_matrix_members_scaled(_t(Xb), _t(nvalid, torch.int32), _t(ls), _t(os_), kind,
                                             diag_add=_t(noise)).cpu().numpy()
        for b in range(B):
            nv = int(nvalid[b])
            want = os_[b] * ref.train_matrix(Xb[b, :nv], ls[b], 0.0, kind) + noise[b] * np.eye(nv)
            err = np.abs(K[b, :nv, :nv] - want).max()
            assert err <= 1e-12, (kind, b, err)
            assert np.array_equal(K[b, :nv, :nv], K[b, :nv, :nv].T)
            assert np.all(K[b, nv:, :] == eye[nv:, :]) and np.all(K[b, :, nv:] == eye[:, nv:]), (kind, b)
    # an unpadded member is the shared-X scaled train matrix, bit for bit
    Km = ops.kernel_matrix_members_scaled(_t(Xb[:1]), _t([n], torch.int32), _t(ls[:1]), _t(os_[:1]), 3,
                                          diag_add=_t(noise[:1]))
    Ks = ops.kernel_matrix(_t(Xb[0]), _t(Xb[0]), _t(ls[:1]), 3, outputscale=_t(os_[:1]), diag_add=_t(noise[:1]))
    assert torch.equal(Km, Ks)
