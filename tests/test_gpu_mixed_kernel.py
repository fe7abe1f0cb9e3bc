"""GPU: the mixed continuous / categorical kernel entry points alone, through everest_amd.ops,
against the plain long-double reference (tests/mixed_kernel_reference.py, itself checked on the
CPU by tests/test_mixed_kernel_reference.py), at the dispatch edges:

* evr_mixed_kernel_matrix: one 64 x 64 tile kernel per family; shapes below a tile, ragged, more
  than one tile each way (1 x 1, 5 x 3, 33 x 65, 257 x 130); dc = 1 .. 32, nc = 1, 3, 8 with 2 .. 5
  levels; B = 1, 3 with their own parameters; duplicated rows (zero distance), rows equal in every
  category and rows different in every category.
  Bar: the VALU kernel-assembly bar of tests/test_gpu_linalg.py, rtol 1e-12, atol 1e-13 k(x, x).
* evr_mixed_kernel_param_grad: mixed_grad_kernel<8, 4> (dc <= 8), <16, 4> (dc <= 16: a wave per
  row), <32, 1> (a workgroup per row), so dc = 1, 8 | 9, 16 | 17, 32; n = 5 (one partial block of
  rows), 64, 65 (a second column round of a wave), 257 (the workgroup's second round); W random and
  not symmetric.
  Bar: |got - ref| <= 1e-12 S elementwise, S the reference's sum of the absolute values of the same
  terms (tests/test_gpu_kernel_grads.py); worst-case rounding of n^2 = 66049 fused terms of one sign
  pattern is about 257 * 1.1e-16 * a few per row sum, well inside.
"""
import numpy as np
import pytest
import torch

from tests import mixed_kernel_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (5, 3), (33, 65), (257, 130)]
GRAD_N = [5, 64, 65, 257]
DCS = [1, 8, 9, 16, 17, 32]          # either side of the gradient's cuts at 8 and 16, and the ends
NCS = [1, 3, 8]
GRID = [(dc, nc, kind) for dc in DCS for nc in NCS for kind in ref.FAMILIES]
MAXRATIO = {}


def _t(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _inst(dc):
    return "mixed_grad_kernel<8,4>" if dc <= 8 else "mixed_grad_kernel<16,4>" if dc <= 16 else "mixed_grad_kernel<32,1>"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXRATIO):
        print(f"max error / bar  {k}: {MAXRATIO[k]:.3e}")


def _note(label, r):
    MAXRATIO[label] = max(MAXRATIO.get(label, 0.0), r)


@pytest.mark.parametrize("idx,dc,nc,kind", [(i, *c) for i, c in enumerate(GRID)])
def test_matrix_matches_reference(idx, dc, nc, kind):
    from everest_amd import ops

    B = 3 if idx % 2 == 0 else 1     # both member counts for every dc, every nc and every family
    for n1, n2 in SHAPES:
        Xc1, C1, Xc2, C2, params = ref.kernel_case(n1, n2, dc, nc, B)
        K = ops.mixed_kernel_matrix(_t(Xc1), _t(C1, np.int32), _t(Xc2), _t(C2, np.int32), _t(params), kind)
        assert K.shape == (B, n1, n2)
        want = ref.kernel_matrix(Xc1, C1, Xc2, C2, params, kind)
        err = np.abs(K.cpu().numpy().astype(ref.LD) - want)
        bar = 1e-12 * np.abs(want) + 1e-13 * ref.kxx(params)[:, None, None]
        r = float((err / bar).max())
        _note(f"matrix kind {kind}", r)
        print(f"matrix dc={dc} nc={nc} kind={kind} B={B} {n1}x{n2}: max error / bar = {r:.3e}")
        assert r <= 1.0


@pytest.mark.parametrize("kind", ref.FAMILIES)
@pytest.mark.parametrize("dc,nc,n", [(1, 1, 1), (8, 3, 5), (9, 8, 65), (32, 8, 257), (17, 1, 130)])
def test_train_matrix_symmetric_and_diag_add(dc, nc, n, kind):
    """K(X, X) is bitwise symmetric, bitwise the cross call with X2 = X (a copy), and diag_add
    lands on the diagonal alone."""
    from everest_amd import ops

    B = 3
    Xc, C, _, _, params = ref.kernel_case(n, n, dc, nc, B)
    X, Ct, p = _t(Xc), _t(C, np.int32), _t(params)
    K = ops.mixed_kernel_matrix(X, Ct, X, Ct, p, kind)
    assert torch.equal(K, K.transpose(1, 2))
    assert torch.equal(K, ops.mixed_kernel_matrix(X, Ct, X.clone(), Ct.clone(), p, kind))
    dg = _t([0.25, 1e-3, 7.0])
    Kd = ops.mixed_kernel_matrix(X, Ct, X, Ct, p, kind, diag_add=dg)
    eye = torch.eye(n, dtype=torch.bool, device=DEV)
    assert torch.equal(Kd[:, ~eye], K[:, ~eye])
    assert torch.equal(Kd[:, eye], K[:, eye] + dg[:, None])
    # the diagonal itself: k(x, x) = s_sum (1 + s_cat) + s_prod
    kxx = ref.kxx(params)
    assert np.all(np.abs(K[:, eye].cpu().numpy() - kxx[:, None]) <= 1e-12 * kxx[:, None])


@pytest.mark.parametrize("idx,dc,nc,kind", [(i, *c) for i, c in enumerate(GRID)])
def test_param_grad_matches_reference(idx, dc, nc, kind):
    from everest_amd import ops

    for k, n in enumerate(GRAD_N):
        B = 3 if (idx + k) % 2 == 0 else 1     # every n and every (dc, nc, family) meets both member counts
        Xc, C, _, _, params = ref.kernel_case(n, n, dc, nc, B)
        W = np.random.default_rng(1000 * n + idx).normal(size=(B, n, n))
        args = (_t(Xc), _t(C, np.int32), _t(params), _t(W), kind)
        g = ops.mixed_kernel_param_grad(*args)
        assert g.shape == (B, ref.n_params(dc, nc))
        assert torch.equal(g, ops.mixed_kernel_param_grad(*args))       # bitwise reproducible
        want, S = ref.param_grad(Xc, C, params, W, kind)
        err = np.abs(g.cpu().numpy().astype(ref.LD) - want)
        ok = S > 0
        assert np.all(err[~ok] == 0)
        r = float((err[ok] / S[ok]).max())
        _note(f"param_grad {_inst(dc)}", r / 1e-12)
        print(f"param_grad {_inst(dc)} dc={dc} nc={nc} kind={kind} B={B} n={n}: max |err| / S = {r:.3e}")
        assert np.all(err <= 1e-12 * S), (err / np.where(ok, S, 1)).max()


@pytest.mark.parametrize("dc,nc", [(33, 1), (1, 9), (0, 1), (1, 0)])
def test_limits_raise(dc, nc):
    from everest_amd import ops

    n = 4
    Xc, C = torch.zeros(n, dc, dtype=torch.float64, device=DEV), torch.zeros(n, nc, dtype=torch.int32, device=DEV)
    params = torch.ones(1, ref.n_params(dc, nc), dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="unsupported"):
        ops.mixed_kernel_matrix(Xc, C, Xc, C, params, 3)
    with pytest.raises(NotImplementedError, match="unsupported"):
        ops.mixed_kernel_param_grad(Xc, C, params, torch.zeros(1, n, n, dtype=torch.float64, device=DEV), 3)
