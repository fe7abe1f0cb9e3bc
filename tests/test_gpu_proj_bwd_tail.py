"""GPU: the projection backward (qn_proj_bwd, dKx = M^T gR) must not depend on the memory that
follows the operator M.  Its row segments run in whole 16-deep k-steps; past a segment's end the
other operand is 0, but M's fetch was unguarded, so for the last output the steps past row Rr read
whatever lay behind M — and 0 x (a stale NaN) made that output's dKx, and with it every entry of
dX, NaN, depending on what earlier work had left in freed device memory.

Here M sits at the front of a buffer whose tail is NaN, then zeros: the two results are bitwise
equal and finite.  Shapes: the (n, d, m, S, prune) cases of tests/test_gpu_qlognehvi.py that showed
the fault, b = 40 candidates (above 32: the tile path, not the small-batch kernels)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_qlognehvi import _matched

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,d,m,S,prune,ehvi", [(16, 8, 7, 8, True, False), (24, 3, 2, 32, False, True),
                                                (50, 5, 4, 16, False, True)])
def test_projection_backward_ignores_memory_behind_M(n, d, m, S, prune, ehvi):
    from everest_amd import ops

    X, lo, hi, _, dq = _matched(n, d, m, S, seed=n, prune=prune, ehvi=ehvi)
    b = 40
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(5).uniform(size=(b, d)), device="cuda")
    Kx = dq._cross(Xc)
    R, P = ops.qnehvi_project(dq.state, dq.M, Kx, b)
    G, L22, flags = ops.qnehvi_samples_norms(dq.state, R, P, b)
    _, dG = ops.hvi_forward_backward(dq.state, G, b, flags, None)
    M = dq.M
    nn = M.shape[2]
    out = {}
    for name, fill in (("nan", float("nan")), ("zero", 0.0)):
        buf = torch.full((M.numel() + 64 * nn,), fill, dtype=torch.float64, device="cuda")
        Mv = buf[:M.numel()].view_as(M)
        Mv.copy_(M)
        out[name] = ops.qnehvi_project_backward(dq.state, Mv, R, L22, dG, b)
    torch.cuda.synchronize()
    assert torch.isfinite(out["nan"]).all(), "memory behind M leaked into dKx"
    assert torch.equal(out["nan"], out["zero"])
