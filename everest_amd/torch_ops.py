"""PyTorch-ROCm custom operators of the hot path (TORCH_LIBRARY(everest_amd), built from
everest_amd/csrc/torch_ops.cpp into _lib/libeverest_amd_torch.so) and their autograd
wrappers — SURVEY.md §8(b)'s numeric op boundary, replacing the BoTorch Model.posterior /
AcquisitionFunction.forward protocols called at bofire/strategies/predictives/botorch.py:
180,223,384:

    torch.ops.everest_amd.kernel_matrix(X1, X2, lengthscales, kind) -> K (B x n1 x n2)
    torch.ops.everest_amd.cholesky(A, jitter0, max_tries) -> (L, jitter, info)
    torch.ops.everest_amd.gp_posterior(Xn, X, shift, scale, ls, M, kind, c, ym, ys, kxx, noise?)
    torch.classes.everest_amd.QnehviAcq(state, scan_state, model, fast, keep)  (owns state + plans)
    torch.ops.everest_amd.qnehvi_forward(acq, X) -> acq values
    torch.ops.everest_amd.qnehvi_forward_backward(acq, X) -> (acq values, dX)
    torch.ops.everest_amd.qnehvi_backward(acq, X, grad_out) -> dX
    torch.classes.everest_amd.QneiAcq(state, model, log, tau_relu, tau_max, best, a, b, keep)
    torch.ops.everest_amd.qnei_forward / qnei_forward_backward / qnei_backward   (qNEI, qLogNEI, qLogEI)
    torch.classes.everest_amd.QsoboAcq(state, model, log, tau_relu, tau_max, best, terms, constraints, keep)
    torch.ops.everest_amd.qsobo_forward / qsobo_forward_backward   (scalarised / output-constrained SOBO)
    torch.classes.everest_amd.QparegoAcq(state, model, log, tau_relu, tau_max, best, alpha, terms, constraints, keep)
    torch.ops.everest_amd.qparego_forward / qparego_forward_backward   (qParEGO: augmented Chebyshev utility)
    torch.classes.everest_amd.QmultAcq(state, model, log, tau_relu, tau_max, best, factors, addends, keep)
    torch.ops.everest_amd.qmult_forward / qmult_forward_backward   (multiplicative / multiplicative-additive SOBO)
    torch.classes.everest_amd.QrewardAcq(state, model, mode, ucb_scale, tau, infeasible_cost, best, terms,
                                         constraints, keep)
    torch.ops.everest_amd.qreward_forward / qreward_forward_backward   (qSR, qUCB, qPI)

The six autograd wrappers (QnehviFunction, QneiFunction, QsoboFunction, QparegoFunction,
QmultFunction, QrewardFunction) are instances of one body, _chain_function(prefix), that differ in the operator
prefix only.

No fallback: a missing library raises NativeLibraryError."""
from __future__ import annotations

import os

import torch

from ._native import NativeLibraryError

_HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_LIB_PATH = os.path.join(_HERE, "_lib", "libeverest_amd_torch.so")
_loaded = False


def load():
    """Register the operators (once); returns the torch.ops.everest_amd namespace."""
    global _loaded
    if not _loaded:
        if not os.path.exists(TORCH_LIB_PATH):
            raise NativeLibraryError(f"everest_amd torch operator library not found at {TORCH_LIB_PATH}; build it "
                                     "with `python -c 'import __graft_entry__ as g; g.build()'`")
        from . import _native
        _native.load()            # the C-ABI library first (same file the operators link)
        torch.ops.load_library(TORCH_LIB_PATH)
        _loaded = True
    return torch.ops.everest_amd


def _chain_function(prefix: str, doc: str):
    """The autograd.Function over torch.ops.everest_amd.<prefix>_forward / _forward_backward on the
    matching torch.classes.everest_amd object.  When X needs a gradient the forward runs
    <prefix>_forward_backward — ONE device chain for the value and the analytic gradient — and
    saves dX; backward only scales it by grad_out (candidates are independent; dX is b x d on the
    qNEHVI q = 1 fast path, b x q x d otherwise)."""

    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = getattr(ops, prefix + "_forward_backward")(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return getattr(ops, prefix + "_forward")(acq, X)

    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        return dX * grad_out.reshape((dX.shape[0],) + (1,) * (dX.dim() - 1)), None

    return type(f"Q{prefix[1:]}Function", (torch.autograd.Function,),
                {"__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})


QnehviFunction = _chain_function("qnehvi", "acq = qNEHVI / qEHVI(X) on a QnehviAcq (which owns the acquisition "
                                           "state and caches its plans); X b x d (q = 1 fast path) or b x q x d.")
QneiFunction = _chain_function("qnei", "acq = qNEI / qLogNEI / qLogEI(X), X b x q x d, on a QneiAcq.")
QsoboFunction = _chain_function("qsobo", "acq = QSoboNEI / QSoboLogNEI / QSoboLogEI(X), X b x q x d, on a QsoboAcq.")
QparegoFunction = _chain_function("qparego",
                                  "acq = QParegoNEI / QParegoLogNEI / QParegoLogEI(X), X b x q x d, on a QparegoAcq.")
QmultFunction = _chain_function("qmult", "acq = QMultNEI / QMultLogNEI / QMultLogEI(X), X b x q x d, on a QmultAcq.")
QrewardFunction = _chain_function("qreward", "acq = QSoboSR / QSoboUCB / QSoboPI(X), X b x q x d, on a QrewardAcq.")
