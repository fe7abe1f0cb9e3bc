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
    torch.classes.everest_amd.QrewardAcq(state, model, mode, ucb_scale, tau, infeasible_cost, best, terms,
                                         constraints, keep)
    torch.ops.everest_amd.qreward_forward / qreward_forward_backward   (qSR, qUCB, qPI)

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


class QnehviFunction(torch.autograd.Function):
    """acq = qNEHVI / qEHVI(X) through the torch operators on a
    torch.classes.everest_amd.QnehviAcq (which owns the acquisition state and caches its
    plans).  When X needs a gradient the forward runs qnehvi_forward_backward — ONE device
    chain for the value and the analytic gradient — and saves dX; backward only scales it by
    grad_out (candidates are independent)."""

    @staticmethod
    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = ops.qnehvi_forward_backward(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return ops.qnehvi_forward(acq, X)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        shape = (dX.shape[0],) + (1,) * (dX.dim() - 1)
        return dX * grad_out.reshape(shape), None


class QneiFunction(torch.autograd.Function):
    """acq = qNEI / qLogNEI / qLogEI(X), X b x q x d, through torch.ops.everest_amd.qnei_* on a
    torch.classes.everest_amd.QneiAcq; as QnehviFunction, one device chain gives the value and
    the analytic gradient, and backward scales the saved dX by grad_out."""

    @staticmethod
    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = ops.qnei_forward_backward(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return ops.qnei_forward(acq, X)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        return dX * grad_out.reshape(-1, 1, 1), None


class QsoboFunction(torch.autograd.Function):
    """acq = QSoboNEI / QSoboLogNEI / QSoboLogEI(X), X b x q x d, through
    torch.ops.everest_amd.qsobo_* on a torch.classes.everest_amd.QsoboAcq; as QneiFunction."""

    @staticmethod
    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = ops.qsobo_forward_backward(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return ops.qsobo_forward(acq, X)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        return dX * grad_out.reshape(-1, 1, 1), None


class QparegoFunction(torch.autograd.Function):
    """acq = QParegoNEI / QParegoLogNEI / QParegoLogEI(X), X b x q x d, through
    torch.ops.everest_amd.qparego_* on a torch.classes.everest_amd.QparegoAcq; as QneiFunction."""

    @staticmethod
    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = ops.qparego_forward_backward(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return ops.qparego_forward(acq, X)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        return dX * grad_out.reshape(-1, 1, 1), None


class QrewardFunction(torch.autograd.Function):
    """acq = QSoboSR / QSoboUCB / QSoboPI(X), X b x q x d, through torch.ops.everest_amd.qreward_*
    on a torch.classes.everest_amd.QrewardAcq; as QneiFunction."""

    @staticmethod
    def forward(ctx, X: torch.Tensor, acq):
        ops = load()
        if ctx.needs_input_grad[0]:
            a, dX = ops.qreward_forward_backward(acq, X)
            ctx.save_for_backward(dX)
            return a
        ctx.save_for_backward(None)
        return ops.qreward_forward(acq, X)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dX,) = ctx.saved_tensors
        return dX * grad_out.reshape(-1, 1, 1), None
