"""Torch-tensor level wrappers over the C-ABI (include/everest_amd.h).

Every op runs on torch's *current* HIP stream, takes float64 device tensors, allocates
its outputs with the torch caching allocator and never frees caller memory.  Shape,
dtype and device errors raise (``ValueError`` / ``RuntimeError``); there is no CPU path.
The posterior, kernel matrix, Cholesky and qNEHVI entry points are also registered as PyTorch
custom operators (``torch.ops.everest_amd.*``, everest_amd/csrc/torch_ops.cpp, everest_amd/torch_ops.py).
"""
from __future__ import annotations

import ctypes
import math
import os
import warnings
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native import EvrQnehviState, EvrQnGeneral, call

KERNELS = {"rbf": 0, "matern05": 1, "matern15": 2, "matern25": 3}
KIND_BY_NU = {0.5: 1, 1.5: 2, 2.5: 3}


class NotPSDError(RuntimeError):
    """Raised when the jitter ladder of psd_safe_cholesky is exhausted ([upstream]
    linear_operator NotPSDError, caught by fit_gpytorch_mll's retries)."""


# joint batch limit of the general q-point kernels (include/everest_amd.h EVR_QNG_MAX_Q): the
# [upstream] inclusion-exclusion enumerates all 2^q - 1 subsets of the q (+ pending) points
QNG_MAX_Q = 12

def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=torch.float64) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: everest_amd ops run on the MI355X only (got device {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------
# kernel matrices
# ---------------------------------------------------------------------------------------
def kernel_matrix(X1, X2, lengthscales, kind: int = 0, shift1=None, scale1=None, shift2=None, scale2=None,
                  outputscale=None, diag_add=None) -> torch.Tensor:
    """K[b] = os_b * k(norm(X1), norm(X2); ls_b) (+ diag_add_b on i==j).  ls: B x d."""
    X1 = _dev(X1, "X1")
    X2 = _dev(X2, "X2")
    ls = _dev(lengthscales, "lengthscales")
    if ls.dim() == 1:
        ls = ls.unsqueeze(0)
    B, d = ls.shape
    if X1.shape[-1] != d or X2.shape[-1] != d:
        raise ValueError(f"kernel_matrix: dims mismatch X1 {tuple(X1.shape)} X2 {tuple(X2.shape)} ls {tuple(ls.shape)}")
    n1, n2 = X1.shape[0], X2.shape[0]
    K = torch.empty(B, n1, n2, dtype=torch.float64, device=X1.device)
    opt = [None if t is None else _dev(t, "aux") for t in (shift1, scale1, shift2, scale2, outputscale, diag_add)]
    call("evr_kernel_matrix", _stream(), int(kind), B, n1, n2, d, X1.data_ptr(), _p(opt[0]), _p(opt[1]),
         X2.data_ptr(), _p(opt[2]), _p(opt[3]), ls.data_ptr(), _p(opt[4]), _p(opt[5]), K.data_ptr())
    return K


def _workspace(ndoubles: int, device) -> torch.Tensor:
    """Scratch for a native op (torch caching allocator; no device-side malloc)."""
    return torch.empty(max(int(ndoubles), 1), dtype=torch.float64, device=device)


def kernel_cross_grad(X1, X2, lengthscales, G, kind=0, shift1=None, scale1=None, shift2=None, scale2=None,
                      outputscale=None) -> torch.Tensor:
    X1, X2, ls, G = _dev(X1, "X1"), _dev(X2, "X2"), _dev(lengthscales, "ls"), _dev(G, "G")
    B, d = ls.shape
    n1, n2 = X1.shape[0], X2.shape[0]
    if tuple(G.shape) != (B, n1, n2):
        raise ValueError(f"kernel_cross_grad: G shape {tuple(G.shape)} != {(B, n1, n2)}")
    dX = torch.empty(n2, d, dtype=torch.float64, device=X1.device)
    opt = [None if t is None else _dev(t, "aux") for t in (shift1, scale1, shift2, scale2, outputscale)]
    work = _workspace(_native.load().evr_kernel_cross_grad_workspace_doubles(n1, n2, d), X1.device)
    call("evr_kernel_cross_grad", _stream(), int(kind), B, n1, n2, d, X1.data_ptr(), _p(opt[0]), _p(opt[1]),
         X2.data_ptr(), _p(opt[2]), _p(opt[3]), ls.data_ptr(), _p(opt[4]), G.data_ptr(), dX.data_ptr(),
         work.data_ptr())
    return dX


def kernel_lengthscale_grad(X, lengthscales, W, kind=0) -> torch.Tensor:
    X, ls, W = _dev(X, "X"), _dev(lengthscales, "ls"), _dev(W, "W")
    B, d = ls.shape
    n = X.shape[0]
    g = torch.empty(B, d, dtype=torch.float64, device=X.device)
    work = torch.empty(B, n, d, dtype=torch.float64, device=X.device)
    call("evr_kernel_lengthscale_grad", _stream(), int(kind), B, n, d, X.data_ptr(), ls.data_ptr(), W.data_ptr(),
         g.data_ptr(), work.data_ptr())
    return g


def _members(Xb, lengthscales, nvalid=None):
    Xb, ls = _dev(Xb, "Xb"), _dev(lengthscales, "lengthscales")
    if Xb.dim() != 3 or ls.dim() != 2 or ls.shape[0] != Xb.shape[0] or ls.shape[1] != Xb.shape[2]:
        raise ValueError(f"members: Xb {tuple(Xb.shape)} must be B x n x d and ls {tuple(ls.shape)} B x d")
    if nvalid is not None:
        nvalid = _dev(nvalid, "nvalid", torch.int32)
        if tuple(nvalid.shape) != (Xb.shape[0],):
            raise ValueError(f"members: nvalid {tuple(nvalid.shape)} must hold one count per member")
    return Xb, ls, nvalid


def kernel_matrix_members(Xb, nvalid, lengthscales, kind: int = 0, diag_add=None) -> torch.Tensor:
    """Train matrices of B members on their own rows (evr_kernel_matrix_members): Xb B x n x d,
    nvalid (B, int32, device; counts in 1..n are the caller's to guarantee) the real rows of
    each; padded rows / columns are the identity."""
    Xb, ls, nvalid = _members(Xb, lengthscales, nvalid)
    B, n, d = Xb.shape
    K = torch.empty(B, n, n, dtype=torch.float64, device=Xb.device)
    dg = None if diag_add is None else _dev(diag_add, "diag_add")
    call("evr_kernel_matrix_members", _stream(), int(kind), B, n, d, Xb.data_ptr(), nvalid.data_ptr(), ls.data_ptr(),
         _p(dg), K.data_ptr())
    return K


def kernel_lengthscale_grad_members(Xb, lengthscales, W, kind=0) -> torch.Tensor:
    """kernel_lengthscale_grad with member b on its own inputs Xb[b] (B x n x d)."""
    Xb, ls, _ = _members(Xb, lengthscales)
    W = _dev(W, "W")
    B, n, d = Xb.shape
    if tuple(W.shape) != (B, n, n):
        raise ValueError(f"kernel_lengthscale_grad_members: W shape {tuple(W.shape)} != {(B, n, n)}")
    g = torch.empty(B, d, dtype=torch.float64, device=Xb.device)
    work = torch.empty(B, n, d, dtype=torch.float64, device=Xb.device)
    call("evr_kernel_lengthscale_grad_members", _stream(), int(kind), B, n, d, Xb.data_ptr(), ls.data_ptr(),
         W.data_ptr(), g.data_ptr(), work.data_ptr())
    return g


def _outputscale(outputscale, B: int) -> torch.Tensor:
    os_ = _dev(outputscale, "outputscale")
    if tuple(os_.shape) != (B,):
        raise ValueError(f"outputscale {tuple(os_.shape)} must hold one value per member ({B})")
    return os_


def kernel_hyper_grad(X, lengthscales, outputscale, W, kind=0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gls B x d, gos B) of the scaled kernel k = outputscale k_base in one pass over W
    (evr_kernel_hyper_grad): gls = outputscale sum W dk_base/dls, gos = sum W k_base."""
    X, ls, W = _dev(X, "X"), _dev(lengthscales, "ls"), _dev(W, "W")
    B, d = ls.shape
    n = X.shape[0]
    if tuple(W.shape) != (B, n, n) or X.shape[1] != d:
        raise ValueError(f"kernel_hyper_grad: X {tuple(X.shape)}, ls {tuple(ls.shape)}, W {tuple(W.shape)} do not match")
    os_ = _outputscale(outputscale, B)
    out = torch.empty(B * (d + 1), dtype=torch.float64, device=X.device)
    work = torch.empty(B, n, d + 1, dtype=torch.float64, device=X.device)
    call("evr_kernel_hyper_grad", _stream(), int(kind), B, n, d, X.data_ptr(), ls.data_ptr(), os_.data_ptr(),
         W.data_ptr(), out.data_ptr(), work.data_ptr())
    return out[:B * d].reshape(B, d), out[B * d:]


def kernel_hyper_grad_members(Xb, nvalid, lengthscales, outputscale, W, kind=0) -> Tuple[torch.Tensor, torch.Tensor]:
    """kernel_hyper_grad with member b on its own rows Xb[b, :nvalid[b]] (the sums skip the padding)."""
    Xb, ls, nvalid = _members(Xb, lengthscales, nvalid)
    W = _dev(W, "W")
    B, n, d = Xb.shape
    if tuple(W.shape) != (B, n, n):
        raise ValueError(f"kernel_hyper_grad_members: W shape {tuple(W.shape)} != {(B, n, n)}")
    os_ = _outputscale(outputscale, B)
    out = torch.empty(B * (d + 1), dtype=torch.float64, device=Xb.device)
    work = torch.empty(B, n, d + 1, dtype=torch.float64, device=Xb.device)
    call("evr_kernel_hyper_grad_members", _stream(), int(kind), B, n, d, Xb.data_ptr(), nvalid.data_ptr(),
         ls.data_ptr(), os_.data_ptr(), W.data_ptr(), out.data_ptr(), work.data_ptr())
    return out[:B * d].reshape(B, d), out[B * d:]


def kernel_matrix_members_scaled(Xb, nvalid, lengthscales, outputscale, kind: int = 0, diag_add=None) -> torch.Tensor:
    """kernel_matrix_members with outputscale[b] on member b's real block; the padding stays the
    identity (evr_kernel_matrix_members_scaled)."""
    Xb, ls, nvalid = _members(Xb, lengthscales, nvalid)
    B, n, d = Xb.shape
    os_ = _outputscale(outputscale, B)
    K = torch.empty(B, n, n, dtype=torch.float64, device=Xb.device)
    dg = None if diag_add is None else _dev(diag_add, "diag_add")
    call("evr_kernel_matrix_members_scaled", _stream(), int(kind), B, n, d, Xb.data_ptr(), nvalid.data_ptr(),
         ls.data_ptr(), os_.data_ptr(), _p(dg), K.data_ptr())
    return K


# limits of the mixed-kernel entry points (include/everest_amd.h)
MIXED_MAX_DC, MIXED_MAX_NC = 32, 8


def _mixed_args(Xc, C, params, name: str):
    Xc, C, params = _dev(Xc, f"{name}: Xc"), _dev(C, f"{name}: C", torch.int32), _dev(params, f"{name}: params")
    if params.dim() == 1:
        params = params.unsqueeze(0)
    if Xc.dim() != 2 or C.dim() != 2 or C.shape[0] != Xc.shape[0] or params.dim() != 2:
        raise ValueError(f"{name}: Xc {tuple(Xc.shape)} must be n x dc, C {tuple(C.shape)} n x nc, params B x P")
    dc, nc = Xc.shape[1], C.shape[1]
    if params.shape[1] != 2 * dc + 2 * nc + 3:
        raise ValueError(f"{name}: params {tuple(params.shape)} must hold 2 dc + 2 nc + 3 = {2 * dc + 2 * nc + 3} "
                         "values per member")
    return Xc, C, params, dc, nc


def _mixed_call(symbol: str, dc: int, nc: int, *args):
    """The native call; sizes the kernels are not built for (the library's own error, never a
    silent fall-through) surface as NotImplementedError."""
    try:
        call(symbol, *args)
    except RuntimeError as e:
        if not (1 <= dc <= MIXED_MAX_DC and 1 <= nc <= MIXED_MAX_NC):
            raise NotImplementedError(str(e)) from e
        raise


def mixed_kernel_matrix(X1c, C1, X2c, C2, params, kind: int = 3, diag_add=None) -> torch.Tensor:
    """K[b] (B x n1 x n2) of the mixed kernel (evr_mixed_kernel_matrix):
    s_sum (k_c(r1) + s_cat h1) + s_prod k_c(r2) h2 (+ diag_add_b on i == j).  X?c: n? x dc normalised
    continuous columns, C?: n? x nc int32 category codes, params: B x (2 dc + 2 nc + 3) =
    [ls1 | ls2 | lam1 | lam2 | s_sum | s_cat | s_prod].  1 <= dc <= 32, 1 <= nc <= 8."""
    X1c, C1, params, dc, nc = _mixed_args(X1c, C1, params, "mixed_kernel_matrix")
    X2c, C2 = _dev(X2c, "mixed_kernel_matrix: X2c"), _dev(C2, "mixed_kernel_matrix: C2", torch.int32)
    if X2c.dim() != 2 or C2.dim() != 2 or X2c.shape[1] != dc or C2.shape[1] != nc or C2.shape[0] != X2c.shape[0]:
        raise ValueError(f"mixed_kernel_matrix: X2c {tuple(X2c.shape)} / C2 {tuple(C2.shape)} do not match "
                         f"dc = {dc}, nc = {nc}")
    B, n1, n2 = params.shape[0], X1c.shape[0], X2c.shape[0]
    K = torch.empty(B, n1, n2, dtype=torch.float64, device=X1c.device)
    dg = None if diag_add is None else _dev(diag_add, "diag_add")
    if dg is not None and dg.numel() != B:
        raise ValueError(f"mixed_kernel_matrix: diag_add holds {dg.numel()} values for {B} members")
    _mixed_call("evr_mixed_kernel_matrix", dc, nc, _stream(), int(kind), B, n1, n2, dc, nc, X1c.data_ptr(),
                C1.data_ptr(), X2c.data_ptr(), C2.data_ptr(), params.data_ptr(), _p(dg), K.data_ptr())
    return K


def mixed_kernel_param_grad(Xc, C, params, W, kind: int = 3) -> torch.Tensor:
    """g[b][p] = sum_ij W[b][i][j] dK_b[i][j] / dparams_p (B x P) in one pass over W (B x n x n, need
    not be symmetric); evr_mixed_kernel_param_grad.  Bitwise reproducible."""
    Xc, C, params, dc, nc = _mixed_args(Xc, C, params, "mixed_kernel_param_grad")
    W = _dev(W, "W")
    B, P = params.shape
    n = Xc.shape[0]
    if tuple(W.shape) != (B, n, n):
        raise ValueError(f"mixed_kernel_param_grad: W shape {tuple(W.shape)} != {(B, n, n)}")
    g = torch.empty(B, P, dtype=torch.float64, device=Xc.device)
    work = torch.empty(B, n, P, dtype=torch.float64, device=Xc.device)
    _mixed_call("evr_mixed_kernel_param_grad", dc, nc, _stream(), int(kind), B, n, dc, nc, Xc.data_ptr(),
                C.data_ptr(), params.data_ptr(), W.data_ptr(), g.data_ptr(), work.data_ptr())
    return g


def _i32(t, name: str) -> torch.Tensor:
    t = _dev(t, name, torch.int32)
    if t.dim() != 1:
        raise ValueError(f"{name} must be a vector, got {tuple(t.shape)}")
    return t


def mixed_split(X, shift, scale, cont_idx, cat_start, cat_len):
    """(Xc rows x dc, Cc rows x nc int32) of raw transformed rows X (rows x d; evr_mixed_split):
    Xc[:, k] = (X[:, cont_idx[k]] - shift[cont_idx[k]]) * scale[cont_idx[k]] and, per one-hot block
    [cat_start[f], cat_start[f] + cat_len[f]), the arg-max, the first on ties.  shift / scale: d-wide."""
    X, shift, scale = _dev(X, "mixed_split: X"), _dev(shift, "mixed_split: shift"), _dev(scale, "mixed_split: scale")
    ci, cs, cl = (_i32(cont_idx, "mixed_split: cont_idx"), _i32(cat_start, "mixed_split: cat_start"),
                  _i32(cat_len, "mixed_split: cat_len"))
    if X.dim() != 2 or shift.numel() != X.shape[1] or scale.numel() != X.shape[1] or cs.numel() != cl.numel():
        raise ValueError(f"mixed_split: X {tuple(X.shape)} must be rows x d with d-wide shift / scale and one "
                         "start and length per block")
    rows, d = X.shape
    dc, nc = ci.numel(), cs.numel()
    Xc = torch.empty(rows, dc, dtype=torch.float64, device=X.device)
    Cc = torch.empty(rows, nc, dtype=torch.int32, device=X.device)
    _mixed_call("evr_mixed_split", dc, nc, _stream(), rows, d, dc, nc, X.data_ptr(), shift.data_ptr(),
                scale.data_ptr(), ci.data_ptr(), cs.data_ptr(), cl.data_ptr(), Xc.data_ptr(), Cc.data_ptr())
    return Xc, Cc


def mixed_kernel_cross_grad(Xc, C, X2c, C2, params, G, scale, cont_idx, kind: int = 3) -> torch.Tensor:
    """dX (rows x d) of the mixed cross-covariance K(train, candidates) given G = dK (B x n x rows):
    the continuous columns' gradient scattered to cont_idx with the factor scale (d-wide, 1 / (hi -
    lo)), every other column exactly 0 (evr_mixed_kernel_cross_grad).  Bitwise reproducible."""
    Xc, C, params, dc, nc = _mixed_args(Xc, C, params, "mixed_kernel_cross_grad")
    X2c, C2 = _dev(X2c, "mixed_kernel_cross_grad: X2c"), _dev(C2, "mixed_kernel_cross_grad: C2", torch.int32)
    G, scale = _dev(G, "G"), _dev(scale, "mixed_kernel_cross_grad: scale")
    ci = _i32(cont_idx, "mixed_kernel_cross_grad: cont_idx")
    B, n, rows, d = params.shape[0], Xc.shape[0], X2c.shape[0], scale.numel()
    if (X2c.dim() != 2 or X2c.shape[1] != dc or tuple(C2.shape) != (rows, nc) or tuple(G.shape) != (B, n, rows)
            or ci.numel() != dc):
        raise ValueError(f"mixed_kernel_cross_grad: X2c {tuple(X2c.shape)} / C2 {tuple(C2.shape)} / G "
                         f"{tuple(G.shape)} / cont_idx ({ci.numel()}) do not match B = {B}, n = {n}, dc = {dc}, "
                         f"nc = {nc}")
    # cont_idx is not read back here (no host sync per call): the reduction only matches column
    # numbers against it, so an index outside the row selects nothing; MixedGPBatch.set_layout
    # validates the map once, on the host
    dX = torch.empty(rows, d, dtype=torch.float64, device=Xc.device)
    lib = _native.load()
    work = _workspace(lib.evr_mixed_kernel_cross_grad_workspace_doubles(n, rows, dc), Xc.device)
    _mixed_call("evr_mixed_kernel_cross_grad", dc, nc, _stream(), int(kind), B, n, rows, d, dc, nc, Xc.data_ptr(),
                C.data_ptr(), X2c.data_ptr(), C2.data_ptr(), params.data_ptr(), scale.data_ptr(), ci.data_ptr(),
                G.data_ptr(), dX.data_ptr(), work.data_ptr())
    return dX


# powers of the dot-product kernel entry points (include/everest_amd.h): 0 = linear, p = polynomial
DOT_MAX_POWER = 8


def _dot_args(G, theta, power, name: str):
    if isinstance(power, bool) or int(power) != power:
        raise ValueError(f"{name}: power must be an integer, got {power!r}")
    G, theta = _dev(G, f"{name}: G"), _dev(theta, f"{name}: theta")
    if G.dim() != 2 or theta.dim() != 1 or theta.numel() < 1:
        raise ValueError(f"{name}: G {tuple(G.shape)} must be n1 x n2 and theta {tuple(theta.shape)} a vector of B >= 1 "
                         "values")
    return G, theta, int(power)


def _dot_call(symbol: str, power: int, *args):
    """The native call; a power the kernels are not built for (the library's own error, never a
    silent fall-through) surfaces as NotImplementedError."""
    try:
        call(symbol, *args)
    except RuntimeError as e:
        if not 0 <= power <= DOT_MAX_POWER:
            raise NotImplementedError(str(e)) from e
        raise


def dot_kernel_apply(G, theta, power: int, diag_add=None) -> torch.Tensor:
    """K[b] (B x n1 x n2) of the dot-product kernels on the Gram matrix G = X1n X2n^T (n1 x n2, shared by
    the members; evr_dot_kernel_apply): power 0 the linear kernel theta_b g, power p in 1..8 the polynomial
    kernel (g + theta_b)^p (+ diag_add_b on i == j).  theta: B values."""
    G, theta, power = _dot_args(G, theta, power, "dot_kernel_apply")
    B, (n1, n2) = theta.numel(), G.shape
    dg = None if diag_add is None else _dev(diag_add, "diag_add")
    if dg is not None and dg.numel() != B:
        raise ValueError(f"dot_kernel_apply: diag_add holds {dg.numel()} values for {B} members")
    K = torch.empty(B, n1, n2, dtype=torch.float64, device=G.device)
    _dot_call("evr_dot_kernel_apply", power, _stream(), power, B, n1, n2, G.data_ptr(), theta.data_ptr(), _p(dg),
              K.data_ptr())
    return K


def dot_kernel_theta_grad(G, theta, W, power: int) -> torch.Tensor:
    """g[b] = sum_ij W[b][i][j] dk/dtheta(G[i][j]; theta_b) (B values) in one pass over W (B x n x n, need
    not be symmetric) and G (n x n); evr_dot_kernel_theta_grad.  Bitwise reproducible."""
    G, theta, power = _dot_args(G, theta, power, "dot_kernel_theta_grad")
    W = _dev(W, "W")
    B, n = theta.numel(), G.shape[0]
    if G.shape[1] != n or tuple(W.shape) != (B, n, n):
        raise ValueError(f"dot_kernel_theta_grad: G {tuple(G.shape)} must be n x n and W {tuple(W.shape)} "
                         f"{(B, n, n)}")
    g = torch.empty(B, dtype=torch.float64, device=G.device)
    if n == 0:
        return g.zero_()
    work = torch.empty(B, n, dtype=torch.float64, device=G.device)
    _dot_call("evr_dot_kernel_theta_grad", power, _stream(), power, B, n, G.data_ptr(), theta.data_ptr(),
              W.data_ptr(), g.data_ptr(), work.data_ptr())
    return g


def dot_gp_posterior(Xn, X, shift, scale, theta, M, power: int, c, ym, ys, noise_add=None):
    """Mean and variance (B x nt) of B dot-product GPs in one native call (evr_dot_gp_posterior): the raw
    rows X (nt x d) are normalised as (X - shift) * scale, K* = f(Xn Xt^T), R = M K* with
    M = [Linv; alpha^T] (B x (n+1) x n), and the prior variance of each test point comes from its own row."""
    if isinstance(power, bool) or int(power) != power:
        raise ValueError(f"dot_gp_posterior: power must be an integer, got {power!r}")
    power = int(power)
    Xn, X, M, theta = _dev(Xn, "Xn"), _dev(X, "X"), _dev(M, "M"), _dev(theta, "theta")
    if M.dim() != 3 or Xn.dim() != 2 or X.dim() != 2 or theta.dim() != 1:
        raise ValueError("dot_gp_posterior: M must be B x (n+1) x n, Xn n x d, X nt x d and theta a vector")
    B, n1, n = M.shape
    nt, d = X.shape
    aux = [_dev(t, "aux") for t in (shift, scale, c, ym, ys)]
    na = None if noise_add is None else _dev(noise_add, "noise")
    if (n1 != n + 1 or tuple(Xn.shape) != (n, d) or theta.numel() != B or aux[0].numel() != d or aux[1].numel() != d
            or any(a.numel() != B for a in aux[2:]) or (na is not None and na.numel() != B)):
        raise ValueError(f"dot_gp_posterior: shape mismatch (M {tuple(M.shape)}, Xn {tuple(Xn.shape)}, X "
                         f"{tuple(X.shape)}, theta {tuple(theta.shape)})")
    mean = torch.empty(B, nt, dtype=torch.float64, device=X.device)
    var = torch.empty_like(mean)
    work = _workspace(_native.load().evr_dot_gp_posterior_workspace_doubles(B, n, nt, d), X.device)
    _dot_call("evr_dot_gp_posterior", power, _stream(), power, B, n, nt, d, Xn.data_ptr(), X.data_ptr(),
              aux[0].data_ptr(), aux[1].data_ptr(), theta.data_ptr(), M.data_ptr(), aux[2].data_ptr(),
              aux[3].data_ptr(), aux[4].data_ptr(), _p(na), mean.data_ptr(), var.data_ptr(), work.data_ptr())
    return mean, var


def mll_terms(L, Linv, r, alpha) -> torch.Tensor:
    """B x 5: logdet, quad, tr(K^-1), sum(alpha), sum(alpha^2)."""
    L, Linv, r, alpha = _dev(L, "L"), _dev(Linv, "Linv"), _dev(r, "r"), _dev(alpha, "alpha")
    B, n, _ = L.shape
    out = torch.empty(B, 5, dtype=torch.float64, device=L.device)
    call("evr_gp_mll_terms", _stream(), B, n, L.data_ptr(), Linv.data_ptr(), r.data_ptr(), alpha.data_ptr(),
         out.data_ptr())
    return out


# ---------------------------------------------------------------------------------------
# dense linear algebra
# ---------------------------------------------------------------------------------------
def gemm(A, B, transA=False, transB=False, alpha=1.0, beta=0.0, out=None) -> torch.Tensor:
    """Batched C = alpha op(A) op(B) + beta C on the f64 MFMA kernel.  A, B: (batch) x r x c."""
    A, B = _dev(A, "A"), _dev(B, "B")
    a3, b3 = A.dim() == 3, B.dim() == 3
    if A.dim() == 2:
        A = A.unsqueeze(0)
    if B.dim() == 2:
        B = B.unsqueeze(0)
    batch = max(A.shape[0], B.shape[0])
    if A.shape[0] not in (1, batch) or B.shape[0] not in (1, batch):
        raise ValueError("gemm: batch mismatch")
    M, K = (A.shape[2], A.shape[1]) if transA else (A.shape[1], A.shape[2])
    K2, N = (B.shape[2], B.shape[1]) if transB else (B.shape[1], B.shape[2])
    if K != K2:
        raise ValueError(f"gemm: inner dims {K} != {K2}")
    if out is None:  # beta = 0: the kernel never reads C
        out = torch.empty(batch, M, N, dtype=torch.float64, device=A.device)
        beta = 0.0
    else:
        if out.dim() == 2:
            out = out.unsqueeze(0)
        if tuple(out.shape) != (batch, M, N) or not out.is_contiguous():
            raise ValueError("gemm: bad out tensor")
    sA = 0 if A.shape[0] == 1 else A.shape[1] * A.shape[2]
    sB = 0 if B.shape[0] == 1 else B.shape[1] * B.shape[2]
    call("evr_gemm_f64", _stream(), int(transA), int(transB), M, N, K, float(alpha), A.data_ptr(), A.shape[2], sA,
         B.data_ptr(), B.shape[2], sB, float(beta), out.data_ptr(), N, M * N, batch)
    return out if (a3 or b3) else out[0]


def gemm_into(out_view: torch.Tensor, A, B, transA=False, transB=False, alpha=1.0, beta=0.0, batch_strides=None):
    """GEMM writing into a strided 2-D/3-D row block (rows contiguous with leading dim ld)."""
    A, B = _dev(A, "A"), _dev(B, "B")
    if A.dim() == 2:
        A = A.unsqueeze(0)
    if B.dim() == 2:
        B = B.unsqueeze(0)
    o = out_view if out_view.dim() == 3 else out_view.unsqueeze(0)
    batch = o.shape[0]
    M, K = (A.shape[2], A.shape[1]) if transA else (A.shape[1], A.shape[2])
    K2, N = (B.shape[2], B.shape[1]) if transB else (B.shape[1], B.shape[2])
    if K != K2 or o.shape[1] != M or o.shape[2] != N or o.stride(2) != 1:
        raise ValueError("gemm_into: shape mismatch")
    sA = 0 if A.shape[0] == 1 else A.stride(0)
    sB = 0 if B.shape[0] == 1 else B.stride(0)
    call("evr_gemm_f64", _stream(), int(transA), int(transB), M, N, K, float(alpha), A.data_ptr(), A.stride(1), sA,
         B.data_ptr(), B.stride(1), sB, float(beta), o.data_ptr(), o.stride(1), o.stride(0), batch)


def cholesky(A: torch.Tensor, jitter0: float = 1e-8, max_tries: int = 3, raise_on_fail: bool = True):
    """psd_safe_cholesky on a batch (B x n x n).  Returns (L, jitter_used[B], info[B])."""
    A = _dev(A, "A")
    squeeze = A.dim() == 2
    if squeeze:
        A = A.unsqueeze(0)
    B, n, n2 = A.shape
    if n != n2:
        raise ValueError("cholesky: matrix not square")
    L = torch.empty_like(A)
    jit = torch.empty(B, dtype=torch.float64, device=A.device)
    info = torch.empty(B, dtype=torch.int32, device=A.device)
    call("evr_cholesky", _stream(), B, n, A.data_ptr(), n, n * n, L.data_ptr(), n, n * n, float(jitter0),
         int(max_tries), jit.data_ptr(), info.data_ptr())
    if raise_on_fail:
        bad = info.cpu()
        if bool(bad.any()):
            raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to "
                              f"{jitter0 * 10 ** (max_tries - 1):.1e} (batch members {bad.nonzero().view(-1).tolist()})")
    if squeeze:
        return L[0], jit[0], info[0]
    return L, jit, info


def cholesky_inverse(A: torch.Tensor, jitter0: float = 1e-8, max_tries: int = 3, raise_on_fail: bool = True):
    """(L, L^-1, jitter_used, info) from one blocked pass (psd_safe_cholesky semantics)."""
    A = _dev(A, "A")
    squeeze = A.dim() == 2
    if squeeze:
        A = A.unsqueeze(0)
    B, n, n2 = A.shape
    if n != n2:
        raise ValueError("cholesky_inverse: matrix not square")
    L = torch.empty_like(A)
    Li = torch.empty_like(A)
    jit = torch.empty(B, dtype=torch.float64, device=A.device)
    info = torch.empty(B, dtype=torch.int32, device=A.device)
    call("evr_cholesky_inverse", _stream(), B, n, A.data_ptr(), n, n * n, L.data_ptr(), n, n * n, Li.data_ptr(), n,
         n * n, float(jitter0), int(max_tries), jit.data_ptr(), info.data_ptr())
    if raise_on_fail:
        bad = info.cpu()
        if bool(bad.any()):
            raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to "
                              f"{jitter0 * 10 ** (max_tries - 1):.1e} (batch members {bad.nonzero().view(-1).tolist()})")
    if squeeze:
        return L[0], Li[0], jit[0], info[0]
    return L, Li, jit, info


def trsm(L: torch.Tensor, B: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """In place: B <- L^-1 B (or L^-T B).  L: (batch) x n x n, B: (batch) x n x nrhs."""
    L = _dev(L, "L")
    if not B.is_contiguous() or B.dtype != torch.float64 or B.device.type != "cuda":
        raise ValueError("trsm: B must be a contiguous float64 device tensor (solved in place)")
    L3 = L if L.dim() == 3 else L.unsqueeze(0)
    B3 = B if B.dim() == 3 else B.unsqueeze(0)
    batch = B3.shape[0]
    n = L3.shape[1]
    nrhs = B3.shape[2]
    sL = 0 if L3.shape[0] == 1 else n * n
    call("evr_trsm_lower", _stream(), batch, n, nrhs, L3.data_ptr(), n, sL, int(transpose), B3.data_ptr(), nrhs,
         n * nrhs)
    return B


def tri_inv(L: torch.Tensor) -> torch.Tensor:
    L = _dev(L, "L")
    L3 = L if L.dim() == 3 else L.unsqueeze(0)
    batch, n, _ = L3.shape
    out = torch.empty_like(L3)
    call("evr_tri_inv_lower", _stream(), batch, n, L3.data_ptr(), n, n * n, out.data_ptr(), n, n * n)
    return out if L.dim() == 3 else out[0]


def posterior_finalize(R, c, ym, ys, kxx, noise_add=None):
    R = _dev(R, "R")
    B, n1, nt = R.shape
    mean = torch.empty(B, nt, dtype=torch.float64, device=R.device)
    var = torch.empty_like(mean)
    args = [_dev(t, "aux") for t in (c, ym, ys, kxx)]
    na = None if noise_add is None else _dev(noise_add, "noise")
    call("evr_gp_posterior_finalize", _stream(), B, n1 - 1, nt, R.data_ptr(), *[a.data_ptr() for a in args],
         _p(na), mean.data_ptr(), var.data_ptr())
    return mean, var


def gp_posterior(Xn, X, shift, scale, lengthscales, M, kind, c, ym, ys, kxx, noise_add=None):
    """Mean and variance (B x nt) in one native call: kernel_matrix -> R = M K_x -> finalize."""
    Xn, X, M = _dev(Xn, "Xn"), _dev(X, "X"), _dev(M, "M")
    B, n1, n = M.shape
    nt, d = X.shape
    if n1 != n + 1 or Xn.shape != (n, d):
        raise ValueError("gp_posterior: shape mismatch")
    mean = torch.empty(B, nt, dtype=torch.float64, device=X.device)
    var = torch.empty_like(mean)
    work = _workspace(_native.load().evr_gp_posterior_workspace_doubles(B, n, nt), X.device)
    aux = [_dev(t, "aux") for t in (shift, scale, lengthscales, c, ym, ys, kxx)]
    na = None if noise_add is None else _dev(noise_add, "noise")
    call("evr_gp_posterior", _stream(), B, n, nt, d, int(kind), Xn.data_ptr(), X.data_ptr(), aux[0].data_ptr(),
         aux[1].data_ptr(), aux[2].data_ptr(), M.data_ptr(), aux[3].data_ptr(), aux[4].data_ptr(), aux[5].data_ptr(),
         aux[6].data_ptr(), _p(na), mean.data_ptr(), var.data_ptr(), work.data_ptr())
    return mean, var


# ---------------------------------------------------------------------------------------
# qNEHVI pieces
# ---------------------------------------------------------------------------------------
def make_state(n, nb, S, m, c, ym, ys, kxx, zq, obj_a, obj_b, cells: "Cells", no_h: bool = False) -> EvrQnehviState:
    """no_h: the operator M carries no H^T rows (qEHVI: samples mu + L22 z, nb = 0)."""
    st = EvrQnehviState()
    st.n, st.nb, st.S, st.m = int(n), int(nb), int(S), int(m)
    st.no_h = int(bool(no_h))
    st.c, st.ym, st.ys, st.kxx = c.data_ptr(), ym.data_ptr(), ys.data_ptr(), kxx.data_ptr()
    st.zq, st.obj_a, st.obj_b = zq.data_ptr(), obj_a.data_ptr(), obj_b.data_ptr()
    st.cell_lo, st.cell_hi = _p(cells.lo), _p(cells.hi)
    st.cell_off = cells.off.data_ptr()
    st.max_cells = int(cells.max_cells)
    st.cell_keys, st.cell_pts, st.cell_rank0 = _p(cells.keys), _p(cells.pts), _p(cells.rank0)
    st.pts_stride = int(cells.stride)
    kd = cells.kd
    if kd is not None:
        st.grp_off, st.grp_keys, st.grp_rank = kd.goff.data_ptr(), kd.keys.data_ptr(), kd.rank.data_ptr()
        st.grp_box, st.sorted_lo, st.max_groups = kd.box.data_ptr(), kd.sorted_lo.data_ptr(), int(kd.max_groups)
    return st


def qnehvi_samples(st: EvrQnehviState, R: torch.Tensor, b: int):
    dev = R.device
    G = torch.empty(st.S, st.m, b, dtype=torch.float64, device=dev)
    L22 = torch.empty(st.m, b, dtype=torch.float64, device=dev)
    flags = torch.empty(st.m, b, dtype=torch.int32, device=dev)
    call("evr_qnehvi_samples", _stream(), ctypes.byref(st), b, R.data_ptr(), G.data_ptr(), L22.data_ptr(),
         flags.data_ptr())
    return G, L22, flags


def qnehvi_project(st: EvrQnehviState, M: torch.Tensor, Kx: torch.Tensor, b: int):
    """R = M Kx (m x Rr x b) and the partial norms the sampling step needs (one fused GEMM)."""
    dev = Kx.device
    Rr = st.n + st.nb + (0 if st.no_h else st.S) + 1
    R = torch.empty(st.m, Rr, b, dtype=torch.float64, device=dev)
    nrt = _native.load().evr_qnehvi_norms_rows(ctypes.byref(st))
    P = torch.empty(st.m, nrt, 2, b, dtype=torch.float64, device=dev)
    work = _workspace(_native.load().evr_qnehvi_project_workspace_doubles(ctypes.byref(st), b), dev)
    call("evr_qnehvi_project", _stream(), ctypes.byref(st), b, _dev(M, "M").data_ptr(), _dev(Kx, "Kx").data_ptr(),
         R.data_ptr(), P.data_ptr(), work.data_ptr())
    return R, P


def qnehvi_samples_norms(st: EvrQnehviState, R: torch.Tensor, P: torch.Tensor, b: int):
    dev = R.device
    G = torch.empty(st.S, st.m, b, dtype=torch.float64, device=dev)
    L22 = torch.empty(st.m, b, dtype=torch.float64, device=dev)
    flags = torch.empty(st.m, b, dtype=torch.int32, device=dev)
    call("evr_qnehvi_samples_norms", _stream(), ctypes.byref(st), b, R.data_ptr(), P.data_ptr(), G.data_ptr(),
         L22.data_ptr(), flags.data_ptr())
    return G, L22, flags


def qnehvi_project_backward(st: EvrQnehviState, M: torch.Tensor, R: torch.Tensor, L22: torch.Tensor,
                            dG: torch.Tensor, b: int) -> torch.Tensor:
    """dKx = M^T gR (m x n x b) with gR generated inside the GEMM."""
    dK = torch.empty(st.m, st.n, b, dtype=torch.float64, device=R.device)
    work = _workspace(_native.load().evr_qnehvi_project_backward_workspace_doubles(ctypes.byref(st), b), R.device)
    call("evr_qnehvi_project_backward", _stream(), ctypes.byref(st), b, M.data_ptr(), R.data_ptr(), L22.data_ptr(),
         dG.data_ptr(), dK.data_ptr(), work.data_ptr())
    return dK


def qnehvi_small_applies(st: EvrQnehviState, b: int, d: int) -> bool:
    """Whether the native plan runs the b <= 32 restart-batch kernels (qnehvi_small.hip) for
    this batch (EVR_SMALL=0 disables them, as in the plan)."""
    return (os.environ.get("EVR_SMALL", "1") != "0"
            and bool(_native.load().evr_qnehvi_small_applies(ctypes.byref(st), int(b), int(d))))


def qnehvi_small_forward(st: EvrQnehviState, model, Kx: torch.Tensor, b: int):
    """Restart-batch projection: R = M Kx and 16-row-tile partial norms (qs_fwd)."""
    dev = Kx.device
    lib = _native.load()
    Rr = st.n + st.nb + (0 if st.no_h else st.S) + 1
    R = torch.empty(st.m, Rr, b, dtype=torch.float64, device=dev)
    P = _workspace(lib.evr_qnehvi_small_workspace_doubles(ctypes.byref(st), b, model.d, 0), dev)
    call("evr_qnehvi_small_forward", _stream(), ctypes.byref(st), ctypes.byref(model), b,
         _dev(Kx, "Kx").data_ptr(), R.data_ptr(), P.data_ptr())
    return R, P


def qnehvi_small_samples(st: EvrQnehviState, R: torch.Tensor, P: torch.Tensor, b: int):
    dev = R.device
    G = torch.empty(st.S, st.m, b, dtype=torch.float64, device=dev)
    L22 = torch.empty(st.m, b, dtype=torch.float64, device=dev)
    flags = torch.empty(st.m, b, dtype=torch.int32, device=dev)
    call("evr_qnehvi_small_samples", _stream(), ctypes.byref(st), b, R.data_ptr(), P.data_ptr(), G.data_ptr(),
         L22.data_ptr(), flags.data_ptr())
    return G, L22, flags


def qnehvi_small_backward(st: EvrQnehviState, model, X: torch.Tensor, R: torch.Tensor, L22: torch.Tensor,
                          dG: torch.Tensor, b: int) -> torch.Tensor:
    """Restart-batch backward: dX (b x d) = d sum acq / dX with the cross-covariance gradient
    fused into the M^T gR product (qs_bwd + qs_dx_reduce)."""
    dev = R.device
    lib = _native.load()
    dXp = _workspace(lib.evr_qnehvi_small_workspace_doubles(ctypes.byref(st), b, model.d, 1), dev)
    dX = torch.empty(b, model.d, dtype=torch.float64, device=dev)
    call("evr_qnehvi_small_backward", _stream(), ctypes.byref(st), ctypes.byref(model), b,
         _dev(X, "X").contiguous().data_ptr(), R.data_ptr(), L22.data_ptr(), dG.data_ptr(), dXp.data_ptr(),
         dX.data_ptr())
    return dX


OBJ_AFFINE, OBJ_CLOSE_TO_TARGET = 0, 1


class GeneralSpec:
    """Objectives over selected model outputs and output constraints for the general
    qNEHVI / qEHVI kernels (qnehvi_general.hip, evr_qn_general).

    objectives: [(output, kind, p0, p1)] — kind OBJ_AFFINE: g = p0*y + p1 (Maximize /
    Minimize, bofire/utils/torch_tools.py:389-398), OBJ_CLOSE_TO_TARGET: g = -|y - p0|^p1
    (:399-402).  constraints: [(output, sign, threshold, eta)] — c = sign*(y - threshold)
    <= 0 is feasible, weight exp(sum logsigmoid(-c/eta)) (torch_tools.py:258-337)."""

    def __init__(self, m_model: int, objectives, constraints=()):
        self.m_model = int(m_model)
        self.objectives = [(int(o), int(k), float(a), float(b)) for o, k, a, b in objectives]
        self.constraints = [(int(o), float(sg), float(t), float(e)) for o, sg, t, e in constraints]
        if not 1 <= len(self.objectives) <= 8 or len(self.constraints) > 16:
            raise ValueError("general qNEHVI: 1..8 objectives and at most 16 output constraints")
        for o, *_ in self.objectives + self.constraints:
            if not 0 <= o < self.m_model:
                raise ValueError(f"general qNEHVI: output index {o} outside the model's {self.m_model} outputs")
        ob = self.objectives
        self._arrs = (np.array([o[0] for o in ob], np.int32), np.array([o[1] for o in ob], np.int32),
                      np.array([o[2] for o in ob], np.float64), np.array([o[3] for o in ob], np.float64))
        cs = self.constraints or [(0, 0.0, 0.0, 1.0)]
        self._carrs = (np.array([c[0] for c in cs], np.int32), np.array([c[1] for c in cs], np.float64),
                       np.array([c[2] for c in cs], np.float64), np.array([c[3] for c in cs], np.float64))

    @property
    def m_obj(self) -> int:
        return len(self.objectives)

    @property
    def affine_identity(self) -> bool:
        """Every output carries one affine objective, in output order, and no constraints:
        the q = 1 fast path (obj_a / obj_b fused into the sampling kernel) applies."""
        return (not self.constraints and self.m_obj == self.m_model and
                all(o == j and k == OBJ_AFFINE for j, (o, k, _, _) in enumerate(self.objectives)))

    def struct(self, q: int = 1, zq: Optional[torch.Tensor] = None) -> EvrQnGeneral:
        g = EvrQnGeneral()
        g.q, g.m_obj, g.n_con = int(q), self.m_obj, len(self.constraints)
        g.obj_out, g.obj_kind, g.obj_p0, g.obj_p1 = (a.ctypes.data for a in self._arrs)
        g.con_out, g.con_sign, g.con_thr, g.con_eta = (a.ctypes.data for a in self._carrs)
        g.zq = _p(zq)
        return g

    def host_weights(self, Y: np.ndarray) -> np.ndarray:
        """Smoothed feasibility weights exp(sum_c logsigmoid(-c / eta)) of model-output rows Y
        (... x m_model) on the host ([upstream] compute_smoothed_feasibility_indicator,
        fat=False); 1 without constraints."""
        lw = np.zeros(Y.shape[:-1])
        for o, sg, t, eta in self.constraints:
            x = -sg * (Y[..., o] - t) / eta
            lw += np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))
        return np.exp(lw)

    def host_objective(self, Y: np.ndarray) -> np.ndarray:
        """Objectives of model-output rows Y (... x m_model) on the host (observed data)."""
        cols = []
        for o, k, a, b in self.objectives:
            y = Y[..., o]
            cols.append(a * y + b if k == OBJ_AFFINE else -np.abs(y - a) ** b)
        return np.stack(cols, -1)


def objective_general(Y: torch.Tensor, mu: Optional[torch.Tensor], spec: GeneralSpec, ref: torch.Tensor):
    """Y: m_model x n x S (+ mu m_model x n) -> objectives m_obj x n x S, infeasible samples
    (any constraint c > 0) set to the reference point."""
    Y = _dev(Y, "Y")
    m, n, S = Y.shape
    O = torch.empty(spec.m_obj, n, S, dtype=torch.float64, device=Y.device)
    g = spec.struct()
    call("evr_objective_general", _stream(), m, n, S, ctypes.byref(g), Y.data_ptr(),
         _p(None if mu is None else _dev(mu, "mu")), _dev(ref, "ref").data_ptr(), O.data_ptr())
    return O


def objective_weights(Y: torch.Tensor, spec: GeneralSpec):
    """Y: m_model x n model-output rows on device -> (objectives m_obj x n, feasibility
    weights n) through the general scan's per-point device function (evr_objective_weights)."""
    Y = _dev(Y, "Y")
    m, n = Y.shape
    if m != spec.m_model:
        raise ValueError(f"Y has {m} outputs, the spec {spec.m_model}")
    G = torch.empty(spec.m_obj, n, dtype=torch.float64, device=Y.device)
    W = torch.empty(n, dtype=torch.float64, device=Y.device)
    g = spec.struct()
    call("evr_objective_weights", _stream(), m, n, ctypes.byref(g), Y.data_ptr(), G.data_ptr(), W.data_ptr())
    return G, W


def qng_eval(stm: EvrQnehviState, sth: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel",
             X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """General qNEHVI / qEHVI: X (b*q) x d raw candidates (point i of candidate c at row
    c*q + i) -> acq (b) [, dX (b*q) x d]."""
    X = _dev(X, "X")
    q = int(g.q)
    bq, d = X.shape
    if bq % q:
        raise ValueError(f"{bq} rows are not a multiple of q = {q}")
    b = bq // q
    lib = _native.load()
    work = _workspace(lib.evr_qng_workspace_doubles(ctypes.byref(stm), ctypes.byref(sth), ctypes.byref(g),
                                                    ctypes.byref(model), b, int(backward)), X.device)
    acq = torch.empty(b, dtype=torch.float64, device=X.device)
    dX = torch.empty_like(X) if backward else None
    call("evr_qng_eval", _stream(), ctypes.byref(stm), ctypes.byref(sth), ctypes.byref(g), ctypes.byref(model), b,
         X.data_ptr(), _p(None if gout is None else _dev(gout, "gout")), work.data_ptr(), acq.data_ptr(), _p(dX))
    return acq, dX


def qlog_eval(stm: EvrQnehviState, sth: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel",
              X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """Log-space general qLogNEHVI / qLogEHVI (evr_qlog_eval): X (b*q) x d raw candidates ->
    acq (b) [, dX (b*q) x d]; ``sth`` carries the explicit cells and tau_relu / tau_max."""
    X = _dev(X, "X")
    q = int(g.q)
    bq, d = X.shape
    if bq % q:
        raise ValueError(f"{bq} rows are not a multiple of q = {q}")
    b = bq // q
    lib = _native.load()
    work = _workspace(lib.evr_qlog_workspace_doubles(ctypes.byref(stm), ctypes.byref(sth), ctypes.byref(g),
                                                     ctypes.byref(model), b, int(backward)), X.device)
    acq = torch.empty(b, dtype=torch.float64, device=X.device)
    dX = torch.empty_like(X) if backward else None
    call("evr_qlog_eval", _stream(), ctypes.byref(stm), ctypes.byref(sth), ctypes.byref(g), ctypes.byref(model), b,
         X.data_ptr(), _p(None if gout is None else _dev(gout, "gout")), work.data_ptr(), acq.data_ptr(), _p(dX))
    return acq, dX


def model_state(n, nb, S, c, ym, ys, kxx, no_h: bool = False, m: int = 1) -> EvrQnehviState:
    """Model-side state of a chain without cells (evr_qnei_eval: m = 1; evr_qsobo_eval: m model
    outputs): the operator layout (n, nb, S, no_h) and the per-output constant / standardisation
    / prior variance."""
    st = EvrQnehviState()
    st.n, st.nb, st.S, st.m = int(n), int(nb), int(S), int(m)
    st.no_h = int(bool(no_h))
    st.c, st.ym, st.ys, st.kxx = c.data_ptr(), ym.data_ptr(), ys.data_ptr(), kxx.data_ptr()
    return st


def _improvement(st, log: bool, tau_relu: float, tau_max: float, best: torch.Tensor):
    """The head the improvement scans' structs share: log mode, temperatures and ``best`` (device;
    S per-sample incumbents, or one value: stride 0).  Returns st."""
    best = _dev(best, "best")
    st.log, st.tau_relu, st.tau_max = int(bool(log)), float(tau_relu), float(tau_max)
    st.best, st.best_stride = best.data_ptr(), 0 if best.numel() == 1 else 1
    return st


def nei_struct(log: bool, tau_relu: float, tau_max: float, best: torch.Tensor) -> "_native.EvrNei":
    """evr_nei over ``best`` (device; S per-sample incumbents, or one value: stride 0)."""
    return _improvement(_native.EvrNei(), log, tau_relu, tau_max, best)


def nei_scan(Y: torch.Tensor, q: int, best: torch.Tensor, obj_a: float, obj_b: float, log: bool = False,
             tau_relu: float = 1e-6, tau_max: float = 1e-2, flags: Optional[torch.Tensor] = None,
             gout: Optional[torch.Tensor] = None, backward: bool = False):
    """Improvement scan alone (evr_nei_scan): Y S x (b*q) joint samples (point i of candidate c
    at column c*q + i), best S incumbents or one -> (acq (b), dY S x (b*q) | None)."""
    Y, best = _dev(Y, "Y"), _dev(best, "best")
    S, bq = Y.shape
    q = int(q)
    if q < 1 or bq % q:
        raise ValueError(f"{bq} columns are not a multiple of q = {q}")
    if best.numel() not in (1, S):
        raise ValueError(f"best needs 1 or S = {S} values, got {best.numel()}")
    b = bq // q
    flags = None if flags is None else _dev(flags, "flags", torch.int32)
    gout = None if gout is None else _dev(gout, "gout")
    if (flags is not None and flags.numel() != b) or (gout is not None and gout.numel() != b):
        raise ValueError("flags / gout need one entry per candidate")
    acq = torch.empty(b, dtype=torch.float64, device=Y.device)
    dY = torch.empty_like(Y) if backward else None
    call("evr_nei_scan", _stream(), q, int(bool(log)), S, b, Y.data_ptr(), best.data_ptr(),
         0 if best.numel() == 1 else 1, float(obj_a), float(obj_b), float(tau_relu), float(tau_max), _p(flags),
         _p(gout), acq.data_ptr(), _p(dY))
    return acq, dY


def qnei_eval(stm: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel", nei: "_native.EvrNei",
              X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """qNEI / qLogNEI / qLogEI (evr_qnei_eval): X (b*q) x d raw candidates -> acq (b)
    [, dX (b*q) x d]."""
    return _utility_eval("evr_qnei", stm, g, model, nei, X, backward, gout)


OBJ_SIGMOID, OBJ_TARGET = 2, 3


def _table_arrays(terms, constraints):
    """Host arrays of a spec's term rows (out, kind, four doubles) and constraint rows (out, sign,
    thr, eta), column by column; without constraints one placeholder row keeps the pointers valid."""
    tarrs = (np.array([t[0] for t in terms], np.int32), np.array([t[1] for t in terms], np.int32)) + tuple(
        np.array([t[i] for t in terms], np.float64) for i in (2, 3, 4, 5))
    cs = constraints or [(0, 0.0, 0.0, 1.0)]
    carrs = (np.array([c[0] for c in cs], np.int32), np.array([c[1] for c in cs], np.float64),
             np.array([c[2] for c in cs], np.float64), np.array([c[3] for c in cs], np.float64))
    return tarrs, carrs


def _point_tables(st, spec):
    """The fields every scan struct names alike: the table sizes and the constraint columns."""
    st.n_term, st.n_con = len(spec.terms), len(spec.constraints)
    st.con_out, st.con_sign, st.con_thr, st.con_eta = (a.ctypes.data for a in spec._carrs)


class SoboSpec:
    """Scalarised utility over model outputs with output constraints for the single-objective
    scan (sobo_scan.hip, evr_sobo): u(y) = sum_t w_t g_t(y[out_t]).

    terms: [(output, kind, w, p0, p1, p2)] — OBJ_AFFINE p0*y + p1, OBJ_CLOSE_TO_TARGET
    -|y - p0|^p1, OBJ_SIGMOID 1/(1+exp(-p0*(y-p1))) (p0 = +steepness MaximizeSigmoid,
    -steepness MinimizeSigmoid), OBJ_TARGET sig(p0*(y-(p1-p2))) * (1 - sig(p0*(y-(p1+p2))))
    (bofire/utils/torch_tools.py:384-450).  constraints: [(output, sign, threshold, eta)] as in
    ``GeneralSpec``."""

    def __init__(self, m_model: int, terms, constraints=()):
        self.m_model = int(m_model)
        self.terms = [(int(o), int(k), float(w), float(a), float(b), float(c)) for o, k, w, a, b, c in terms]
        self.constraints = [(int(o), float(sg), float(t), float(e)) for o, sg, t, e in constraints]
        if not 1 <= len(self.terms) <= 8 or len(self.constraints) > 16:
            raise ValueError("sobo scan: 1..8 terms and at most 16 output constraints")
        for o, *_ in self.terms + self.constraints:
            if not 0 <= o < self.m_model:
                raise ValueError(f"sobo scan: output index {o} outside the model's {self.m_model} outputs")
        for _, k, *_ in self.terms:
            if k not in (OBJ_AFFINE, OBJ_CLOSE_TO_TARGET, OBJ_SIGMOID, OBJ_TARGET):
                raise ValueError(f"sobo scan: term kind {k}")
        self._tarrs, self._carrs = _table_arrays(self.terms, self.constraints)

    def struct(self, log: bool, tau_relu: float, tau_max: float, best: torch.Tensor) -> "_native.EvrSobo":
        """evr_sobo over ``best`` (device; S per-sample incumbents, or one value: stride 0).  The
        struct points into this spec's host arrays and into ``best``: keep both alive."""
        sb = _improvement(_native.EvrSobo(), log, tau_relu, tau_max, best)
        _point_tables(sb, self)
        (sb.term_out, sb.term_kind, sb.term_w, sb.term_p0, sb.term_p1,
         sb.term_p2) = (a.ctypes.data for a in self._tarrs)
        return sb

    @staticmethod
    def _term(k: int, a: float, b: float, c: float, y):
        xp = torch if isinstance(y, torch.Tensor) else np
        if k == OBJ_AFFINE:
            return a * y + b
        if k == OBJ_CLOSE_TO_TARGET:
            return -xp.abs(y - a) ** b
        if k == OBJ_SIGMOID:
            return 1.0 / (1.0 + xp.exp(-a * (y - b)))
        return 1.0 / (1.0 + xp.exp(-a * (y - (b - c)))) * (1.0 - 1.0 / (1.0 + xp.exp(-a * (y - (b + c)))))

    def utility(self, Y):
        """u of model-output rows Y (... x m_model; numpy array or torch tensor)."""
        u = 0.0
        for o, k, w, a, b, c in self.terms:
            u = u + w * self._term(k, a, b, c, Y[..., o])
        return u

    def feasible(self, Y):
        """Hard feasibility (every c <= 0) of model-output rows Y (... x m_model)."""
        xp = torch if isinstance(Y, torch.Tensor) else np
        ok = xp.ones_like(Y[..., 0]) > 0
        for o, sg, t, _ in self.constraints:
            ok = ok & (sg * (Y[..., o] - t) <= 0)
        return ok


def sobo_scan(Y: torch.Tensor, q: int, best: torch.Tensor, spec: SoboSpec, log: bool = False,
              tau_relu: float = 1e-6, tau_max: float = 1e-2, flags: Optional[torch.Tensor] = None,
              gout: Optional[torch.Tensor] = None, backward: bool = False):
    """Scalarised, constraint-weighted scan alone (evr_sobo_scan): Y S x m_model x (b*q) joint
    samples (point i of candidate c at column c*q + i), best S incumbents or one ->
    (acq (b), dY like Y | None).  flags: m_model x b."""
    return _utility_scan("evr_sobo_scan", Y, q, best, spec, log, tau_relu, tau_max, flags, gout, backward)


def _scan_args(Y, q, spec, flags, gout):
    """The checks the scans over several model outputs share: Y (S x m_model x (b*q)) against the
    spec and q, flags (m_model x b) and gout (b).  Returns (Y, q, b, flags, gout) as the call
    takes them."""
    Y = _dev(Y, "Y")
    S, m, bq = Y.shape
    q = int(q)
    if m != spec.m_model:
        raise ValueError(f"Y has {m} outputs, the spec {spec.m_model}")
    if q < 1 or bq % q:
        raise ValueError(f"{bq} columns are not a multiple of q = {q}")
    b = bq // q
    flags = None if flags is None else _dev(flags, "flags", torch.int32)
    gout = None if gout is None else _dev(gout, "gout")
    if (flags is not None and flags.numel() != m * b) or (gout is not None and gout.numel() != b):
        raise ValueError("flags need one entry per (output, candidate), gout one per candidate")
    return Y, q, b, flags, gout


def _utility_scan(symbol: str, Y, q, best, spec, log, tau_relu, tau_max, flags, gout, backward):
    Y, q, b, flags, gout = _scan_args(Y, q, spec, flags, gout)
    S, m, _ = Y.shape
    best = _dev(best, "best")
    if best.numel() not in (1, S):
        raise ValueError(f"best needs 1 or S = {S} values, got {best.numel()}")
    acq = torch.empty(b, dtype=torch.float64, device=Y.device)
    dY = torch.empty_like(Y) if backward else None
    sb = spec.struct(log, tau_relu, tau_max, best)
    call(symbol, _stream(), q, m, S, b, ctypes.byref(sb), Y.data_ptr(), _p(flags), _p(gout),
         acq.data_ptr(), _p(dY))
    return acq, dY


def qsobo_eval(stm: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel", sb: "_native.EvrSobo",
               X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """Constrained / scalarised qNEI, qLogNEI, qLogEI, qEI over m model outputs (evr_qsobo_eval):
    X (b*q) x d raw candidates -> acq (b) [, dX (b*q) x d]."""
    return _utility_eval("evr_qsobo", stm, g, model, sb, X, backward, gout)


def _utility_eval(prefix: str, stm, g, model, sb, X, backward, gout):
    X = _dev(X, "X")
    q = int(g.q)
    bq, d = X.shape
    if bq % q:
        raise ValueError(f"{bq} rows are not a multiple of q = {q}")
    b = bq // q
    lib = _native.load()
    work = _workspace(getattr(lib, prefix + "_workspace_doubles")(ctypes.byref(stm), ctypes.byref(g),
                                                                  ctypes.byref(model), b, int(backward)), X.device)
    acq = torch.empty(b, dtype=torch.float64, device=X.device)
    dX = torch.empty_like(X) if backward else None
    call(prefix + "_eval", _stream(), ctypes.byref(stm), ctypes.byref(g), ctypes.byref(model), ctypes.byref(sb), b,
         X.data_ptr(), _p(None if gout is None else _dev(gout, "gout")), work.data_ptr(), acq.data_ptr(), _p(dX))
    return acq, dX


class ParegoSpec:
    """Augmented Chebyshev utility over model outputs with output constraints for the qParEGO scan
    (parego_scan.hip, evr_parego): t_k(y) = A_k g_k(y[out_k]) + B_k,
    u(y) = min_k t_k(y) + alpha sum_k t_k(y).

    terms: [(output, kind, p0, p1, A, B)] — OBJ_AFFINE p0*y + p1 or OBJ_CLOSE_TO_TARGET
    -|y - p0|^p1, A > 0.  constraints: [(output, sign, threshold, eta)] as in ``SoboSpec``, whose
    interface this class has (struct / utility / feasible)."""

    def __init__(self, m_model: int, terms, alpha: float, constraints=()):
        self.m_model = int(m_model)
        self.alpha = float(alpha)
        self.terms = [(int(o), int(k), float(p0), float(p1), float(A), float(B)) for o, k, p0, p1, A, B in terms]
        self.constraints = [(int(o), float(sg), float(t), float(e)) for o, sg, t, e in constraints]
        if not 2 <= len(self.terms) <= 8 or len(self.constraints) > 16:
            raise ValueError("parego scan: 2..8 terms and at most 16 output constraints")
        if not self.alpha >= 0.0:
            raise ValueError(f"parego scan: alpha = {self.alpha} is negative")
        for o, *_ in self.terms + self.constraints:
            if not 0 <= o < self.m_model:
                raise ValueError(f"parego scan: output index {o} outside the model's {self.m_model} outputs")
        for _, k, _, _, A, _ in self.terms:
            if k not in (OBJ_AFFINE, OBJ_CLOSE_TO_TARGET):
                raise ValueError(f"parego scan: term kind {k}")
            if not A > 0.0:
                raise ValueError(f"parego scan: term scale A = {A} must be positive")
        self._tarrs, self._carrs = _table_arrays(self.terms, self.constraints)

    def struct(self, log: bool, tau_relu: float, tau_max: float, best: torch.Tensor) -> "_native.EvrParego":
        """evr_parego over ``best`` (device; S per-sample incumbents, or one value: stride 0).  The
        struct points into this spec's host arrays and into ``best``: keep both alive."""
        pg = _improvement(_native.EvrParego(), log, tau_relu, tau_max, best)
        pg.alpha = self.alpha
        _point_tables(pg, self)
        (pg.term_out, pg.term_kind, pg.term_p0, pg.term_p1, pg.term_a,
         pg.term_b) = (a.ctypes.data for a in self._tarrs)
        return pg

    def term_values(self, Y):
        """The terms t_k of model-output rows Y (... x m_model), stacked on a new last axis."""
        xp = torch if isinstance(Y, torch.Tensor) else np
        return xp.stack([A * SoboSpec._term(k, p0, p1, 0.0, Y[..., o]) + B for o, k, p0, p1, A, B in self.terms], -1)

    def utility(self, Y):
        """u of model-output rows Y (... x m_model; numpy array or torch tensor)."""
        t = self.term_values(Y)
        mn = t.min(-1)
        if isinstance(Y, torch.Tensor):
            mn = mn.values
        return mn + self.alpha * t.sum(-1)

    def term_slopes(self, Y) -> np.ndarray:
        """d u / d t_k of model-output rows Y (numpy, ... x m_model) as the scan's backward takes
        it: alpha + [k == k*], k* the FIRST arg-min (the lowest term index on ties)."""
        t = self.term_values(np.asarray(Y, dtype=np.float64))
        first = np.argmin(t, axis=-1)               # numpy: the first occurrence of the minimum
        return self.alpha + (np.arange(t.shape[-1]) == first[..., None])

    feasible = SoboSpec.feasible


def parego_scan(Y: torch.Tensor, q: int, best: torch.Tensor, spec: ParegoSpec, log: bool = False,
                tau_relu: float = 1e-6, tau_max: float = 1e-2, flags: Optional[torch.Tensor] = None,
                gout: Optional[torch.Tensor] = None, backward: bool = False):
    """Augmented Chebyshev, constraint-weighted scan alone (evr_parego_scan); arguments and results
    as ``sobo_scan``."""
    return _utility_scan("evr_parego_scan", Y, q, best, spec, log, tau_relu, tau_max, flags, gout, backward)


def qparego_eval(stm: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel", pg: "_native.EvrParego",
                 X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """qParEGO's qNEI, qLogNEI, qLogEI, qEI over m model outputs (evr_qparego_eval):
    X (b*q) x d raw candidates -> acq (b) [, dX (b*q) x d]."""
    return _utility_eval("evr_qparego", stm, g, model, pg, X, backward, gout)


class MultSpec:
    """Multiplicative / multiplicative-additive utility over model outputs for the scan of
    mult_scan.hip (evr_mult):

        u(y) = [prod_k g_k(y[out_k]) ** w_k] * [1 + sum_a w_a g_a(y[out_a])]

    factors / addends: [(output, kind, w, p0, p1, p2)] with the kinds and parameters of
    ``SoboSpec``; either list may be empty, not both, and they hold 8 rows at most together.  A
    factor's weight is finite and >= 1 (the normalised weights of bofire/utils/torch_tools.py:
    655-657), an addend's finite.  ``**`` is C pow (torch.pow(tensor, float)): a negative base is
    real with an integer-valued exponent and NaN with any other.  There are no output
    constraints.  The class has ``SoboSpec``'s interface (struct / utility / feasible /
    constraints / m_model)."""

    def __init__(self, m_model: int, factors, addends=()):
        self.m_model = int(m_model)
        row = lambda r: (int(r[0]), int(r[1])) + tuple(float(v) for v in r[2:6])  # noqa: E731
        self.factors = [row(r) for r in factors]
        self.addends = [row(r) for r in addends]
        self.constraints = []
        if not 1 <= len(self.factors) + len(self.addends) <= 8:
            raise ValueError("mult scan: 1..8 factors and addends in all")
        for what, rows in (("factor", self.factors), ("addend", self.addends)):
            for o, k, w, *_ in rows:
                if not 0 <= o < self.m_model:
                    raise ValueError(f"mult scan: output index {o} outside the model's {self.m_model} outputs")
                if k not in (OBJ_AFFINE, OBJ_CLOSE_TO_TARGET, OBJ_SIGMOID, OBJ_TARGET):
                    raise ValueError(f"mult scan: {what} kind {k}")
                if not math.isfinite(w) or (what == "factor" and w < 1.0):
                    raise ValueError(f"mult scan: {what} weight {w} (finite; a factor's >= 1 after normalisation)")
        # an empty group keeps one placeholder row: the pointers stay valid, the count says 0
        pad = [(0, OBJ_AFFINE, 1.0, 0.0, 0.0, 0.0)]
        self._farrs, _ = _table_arrays(self.factors or pad, [])
        self._aarrs, _ = _table_arrays(self.addends or pad, [])

    @property
    def terms(self):
        """Factors, then addends (the device table's order)."""
        return self.factors + self.addends

    def struct(self, log: bool, tau_relu: float, tau_max: float, best: torch.Tensor) -> "_native.EvrMult":
        """evr_mult over ``best`` (device; S per-sample incumbents, or one value: stride 0).  The
        struct points into this spec's host arrays and into ``best``: keep both alive."""
        mt = _improvement(_native.EvrMult(), log, tau_relu, tau_max, best)
        mt.n_fac, mt.n_add = len(self.factors), len(self.addends)
        (mt.fac_out, mt.fac_kind, mt.fac_w, mt.fac_p0, mt.fac_p1, mt.fac_p2) = (a.ctypes.data for a in self._farrs)
        (mt.add_out, mt.add_kind, mt.add_w, mt.add_p0, mt.add_p1, mt.add_p2) = (a.ctypes.data for a in self._aarrs)
        return mt

    def utility(self, Y):
        """u of model-output rows Y (... x m_model; numpy array or torch tensor), multiplied and
        summed up in the reference's order: 1 * g_0 ** w_0 * ..., then 1 + g_a w_a + ..."""
        add = 1.0
        for o, k, w, a, b, c in self.addends:
            add = add + SoboSpec._term(k, a, b, c, Y[..., o]) * w
        mul = 1.0
        for o, k, w, a, b, c in self.factors:
            mul = mul * SoboSpec._term(k, a, b, c, Y[..., o]) ** w
        return mul * add

    feasible = SoboSpec.feasible


def mult_scan(Y: torch.Tensor, q: int, best: torch.Tensor, spec: MultSpec, log: bool = False,
              tau_relu: float = 1e-6, tau_max: float = 1e-2, flags: Optional[torch.Tensor] = None,
              gout: Optional[torch.Tensor] = None, backward: bool = False):
    """Multiplicative / multiplicative-additive scan alone (evr_mult_scan); arguments and results as
    ``sobo_scan``."""
    return _utility_scan("evr_mult_scan", Y, q, best, spec, log, tau_relu, tau_max, flags, gout, backward)


def qmult_eval(stm: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel", mt: "_native.EvrMult",
               X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """The multiplicative strategies' qNEI, qLogNEI, qLogEI, qEI over m model outputs
    (evr_qmult_eval): X (b*q) x d raw candidates -> acq (b) [, dX (b*q) x d]."""
    return _utility_eval("evr_qmult", stm, g, model, mt, X, backward, gout)


REWARD_SR, REWARD_UCB, REWARD_PI = 0, 1, 2


def ucb_scale(beta: float) -> float:
    """[upstream] qUpperConfidenceBound: k = sqrt(beta pi / 2)."""
    beta = float(beta)
    if not (beta >= 0.0 and math.isfinite(beta)):
        raise ValueError(f"qUCB: beta = {beta} must be non-negative and finite")
    return math.sqrt(beta * math.pi / 2.0)


def reward_struct(spec: SoboSpec, mode: int, beta: float = 0.2, tau: float = 1e-3,
                  best: Optional[torch.Tensor] = None, infeasible_cost: float = 0.0) -> "_native.EvrReward":
    """evr_reward over the tables of ``spec``: mode REWARD_SR / REWARD_UCB (beta) / REWARD_PI (tau
    and ``best``, one device double).  infeasible_cost: M >= 0 of the constrained reward (SR /
    UCB).  The struct points into the spec's host arrays and into ``best``: keep both alive."""
    if mode not in (REWARD_SR, REWARD_UCB, REWARD_PI):
        raise ValueError(f"reward scan: mode {mode}")
    if not isinstance(spec, SoboSpec):
        raise TypeError(f"reward scan needs an ops.SoboSpec, got {type(spec).__name__}")
    rw = _native.EvrReward()
    rw.mode = int(mode)
    rw.ucb_scale = ucb_scale(beta) if mode == REWARD_UCB else 0.0
    rw.tau = float(tau)
    if mode == REWARD_PI:
        if best is None or best.numel() != 1:
            raise ValueError("qPI needs the incumbent: one device double")
        if not float(tau) > 0.0:
            raise ValueError(f"qPI: tau = {tau} must be positive")
        rw.best = _dev(best, "best").data_ptr()
    else:
        if not float(infeasible_cost) >= 0.0:
            raise ValueError(f"reward scan: infeasible cost {infeasible_cost} must be non-negative")
    rw.infeasible_cost = float(infeasible_cost)
    _point_tables(rw, spec)
    (rw.term_out, rw.term_kind, rw.term_w, rw.term_p0, rw.term_p1,
     rw.term_p2) = (a.ctypes.data for a in spec._tarrs)
    return rw


def reward_scan(Y: torch.Tensor, q: int, spec: SoboSpec, mode: int, beta: float = 0.2, tau: float = 1e-3,
                best: Optional[torch.Tensor] = None, infeasible_cost: float = 0.0,
                flags: Optional[torch.Tensor] = None, gout: Optional[torch.Tensor] = None, backward: bool = False):
    """qSR / qUCB / qPI scan alone (evr_reward_scan): Y S x m_model x (b*q) joint samples (point i
    of candidate c at column c*q + i) -> (acq (b), dY like Y | None).  flags: m_model x b."""
    Y, q, b, flags, gout = _scan_args(Y, q, spec, flags, gout)
    S, m, _ = Y.shape
    best = None if best is None else _dev(best, "best")
    acq = torch.empty(b, dtype=torch.float64, device=Y.device)
    dY = torch.empty_like(Y) if backward else None
    rw = reward_struct(spec, mode, beta, tau, best, infeasible_cost)
    call("evr_reward_scan", _stream(), q, m, S, b, ctypes.byref(rw), Y.data_ptr(), _p(flags), _p(gout),
         acq.data_ptr(), _p(dY))
    return acq, dY


def qreward_eval(stm: EvrQnehviState, g: EvrQnGeneral, model: "_native.EvrQnehviModel", rw: "_native.EvrReward",
                 X: torch.Tensor, backward: bool, gout: Optional[torch.Tensor] = None):
    """qSR, qUCB, qPI over m model outputs (evr_qreward_eval): X (b*q) x d raw candidates -> acq (b)
    [, dX (b*q) x d]."""
    return _utility_eval("evr_qreward", stm, g, model, rw, X, backward, gout)


class QnehviPlan:
    """Native evaluation plan of the whole qNEHVI chain for a fixed batch size b
    (qnehvi_plan.hip): persistent device buffers X (b x d), out = [acq (b) | dX (b x d)] and
    the workspace; run() is one C-ABI call (one hipGraph launch when ``graph``)."""

    def __init__(self, st: EvrQnehviState, model: "_native.EvrQnehviModel", b: int, backward: bool, device,
                 graph: bool = True):
        lib = _native.load()
        d = int(model.d)
        self.b, self.d, self.backward = int(b), d, bool(backward)
        self.X = torch.zeros(b, d, dtype=torch.float64, device=device)
        self.out = torch.empty(b * (1 + d), dtype=torch.float64, device=device)
        nbytes = lib.evr_qnehvi_plan_workspace_bytes(ctypes.byref(st), ctypes.byref(model), b, int(backward))
        self.work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        self.acq = self.out[:b]
        self.dX = self.out[b:].view(b, d)
        self.host = torch.zeros(b * (1 + d), dtype=torch.float64)
        h = ctypes.c_void_p()
        call("evr_qnehvi_plan_create", _stream(), ctypes.byref(st), ctypes.byref(model), b, int(backward),
             self.X.data_ptr(), self.work.data_ptr(), self.acq.data_ptr(),
             self.dX.data_ptr() if backward else None, int(graph), ctypes.byref(h))
        self._h = h
        self._lib = lib

    def run(self):
        call("evr_qnehvi_plan_run", _stream(), self._h)

    def run_host(self, x: np.ndarray) -> np.ndarray:
        """x (b x d numpy) -> host [acq | dX] (evr_qnehvi_plan_eval_host: one graph launch
        reading x from and writing the results to pinned host memory)."""
        xh = np.ascontiguousarray(x, dtype=np.float64).reshape(self.b, self.d)
        out = self.host.numpy()
        call("evr_qnehvi_plan_eval_host", _stream(), self._h, xh.ctypes.data, out.ctypes.data)
        return out

    def minimize(self, x0: np.ndarray, lb: np.ndarray, ub: np.ndarray, maxiter: int, maxfun: int = 15000,
                 maxcor: int = 10, ftol: float = 2.220446049250313e-09, gtol: float = 1e-5, maxls: int = 20):
        """Native L-BFGS-B over the b restarts of this (backward) plan, the whole loop in C++
        (evr_qnehvi_plan_minimize): returns (x (b*d, clipped), acq (b) at x,
        [iterations, evaluations, status, task]).  Raises NotPSDError on a NaN evaluation."""
        if not self.backward:
            raise ValueError("minimize needs a backward plan")
        n = self.b * self.d
        f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(n))  # noqa: E731
        x0, lb, ub = f64(x0), f64(lb), f64(ub)
        x = np.empty(n)
        acq = np.empty(self.b)
        info = np.zeros(4, dtype=np.int32)
        rc = self._lib.evr_qnehvi_plan_minimize(_stream(), self._h, x0.ctypes.data, lb.ctypes.data, ub.ctypes.data,
                                                int(maxiter), int(maxfun), ftol / float(np.finfo(float).eps),
                                                float(gtol), int(maxcor), int(maxls), x.ctypes.data,
                                                acq.ctypes.data, info.ctypes.data)
        if rc == 7:
            raise NotPSDError(self._lib.evr_last_error().decode(errors="replace"))
        _native.check(rc, "evr_qnehvi_plan_minimize")
        return x, acq, info.tolist()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.evr_qnehvi_plan_destroy(h)
            self._h = None


def _hvi_work(st: EvrQnehviState, b: int, backward: bool, device) -> torch.Tensor:
    n = _native.load().evr_hvi_workspace_doubles(ctypes.byref(st), b, int(backward))
    return torch.empty(max(1, n), dtype=torch.float64, device=device)


def hvi_forward(st: EvrQnehviState, G: torch.Tensor, b: int, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acq[c] = mean_s HVI_s (register-tiled scan + deterministic reduction); NaN where
    ``flags`` (m x b int32 from qnehvi_samples) marks a failed new-point Cholesky."""
    acq = torch.empty(b, dtype=torch.float64, device=G.device)
    work = _hvi_work(st, b, False, G.device)
    call("evr_hvi_forward", _stream(), ctypes.byref(st), b, G.data_ptr(), _p(flags), work.data_ptr(),
         acq.data_ptr())
    return acq


def mean_over_samples(partial: torch.Tensor):
    S, b = partial.shape
    acq = torch.empty(b, dtype=torch.float64, device=partial.device)
    call("evr_mean_over_samples", _stream(), S, b, partial.data_ptr(), acq.data_ptr())
    return acq


def hvi_backward(st: EvrQnehviState, G: torch.Tensor, gout: Optional[torch.Tensor], b: int):
    """dG = gout/S * dHVI/dG (gout None = ones)."""
    dG = torch.empty_like(G)
    if gout is not None:
        gout = _dev(gout, "gout")
    work = _hvi_work(st, b, True, G.device)
    call("evr_hvi_backward", _stream(), ctypes.byref(st), b, G.data_ptr(), _p(gout), work.data_ptr(),
         dG.data_ptr())
    return dG


def hvi_forward_backward(st: EvrQnehviState, G: torch.Tensor, b: int, flags: Optional[torch.Tensor] = None,
                         gout: Optional[torch.Tensor] = None):
    """One fused scan: (acq (b), dG = gout/S * dHVI/dG)."""
    acq = torch.empty(b, dtype=torch.float64, device=G.device)
    dG = torch.empty_like(G)
    if gout is not None:
        gout = _dev(gout, "gout")
    work = _hvi_work(st, b, True, G.device)
    call("evr_hvi_forward_backward", _stream(), ctypes.byref(st), b, G.data_ptr(), _p(flags), _p(gout),
         work.data_ptr(), acq.data_ptr(), dG.data_ptr())
    return acq, dG


def hvi_restart_fb_applies(st: EvrQnehviState, b: int) -> bool:
    return bool(_native.load().evr_hvi_restart_fb_applies(ctypes.byref(st), int(b)))


def hvi_restart_fb(st: EvrQnehviState, G: torch.Tensor, b: int):
    """The restart-batch scan in one launch (hvi_kd3, b <= 32): (per-sample values S x b,
    dG = dHVI/dG / S); acq = mean_over_samples(values)."""
    S = int(st.S)
    sval = torch.empty(S, b, dtype=torch.float64, device=G.device)
    dG = torch.empty_like(G)
    call("evr_hvi_restart_fb", _stream(), ctypes.byref(st), b, G.data_ptr(), sval.data_ptr(), dG.data_ptr())
    return sval, dG


def qnehvi_samples_backward(st: EvrQnehviState, R, L22, dG, b: int):
    gR = torch.empty_like(R)
    call("evr_qnehvi_samples_backward", _stream(), ctypes.byref(st), b, R.data_ptr(), L22.data_ptr(), dG.data_ptr(),
         gR.data_ptr())
    return gR


def pareto_mask(O: torch.Tensor, ref: torch.Tensor, dedup: bool, want_mask=True, want_counts=False):
    """O: m x n x S.  Returns (mask S x n uint8 | None, counts n int32 | None)."""
    O, ref = _dev(O, "O"), _dev(ref, "ref")
    m, n, S = O.shape
    mask = torch.empty(S, n, dtype=torch.uint8, device=O.device) if want_mask else None
    counts = torch.zeros(n, dtype=torch.int32, device=O.device) if want_counts else None
    call("evr_pareto_mask", _stream(), S, n, m, O.data_ptr(), ref.data_ptr(), int(dedup), _p(mask), _p(counts))
    return mask, counts


def objective_affine(Y: torch.Tensor, mu: Optional[torch.Tensor], a: torch.Tensor, b: torch.Tensor):
    Y = _dev(Y, "Y")
    m, n, S = Y.shape
    O = torch.empty_like(Y)
    mu = None if mu is None else _dev(mu, "mu")
    call("evr_objective_affine", _stream(), m, n, S, Y.data_ptr(), _p(mu), _dev(a, "a").data_ptr(),
         _dev(b, "b").data_ptr(), O.data_ptr())
    return O


def qei(R: torch.Tensor, c: float, ym: float, ys: float, kxx: float, z: torch.Tensor, a: float, b: float,
        best_f: float, with_grad: bool):
    R, z = _dev(R, "R"), _dev(z, "z")
    n1, nb = R.shape
    acq = torch.empty(nb, dtype=torch.float64, device=R.device)
    gR = torch.empty_like(R) if with_grad else None
    flags = torch.empty(nb, dtype=torch.int32, device=R.device)
    call("evr_qei", _stream(), n1 - 1, nb, z.numel(), R.data_ptr(), float(c), float(ym), float(ys), float(kxx),
         z.data_ptr(), float(a), float(b), float(best_f), acq.data_ptr(), _p(gR), flags.data_ptr())
    return acq, gR, flags


def nipv_reduce(C: torch.Tensor, Vx: torch.Tensor, X: torch.Tensor, lo, inv_range, lengthscales, kind: int, noise,
                coef, v0, n: Optional[int] = None, backward: bool = False, gout: Optional[torch.Tensor] = None):
    """Per-candidate step of the negative integrated posterior variance (evr_nipv_reduce,
    nipv.hip): C B x N x (b*q) posterior cross-covariances to the N integration points, Vx
    B x ldv x (b*q) of which rows 0..n-1 per output are used (``n`` defaults to ldv; rows 0..n-1 of
    R = M K_x pass with n = ldv - 1), X b x q x d raw candidates (point i of candidate c at column
    c*q + i) -> (acq (b), flags (b, int32), dC like C | None, dVx B x n x (b*q) | None,
    dXself b x q x d | None).  flags != 0: a pivot of a q x q Cholesky was <= 0."""
    C, Vx, X = _dev(C, "C"), _dev(Vx, "Vx"), _dev(X, "X")
    ls = _dev(lengthscales, "lengthscales")
    if X.dim() != 3 or C.dim() != 3 or Vx.dim() != 3 or ls.dim() != 2:
        raise ValueError("nipv_reduce: C, Vx and X are 3-D, lengthscales 2-D")
    b, q, d = X.shape
    B, N, bq = C.shape
    ldv = Vx.shape[1]
    n = ldv if n is None else int(n)
    if bq != b * q or Vx.shape[0] != B or Vx.shape[2] != bq or tuple(ls.shape) != (B, d) or not 1 <= n <= ldv:
        raise ValueError(f"nipv_reduce: shapes C {tuple(C.shape)} Vx {tuple(Vx.shape)} X {tuple(X.shape)} "
                         f"ls {tuple(ls.shape)} n {n}")
    lo, inv_range = _dev(lo, "lo"), _dev(inv_range, "inv_range")
    noise, coef, v0 = _dev(noise, "noise"), _dev(coef, "coef"), _dev(v0, "v0")
    if lo.numel() != d or inv_range.numel() != d or noise.numel() != B or coef.numel() != B or v0.numel() != B:
        raise ValueError("nipv_reduce: lo / inv_range need d values, noise / coef / v0 one per output")
    if gout is not None:
        if not backward:
            raise ValueError("nipv_reduce: gout weights the backward only")
        gout = _dev(gout, "gout")
        if gout.numel() != b:
            raise ValueError("nipv_reduce: gout needs one value per candidate")
    dev = C.device
    acq = torch.empty(b, dtype=torch.float64, device=dev)
    flags = torch.empty(b, dtype=torch.int32, device=dev)
    dC = torch.empty_like(C) if backward else None
    dVx = torch.empty(B, n, bq, dtype=torch.float64, device=dev) if backward else None
    dXs = torch.empty_like(X) if backward else None
    call("evr_nipv_reduce", _stream(), int(q), B, n, N, b, d, int(kind), C.data_ptr(), Vx.data_ptr(), ldv,
         X.data_ptr(), lo.data_ptr(), inv_range.data_ptr(), ls.data_ptr(), noise.data_ptr(), coef.data_ptr(),
         v0.data_ptr(), _p(gout), acq.data_ptr(), flags.data_ptr(), _p(dC), _p(dVx), _p(dXs))
    return acq, flags, dC, dVx, dXs


def scale_batched(X: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """In place X[b] *= alpha[b]."""
    if not X.is_contiguous():
        raise ValueError("scale_batched: X must be contiguous")
    B = X.shape[0]
    call("evr_scale_batched", _stream(), B, X.numel() // B, _dev(alpha, "alpha").data_ptr(), X.data_ptr())
    return X


def add_selection(E: torch.Tensor, idx: torch.Tensor, val: Optional[torch.Tensor]) -> torch.Tensor:
    """In place E[b][r][idx[r]] += val[b]; E: B x nb x n, idx int32 (nb)."""
    B, nb, n = E.shape
    idx = _dev(idx, "idx", torch.int32)
    call("evr_add_selection", _stream(), B, nb, n, idx.data_ptr(), _p(None if val is None else _dev(val, "val")),
         E.data_ptr())
    return E


def box_device_supported(n: int, m: int) -> bool:
    return _native.load().evr_box_device_limits(int(n), int(m), None, None) == 0


def hvi_scan_supported(stride: int, m: int) -> bool:
    """The linear HVI scans take compressed cells over point tables of ``stride`` rows (the
    device box decomposition's output has stride = n + m)."""
    return _native.load().evr_hvi_scan_limits(int(stride), int(m)) == 0


class Cells:
    """Box cells of S samples on the device, ragged by ``off`` (S+1 int32): either explicit
    (``lo``/``hi``, C x m) or compressed (``keys`` C uint64 + per-sample point tables ``pts``
    S x stride x m and ``rank0`` S x stride, the device box decomposition's output)."""

    def __init__(self, off, counts, m, lo=None, hi=None, keys=None, pts=None, rank0=None, stride=0):
        self.off, self.counts, self.m = off, np.asarray(counts, dtype=np.int64), int(m)
        self.lo, self.hi, self.keys, self.pts, self.rank0, self.stride = lo, hi, keys, pts, rank0, int(stride)
        self.kd: Optional[KdGroups] = None

    @property
    def S(self) -> int:
        return int(self.counts.shape[0])

    @property
    def total(self) -> int:
        return int(self.counts.sum())

    @property
    def max_cells(self) -> int:
        return int(self.counts.max()) if self.S else 0

    def explicit(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lo, hi) rows (C x m, maximisation space); expands compressed cells on the device."""
        if self.keys is None:
            return self.lo, self.hi
        lo = torch.empty(self.total, self.m, dtype=torch.float64, device=self.off.device)
        hi = torch.empty_like(lo)
        call("evr_cells_from_keys", _stream(), self.S, self.m, self.stride, self.off.data_ptr(), self.max_cells,
             self.keys.data_ptr(), self.pts.data_ptr(), self.rank0.data_ptr(), lo.data_ptr(), hi.data_ptr())
        return lo, hi


class KdGroups:
    """kd-ordered groups of 16 compressed cells (cells_kd.hip) for the sparse HVI scan."""

    def __init__(self, goff, keys, rank, box, sorted_lo, max_groups):
        self.goff, self.keys, self.rank, self.box = goff, keys, rank, box
        self.sorted_lo, self.max_groups = sorted_lo, int(max_groups)


def kd_supported(cells: Cells) -> bool:
    if cells.keys is None or cells.S == 0:
        return False
    return _native.load().evr_cells_kd_limits(cells.stride, cells.m, cells.max_cells, None) == 0


def cells_kd_order(cells: Cells) -> KdGroups:
    """kd order + rank index of compressed cells (one workgroup per sample); attaches and
    returns the KdGroups (the HVI scan then runs the sparse three-level filter)."""
    if cells.keys is None:
        raise ValueError("cells_kd_order needs compressed cells (device box decomposition)")
    S, m, stride = cells.S, cells.m, cells.stride
    dev = cells.off.device
    ng = (cells.counts + 15) // 16
    goff_h = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(ng, out=goff_h[1:])
    G = int(goff_h[-1])
    goff = torch.as_tensor(goff_h.astype(np.int32)).to(dev)
    keys = torch.empty(max(G, 1) * 16, dtype=torch.int64, device=dev)
    rank = torch.empty(max(G, 1) * m * 16, dtype=torch.int16, device=dev)       # uint16 bit patterns
    box = torch.empty(max(G, 1) * 8, dtype=torch.int16, device=dev)
    sorted_lo = torch.empty(S, m, stride, dtype=torch.float64, device=dev)
    call("evr_cells_kd_order_device", _stream(), S, m, stride, cells.off.data_ptr(), goff.data_ptr(),
         cells.max_cells, cells.keys.data_ptr(), cells.pts.data_ptr(), cells.rank0.data_ptr(), keys.data_ptr(),
         rank.data_ptr(), box.data_ptr(), sorted_lo.data_ptr())
    cells.kd = KdGroups(goff, keys, rank, box, sorted_lo, int(ng.max()) if S else 0)
    return cells.kd


class BoxCapacityError(RuntimeError):
    """The device box decomposition needs more LUB slots than its capacity / memory bound
    (the caller falls back to the exact host partition)."""


def box_decompose_device(O: torch.Tensor, ref: torch.Tensor, cap: int = 16384, max_cap: int = 1 << 20,
                         max_workspace_bytes: int = 8 << 30) -> Cells:
    """Device box decomposition of every sample of O (m x n x S objective values) above ref,
    returned compressed (64-bit keys + point tables, see Cells).

    One host sync (the per-sample cell counts size the packed arrays and the HVI plan); a
    sample overflowing ``cap`` LUB slots reruns the batch with 4x the capacity, up to
    ``max_cap`` slots and ``max_workspace_bytes`` of workspace, beyond which it raises
    BoxCapacityError."""
    O, ref = _dev(O, "O"), _dev(ref, "ref")
    m, n, S = O.shape
    dev = O.device
    while True:
        nbytes = _native.load().evr_box_device_workspace_bytes(S, n, m, cap)
        if nbytes > max_workspace_bytes:
            raise BoxCapacityError(f"box decomposition: {cap} LUB slots x {S} samples need {nbytes} B of workspace")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cs = torch.empty(2, S, dtype=torch.int32, device=dev)
        call("evr_box_decompose_device", _stream(), S, n, m, O.data_ptr(), ref.data_ptr(), cap, ws.data_ptr(),
             cs[0].data_ptr(), cs[1].data_ptr())
        h = cs.cpu().numpy()
        if not h[1].any():
            break
        if cap >= max_cap:
            raise BoxCapacityError(f"box decomposition: more than {max_cap} local upper bounds in one sample")
        cap *= 4
    counts = h[0].astype(np.int64)
    off_h = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    total = int(off_h[-1])
    off = torch.as_tensor(off_h.astype(np.int32)).to(dev)
    stride = n + m
    keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)      # uint64 bit patterns
    pts = torch.empty(S, stride, m, dtype=torch.float64, device=dev)
    rank0 = torch.empty(S, stride, dtype=torch.int32, device=dev)
    call("evr_box_pack_keys_device", _stream(), S, n, m, cap, ws.data_ptr(), off.data_ptr(),
         int(counts.max()) if S else 0, keys.data_ptr(), pts.data_ptr(), rank0.data_ptr())
    return Cells(off, counts, m, keys=keys, pts=pts, rank0=rank0, stride=stride)


def box_decompose_kd_device(O: torch.Tensor, ref: torch.Tensor, want_kd: bool = True, cap: int = 16384,
                            max_cap: int = 1 << 20, max_workspace_bytes: int = 8 << 30):
    """box_decompose_device + cells_kd_order in one native call (evr_box_kd_pipeline): the
    count read-back, the offsets and the pack / kd launches happen in C++ with the GIL released,
    so no Python runs between the kernels.  Outputs are allocated for the capacity and returned
    as views of the used prefix.  Returns (cells, kd_built); cells.kd is attached when built."""
    O, ref = _dev(O, "O"), _dev(ref, "ref")
    m, n, S = O.shape
    dev = O.device
    stride = n + m
    lib = _native.load()
    counts_h = np.zeros(S, dtype=np.int32)
    info = np.zeros(3, dtype=np.int32)
    cap0 = cap
    while True:
        nbytes = lib.evr_box_device_workspace_bytes(S, n, m, cap)
        G = S * cap // 16 + S
        # the capacity-sized outputs count against the budget too (they live as long as the
        # acquisition when not trimmed below)
        out_bytes = 8 * S * cap + 8 * S * stride * m + 4 * S * stride + 16 * S + 8
        if want_kd:
            out_bytes += G * 16 * 8 + G * m * 16 * 2 + G * 8 * 2 + 8 * S * m * stride
        if nbytes + out_bytes > max_workspace_bytes:
            raise BoxCapacityError(f"box decomposition: {cap} LUB slots x {S} samples need {nbytes + out_bytes} B "
                                   "of workspace and outputs")
        try:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            cs = torch.empty(2, S, dtype=torch.int32, device=dev)
            offs = torch.empty(2, S + 1, dtype=torch.int32, device=dev)
            keys = torch.empty(S * cap, dtype=torch.int64, device=dev)           # uint64 bit patterns
            pts = torch.empty(S, stride, m, dtype=torch.float64, device=dev)
            rank0 = torch.empty(S, stride, dtype=torch.int32, device=dev)
            if want_kd:
                okeys = torch.empty(G * 16, dtype=torch.int64, device=dev)
                ork = torch.empty(G * m * 16, dtype=torch.int16, device=dev)    # uint16 bit patterns
                ogb = torch.empty(G * 8, dtype=torch.int16, device=dev)
                osv = torch.empty(S, m, stride, dtype=torch.float64, device=dev)
            else:
                okeys = ork = ogb = osv = None
        except torch.OutOfMemoryError as e:
            raise BoxCapacityError(f"box decomposition: out of device memory at {cap} LUB slots x {S} samples") from e
        call("evr_box_kd_pipeline", _stream(), S, n, m, O.data_ptr(), ref.data_ptr(), cap, ws.data_ptr(),
             cs[0].data_ptr(), cs[1].data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), keys.data_ptr(),
             pts.data_ptr(), rank0.data_ptr(), int(bool(want_kd)), _p(okeys), _p(ork), _p(ogb), _p(osv),
             counts_h.ctypes.data, info.ctypes.data)
        if not info[0]:
            break
        if cap >= max_cap:
            raise BoxCapacityError(f"box decomposition: more than {max_cap} local upper bounds in one sample")
        cap *= 4
    counts = counts_h.astype(np.int64)
    total = int(counts.sum())
    del ws
    # a capacity rerun leaves outputs sized for 4x the slots or more: keep copies of the used
    # prefixes instead of views that pin the whole allocation (the first-try capacity keeps
    # views: no copy on the ask's critical path)
    trim = (lambda t: t.clone()) if cap > cap0 else (lambda t: t)
    cells = Cells(offs[0], counts, m, keys=trim(keys[:max(total, 1)]), pts=pts, rank0=rank0, stride=stride)
    if info[1]:
        ng = (counts + 15) // 16
        Gu = int(ng.sum())
        cells.kd = KdGroups(offs[1], trim(okeys[:max(Gu, 1) * 16]), trim(ork[:max(Gu, 1) * m * 16]),
                            trim(ogb[:max(Gu, 1) * 8]), osv, int(ng.max()) if S else 0)
    return cells, bool(info[1])


_SOBOL_DIRECTIONS = {}


def _sobol_directions(dim: int) -> torch.Tensor:
    """Unscrambled 30-bit direction numbers of torch's SobolEngine (Joe-Kuo D(6) table as
    torch ships it), cached per dimension; scrambled per seed by evr_sobol_scramble."""
    V = _SOBOL_DIRECTIONS.get(dim)
    if V is None:
        V = torch.zeros(dim, 30, dtype=torch.long)
        torch._sobol_engine_initialize_state_(V, dim)
        if len(_SOBOL_DIRECTIONS) > 16:
            _SOBOL_DIRECTIONS.clear()
        _SOBOL_DIRECTIONS[dim] = V
    return V


SOBOL_MAXDIM = 21201     # torch.quasirandom.SobolEngine.MAXDIM


def _iid_normal(n: int, dim: int, seed: int, device, d0: int, nd: int, layout: int, m: int) -> torch.Tensor:
    """[upstream] get_sampler's fallback beyond SobolEngine.MAXDIM dims: IIDNormalSampler,
    torch.randn of the (n, dim) base-sample shape under manual_seed(seed) (CPU generator),
    restricted to dims [d0, d0+nd) in the requested layout."""
    warnings.warn(f"{dim} base-sample dims exceed SobolEngine.MAXDIM={SOBOL_MAXDIM}: IID normal base samples",
                  RuntimeWarning)
    g = torch.Generator().manual_seed(int(seed))
    Z = torch.randn(n, dim, generator=g, dtype=torch.float64)[:, d0:d0 + nd]
    if layout == 0:
        return Z.contiguous().to(device)
    return Z.reshape(n, nd // m, m).permute(2, 1, 0).contiguous().to(device)


def sobol_scramble(dim: int, seed: int, d0: int = 0, nd: Optional[int] = None):
    """Host half of draw_sobol_normal_samples: the scrambled direction numbers (nd x 30) and
    shifts (nd) of dims [d0, d0+nd) of SobolEngine(dim, scramble=True, seed) (CPU int64
    tensors; evr_sobol_scramble_range).  None beyond SOBOL_MAXDIM (IID fallback).  Releases the
    GIL: the acquisition prefetches it on a worker thread."""
    nd = dim - d0 if nd is None else nd
    if not (0 <= d0 and nd >= 1 and d0 + nd <= dim):
        raise ValueError("sobol_scramble: dims out of range")
    if dim > SOBOL_MAXDIM:
        return None
    V, shift = _pinned_scramble_out(dim, d0, nd)
    call("evr_sobol_scramble_range", dim, int(seed), d0, nd, V.data_ptr(), shift.data_ptr())
    return V, shift


def _pinned_scramble_out(dim: int, d0: int, nd: int):
    """(direction numbers of dims [d0, d0+nd), shift buffer) in pinned host memory when a GPU
    is present, so that sobol_normal's uploads are asynchronous (a pageable .to(device) blocks
    the host until the stream has drained)."""
    pin = os.environ.get("EVR_SOBOL_PINNED", "1") != "0" and torch.cuda.is_available()
    V = torch.empty(nd, 30, dtype=torch.long, pin_memory=pin)
    V.copy_(_sobol_directions(dim)[d0:d0 + nd])
    return V, torch.empty(nd, dtype=torch.long, pin_memory=pin)


class SobolStream:
    """The raw mt19937 stream of one seed, long enough for draws of up to ``max_dim``
    dimensions (evr_sobol_stream_create; releases the GIL, so it can be generated on a worker
    thread before the draw's dimension count is known)."""

    def __init__(self, seed: int, max_dim: int):
        lib = _native.load()
        self._lib = lib
        self.seed, self.max_dim = int(seed), int(max_dim)
        h = ctypes.c_void_p()
        call("evr_sobol_stream_create", self.seed, lib.evr_sobol_stream_words(self.max_dim), ctypes.byref(h))
        self._h = h

    def scramble(self, dim: int, d0: int = 0, nd: Optional[int] = None):
        """(V, shift) of dims [d0, d0+nd) of SobolEngine(dim, scramble=True, seed) — as
        sobol_scramble — or None beyond SOBOL_MAXDIM / this stream's length."""
        nd = dim - d0 if nd is None else nd
        if dim > SOBOL_MAXDIM or dim > self.max_dim or nd < 1:
            return None
        V, shift = _pinned_scramble_out(dim, d0, nd)
        call("evr_sobol_scramble_stream", self._h, dim, d0, nd, V.data_ptr(), shift.data_ptr())
        return V, shift

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None:
            try:
                self._lib.evr_sobol_stream_destroy(h)
            except Exception:
                pass
            self._h = None


def sobol_normal(n: int, dim: int, seed: int, device, d0: int = 0, nd: Optional[int] = None,
                 layout: int = 0, m: int = 1, scrambled=None) -> torch.Tensor:
    """Device draw_sobol_normal_samples(dim, n, seed) restricted to dims [d0, d0+nd).

    layout 0 -> n x nd; layout 1 -> m x (nd/m) x n (sample index fastest, the GEMM-ready
    layout of the baseline / prune samples: dim t = point*m + output).  ``scrambled``: the
    (V, shift) of sobol_scramble(dim, seed, d0, nd) when already computed."""
    nd = dim - d0 if nd is None else nd
    if not (0 <= d0 and d0 + nd <= dim):
        raise ValueError("sobol_normal: dims out of range")
    if dim > SOBOL_MAXDIM:
        return _iid_normal(n, dim, seed, device, d0, nd, layout, m)
    if layout == 0:
        out = torch.empty(n, nd, dtype=torch.float64, device=device)
    else:
        out = torch.empty(m, nd // m, n, dtype=torch.float64, device=device)
    if nd == 0:
        return out
    V, shift = scrambled if scrambled is not None else sobol_scramble(dim, seed, d0, nd)
    Vd = V.to(device, non_blocking=V.is_pinned())
    sd = shift.to(device, non_blocking=shift.is_pinned())
    call("evr_sobol_normal", _stream(), n, nd, 0, Vd.data_ptr(), sd.data_ptr(), layout, m, out.data_ptr())
    return out


def box_decompose(obj: np.ndarray, ref: np.ndarray, mask: Optional[np.ndarray] = None, num_threads: int = 0,
                  layout: str = "jis", alpha: float = 0.0):
    """Host box decomposition.  obj: float64 numpy array, layout 'jis' (m x n x S) or 'sij'
    (S x n x m).  alpha > 0 (m > 2): the approximate partition of [upstream]
    NondominatedPartitioning(alpha).  Returns (lo [C x m], hi [C x m], off [S+1]) numpy arrays."""
    lib = _native.load()
    obj = np.ascontiguousarray(obj, dtype=np.float64)
    if layout == "jis":
        m, n, S = obj.shape
        ss, si, sj = 1, S, n * S
    elif layout == "sij":
        S, n, m = obj.shape
        ss, si, sj = n * m, m, 1
    else:
        raise ValueError(layout)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    handle = ctypes.c_void_p()
    _native.check(lib.evr_box_decompose_approx(S, n, m, obj.ctypes.data, ss, si, sj,
                                               None if mk is None else mk.ctypes.data, ref.ctypes.data,
                                               float(alpha), int(num_threads), ctypes.byref(handle)),
                  "evr_box_decompose_approx")
    try:
        total = lib.evr_cells_total(handle)
        lo = np.empty((total, m), dtype=np.float64)
        hi = np.empty((total, m), dtype=np.float64)
        off = np.empty(S + 1, dtype=np.int32)
        lib.evr_cells_copy(handle, lo.ctypes.data, hi.ctypes.data, off.ctypes.data)
    finally:
        lib.evr_cells_free(handle)
    return lo, hi, off


def device_arch(device: int = 0) -> str:
    buf = ctypes.create_string_buffer(64)
    call("evr_device_arch", device, buf, 64)
    return buf.value.decode()
