"""Exact GPs resident in HBM: batched posterior and MLL (value + gradient) on the HIP kernels.

Mirrors BoFire's ``SingleTaskGPSurrogate`` model (bofire/surrogates/single_task_gp.py:39-71)
on top of [upstream] BoTorch ``SingleTaskGP``: Normalize(bounds) inputs, Standardize outputs,
ConstantMean, RBF/Matérn ARD kernel (no outputscale by default), Gaussian likelihood with
noise >= 1e-4 and hyperpriors; fit = scipy L-BFGS-B on the raw parameters
(``fit_gpytorch_mll``, max_attempts=10), every loss/gradient evaluated on the device.

``GPBatch`` holds B exact GPs over one set of normalized training rows (the ModelListGP of
BotorchSurrogates.compatibilize, bofire/surrogates/botorch_surrogates.py:79-128) so that
posteriors for all outputs are one batched launch.  The members may differ in kernel family
(one per output, EVR_KERNEL_MIXED) and in training rows: with a row mask, output j's GP is
exact over its own rows V_j only — K_j is padded to the union with identity rows / columns
outside V_j, so chol(K_pad) is L_j interleaved with identity rows, and L^-1's rows outside V_j
(and with them alpha's entries) are zeroed: L^-T L^-1 = K_j^-1 embedded, and every posterior,
root and projection formula runs unchanged over the union rows.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native, ops

MIN_INFERRED_NOISE_LEVEL = 1e-4
KIND_MIXED, KIND_MAX_MIXED = 16, 13     # include/everest_amd.h EVR_KERNEL_MIXED


def kind_code(kinds: Sequence[int]) -> int:
    """Kernel family code of a batch of outputs: the family itself when all agree, else
    EVR_KERNEL_MIXED with 2 bits per output (kind_j << (5 + 2 j))."""
    kinds = [int(k) for k in kinds]
    if any(k < 0 or k > 3 for k in kinds):
        raise ValueError(f"kernel kinds must be in 0..3, got {kinds}")
    if len(set(kinds)) <= 1:
        return kinds[0] if kinds else 0
    if len(kinds) > KIND_MAX_MIXED:
        raise NotImplementedError(f"mixed kernel families are supported for at most {KIND_MAX_MIXED} outputs")
    code = KIND_MIXED
    for j, k in enumerate(kinds):
        code |= k << (5 + 2 * j)
    return code


def kinds_of(code: int, B: int) -> List[int]:
    code = int(code)
    return [code] * B if code < KIND_MIXED else [(code >> (5 + 2 * j)) & 3 for j in range(B)]


def softplus_np(x):
    return np.logaddexp(0.0, x)


def _softplus_libm(v: float) -> float:
    """numpy.logaddexp(0, v) with the C library's scalar exp / log1p (CPython's math module):
    the arithmetic of the native fit driver's softplus (mll_plan.hip)."""
    v = float(v)
    if v == 0.0:
        return 0.6931471805599453
    return v + math.log1p(math.exp(-v)) if v > 0.0 else math.log1p(math.exp(v))


def sigmoid_np(x):
    return 1.0 / (1.0 + np.exp(-x))


def _prior(p):
    """Normalise a prior spec: None, (loc, scale) [LogNormal] or (family, p1, p2)."""
    if p is None:
        return None
    if len(p) == 2:
        return ("lognormal", float(p[0]), float(p[1]))
    return (p[0], float(p[1]), float(p[2]))


def prior_logpdf_np(p, x):
    """gpytorch LogNormalPrior / GammaPrior / NormalPrior log densities (elementwise)."""
    fam, a, b = p
    x = np.asarray(x, dtype=np.float64)
    if fam == "lognormal":
        lx = np.log(x)
        return -lx - math.log(b) - 0.5 * math.log(2 * math.pi) - 0.5 * ((lx - a) / b) ** 2
    if fam == "gamma":
        return a * math.log(b) - math.lgamma(a) + (a - 1) * np.log(x) - b * x
    if fam == "normal":
        return -0.5 * math.log(2 * math.pi * b * b) - 0.5 * ((x - a) / b) ** 2
    raise ValueError(fam)


def prior_dlogpdf_np(p, x):
    fam, a, b = p
    x = np.asarray(x, dtype=np.float64)
    if fam == "lognormal":
        return (-1.0 - (np.log(x) - a) / b ** 2) / x
    if fam == "gamma":
        return (a - 1) / x - b
    if fam == "normal":
        return -(x - a) / (b * b)
    raise ValueError(fam)


def prior_sample_np(p, rng, size):
    fam, a, b = p
    if fam == "lognormal":
        return np.exp(rng.normal(a, b, size))
    if fam == "gamma":
        return rng.gamma(a, 1.0 / b, size)
    if fam == "normal":
        return np.abs(rng.normal(a, b, size))
    raise ValueError(fam)


def standardize_params(y: np.ndarray) -> Tuple[float, float]:
    """[upstream] Standardize(m=1): mean, unbiased std, std < 1e-8 -> 1, n == 1 -> 1."""
    mean = float(np.mean(y))
    if y.shape[0] == 1:
        return mean, 1.0
    std = float(np.std(y, ddof=1))
    return mean, (std if std >= 1e-8 else 1.0)


@dataclass
class GPHyper:
    lengthscale: np.ndarray   # d
    noise: float
    constant: float
    y_mean: float
    y_std: float
    outputscale: Optional[float] = None   # sigma^2 of k = sigma^2 k_base (ScaleKernel); None: no scale


def fold_outputscale(h: GPHyper) -> GPHyper:
    """The unscaled GP that is exactly the scaled one: a GP with (sigma^2, noise s^2, constant c,
    y_std) on the standardised targets is the GP with kernel k_base, noise s^2 / sigma^2, constant
    c / sigma and y_std sigma (divide the standardised targets by sigma) — the same mean, variance,
    observation noise and joint samples in physical units.  Everything downstream of the fit
    (GPBatch, the posterior, the acquisition chains) takes this form."""
    if h.outputscale is None:
        return h
    s2 = float(h.outputscale)
    s = math.sqrt(s2)
    return GPHyper(lengthscale=h.lengthscale, noise=h.noise / s2, constant=h.constant / s, y_mean=h.y_mean,
                   y_std=h.y_std * s)


class GPBatch:
    """B exact GPs on shared normalized inputs Xn (n x d, device).  ``kind``: one family, a
    per-output list, or a kind code; ``mask`` (B x n, optional): the rows each output is
    trained on (Y's entries outside them are ignored)."""

    def __init__(self, Xn: torch.Tensor, Y: torch.Tensor, hypers: Sequence[GPHyper], kind,
                 lo: torch.Tensor, hi: torch.Tensor, mask: Optional[np.ndarray] = None):
        self.Xn = Xn.contiguous()
        B_ = len(hypers)
        if isinstance(kind, (list, tuple, np.ndarray)):
            if len(kind) != B_:
                raise ValueError(f"{len(kind)} kernel kinds for {B_} outputs")
            kind = kind_code(kind)
        self.kind = int(kind)
        self.kinds = kinds_of(self.kind, B_)
        self.lo = lo
        self.hi = hi
        self.inv_range = 1.0 / (hi - lo)
        self.hypers = list(hypers)
        dev = Xn.device
        self.device = dev
        self.B = len(hypers)
        self.n, self.d = Xn.shape
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        self.ls = t(np.stack([h.lengthscale for h in hypers]))
        self.noise = t([h.noise for h in hypers])
        self.const = t([h.constant for h in hypers])
        self.ym = t([h.y_mean for h in hypers])
        self.ys = t([h.y_std for h in hypers])
        self.kxx = torch.ones(self.B, dtype=torch.float64, device=dev)
        self.mask = None
        if mask is not None:
            mk = np.asarray(mask, dtype=bool).reshape(self.B, self.n)
            if not mk.any(axis=1).all():
                raise ValueError("every output needs at least one training row")
            if not mk.all():
                self.mask = torch.as_tensor(mk.astype(np.float64), device=dev)
        # standardized targets (B x n); zero (the prior mean's residual is masked) outside each
        # output's own rows
        Yc = Y.to(device=dev, dtype=torch.float64).reshape(self.n, self.B).T.contiguous()
        self.y = ((Yc - self.ym[:, None]) / self.ys[:, None]).contiguous()
        if self.mask is not None:
            self.y = torch.where(self.mask > 0, self.y, torch.zeros_like(self.y)).contiguous()
        self.refresh()

    def valid_all_rows(self) -> np.ndarray:
        """Rows every output is trained on (n bools)."""
        if self.mask is None:
            return np.ones(self.n, dtype=bool)
        return (self.mask.min(0).values > 0).cpu().numpy()

    # -- caches: L = chol(K + s2 I), Linv, alpha, M = [Linv; alpha^T] ----------------------
    def refresh(self):
        Ky = ops.kernel_matrix(self.Xn, self.Xn, self.ls, self.kind, diag_add=self.noise)
        if self.mask is not None:
            # K_j padded: identity rows / columns outside output j's rows
            mk = self.mask
            Ky.mul_(mk[:, :, None] * mk[:, None, :])
            Ky.diagonal(dim1=-2, dim2=-1).add_(1.0 - mk)
        self.L, self.Linv, _, _ = ops.cholesky_inverse(Ky, 1e-8, 3)
        if self.mask is not None:
            self.Linv.mul_(self.mask[:, :, None])                               # K_j^-1 embedded
        r = (self.y - self.const[:, None]).unsqueeze(-1)                        # B x n x 1
        if self.mask is not None:
            r = r * self.mask[:, :, None]
        r = r.contiguous()
        v = ops.gemm(self.Linv, r)
        self.alpha = ops.gemm(self.Linv, v, transA=True)[..., 0].contiguous()  # B x n
        self.M = torch.cat([self.Linv, self.alpha.unsqueeze(1)], dim=1).contiguous()  # B x (n+1) x n

    def kernel_train(self, noise: bool = False) -> torch.Tensor:
        return ops.kernel_matrix(self.Xn, self.Xn, self.ls, self.kind, diag_add=self.noise if noise else None)

    def cross(self, Xraw: torch.Tensor) -> torch.Tensor:
        """K(Xtr, normalize(Xraw)) : B x n x nt."""
        return ops.kernel_matrix(self.Xn, Xraw, self.ls, self.kind, shift2=self.lo, scale2=self.inv_range)

    def posterior(self, Xraw: torch.Tensor, observation_noise: bool = False):
        """Mean and variance (B x nt) at raw (transformed, unnormalized) inputs."""
        from . import torch_ops

        Xraw = Xraw.to(device=self.device, dtype=torch.float64).contiguous()
        # the registered operator torch.ops.everest_amd.gp_posterior (evr_gp_posterior)
        return torch_ops.load().gp_posterior(self.Xn, Xraw, self.lo, self.inv_range, self.ls, self.M, self.kind,
                                             self.const, self.ym, self.ys, self.kxx,
                                             self.noise if observation_noise else None)


# ---------------------------------------------------------------------------------------
# device MLL value + gradient (one output)
# ---------------------------------------------------------------------------------------
class MLLEvaluator:
    """Exact MLL / n with hyperpriors for one GP on device; raw parameter vector
    x = [noise, constant, raw_lengthscale(d)] (BoTorch bounds: noise >= 1e-4).  Scaled
    (``scaled`` or an ``outputscale_prior``): k = sigma^2 k_base, sigma^2 = softplus(raw) one entry
    more at the end of x, its prior evaluated on sigma^2."""

    def __init__(self, Xn: torch.Tensor, y_std_space: np.ndarray, kind: int,
                 ls_prior: Optional[Tuple[float, float]], noise_prior: Optional[Tuple[float, float]],
                 outputscale_prior=None, scaled: bool = False):
        self.Xn = Xn.contiguous()
        self.n, self.d = Xn.shape
        self.kind = kind
        self.y = np.asarray(y_std_space, dtype=np.float64)
        self.ls_prior = _prior(ls_prior)
        self.noise_prior = _prior(noise_prior)
        self.os_prior = _prior(outputscale_prior)
        self.scaled = bool(scaled) or self.os_prior is not None
        self.dev = Xn.device

    def __call__(self, x: np.ndarray):
        n, d = self.n, self.d
        noise, const, raw = float(x[0]), float(x[1]), np.asarray(x[2:2 + d], dtype=np.float64)
        ls = softplus_np(raw)
        dev = self.dev
        ls_t = torch.as_tensor(ls[None, :], device=dev)
        os_t = None
        if self.scaled:
            raw_os = float(x[2 + d])
            os_ = float(softplus_np(raw_os))
            os_t = torch.tensor([os_], dtype=torch.float64, device=dev)
        Ky = ops.kernel_matrix(self.Xn, self.Xn, ls_t, self.kind, outputscale=os_t,
                               diag_add=torch.tensor([noise], dtype=torch.float64, device=dev))
        L, Linv, _, _ = ops.cholesky_inverse(Ky, 1e-8, 3)
        r = torch.as_tensor((self.y - const)[None, :, None], device=dev)
        v = ops.gemm(Linv, r)
        alpha = ops.gemm(Linv, v, transA=True)                       # 1 x n x 1
        W = ops.gemm(alpha, alpha, transB=True)                      # alpha alpha^T
        ops.gemm(Linv, Linv, transA=True, alpha=-1.0, beta=1.0, out=W)   # - K^-1
        if self.scaled:
            gls, gos = ops.kernel_hyper_grad(self.Xn, ls_t, os_t, W, self.kind)   # 1 x d, 1
            gos = float(gos.cpu().numpy()[0])
        else:
            gls = ops.kernel_lengthscale_grad(self.Xn, ls_t, W, self.kind)  # 1 x d
        terms = ops.mll_terms(L, Linv, r[..., 0].contiguous(), alpha[..., 0].contiguous())
        terms = terms.cpu().numpy()[0]
        gls = gls.cpu().numpy()[0]
        logdet, quad, trKinv, sum_a, sum_a2 = terms
        ll = -0.5 * quad - 0.5 * logdet - 0.5 * n * math.log(2 * math.pi)
        d_noise = 0.5 * (sum_a2 - trKinv)
        d_const = sum_a
        d_ls = 0.5 * gls
        if self.ls_prior is not None:
            ll += float(np.sum(prior_logpdf_np(self.ls_prior, ls)))
            d_ls = d_ls + prior_dlogpdf_np(self.ls_prior, ls)
        if self.noise_prior is not None:
            ll += float(prior_logpdf_np(self.noise_prior, noise))
            d_noise += float(prior_dlogpdf_np(self.noise_prior, noise))
        d_raw = d_ls * sigmoid_np(raw)
        if self.scaled:
            d_os = 0.5 * gos
            if self.os_prior is not None:
                ll += float(prior_logpdf_np(self.os_prior, os_))
                d_os += float(prior_dlogpdf_np(self.os_prior, os_))
            d_raw = np.concatenate([d_raw, [d_os * float(sigmoid_np(raw_os))]])
        g = np.concatenate([[d_noise, d_const], d_raw]) / n
        return ll / n, g


# floor of a resampled outputscale: a NormalPrior's draw (taken in absolute value, as the other
# resamples are) can land at or next to 0, whose inverse softplus is -inf
MIN_RESAMPLED_OUTPUTSCALE = 1e-6


def outputscale_restart_raw(os_prior, rng) -> float:
    """The raw outputscale a fit restarts from after NotPSDError: a draw from its prior (clamped to
    MIN_RESAMPLED_OUTPUTSCALE, as the noise draw is clamped to its bound) through the inverse
    softplus; without a prior the start value, raw 0."""
    osp = _prior(os_prior)
    if osp is None:
        return 0.0
    v = max(float(prior_sample_np(osp, rng, 1)[0]), MIN_RESAMPLED_OUTPUTSCALE)
    return float(v + math.log(-math.expm1(-v)))


def noise_start(noise_prior) -> float:
    """The fit's start value of the noise: the prior's mode (LogNormal: exp(loc - scale^2); Gamma
    with concentration > 1: (concentration - 1) / rate), else twice the lower bound."""
    nzp = _prior(noise_prior)
    if nzp is not None and nzp[0] == "lognormal":
        noise0 = math.exp(nzp[1] - nzp[2] ** 2)
    elif nzp is not None and nzp[0] == "gamma" and nzp[1] > 1:
        noise0 = (nzp[1] - 1) / nzp[2]
    else:
        noise0 = 2 * MIN_INFERRED_NOISE_LEVEL
    return max(noise0, MIN_INFERRED_NOISE_LEVEL)


def fit_single(Xn: torch.Tensor, y_raw: np.ndarray, kind: int, ls_prior, noise_prior=(-4.0, 1.0),
               max_attempts: int = 10, seed: int = 0, options: Optional[dict] = None,
               standardize: bool = True, outputscale_prior=None, scaled: bool = False) -> GPHyper:
    """fit_gpytorch_mll restated on device kernels: minimise -mll with scipy L-BFGS-B over
    (noise >= 1e-4, constant, raw lengthscale) starting from noise = prior mode (LogNormal
    noise prior: exp(loc - scale^2)), constant 0, lengthscale softplus(0) = ln 2; on
    NotPSDError resample the hyperparameters from their priors and retry (max_attempts=10,
    bofire/surrogates/single_task_gp.py:71).  ``scaled`` (or an ``outputscale_prior``): the
    ScaleKernel form, k = sigma^2 k_base with sigma^2 = softplus(raw), raw 0 at the start, the last
    entry of x; resampled from its prior with the others, without one it goes back to its start."""
    from scipy.optimize import minimize

    if standardize:
        y_mean, y_std = standardize_params(y_raw)
    else:
        y_mean, y_std = 0.0, 1.0
    y = (y_raw - y_mean) / y_std
    d = Xn.shape[1]
    lsp, nzp, osp = _prior(ls_prior), _prior(noise_prior), _prior(outputscale_prior)
    ev = MLLEvaluator(Xn, y, kind, lsp, nzp, osp, scaled)
    sc = int(ev.scaled)
    x0 = np.concatenate([[noise_start(nzp), 0.0], np.zeros(d + sc)])
    bounds = [(MIN_INFERRED_NOISE_LEVEL, None), (None, None)] + [(None, None)] * (d + sc)
    rng = np.random.default_rng(seed)
    last_err = None
    for attempt in range(max_attempts):
        try:
            res = minimize(lambda x: tuple(-v for v in ev(x)), x0, jac=True, method="L-BFGS-B", bounds=bounds,
                           options=options or {})
            xv = res.x
            return GPHyper(lengthscale=softplus_np(xv[2:2 + d]), noise=float(xv[0]), constant=float(xv[1]),
                           y_mean=y_mean, y_std=y_std, outputscale=float(softplus_np(xv[2 + d])) if sc else None)
        except ops.NotPSDError as e:  # sample_all_priors, then retry
            last_err = e
            ls = prior_sample_np(lsp, rng, d) if lsp else np.full(d, math.log(2.0))
            nz = max(float(prior_sample_np(nzp, rng, 1)[0]) if nzp else 1e-3, MIN_INFERRED_NOISE_LEVEL)
            x0 = np.concatenate([[nz, 0.0], np.log(np.expm1(ls))])
            if sc:
                x0 = np.append(x0, outputscale_restart_raw(osp, rng))
    raise RuntimeError(f"GP fit failed after {max_attempts} attempts: {last_err}")


# ---------------------------------------------------------------------------------------
# lock-step fit of several outputs on shared inputs: one batched MLL launch chain per round
# ---------------------------------------------------------------------------------------
class MLLBatch:
    """MLL / n (+ hyperpriors) value and gradient of B GPs sharing Xn (one per output),
    evaluated for any subset of the outputs in one batched launch chain (kernel matrices,
    psd_safe Cholesky + inverse, alpha, W = alpha alpha^T - K^-1, lengthscale gradients, the
    scalar terms) and one device->host copy.  Returns None for a member whose Cholesky stays
    not p.d. after the jitter ladder (NotPSDError of that fit).

    Member form (``nvalid`` given): member b has its own inputs ``Xn[b]`` (Xn is B x n x d) of
    which the first ``nvalid[b]`` rows are real; the rest is padding (zeros) that the member
    kernels turn into identity rows / columns of K (include/everest_amd.h, member form), and
    every value is that of the member's own GP on its own rows, MLL / nvalid[b].

    Scaled form (``scaled`` or an ``outputscale_prior``): k = sigma^2 k_base; a member's x has one
    entry more, the raw outputscale (last), and the chain, the plan and the assembly are the
    scaled ones (evr_kernel_hyper_grad, evr_mll_plan_create_scaled, evr_mll_assemble_scaled)."""

    def __init__(self, Xn: torch.Tensor, Ys: np.ndarray, kind: int, ls_prior, noise_prior, nvalid=None,
                 outputscale_prior=None, scaled: bool = False):
        self.Xn = Xn.contiguous()
        self.n, self.d = Xn.shape[-2:]
        self.kind = kind
        self.Y = torch.as_tensor(np.asarray(Ys, dtype=np.float64), device=Xn.device)   # B x n (standardized)
        self.ls_prior = _prior(ls_prior)
        self.noise_prior = _prior(noise_prior)
        self.os_prior = _prior(outputscale_prior)
        self.scaled = bool(scaled) or self.os_prior is not None
        self.nx = self.d + 2 + int(self.scaled)      # a member's raw vector
        self.use_plan = os.environ.get("EVR_MLL_PLAN", "1") != "0"
        self._plan = None
        self.nvalid = None
        if nvalid is not None:
            self.nvalid = np.ascontiguousarray(nvalid, dtype=np.int32)
            if self.Xn.dim() != 3 or self.nvalid.shape != (self.Xn.shape[0],) or self.Y.shape != self.Xn.shape[:2]:
                raise ValueError(f"members: Xn {tuple(self.Xn.shape)} (B x n x d), Y {tuple(self.Y.shape)} (B x n) "
                                 f"and nvalid {self.nvalid.shape} (B) do not match")
            if self.nvalid.min() < 1 or self.nvalid.max() > self.n:
                raise ValueError(f"members: nvalid must lie in 1..{self.n}")
            self._nvalid_t = torch.as_tensor(self.nvalid, device=Xn.device)
            # 1 on a member's real rows, 0 on its padding
            self._real = (torch.arange(self.n, device=Xn.device)[None, :] < self._nvalid_t[:, None]).to(torch.float64)

    def _eval_ops(self, idx, ls, noise, const, os_=None):
        """The op-by-op chain with the psd_safe_cholesky jitter ladder (host arrays); ``os_``: the
        outputscales of the scaled form (the ladder acts on sigma^2 K_base + noise I)."""
        dev = self.Xn.device
        ls_t = torch.as_tensor(ls, device=dev)
        it = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=dev)
        members = self.nvalid is not None
        os_t = torch.as_tensor(np.ascontiguousarray(os_), device=dev) if self.scaled else None
        if members:
            Xb, real = self.Xn[it].contiguous(), self._real[it]
            nv_t = self._nvalid_t[it].contiguous()
            if self.scaled:     # sigma^2 on the real block, the padding stays the identity
                Ky = ops.kernel_matrix_members_scaled(Xb, nv_t, ls_t, os_t, self.kind,
                                                      diag_add=torch.as_tensor(noise, device=dev))
            else:
                Ky = ops.kernel_matrix_members(Xb, nv_t, ls_t, self.kind, diag_add=torch.as_tensor(noise, device=dev))
        else:
            Ky = ops.kernel_matrix(self.Xn, self.Xn, ls_t, self.kind, outputscale=os_t,
                                   diag_add=torch.as_tensor(noise, device=dev))
        L, Linv, _, info = ops.cholesky_inverse(Ky, 1e-8, 3, raise_on_fail=False)
        r = self.Y[it] - torch.as_tensor(const, device=dev)[:, None]
        if members:
            r = r * real                                                     # r = 0 on padded rows
        r = r.unsqueeze(-1).contiguous()                                     # B x n x 1
        v = ops.gemm(Linv, r)
        alpha = ops.gemm(Linv, v, transA=True)
        W = ops.gemm(alpha, alpha, transB=True)
        ops.gemm(Linv, Linv, transA=True, alpha=-1.0, beta=1.0, out=W)
        gos = None
        if self.scaled and members:
            # the member kernel sums over the member's own rows and columns: the padding's share of
            # gos (W = -1 / (1 + jitter) on its diagonal, k_base = 1) never enters
            gls, gos = ops.kernel_hyper_grad_members(Xb, nv_t, ls_t, os_t, W, self.kind)
        elif self.scaled:
            gls, gos = ops.kernel_hyper_grad(self.Xn, ls_t, os_t, W, self.kind)
        elif members:
            gls = ops.kernel_lengthscale_grad_members(Xb, ls_t, W, self.kind)
        else:
            gls = ops.kernel_lengthscale_grad(self.Xn, ls_t, W, self.kind)
        terms = ops.mll_terms(L, Linv, r[..., 0].contiguous(), alpha[..., 0].contiguous())
        if members:
            # the padded block of the factor is sqrt(1 + jitter) I (jitter 0 unless the ladder was
            # climbed): its share of log det and of tr K^-1 = ||L^-1||_F^2 is taken off exactly;
            # r.alpha, sum alpha and sum alpha^2 get zeros from it
            pad = 1.0 - real
            terms[:, 0] -= 2.0 * (torch.log(L.diagonal(dim1=-2, dim2=-1)) * pad).sum(1)
            terms[:, 2] -= (Linv.diagonal(dim1=-2, dim2=-1) ** 2 * pad).sum(1)
        pieces = [terms.reshape(-1), gls.reshape(-1)] + ([gos.reshape(-1)] if self.scaled else [])
        return torch.cat(pieces + [info.to(torch.float64)]).cpu().numpy()

    def plan_handle(self):
        """The native MLL plan (evr_mll_plan_create[_members]), built on first use."""
        if self._plan is None:
            Bt, d = self.Y.shape[0], self.d
            h = ctypes.c_void_p()
            sfx = "_scaled" if self.scaled else ""
            if self.nvalid is not None:
                ops.call(f"evr_mll_plan_create{sfx}_members", ops._stream(), int(self.kind), Bt, self.n, d,
                         self.Xn.data_ptr(), self.Y.data_ptr(), self.nvalid.ctypes.data, ctypes.byref(h))
            else:
                ops.call(f"evr_mll_plan_create{sfx}", ops._stream(), int(self.kind), Bt, self.n, d, self.Xn.data_ptr(),
                         self.Y.data_ptr(), ctypes.byref(h))
            self._plan = h
            self._lib = _native.load()
            self._params = None
            self._pout = np.empty(Bt * (5 + d + int(self.scaled) + 1))
        return self._plan

    def prior_spec(self) -> np.ndarray:
        """[ls family, a, b, noise family, a, b] for evr_mll_fit_rounds (family 0 none,
        1 LogNormal, 2 Gamma, 3 Normal); the scaled form has three entries more, the outputscale
        prior's."""
        fam = {"lognormal": 1, "gamma": 2, "normal": 3}
        out = np.zeros(9 if self.scaled else 6)
        for k, p in enumerate((self.ls_prior, self.noise_prior) + ((self.os_prior,) if self.scaled else ())):
            if p is not None:
                out[3 * k:3 * k + 3] = (fam[p[0]], p[1], p[2])
        return out

    def _eval_plan(self, idx, ls, noise, const, os_=None):
        """All members through the native MLL plan (evr_mll_plan_eval: one graph launch);
        members outside idx keep their last parameters.  None when an active member's
        attempt-0 factor fails (the caller takes the ladder path)."""
        Bt, d = self.Y.shape[0], self.d
        self.plan_handle()
        sc = int(self.scaled)
        if self._params is None:
            self._params = np.empty((Bt, d + 2 + sc))
            self._params[:, :d] = ls[0]
            self._params[:, d] = noise[0]
            self._params[:, d + 1] = const[0]
            if sc:
                self._params[:, d + 2] = os_[0]
        P = self._params
        for k, b in enumerate(idx):
            P[b, :d], P[b, d], P[b, d + 1] = ls[k], noise[k], const[k]
            if sc:
                P[b, d + 2] = os_[k]
        flat = np.concatenate([P[:, :d].reshape(-1), P[:, d], P[:, d + 1]] + ([P[:, d + 2]] if sc else []))
        _native.check(self._lib.evr_mll_plan_eval(ops._stream(), self._plan, flat.ctypes.data, self._pout.ctypes.data),
                      "evr_mll_plan_eval")
        o = self._pout
        terms, gls = o[:5 * Bt].reshape(Bt, 5), o[5 * Bt:5 * Bt + Bt * d].reshape(Bt, d)
        gos, info = o[5 * Bt + Bt * d:5 * Bt + Bt * (d + sc)], o[5 * Bt + Bt * (d + sc):]
        ii = np.asarray(idx, dtype=np.int64)
        if np.any(info[ii] != 0):
            return None
        return np.concatenate([terms[ii].reshape(-1), gls[ii].reshape(-1)] + ([gos[ii]] if sc else []) + [info[ii]])

    def __del__(self):
        h = getattr(self, "_plan", None)
        if h is not None and getattr(self, "_lib", None) is not None:
            try:
                self._lib.evr_mll_plan_destroy(h)
            except Exception:
                pass
            self._plan = None

    def __call__(self, idx: Sequence[int], xs: Sequence[np.ndarray]):
        n, d = self.n, self.d
        xs = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64) for x in xs]))
        sc = int(self.scaled)
        if xs.shape[1] != self.nx:
            raise ValueError(f"MLLBatch: raw vectors of {xs.shape[1]} entries, expected {self.nx}")
        noise, const, raw = xs[:, 0], xs[:, 1], xs[:, 2:2 + d]
        # softplus with libm's scalar exp / log1p: the native round driver's arithmetic
        ls = np.array([[_softplus_libm(v) for v in row] for row in raw]).reshape(raw.shape)
        os_ = np.array([_softplus_libm(v) for v in xs[:, 2 + d]]) if sc else None
        host = self._eval_plan(idx, ls, noise, const, os_) if self.use_plan else None
        if host is None:
            host = self._eval_ops(idx, ls, noise, const, os_)
        B = len(idx)
        terms_h = np.ascontiguousarray(host[:5 * B].reshape(B, 5))
        gls_h = np.ascontiguousarray(host[5 * B:5 * B + B * d].reshape(B, d))
        gos_h = np.ascontiguousarray(host[5 * B + B * d:5 * B + B * (d + sc)])
        info_h = host[5 * B + B * (d + sc):]
        # ll / n and its gradient with the priors: evr_mll_assemble, the code the native driver
        # (evr_mll_fit_rounds) runs, so both drivers take bitwise the same L-BFGS-B steps
        ll = np.empty(B)
        g = np.empty((B, self.nx))
        lib = _native.load()
        if sc and self.nvalid is not None:
            nv = np.ascontiguousarray(self.nvalid[np.asarray(idx, dtype=np.int64)])
            _native.check(lib.evr_mll_assemble_scaled_members(B, nv.ctypes.data, d, self.prior_spec().ctypes.data,
                                                              xs.ctypes.data, terms_h.ctypes.data, gls_h.ctypes.data,
                                                              gos_h.ctypes.data, ll.ctypes.data, g.ctypes.data),
                          "evr_mll_assemble_scaled_members")
        elif sc:
            _native.check(lib.evr_mll_assemble_scaled(B, n, d, self.prior_spec().ctypes.data, xs.ctypes.data,
                                                      terms_h.ctypes.data, gls_h.ctypes.data, gos_h.ctypes.data,
                                                      ll.ctypes.data, g.ctypes.data), "evr_mll_assemble_scaled")
        elif self.nvalid is not None:      # member b's own size in the -n/2 log 2 pi term and the 1 / n
            nv = np.ascontiguousarray(self.nvalid[np.asarray(idx, dtype=np.int64)])
            _native.check(lib.evr_mll_assemble_members(B, nv.ctypes.data, d, self.prior_spec().ctypes.data,
                                                       xs.ctypes.data, terms_h.ctypes.data, gls_h.ctypes.data,
                                                       ll.ctypes.data, g.ctypes.data), "evr_mll_assemble_members")
        else:
            _native.check(lib.evr_mll_assemble(B, n, d, self.prior_spec().ctypes.data, xs.ctypes.data,
                                               terms_h.ctypes.data, gls_h.ctypes.data, ll.ctypes.data,
                                               g.ctypes.data), "evr_mll_assemble")
        return [None if info_h[k] != 0 or not np.all(np.isfinite(terms_h[k])) else (float(ll[k]), g[k].copy())
                for k in range(B)]


# the last fit_batch's per-output L-BFGS-B evaluation / iteration counts (tools/fit_probe.py)
LAST_FIT_STATS: dict = {}


def _fit_rounds_native(ev: "MLLBatch", B: int, d: int, x0: np.ndarray, lb: np.ndarray, ub: np.ndarray, maxiter: int,
                       maxfun: int, restart_x) -> List[np.ndarray]:
    """fit_batch's lock-step loop in native code (evr_mll_fit_rounds: per round one MLL plan
    evaluation, the -MLL / n value and gradient with the priors, and every member's L-BFGS-B
    steps, with no Python between rounds).  A round in which a member's attempt-0 factor
    fails comes back here: it is evaluated through MLLBatch (the jitter ladder), members that
    stay not p.d. restart from a prior sample, and the others advance (evr_lbfgsb_advance).
    Same algorithm and state machine as the generator loop (lbfgsb_steps)."""
    from .optim import _EPS, LBFGSB_FG

    lib = _native.load()
    nx = ev.nx       # d + 2, or d + 3 over a scaled plan
    lo = np.ascontiguousarray(lb, dtype=np.float64)
    hi = np.ascontiguousarray(ub, dtype=np.float64)
    runs = (ctypes.c_void_p * B)()
    task = np.zeros(B, dtype=np.int32)
    nit = np.zeros(B, dtype=np.int32)
    nfev = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    X = np.zeros((B, nx))
    F = np.zeros(B)
    G = np.zeros((B, nx))
    params = np.zeros(B * nx)
    prior = ev.prior_spec()
    plan = ev.plan_handle()
    i32 = lambda a, k=0: a.ctypes.data + 4 * k  # noqa: E731

    def start(b, xb0):
        if runs[b]:
            lib.evr_lbfgsb_destroy(runs[b])
            runs[b] = None
        h = ctypes.c_void_p()
        _native.check(lib.evr_lbfgsb_create(nx, 10, lo.ctypes.data, hi.ctypes.data, 2.220446049250313e-09 / _EPS,
                                            1e-5, 20, ctypes.byref(h)), "evr_lbfgsb_create")
        runs[b] = h.value
        x0c = np.ascontiguousarray(xb0, dtype=np.float64)
        task[b] = lib.evr_lbfgsb_start(runs[b], x0c.ctypes.data, X[b].ctypes.data)
        nit[b] = nfev[b] = status[b] = 0

    try:
        for b in range(B):
            start(b, x0)
        pending = ctypes.c_int(0)
        while True:
            _native.check(lib.evr_mll_fit_rounds(ops._stream(), plan, ctypes.addressof(runs), task.ctypes.data,
                                                 X.ctypes.data,
                                                 F.ctypes.data, G.ctypes.data, nit.ctypes.data, nfev.ctypes.data,
                                                 status.ctypes.data, int(maxiter), int(maxfun), prior.ctypes.data,
                                                 params.ctypes.data, ctypes.byref(pending)), "evr_mll_fit_rounds")
            if not pending.value:
                break
            idx = [b for b in range(B) if task[b] == LBFGSB_FG]
            vals = ev(idx, [X[b].copy() for b in idx])
            for b, v in zip(idx, vals):
                if v is None:
                    start(b, restart_x(b))
                    continue
                f, g = v
                F[b] = -f
                G[b] = -np.asarray(g, dtype=np.float64)
                _native.check(lib.evr_lbfgsb_advance(runs[b], float(F[b]), G[b].ctypes.data, X[b].ctypes.data,
                                                     i32(task, b), i32(nit, b), i32(nfev, b), i32(status, b),
                                                     int(maxiter), int(maxfun)), "evr_lbfgsb_advance")
        # per-member evaluation / iteration counts (tools/fit_probe.py): max nfev is the number
        # of lock-step rounds since the last restart
        ev.native_stats = {"nfev": nfev.tolist(), "nit": nit.tolist(), "status": status.tolist()}
        LAST_FIT_STATS.update(driver="native", nfev=nfev.tolist(), nit=nit.tolist())
        return [X[b].copy() for b in range(B)]
    finally:
        for b in range(B):
            if runs[b]:
                lib.evr_lbfgsb_destroy(runs[b])


def fit_batch(Xn: torch.Tensor, Y_raw: np.ndarray, kind: int, ls_prior, noise_prior=(-4.0, 1.0),
              max_attempts: int = 10, seed: int = 0, options: Optional[dict] = None,
              standardize: bool = True, outputscale_prior=None, scaled: bool = False) -> List[GPHyper]:
    """fit_single for the B columns of ``Y_raw`` (n x B) on shared inputs, in lock-step: each
    output runs its own L-BFGS-B (the native restatement of scipy's, csrc/lbfgsb.cpp; same
    start, bounds and NotPSDError retries with prior samples as fit_single), and every round
    evaluates the outputs that asked for a function value in ONE batched MLL launch chain.
    The fits stay independent problems, as in the reference's per-surrogate
    fit_gpytorch_mll (bofire/surrogates/single_task_gp.py:70-71)."""
    Y_raw = np.asarray(Y_raw, dtype=np.float64).reshape(Xn.shape[0], -1)
    B = Y_raw.shape[1]
    stats, Ys = [], []
    for b in range(B):
        ym, ys = standardize_params(Y_raw[:, b]) if standardize else (0.0, 1.0)
        stats.append((ym, ys))
        Ys.append((Y_raw[:, b] - ym) / ys)
    lsp, nzp = _prior(ls_prior), _prior(noise_prior)
    ev = MLLBatch(Xn, np.stack(Ys), kind, lsp, nzp, outputscale_prior=outputscale_prior, scaled=scaled)
    return _fit_lockstep(ev, stats, max_attempts, seed, options)


def _fit_lockstep(ev: MLLBatch, stats, max_attempts: int, seed: int, options: Optional[dict]) -> List[GPHyper]:
    """The lock-step L-BFGS-B loop of fit_batch / fit_folds over the members of ``ev`` (shared
    inputs or member form alike); ``stats``: each member's (y_mean, y_std)."""
    from .optim import lbfgsb_steps

    B, d = ev.Y.shape[0], ev.d
    lsp, nzp, osp, sc = ev.ls_prior, ev.noise_prior, ev.os_prior, int(ev.scaled)
    opts = dict(options or {})
    maxiter, maxfun = int(opts.get("maxiter", 15000)), int(opts.get("maxfun", 15000))
    if nzp is not None and nzp[0] == "lognormal":
        noise0 = math.exp(nzp[1] - nzp[2] ** 2)
    elif nzp is not None and nzp[0] == "gamma" and nzp[1] > 1:
        noise0 = (nzp[1] - 1) / nzp[2]
    else:
        noise0 = 2 * MIN_INFERRED_NOISE_LEVEL
    noise0 = max(noise0, MIN_INFERRED_NOISE_LEVEL)
    lb = np.r_[MIN_INFERRED_NOISE_LEVEL, -np.inf, np.full(d + sc, -np.inf)]
    ub = np.full(d + 2 + sc, np.inf)
    rngs = [np.random.default_rng(seed) for _ in range(B)]
    attempts = [0] * B

    def restart_x(b):   # NotPSDError: sample_all_priors, then retry (max_attempts)
        attempts[b] += 1
        if attempts[b] >= max_attempts:
            raise RuntimeError(f"GP fit of output {b} failed after {max_attempts} attempts (NotPSDError)")
        ls = prior_sample_np(lsp, rngs[b], d) if lsp else np.full(d, math.log(2.0))
        nz = max(float(prior_sample_np(nzp, rngs[b], 1)[0]) if nzp else 1e-3, MIN_INFERRED_NOISE_LEVEL)
        x = np.concatenate([[nz, 0.0], np.log(np.expm1(ls))])
        if sc:    # sigma^2 from its prior with the others; without one it goes back to its start
            x = np.append(x, outputscale_restart_raw(osp, rngs[b]))
        return x

    def hyper(b, x):
        return GPHyper(lengthscale=softplus_np(x[2:2 + d]), noise=float(x[0]), constant=float(x[1]),
                       y_mean=stats[b][0], y_std=stats[b][1],
                       outputscale=float(softplus_np(x[2 + d])) if sc else None)

    x_start = np.concatenate([[noise0, 0.0], np.zeros(d + sc)])
    if ev.use_plan and os.environ.get("EVR_FIT_NATIVE", "1") != "0":
        xs = _fit_rounds_native(ev, B, d, x_start, lb, ub, maxiter, maxfun, restart_x)
        return [hyper(b, xs[b]) for b in range(B)]

    def start(x0):
        gen = lbfgsb_steps(x0, lb, ub, maxiter, maxfun)
        return gen, next(gen)

    runs = {b: start(x_start) for b in range(B)}
    result, counts = {}, {}
    while runs:
        idx = sorted(runs)
        vals = ev(idx, [runs[b][1] for b in idx])
        for b, v in zip(idx, vals):
            gen, _ = runs[b]
            if v is None:        # NotPSDError: sample_all_priors, then retry (max_attempts)
                gen.close()
                runs[b] = start(restart_x(b))
                continue
            f, g = v
            try:
                runs[b] = (gen, gen.send((-f, -g)))
            except StopIteration as stop:
                result[b] = stop.value.x
                counts[b] = (stop.value.nfev, stop.value.nit)
                del runs[b]
    LAST_FIT_STATS.update(driver="python", nfev=[counts[b][0] for b in range(B)], nit=[counts[b][1] for b in range(B)])
    return [hyper(b, result[b]) for b in range(B)]


# ---------------------------------------------------------------------------------------
# lock-step fit of members on their own rows: the folds of a cross-validation
# ---------------------------------------------------------------------------------------
# Cap on the device workspace of one member plan (evr_mll_plan_create_members), in bytes: more
# members than fit under it are fitted chunk after chunk.  A memory bound, not a tuning knob.
CV_PLAN_BYTES = 2 << 30


def plan_member_bytes(n: int, d: int) -> int:
    """Device bytes of one member of an MLL plan over n rows and d inputs: K, L and L^-1
    (3 n^2), the factorisation's 64-row panel (64 n), the lengthscale-gradient partials (n d),
    the member's inputs (n d) and its n-vectors (Y, r, v, alpha and the block inverses' share)."""
    return 8 * (3 * n * n + 64 * n + 2 * n * d + 8 * n)


def member_chunks(B: int, n: int, d: int) -> List[range]:
    """Consecutive member ranges whose plans stay under CV_PLAN_BYTES (at least one member each)."""
    per = max(1, CV_PLAN_BYTES // plan_member_bytes(n, d))
    return [range(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def fit_folds(Xb, Y_raw_b: np.ndarray, nvalid, kind: int, ls_prior, noise_prior, standardize: bool,
              max_attempts: int = 10, seed: int = 0, options: Optional[dict] = None, outputscale_prior=None,
              scaled: bool = False) -> List[GPHyper]:
    """fit_batch for B members that each train on their own rows (the folds of
    SingleTaskGPSurrogate.cross_validate): member b has the normalised inputs ``Xb[b]``
    (B x nmax x d, device; rows >= ``nvalid[b]`` are padding and must be zeros) and the raw
    targets ``Y_raw_b[b, :nvalid[b]]``, standardised here with its own statistics.  The same
    lock-step loop, start point, bounds and restarts as fit_batch, over a member MLL plan;
    the members are split into chunks of at most CV_PLAN_BYTES of plan workspace, fitted one
    chunk after another (independent problems: a member's fit does not depend on its chunk
    beyond batched-kernel rounding).  LAST_FIT_STATS holds all members' counts."""
    Xb = torch.as_tensor(Xb, dtype=torch.float64)
    if Xb.device.type != "cuda":
        Xb = Xb.to(torch.device("cuda", torch.cuda.current_device()))
    Xb = Xb.contiguous()
    nvalid = np.asarray(nvalid, dtype=np.int32)
    Y_raw_b = np.asarray(Y_raw_b, dtype=np.float64)
    B, n, d = Xb.shape
    if Y_raw_b.shape != (B, n) or nvalid.shape != (B,) or nvalid.min() < 1 or nvalid.max() > n:
        raise ValueError(f"fit_folds: Xb {tuple(Xb.shape)}, Y {Y_raw_b.shape}, nvalid {nvalid.shape} do not match")
    stats, Ys = [], np.zeros((B, n))
    for b in range(B):
        yb = Y_raw_b[b, :nvalid[b]]
        ym, ys = standardize_params(yb) if standardize else (0.0, 1.0)
        stats.append((ym, ys))
        Ys[b, :nvalid[b]] = (yb - ym) / ys
    lsp, nzp = _prior(ls_prior), _prior(noise_prior)
    hypers, nfev, nit, driver = [], [], [], None
    for ch in member_chunks(B, n, d):
        sl = slice(ch.start, ch.stop)
        ev = MLLBatch(Xb[sl], Ys[sl], kind, lsp, nzp, nvalid=nvalid[sl], outputscale_prior=outputscale_prior,
                      scaled=scaled)
        hypers += _fit_lockstep(ev, stats[sl], max_attempts, seed, options)
        nfev += LAST_FIT_STATS["nfev"]
        nit += LAST_FIT_STATS["nit"]
        driver = LAST_FIT_STATS["driver"]
        del ev          # the chunk's plan is freed before the next one is built
    LAST_FIT_STATS.update(driver=driver, nfev=nfev, nit=nit)
    return hypers


# ---------------------------------------------------------------------------------------
# mixed continuous / categorical GP ([upstream] BoTorch >= 0.13 MixedSingleTaskGP as built by
# bofire/surrogates/mixed_single_task_gp.py:46-112)
# ---------------------------------------------------------------------------------------
# [upstream] restated (BoTorch is not installed; this is the specification the code follows):
#   inputs    the transformed row is split into Xc (n x dc, continuous columns, Normalize bounds)
#             and C (n x nc int32 category codes, OneHotToNumeric: arg-max of each one-hot block)
#   kernel    K(x, x') = s_sum (k_c(r1) + s_cat h1) + s_prod k_c(r2) h2 — ScaleKernel(k_c + ScaleKernel(
#             CategoricalKernel)) + ScaleKernel(k_c * CategoricalKernel), the kernel factories
#             called twice, so two independent continuous and two independent categorical kernels;
#             r_t^2 = sum_k ((xc_k - xc'_k) / ls_t,k)^2, h_t = exp(-(1 / nc) sum_f [c_f != c'_f] / lam_t,f)
#   raw       ls = softplus(raw), lam = 1e-6 + softplus(raw) (GreaterThan(1e-6)), outputscales =
#             softplus(raw), all raw 0 at the start; noise a direct parameter >= 1e-6 starting at
#             1e-3; constant mean a direct parameter starting at 0
#   priors    the data model's lengthscale prior on ls1 and on ls2, its noise prior on the noise;
#             none on lam and the outputscales
#   loss      (MLL + sum log prior) / n on standardised targets, as MLLEvaluator
#   fit       scipy L-BFGS-B; on NotPSDError the parameters with priors are resampled, 5 attempts
#             (fit_gpytorch_mll's default: the reference passes no max_attempts here)
MIXED_MIN_NOISE = 1e-6
MIXED_MIN_LAM = 1e-6
MIXED_NOISE0 = 1e-3


@dataclass
class MixedGPHyper:
    params: np.ndarray        # P = 2 dc + 2 nc + 3: [ls1 | ls2 | lam1 | lam2 | s_sum | s_cat | s_prod]
    noise: float
    constant: float
    y_mean: float
    y_std: float


def mixed_kxx(params: np.ndarray) -> float:
    """k(x, x) = s_sum (1 + s_cat) + s_prod."""
    s_sum, s_cat, s_prod = np.asarray(params, dtype=np.float64)[-3:]
    return float(s_sum * (1.0 + s_cat) + s_prod)


class MixedMLLEvaluator:
    """Exact MLL / n with hyperpriors of the mixed GP on the device, the op-by-op chain of
    MLLEvaluator with the mixed kernel.  Raw parameter vector
    x = [noise, constant, raw ls1, raw ls2, raw lam1 (nc), raw lam2 (nc), raw s_sum, raw s_cat,
    raw s_prod]; raw ls1 / ls2 hold dc values each, or one each with ``ard=False`` (the shared
    lengthscale is broadcast and its gradient summed here)."""

    def __init__(self, Xc: torch.Tensor, C: torch.Tensor, y_std_space: np.ndarray, kind: int, ls_prior,
                 noise_prior, ard: bool = True):
        self.Xc = Xc.contiguous()
        self.C = C.contiguous()
        self.n, self.dc = Xc.shape
        self.nc = C.shape[1]
        self.kind = int(kind)
        self.ard = bool(ard)
        self.nls = self.dc if self.ard else 1
        self.y = np.asarray(y_std_space, dtype=np.float64)
        self.ls_prior = _prior(ls_prior)
        self.noise_prior = _prior(noise_prior)
        self.dev = Xc.device

    @property
    def nx(self) -> int:
        return 2 + 2 * self.nls + 2 * self.nc + 3

    def start(self) -> np.ndarray:
        x0 = np.zeros(self.nx)
        x0[0] = MIXED_NOISE0
        return x0

    def bounds(self):
        return [(MIXED_MIN_NOISE, None)] + [(None, None)] * (self.nx - 1)

    def split(self, x):
        """(noise, constant, raw kernel part in the device layout's order) of x."""
        x = np.asarray(x, dtype=np.float64)
        return float(x[0]), float(x[1]), x[2:]

    def params_of(self, x) -> np.ndarray:
        """The device parameter vector (P) of x."""
        _, _, raw = self.split(x)
        nls, nc, dc = self.nls, self.nc, self.dc
        ls = softplus_np(raw[:2 * nls]).reshape(2, nls)
        lam = MIXED_MIN_LAM + softplus_np(raw[2 * nls:2 * nls + 2 * nc])
        s = softplus_np(raw[2 * nls + 2 * nc:])
        return np.concatenate([np.broadcast_to(ls[:, :1] if not self.ard else ls, (2, dc)).reshape(-1), lam, s])

    def x_of(self, params, noise: float, constant: float) -> np.ndarray:
        """Raw vector of given parameter values (ard=False: the first lengthscale of each kernel)."""
        params = np.asarray(params, dtype=np.float64)
        dc, nc = self.dc, self.nc
        ls = params[:2 * dc].reshape(2, dc)[:, :self.nls].reshape(-1)
        lam = params[2 * dc:2 * dc + 2 * nc] - MIXED_MIN_LAM
        inv = lambda v: v + np.log(-np.expm1(-v))   # noqa: E731
        return np.concatenate([[noise, constant], inv(ls), inv(lam), inv(params[-3:])])

    def hyper(self, x, y_mean: float, y_std: float) -> MixedGPHyper:
        noise, const, _ = self.split(x)
        return MixedGPHyper(params=self.params_of(x), noise=noise, constant=const, y_mean=y_mean, y_std=y_std)

    def __call__(self, x: np.ndarray):
        n, dc = self.n, self.dc
        noise, const, raw = self.split(x)
        params = self.params_of(x)
        dev = self.dev
        p_t = torch.as_tensor(params[None, :], device=dev)
        Ky = ops.mixed_kernel_matrix(self.Xc, self.C, self.Xc, self.C, p_t, self.kind,
                                     diag_add=torch.tensor([noise], dtype=torch.float64, device=dev))
        L, Linv, _, _ = ops.cholesky_inverse(Ky, 1e-8, 3)
        r = torch.as_tensor((self.y - const)[None, :, None], device=dev)
        v = ops.gemm(Linv, r)
        alpha = ops.gemm(Linv, v, transA=True)                       # 1 x n x 1
        W = ops.gemm(alpha, alpha, transB=True)                      # alpha alpha^T
        ops.gemm(Linv, Linv, transA=True, alpha=-1.0, beta=1.0, out=W)   # - K^-1
        gk = ops.mixed_kernel_param_grad(self.Xc, self.C, p_t, W, self.kind)  # 1 x P
        terms = ops.mll_terms(L, Linv, r[..., 0].contiguous(), alpha[..., 0].contiguous())
        terms = terms.cpu().numpy()[0]
        gk = 0.5 * gk.cpu().numpy()[0]
        logdet, quad, trKinv, sum_a, sum_a2 = terms
        ll = -0.5 * quad - 0.5 * logdet - 0.5 * n * math.log(2 * math.pi)
        d_noise = 0.5 * (sum_a2 - trKinv)
        d_const = sum_a
        # the lengthscales as the optimiser sees them (2 x nls): ard=False sums the dc gradients
        d_ls = gk[:2 * dc].reshape(2, dc)
        ls = params[:2 * dc].reshape(2, dc)
        if not self.ard:
            d_ls, ls = d_ls.sum(1, keepdims=True), ls[:, :1]
        if self.ls_prior is not None:
            ll += float(np.sum(prior_logpdf_np(self.ls_prior, ls)))
            d_ls = d_ls + prior_dlogpdf_np(self.ls_prior, ls)
        if self.noise_prior is not None:
            ll += float(prior_logpdf_np(self.noise_prior, noise))
            d_noise += float(prior_dlogpdf_np(self.noise_prior, noise))
        d_val = np.concatenate([d_ls.reshape(-1), gk[2 * dc:]])      # d / d(ls, lam, scales)
        with np.errstate(over="ignore"):     # exp(-raw) = inf at a very negative raw: sigmoid 0, as it should be
            g = np.concatenate([[d_noise, d_const], d_val * sigmoid_np(raw)]) / n
        return ll / n, g


def fit_mixed(Xc: torch.Tensor, C: torch.Tensor, y_raw: np.ndarray, kind: int, ls_prior, noise_prior,
              ard: bool = True, max_attempts: int = 5, seed: int = 0, options: Optional[dict] = None,
              standardize: bool = True) -> MixedGPHyper:
    """fit_gpytorch_mll of the mixed GP restated on the device kernels: scipy L-BFGS-B on -MLL / n
    over the raw parameters of MixedMLLEvaluator (noise >= 1e-6), from noise 1e-3, constant 0 and
    every raw kernel parameter 0; on NotPSDError the parameters with priors (both lengthscale
    sets, the noise) are resampled from them, the others go back to the start, and the fit is
    retried (max_attempts = 5, fit_gpytorch_mll's default)."""
    from scipy.optimize import minimize

    y_raw = np.asarray(y_raw, dtype=np.float64)
    y_mean, y_std = standardize_params(y_raw) if standardize else (0.0, 1.0)
    ev = MixedMLLEvaluator(Xc, C, (y_raw - y_mean) / y_std, kind, ls_prior, noise_prior, ard=ard)
    x0 = ev.start()
    rng = np.random.default_rng(seed)
    last_err = None
    for _ in range(max_attempts):
        try:
            res = minimize(lambda x: tuple(-v for v in ev(x)), x0, jac=True, method="L-BFGS-B", bounds=ev.bounds(),
                           options=options or {})
            return ev.hyper(res.x, y_mean, y_std)
        except ops.NotPSDError as e:  # sample_all_priors, then retry
            last_err = e
            x0 = ev.start()
            if ev.ls_prior is not None:
                ls = prior_sample_np(ev.ls_prior, rng, 2 * ev.nls)
                x0[2:2 + 2 * ev.nls] = np.log(np.expm1(ls))
            if ev.noise_prior is not None:
                x0[0] = max(float(prior_sample_np(ev.noise_prior, rng, 1)[0]), MIXED_MIN_NOISE)
    raise RuntimeError(f"mixed GP fit failed after {max_attempts} attempts: {last_err}")


class MixedGPBatch:
    """B mixed GPs on shared training inputs: Xc (n x dc, normalised continuous columns, device)
    and C (n x nc int32 category codes, device).  Test inputs are given the same way (the caller
    normalises and encodes) — or, once ``set_layout`` has described the transformed row, as raw
    d-wide rows that are split on the device (ops.mixed_split): that is the form the
    single-objective acquisitions read, beside the attributes they share with GPBatch (lo,
    inv_range, d, kxx, M, ...; X_raw, output_keys and rows are set by compatibilize)."""

    mask = None       # every member is trained on every row

    def __init__(self, Xc: torch.Tensor, C: torch.Tensor, Y: torch.Tensor, hypers: Sequence[MixedGPHyper], kind: int):
        self.Xc = Xc.contiguous()
        self.C = C.to(torch.int32).contiguous()
        self.kind = int(kind)
        self.hypers = list(hypers)
        dev = Xc.device
        self.device = dev
        self.B = len(self.hypers)
        self.n, self.dc = Xc.shape
        self.nc = self.C.shape[1]
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        self.params = t(np.stack([h.params for h in self.hypers]))
        self.noise = t([h.noise for h in self.hypers])
        self.const = t([h.constant for h in self.hypers])
        self.ym = t([h.y_mean for h in self.hypers])
        self.ys = t([h.y_std for h in self.hypers])
        self.kxx = t([mixed_kxx(h.params) for h in self.hypers])
        Yc = Y.to(device=dev, dtype=torch.float64).reshape(self.n, self.B).T.contiguous()
        self.y = ((Yc - self.ym[:, None]) / self.ys[:, None]).contiguous()
        self.d = None
        self.refresh()

    def set_layout(self, lo, hi, cont_cols, cat_blocks) -> "MixedGPBatch":
        """Describe the transformed d-wide row: lo / hi (d) the Normalize bounds, cont_cols (dc)
        the columns of the continuous inputs in Xc's order, cat_blocks (nc arrays) the contiguous
        one-hot block of each categorical feature in C's order.  Returns self."""
        dev = self.device
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        hi = np.asarray(hi, dtype=np.float64).reshape(-1)
        d = lo.shape[0]
        cont = np.asarray(cont_cols, dtype=np.int64).reshape(-1)
        blocks = [np.asarray(b, dtype=np.int64).reshape(-1) for b in cat_blocks]
        if cont.shape[0] != self.dc or len(blocks) != self.nc:
            raise ValueError(f"layout of {cont.shape[0]} continuous columns / {len(blocks)} blocks for a model of "
                             f"{self.dc} / {self.nc}")
        for blk in blocks:
            if blk.size < 1 or not np.array_equal(blk, np.arange(blk[0], blk[0] + blk.size)):
                raise ValueError("every one-hot block must be a contiguous range of columns")
        cols = np.concatenate([cont] + blocks)
        if hi.shape[0] != d or cols.min() < 0 or cols.max() >= d or np.unique(cols).size != cols.size:
            raise ValueError(f"column map does not fit rows of {d} columns")
        self.d = int(d)
        self.lo = torch.as_tensor(lo, device=dev)
        self.hi = torch.as_tensor(hi, device=dev)
        # one-hot columns are not normalised (their entries only decide the arg-max)
        ir = np.ones(d)
        ir[cont] = 1.0 / (hi[cont] - lo[cont])
        self.inv_range = torch.as_tensor(ir, device=dev)
        i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=dev)  # noqa: E731
        self.cont_idx = i32(cont)
        self.cat_start = i32([b[0] for b in blocks])
        self.cat_len = i32([b.size for b in blocks])
        return self

    # -- caches: L = chol(K + s2 I), Linv, alpha, M = [Linv; alpha^T] ----------------------
    def refresh(self):
        Ky = ops.mixed_kernel_matrix(self.Xc, self.C, self.Xc, self.C, self.params, self.kind, diag_add=self.noise)
        self.L, self.Linv, _, _ = ops.cholesky_inverse(Ky, 1e-8, 3)
        r = (self.y - self.const[:, None]).unsqueeze(-1).contiguous()           # B x n x 1
        v = ops.gemm(self.Linv, r)
        self.alpha = ops.gemm(self.Linv, v, transA=True)[..., 0].contiguous()  # B x n
        self.M = torch.cat([self.Linv, self.alpha.unsqueeze(1)], dim=1).contiguous()  # B x (n+1) x n

    def kernel_train(self, noise: bool = False) -> torch.Tensor:
        return ops.mixed_kernel_matrix(self.Xc, self.C, self.Xc, self.C, self.params, self.kind,
                                       diag_add=self.noise if noise else None)

    def split(self, Xraw: torch.Tensor):
        """(Xc, C) of raw transformed rows (rows x d), on the device (ops.mixed_split)."""
        if self.d is None:
            raise ValueError("MixedGPBatch: raw rows need set_layout first")
        return ops.mixed_split(Xraw, self.lo, self.inv_range, self.cont_idx, self.cat_start, self.cat_len)

    def cross(self, Xc: torch.Tensor, C: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K(train, test): B x n x nt; test points as (Xc, C), or raw rows alone."""
        if C is None:
            Xc, C = self.split(Xc)
        return ops.mixed_kernel_matrix(self.Xc, self.C, Xc, C, self.params, self.kind)

    def posterior(self, Xc: torch.Tensor, C: Optional[torch.Tensor] = None, observation_noise: bool = False):
        """Mean and variance (B x nt) at normalised continuous columns Xc and category codes C — or,
        with C omitted, at raw transformed rows (split on the device):
        K_* = cross, R = M K_*, then the posterior finalize with k(x, x) = s_sum (1 + s_cat) + s_prod."""
        Xc = Xc.to(device=self.device, dtype=torch.float64).contiguous()
        if C is None:
            Xc, C = self.split(Xc)
        C = C.to(device=self.device, dtype=torch.int32).contiguous()
        R = ops.gemm(self.M, self.cross(Xc, C))
        return ops.posterior_finalize(R, self.const, self.ym, self.ys, self.kxx,
                                      self.noise if observation_noise else None)


# ---------------------------------------------------------------------------------------
# dot-product GPs ([upstream] SingleTaskGP with a gpytorch LinearKernel / PolynomialKernel, as the
# reference builds it for LinearSurrogate / PolynomialSurrogate: bofire/surrogates/mapper.py,
# bofire/kernels/mapper.py)
# ---------------------------------------------------------------------------------------
# [upstream] restated (BoTorch and gpytorch are not installed; this is the specification the code
# follows, parity-unpinned):
#   inputs    the transformed row, continuous columns with the Normalize bounds of get_scaler,
#             one-hot blocks identity (SingleTaskGPSurrogate._bounds / transform_inputs)
#   kernel    power 0:  k(x, x') = v <x, x'>,       v = softplus(raw_v), raw_v = 0 at the start
#             power p:  k(x, x') = (<x, x'> + c)^p, c = softplus(raw_c), raw_c = 0 at the start
#             (1 <= p <= 8 on the device); the prior variance k(x, x) depends on x
#   priors    variance_prior on v / offset_prior on c (optional), the noise prior on the noise
#   mean      ConstantMean, a direct parameter starting at 0; Gaussian noise a direct parameter
#             >= 1e-4; raw vector x = [noise, constant, raw_theta]
#   loss      (MLL + sum log prior) / n on standardised targets, as MLLEvaluator
#   fit       scipy L-BFGS-B from fit_single's noise start; on NotPSDError noise and theta are
#             resampled from their priors (a parameter without one keeps its start value),
#             max_attempts = 10 (bofire/surrogates/single_task_gp.py:71)
DOT_MAX_POWER = ops.DOT_MAX_POWER


def check_dot_power(power) -> int:
    """0 (linear) or the polynomial degree 1..8 the device kernels are built for."""
    if isinstance(power, bool) or int(power) != power:
        raise ValueError(f"power must be an integer, got {power!r}")
    power = int(power)
    if not 0 <= power <= DOT_MAX_POWER:
        raise NotImplementedError(f"dot-product kernels are built for the linear kernel (power 0) and polynomial "
                                  f"powers 1 <= p <= {DOT_MAX_POWER}, got {power}")
    return power


@dataclass
class DotGPHyper:
    power: int                # 0: linear kernel, p >= 1: polynomial kernel of that degree
    theta: float              # the variance v (linear) or the offset c (polynomial)
    noise: float
    constant: float
    y_mean: float
    y_std: float


class DotMLLEvaluator:
    """Exact MLL / n with hyperpriors of one dot-product GP on the device; raw parameter vector
    x = [noise, constant, raw_theta] (theta = softplus(raw_theta)).  The Gram matrix G = Xn Xn^T
    does not depend on the parameters and is formed once here; an evaluation is the element-wise
    map of G, the batched Cholesky (psd_safe ladder), alpha, W = alpha alpha^T - K^-1, the fused
    theta gradient and the scalar terms, and one device-to-host copy."""

    def __init__(self, Xn: torch.Tensor, y_std_space: np.ndarray, power: int, theta_prior, noise_prior):
        self.Xn = Xn.contiguous()
        self.n, self.d = Xn.shape
        self.power = check_dot_power(power)
        self.y = np.asarray(y_std_space, dtype=np.float64)
        self.theta_prior = _prior(theta_prior)
        self.noise_prior = _prior(noise_prior)
        self.dev = Xn.device
        self.G = ops.gemm(self.Xn, self.Xn, transB=True)

    def __call__(self, x: np.ndarray):
        n, dev = self.n, self.dev
        noise, const, raw = float(x[0]), float(x[1]), float(x[2])
        theta = float(softplus_np(raw))
        th_t = torch.tensor([theta], dtype=torch.float64, device=dev)
        Ky = ops.dot_kernel_apply(self.G, th_t, self.power,
                                  diag_add=torch.tensor([noise], dtype=torch.float64, device=dev))
        L, Linv, _, info = ops.cholesky_inverse(Ky, 1e-8, 3, raise_on_fail=False)
        r = torch.as_tensor((self.y - const)[None, :, None], device=dev)
        v = ops.gemm(Linv, r)
        alpha = ops.gemm(Linv, v, transA=True)                       # 1 x n x 1
        W = ops.gemm(alpha, alpha, transB=True)                      # alpha alpha^T
        ops.gemm(Linv, Linv, transA=True, alpha=-1.0, beta=1.0, out=W)   # - K^-1
        gth = ops.dot_kernel_theta_grad(self.G, th_t, W, self.power)
        terms = ops.mll_terms(L, Linv, r[..., 0].contiguous(), alpha[..., 0].contiguous())
        out = torch.cat([terms[0], gth, info.to(torch.float64)]).cpu().numpy()   # the evaluation's one copy
        if out[6] != 0:
            raise ops.NotPSDError("Matrix not positive definite after repeatedly adding jitter up to 1.0e-06")
        logdet, quad, trKinv, sum_a, sum_a2 = out[:5]
        ll = -0.5 * quad - 0.5 * logdet - 0.5 * n * math.log(2 * math.pi)
        d_noise = 0.5 * (sum_a2 - trKinv)
        d_const = sum_a
        d_theta = 0.5 * out[5]
        if self.theta_prior is not None:
            ll += float(prior_logpdf_np(self.theta_prior, theta))
            d_theta += float(prior_dlogpdf_np(self.theta_prior, theta))
        if self.noise_prior is not None:
            ll += float(prior_logpdf_np(self.noise_prior, noise))
            d_noise += float(prior_dlogpdf_np(self.noise_prior, noise))
        with np.errstate(over="ignore"):     # exp(-raw) = inf at a very negative raw: sigmoid 0, as it should be
            g = np.array([d_noise, d_const, d_theta * float(sigmoid_np(raw))]) / n
        return ll / n, g


def fit_dot(Xn: torch.Tensor, y_raw: np.ndarray, power: int, theta_prior=None, noise_prior=None,
            max_attempts: int = 10, seed: int = 0, options: Optional[dict] = None,
            standardize: bool = True) -> DotGPHyper:
    """fit_gpytorch_mll of a dot-product GP restated on the device kernels: scipy L-BFGS-B on
    -MLL / n over x = [noise >= 1e-4, constant, raw_theta] from the noise start of fit_single,
    constant 0 and raw_theta 0 (theta = ln 2); on NotPSDError noise and theta are resampled from
    their priors (a parameter without a prior keeps its start value) and the fit is retried
    (max_attempts = 10, bofire/surrogates/single_task_gp.py:71)."""
    from scipy.optimize import minimize

    power = check_dot_power(power)
    y_raw = np.asarray(y_raw, dtype=np.float64)
    y_mean, y_std = standardize_params(y_raw) if standardize else (0.0, 1.0)
    thp, nzp = _prior(theta_prior), _prior(noise_prior)
    ev = DotMLLEvaluator(Xn, (y_raw - y_mean) / y_std, power, thp, nzp)
    start = np.array([noise_start(nzp), 0.0, 0.0])
    x0 = start.copy()
    bounds = [(MIN_INFERRED_NOISE_LEVEL, None), (None, None), (None, None)]
    rng = np.random.default_rng(seed)
    last_err = None
    for _ in range(max_attempts):
        try:
            res = minimize(lambda x: tuple(-v for v in ev(x)), x0, jac=True, method="L-BFGS-B", bounds=bounds,
                           options=options or {})
            xv = res.x
            return DotGPHyper(power=power, theta=float(softplus_np(xv[2])), noise=float(xv[0]),
                              constant=float(xv[1]), y_mean=y_mean, y_std=y_std)
        except ops.NotPSDError as e:  # sample_all_priors, then retry
            last_err = e
            x0 = start.copy()
            if thp is not None:
                x0[2] = float(np.log(np.expm1(prior_sample_np(thp, rng, 1)[0])))
            if nzp is not None:
                x0[0] = max(float(prior_sample_np(nzp, rng, 1)[0]), MIN_INFERRED_NOISE_LEVEL)
    raise RuntimeError(f"dot-product GP fit failed after {max_attempts} attempts: {last_err}")


class DotGPBatch:
    """B dot-product GPs of one power on shared normalised training rows Xn (n x d, device); lo /
    hi (d) are the Normalize bounds of the transformed row (one-hot columns 0 / 1).  Test inputs
    are raw transformed rows, normalised on the device."""

    mask = None       # every member is trained on every row

    def __init__(self, Xn: torch.Tensor, Y: torch.Tensor, hypers: Sequence[DotGPHyper], lo: torch.Tensor,
                 hi: torch.Tensor):
        self.Xn = Xn.contiguous()
        self.hypers = list(hypers)
        if not self.hypers:
            raise ValueError("DotGPBatch needs at least one member")
        powers = {check_dot_power(h.power) for h in self.hypers}
        if len(powers) != 1:
            raise ValueError(f"the members of a DotGPBatch share one power, got {sorted(powers)}")
        self.power = powers.pop()
        dev = Xn.device
        self.device = dev
        self.B = len(self.hypers)
        self.n, self.d = Xn.shape
        self.lo, self.hi = lo, hi
        self.inv_range = 1.0 / (hi - lo)
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        self.theta = t([h.theta for h in self.hypers])
        self.noise = t([h.noise for h in self.hypers])
        self.const = t([h.constant for h in self.hypers])
        self.ym = t([h.y_mean for h in self.hypers])
        self.ys = t([h.y_std for h in self.hypers])
        Yc = Y.to(device=dev, dtype=torch.float64).reshape(self.n, self.B).T.contiguous()
        self.y = ((Yc - self.ym[:, None]) / self.ys[:, None]).contiguous()
        self.G = ops.gemm(self.Xn, self.Xn, transB=True)
        self.refresh()

    # -- caches: L = chol(K + s2 I), Linv, alpha, M = [Linv; alpha^T] ----------------------
    def refresh(self):
        Ky = ops.dot_kernel_apply(self.G, self.theta, self.power, diag_add=self.noise)
        self.L, self.Linv, _, _ = ops.cholesky_inverse(Ky, 1e-8, 3)
        r = (self.y - self.const[:, None]).unsqueeze(-1).contiguous()           # B x n x 1
        v = ops.gemm(self.Linv, r)
        self.alpha = ops.gemm(self.Linv, v, transA=True)[..., 0].contiguous()  # B x n
        self.M = torch.cat([self.Linv, self.alpha.unsqueeze(1)], dim=1).contiguous()  # B x (n+1) x n

    def kernel_train(self, noise: bool = False) -> torch.Tensor:
        return ops.dot_kernel_apply(self.G, self.theta, self.power, diag_add=self.noise if noise else None)

    def cross(self, Xraw: torch.Tensor) -> torch.Tensor:
        """K(Xtr, normalize(Xraw)) : B x n x nt."""
        Xraw = Xraw.to(device=self.device, dtype=torch.float64)
        Xt = ((Xraw - self.lo) * self.inv_range).contiguous()
        return ops.dot_kernel_apply(ops.gemm(self.Xn, Xt, transB=True), self.theta, self.power)

    def posterior(self, Xraw: torch.Tensor, observation_noise: bool = False):
        """Mean and variance (B x nt) at raw (transformed, unnormalised) inputs (evr_dot_gp_posterior)."""
        Xraw = Xraw.to(device=self.device, dtype=torch.float64).contiguous()
        return ops.dot_gp_posterior(self.Xn, Xraw, self.lo, self.inv_range, self.theta, self.M, self.power,
                                    self.const, self.ym, self.ys, self.noise if observation_noise else None)
