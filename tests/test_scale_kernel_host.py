"""CPU: the ``ScaleKernel`` data model (validation, JSON round trips alone and inside strategy
specs, the reference's own dumps from tests/golden/scale_kernel.json, written by
tests/golden/make_scale_kernel_golden.py), the prior factories, the refused nestings, the
outputscale fold, and the host-only assembly of the scaled MLL (evr_mll_assemble_scaled[_members])
against a numpy restatement."""
import json
import math
import os

import numpy as np
import pytest
from pydantic import TypeAdapter, ValidationError

import everest_amd.data_models as dm

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "scale_kernel.json")))
_KERNEL = TypeAdapter(dm.AnyKernel)
_STRATEGY = TypeAdapter(dm.AnyStrategy)


def _io(key="c"):
    inputs = dm.Inputs(features=[dm.ContinuousInput(key="a", bounds=(0, 40)),
                                 dm.ContinuousInput(key="b", bounds=(20, 60))])
    return inputs, dm.Outputs(features=[dm.ContinuousOutput(key=key)])


def _threesix():
    return dm.ScaleKernel(base_kernel=dm.MaternKernel(ard=True, nu=2.5,
                                                      lengthscale_prior=dm.THREESIX_LENGTHSCALE_PRIOR()),
                          outputscale_prior=dm.THREESIX_SCALE_PRIOR())


# ---------------------------------------------------------------------------------------
# data models
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["threesix", "mbo", "rbf_no_prior"])
def test_reference_kernel_dump_loads_and_round_trips(name):
    want = G["kernels"][name]
    k = _KERNEL.validate_python(want)
    assert isinstance(k, dm.ScaleKernel)
    assert json.loads(k.model_dump_json()) == want            # the reference's key set and values, unchanged
    assert _KERNEL.validate_json(k.model_dump_json()) == k


def test_built_kernel_equals_the_reference_dump():
    assert json.loads(_threesix().model_dump_json()) == G["kernels"]["threesix"]
    mbo = dm.ScaleKernel(base_kernel=dm.MaternKernel(lengthscale_prior=dm.MBO_LENGTHCALE_PRIOR()),
                         outputscale_prior=dm.MBO_OUTPUTSCALE_PRIOR())
    assert json.loads(mbo.model_dump_json()) == G["kernels"]["mbo"]
    assert dm.ScaleKernel(base_kernel=dm.RBFKernel()).outputscale_prior is None


@pytest.mark.parametrize("name", ["THREESIX_SCALE_PRIOR", "MBO_LENGTHCALE_PRIOR", "MBO_NOISE_PRIOR",
                                  "MBO_OUTPUTSCALE_PRIOR"])
def test_prior_factories(name):
    p = getattr(dm, name)()
    assert isinstance(p, dm.GammaPrior)
    assert json.loads(p.model_dump_json()) == G["priors"][name]


def test_surrogate_takes_the_reference_spec():
    """The reference's SingleTaskGPSurrogate dump with a ScaleKernel (minus the two fields not
    modelled here) validates, and the surrogate round-trips through JSON."""
    ref = G["SingleTaskGPSurrogate"]
    spec = {k: v for k, v in ref.items() if k not in ("hyperconfig", "aggregations", "inputs", "outputs")}
    inputs, outputs = _io()
    s = dm.SingleTaskGPSurrogate(inputs=inputs, outputs=outputs, **spec)
    assert isinstance(s.kernel, dm.ScaleKernel) and isinstance(s.kernel.base_kernel, dm.MaternKernel)
    got = json.loads(s.model_dump_json())
    assert got["kernel"] == ref["kernel"] and got["noise_prior"] == ref["noise_prior"]
    assert TypeAdapter(dm.SingleTaskGPSurrogate).validate_json(s.model_dump_json()) == s


@pytest.mark.parametrize("cls", ["QnehviStrategy", "SoboStrategy", "ActiveLearningStrategy"])
def test_round_trip_inside_strategy_specs(cls):
    inputs = dm.Inputs(features=[dm.ContinuousInput(key=k, bounds=(0, 1)) for k in ("x1", "x2")])
    keys = ("y0", "y1") if cls == "QnehviStrategy" else ("y0",)
    outputs = dm.Outputs(features=[dm.ContinuousOutput(key=k, objective=dm.MinimizeObjective()) for k in keys])
    domain = dm.Domain(inputs=inputs, outputs=outputs)
    specs = dm.BotorchSurrogates(surrogates=[
        dm.SingleTaskGPSurrogate(inputs=inputs, outputs=dm.Outputs(features=[dm.ContinuousOutput(key=k)]),
                                 kernel=_threesix(), noise_prior=dm.THREESIX_NOISE_PRIOR()) for k in keys])
    extra = dict(ref_point={"y0": 1.0, "y1": 1.0}) if cls == "QnehviStrategy" else {}
    s = getattr(dm, cls)(domain=domain, surrogate_specs=specs, **extra)
    again = _STRATEGY.validate_json(s.model_dump_json())
    assert type(again) is type(s) and again == s
    for sur in again.surrogate_specs.surrogates:
        assert isinstance(sur.kernel, dm.ScaleKernel)
        assert sur.kernel.outputscale_prior == dm.THREESIX_SCALE_PRIOR()
        assert sur.kernel.base_kernel.nu == 2.5


@pytest.mark.parametrize("base", [
    {"type": "LinearKernel"},
    {"type": "PolynomialKernel", "power": 2},
    {"type": "HammingDistanceKernel"},
    {"type": "ScaleKernel", "base_kernel": {"type": "RBFKernel"}},
    {"type": "AdditiveKernel", "kernels": [{"type": "RBFKernel"}]},
])
def test_refused_nestings(base):
    with pytest.raises(ValidationError):
        _KERNEL.validate_python({"type": "ScaleKernel", "base_kernel": base})
    with pytest.raises(ValidationError):
        dm.ScaleKernel(base_kernel=base)


def test_refused_priors_and_places():
    inputs, outputs = _io()
    with pytest.raises(ValidationError):        # the dimensionality-scaled prior belongs to lengthscales
        dm.ScaleKernel(base_kernel=dm.RBFKernel(), outputscale_prior=dm.DimensionalityScaledLogNormalPrior())
    for ok in (dm.GammaPrior(concentration=2.0, rate=0.15), dm.NormalPrior(loc=1.0, scale=0.5),
               dm.LogNormalPrior(loc=0.0, scale=1.0)):
        assert dm.ScaleKernel(base_kernel=dm.RBFKernel(), outputscale_prior=ok).outputscale_prior == ok
    # dot-product kernels stay refused as a SingleTaskGPSurrogate kernel
    for bad in (dm.LinearKernel(), dm.PolynomialKernel(power=2)):
        with pytest.raises(ValidationError):
            dm.SingleTaskGPSurrogate(inputs=inputs, outputs=outputs, kernel=bad)
    # the mixed GP's continuous kernel takes the two stationary kernels only, as in the reference
    cat = dm.Inputs(features=[dm.ContinuousInput(key="a", bounds=(0, 1)),
                              dm.CategoricalInput(key="k", categories=["u", "v"])])
    with pytest.raises(ValidationError):
        dm.MixedSingleTaskGPSurrogate(inputs=cat, outputs=outputs, continuous_kernel=_threesix())
    assert dm.MixedSingleTaskGPSurrogate(inputs=cat, outputs=outputs,
                                         continuous_kernel=dm.RBFKernel()).continuous_kernel.type == "RBFKernel"


# ---------------------------------------------------------------------------------------
# the fold: a scaled GP is exactly an unscaled one
# ---------------------------------------------------------------------------------------
def test_fold_outputscale_is_the_same_gp():
    """Posterior mean, variance and observation noise of (sigma^2, s^2, c, y_std) in float64 numpy
    equal those of the folded (1, s^2 / sigma^2, c / sigma, y_std sigma) to rounding."""
    from everest_amd.gp import GPHyper, fold_outputscale

    rng = np.random.default_rng(3)
    n, d, nt = 25, 3, 7
    X, Xt = rng.uniform(size=(n, d)), rng.uniform(size=(nt, d))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.05 * rng.normal(size=n)
    h = GPHyper(lengthscale=np.array([0.4, 0.9, 1.3]), noise=0.02, constant=0.3, y_mean=float(y.mean()),
                y_std=float(y.std(ddof=1)), outputscale=3.7)
    f = fold_outputscale(h)
    assert f.outputscale is None and fold_outputscale(f) is f
    assert np.array_equal(f.lengthscale, h.lengthscale) and f.y_mean == h.y_mean

    def post(hh, s2):
        k = lambda A, B: s2 * np.exp(-0.5 * (((A[:, None] - B[None]) / hh.lengthscale) ** 2).sum(-1))  # noqa: E731
        ys = (y - hh.y_mean) / hh.y_std
        K = k(X, X) + hh.noise * np.eye(n)
        Ks = k(X, Xt)
        mean = hh.constant + Ks.T @ np.linalg.solve(K, ys - hh.constant)
        var = s2 - np.einsum("ij,ij->j", Ks, np.linalg.solve(K, Ks)) + hh.noise
        return hh.y_mean + hh.y_std * mean, hh.y_std ** 2 * var

    m1, v1 = post(h, h.outputscale)
    m2, v2 = post(f, 1.0)
    assert np.allclose(m1, m2, rtol=0, atol=1e-12 * np.abs(m1).max())
    assert np.allclose(v1, v2, rtol=1e-10)


# ---------------------------------------------------------------------------------------
# evr_mll_assemble_scaled[_members] (host-only) against numpy
# ---------------------------------------------------------------------------------------
PRIORS = [  # ls, noise, outputscale
    (("lognormal", 1.2, 1.7), ("lognormal", -4.0, 1.0), ("gamma", 2.0, 0.15)),
    (("gamma", 3.0, 6.0), ("gamma", 1.1, 0.05), ("lognormal", 0.3, 0.8)),
    (None, ("lognormal", -4.0, 1.0), None),
    (("gamma", 2.0, 0.2), None, ("normal", 1.0, 0.5)),
]


def _restate(n, d, priors, x, t, gls, gos):
    from everest_amd.gp import prior_dlogpdf_np, prior_logpdf_np, sigmoid_np, softplus_np

    lsp, nzp, osp = priors
    noise, raw, raw_os = x[0], x[2:2 + d], x[2 + d]
    ls, os_ = softplus_np(raw), softplus_np(raw_os)
    ll = -0.5 * t[1] - 0.5 * t[0] - 0.5 * n * math.log(2 * math.pi)
    d_noise, d_ls, d_os = 0.5 * (t[4] - t[2]), 0.5 * gls, 0.5 * gos
    if lsp:
        ll += prior_logpdf_np(lsp, ls).sum()
        d_ls = d_ls + prior_dlogpdf_np(lsp, ls)
    if nzp:
        ll += prior_logpdf_np(nzp, noise)
        d_noise += prior_dlogpdf_np(nzp, noise)
    if osp:
        ll += prior_logpdf_np(osp, os_)
        d_os += prior_dlogpdf_np(osp, os_)
    g = np.concatenate([[d_noise, t[3]], d_ls * sigmoid_np(raw), [d_os * sigmoid_np(raw_os)]]) / n
    return ll / n, g


@pytest.mark.parametrize("members", [False, True])
@pytest.mark.parametrize("pi", range(len(PRIORS)))
def test_mll_assemble_scaled_matches_numpy(pi, members):
    from everest_amd import _native

    lib = _native.load()
    fam = {"lognormal": 1, "gamma": 2, "normal": 3}
    prior = np.zeros(9)
    for k, p in enumerate(PRIORS[pi]):
        if p is not None:
            prior[3 * k:3 * k + 3] = (fam[p[0]], p[1], p[2])
    rng = np.random.default_rng(40 + pi)
    B, n, d = 4, 37, 5
    x = np.concatenate([rng.uniform(1e-3, 0.3, (B, 1)), rng.normal(size=(B, 1)), rng.normal(size=(B, d + 1)) * 2], 1)
    x[0, 2 + d] = 0.0                      # the start value: softplus(0) = ln 2 exactly
    x[1, 2 + d] = -9.0                     # sigma^2 far below the noise
    terms, gls, gos = rng.normal(size=(B, 5)) * 10, rng.normal(size=(B, d)) * 5, rng.normal(size=B) * 20
    x, terms, gls, gos = (np.ascontiguousarray(a) for a in (x, terms, gls, gos))
    ll, g = np.empty(B), np.empty((B, d + 3))
    nv = np.array([37, 30, 5, 1], dtype=np.int32)
    if members:
        rc = lib.evr_mll_assemble_scaled_members(B, nv.ctypes.data, d, prior.ctypes.data, x.ctypes.data,
                                                 terms.ctypes.data, gls.ctypes.data, gos.ctypes.data, ll.ctypes.data,
                                                 g.ctypes.data)
    else:
        rc = lib.evr_mll_assemble_scaled(B, n, d, prior.ctypes.data, x.ctypes.data, terms.ctypes.data,
                                         gls.ctypes.data, gos.ctypes.data, ll.ctypes.data, g.ctypes.data)
    assert rc == 0
    for b in range(B):
        wl, wg = _restate(int(nv[b]) if members else n, d, PRIORS[pi], x[b], terms[b], gls[b], gos[b])
        assert abs(ll[b] - wl) <= 1e-14 * abs(wl), (b, ll[b], wl)
        assert np.all(np.abs(g[b] - wg) <= 1e-14 * np.abs(wg)), (b, g[b], wg)


def test_unscaled_assemble_is_untouched_by_the_scaled_form():
    """The first d + 2 entries keep their meaning: with gos = 0 and no outputscale prior the scaled
    assembly's value and first d + 2 gradient entries are bitwise the unscaled call's."""
    from everest_amd import _native

    lib = _native.load()
    rng = np.random.default_rng(9)
    B, n, d = 3, 20, 4
    prior6 = np.array([1, 1.2, 1.7, 1, -4.0, 1.0])
    prior9 = np.r_[prior6, 0.0, 0.0, 0.0]
    x3 = np.ascontiguousarray(np.concatenate([rng.uniform(1e-3, 0.3, (B, 1)), rng.normal(size=(B, d + 2))], 1))
    x2 = np.ascontiguousarray(x3[:, :d + 2])
    terms, gls, gos = rng.normal(size=(B, 5)), rng.normal(size=(B, d)), np.zeros(B)
    l2, g2, l3, g3 = np.empty(B), np.empty((B, d + 2)), np.empty(B), np.empty((B, d + 3))
    assert lib.evr_mll_assemble(B, n, d, prior6.ctypes.data, x2.ctypes.data, terms.ctypes.data, gls.ctypes.data,
                                l2.ctypes.data, g2.ctypes.data) == 0
    assert lib.evr_mll_assemble_scaled(B, n, d, prior9.ctypes.data, x3.ctypes.data, terms.ctypes.data,
                                       gls.ctypes.data, gos.ctypes.data, l3.ctypes.data, g3.ctypes.data) == 0
    assert np.array_equal(l2, l3) and np.array_equal(g2, g3[:, :d + 2]) and np.all(g3[:, d + 2] == 0.0)


@pytest.mark.parametrize("kind,prior", [(0, ("gamma", 2.0, 0.15)), (3, ("lognormal", 0.3, 0.8)), (2, None)])
def test_assembly_of_reference_pieces_equals_autograd(kind, prior):
    """The whole scaled formula without the device: W = alpha alpha^T - K^-1 in numpy, the gradient
    pieces from the long-double references (lengthscale_grad times sigma^2, outputscale_grad), the
    five terms, then evr_mll_assemble_scaled — against CPU autograd of the restated MLL."""
    from everest_amd import _native
    from tests import gp_kernel_reference as ref
    from tests import scale_kernel_reference as sref

    n, d = 33, 4
    X, Ys, xs = sref.scaled_case(n, d, 3)
    lsp, nzp = ("lognormal", 1.2, 1.7), ("lognormal", -4.0, 1.0)
    fam = {"lognormal": 1, "gamma": 2, "normal": 3}
    spec = np.zeros(9)
    for k, p in enumerate((lsp, nzp, prior)):
        if p is not None:
            spec[3 * k:3 * k + 3] = (fam[p[0]], p[1], p[2])
    lib = _native.load()
    for b in range(3):
        x = np.ascontiguousarray(xs[b])
        ls, os_ = np.logaddexp(0.0, x[2:2 + d]), float(np.logaddexp(0.0, x[2 + d]))
        K = os_ * ref.train_matrix(X, ls, 0.0, kind) + x[0] * np.eye(n)
        L = np.linalg.cholesky(K)
        Linv = np.linalg.inv(L)
        r = Ys[b] - x[1]
        alpha = Linv.T @ (Linv @ r)
        W = np.outer(alpha, alpha) - Linv.T @ Linv
        gls = (ref.lengthscale_grad(X, ls[None], W[None], kind)[0][0] * os_).astype(np.float64)
        gos = sref.outputscale_grad(X, ls[None], W[None], kind)[0].astype(np.float64)
        terms = ref.mll_terms(L[None], Linv[None], r[None], alpha[None])[0][0].astype(np.float64)
        # the five-term identity gives the same sigma^2 piece (a cross-check; it cancels when sigma^2 << noise)
        ident = (terms[1] - n - x[0] * (terms[4] - terms[2])) / os_
        assert abs(ident - gos[0]) <= 1e-9 * max(1.0, abs(gos[0]))
        ll, g = np.empty(1), np.empty(d + 3)
        terms, gls = np.ascontiguousarray(terms), np.ascontiguousarray(gls)
        assert lib.evr_mll_assemble_scaled(1, n, d, spec.ctypes.data, x.ctypes.data, terms.ctypes.data,
                                           gls.ctypes.data, gos.ctypes.data, ll.ctypes.data, g.ctypes.data) == 0
        wv, wg = sref.mll_value_and_grad(X, Ys[b], x, d, kind, lsp, nzp, prior)
        assert abs(ll[0] - wv) <= 1e-9 * max(1.0, abs(wv))
        assert np.allclose(g, wg, rtol=1e-7, atol=1e-9), (g, wg)


def test_resampled_outputscale_is_finite_for_every_prior():
    """The NotPSDError restart of sigma^2: a draw from the prior through the inverse softplus, finite
    for every family the data model allows (a NormalPrior centred at 0 draws next to 0), raw 0
    without a prior."""
    from everest_amd.gp import MIN_RESAMPLED_OUTPUTSCALE, outputscale_restart_raw

    assert outputscale_restart_raw(None, np.random.default_rng(0)) == 0.0

    class Zero:                                   # a generator whose normal draw is exactly 0
        def normal(self, a, b, size):
            return np.zeros(size)

    raw = outputscale_restart_raw(("normal", 0.0, 1.0), Zero())
    assert np.isfinite(raw) and abs(np.logaddexp(0.0, raw) - MIN_RESAMPLED_OUTPUTSCALE) <= 1e-12
    for prior in (("normal", 0.0, 1e-9), ("normal", 1.0, 0.5), ("gamma", 2.0, 0.15), ("lognormal", 0.3, 0.8)):
        rng = np.random.default_rng(1)
        raws = np.array([outputscale_restart_raw(prior, rng) for _ in range(200)])
        assert np.all(np.isfinite(raws)), prior
        assert np.all(np.logaddexp(0.0, raws) >= MIN_RESAMPLED_OUTPUTSCALE * (1 - 1e-9))
    # a large draw goes through unchanged: softplus(raw) is the draw
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(5)
    v = float(rng_a.gamma(2.0, 1.0 / 0.15, 1)[0])
    assert abs(np.logaddexp(0.0, outputscale_restart_raw(("gamma", 2.0, 0.15), rng_b)) - v) <= 1e-12 * v
