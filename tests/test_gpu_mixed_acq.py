"""GPU: the single-objective acquisition chain on a mixed (MixedSingleTaskGP) model —
forward and forward_backward of QLogEI, QNEI, QLogNEI, QSoboLogEI(log=False) and a two-output
QSoboLogNEI with one sigmoid output constraint against tests/mixed_acq_reference.py (torch
float64, autograd) on the device's own base samples.

n = 24, dc = 2, nc = 2 (3 and 2 levels), S = 32, joint batches of q + pending in {1, 2, 3} (one
case with a pending row of another category) and of 6 and 12 points, b in {1, 5}.
Hyperparameters are fixed draws (noise >= 1e-3), not a fit.  Bars are the chain's (tests/test_gpu_nei.py): plain values rtol
1e-6 / atol 1e-10, log variants 5e-6, gradients rtol 1e-5 / atol 1e-8.  No candidate is left
out: the device returns no NaN and the reference's un-jittered Cholesky succeeds for every
candidate and for the baseline (asserted; the seeds were chosen on the CPU so that it does)."""
import numpy as np
import pytest
import torch

from everest_amd import ops
from everest_amd.gp import MixedGPBatch, MixedGPHyper
from tests import mixed_acq_reference as mar
from tests import nei_reference as nr
from tests import sobo_reference as sr

pytestmark = pytest.mark.gpu

N, DC, NC, S, D = 24, 2, 2, 32, 7
LEVELS = (3, 2)
CONT = np.array([0, 1])
BLOCKS = [np.array([2, 3, 4]), np.array([5, 6])]
LO = np.array([-1.0, 0.5, 0, 0, 0, 0, 0])
HI = np.array([2.0, 3.0, 1, 1, 1, 1, 1])
KIND = 3
A, B = -1.0, 0.0                     # MinimizeObjective(w = 1): g = -y
# (q, pending rows): joint batches of 1, 2, 3 points; the pending row of (1, 1) has the categories
# candidate 0 does not have.  (6, 0) and (11, 1) — the chain's limit of 12 joint points — are what the
# sequential greedy of ask(n) reaches: every pair of the q x q Gram is then computed by its own thread.
CASES = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (6, 0), (11, 1)]


def raw_rows(rng, k):
    """k raw transformed rows: continuous columns inside the bounds, exact one-hot blocks."""
    X = np.zeros((k, D))
    X[:, CONT] = LO[CONT] + rng.uniform(0.05, 0.95, size=(k, DC)) * (HI[CONT] - LO[CONT])
    for blk, lv in zip(BLOCKS, LEVELS):
        X[np.arange(k), blk[rng.integers(0, lv, k)]] = 1.0
    return X


def problem():
    """(X raw n x d, Y n x 2, params 2 x P, noise, const, ym, ys): fixed draws, shared by the GPU
    test and by the CPU check of the reference's Cholesky."""
    rng = np.random.default_rng(20240)
    X = raw_rows(rng, N)
    xc = (X[:, CONT] - LO[CONT]) / (HI[CONT] - LO[CONT])
    c = np.stack([X[:, blk].argmax(1) for blk in BLOCKS], 1)
    off0, off1 = np.array([0.0, 0.6, -0.5]), np.array([0.3, -0.2])
    y0 = ((xc[:, 0] - 0.3) ** 2 + (xc[:, 1] - 0.6) ** 2 + off0[c[:, 0]] + off1[c[:, 1]]
          + 0.02 * rng.normal(size=N))
    y1 = np.sin(3 * xc[:, 0]) + xc[:, 1] * off1[c[:, 1]] + 0.02 * rng.normal(size=N)
    Y = np.stack([y0, y1], 1)
    params = np.concatenate([rng.uniform(0.3, 1.2, (2, 2 * DC)) * np.sqrt(DC), rng.uniform(0.3, 2.0, (2, 2 * NC)),
                             rng.uniform(0.5, 2.0, (2, 3))], 1)
    noise, const = np.array([1e-2, 5e-2]), np.array([0.1, -0.2])
    return X, Y, params, noise, const, Y.mean(0), Y.std(0, ddof=1)


def candidates(q, npend, b):
    """(Xq b x q x d, Xp npend x d | None); the pending rows depend on (q, npend) only."""
    Xp = raw_rows(np.random.default_rng(10 * q + npend), npend) if npend else None
    rng = np.random.default_rng(1000 * q + 100 * npend + b)
    Xq = raw_rows(rng, b * q)
    # most points sit near one of the five best training rows, in its categories: the plain
    # improvements are then positive for most candidates (far from them qEI / qNEI are exactly 0)
    X, Y, *_ = problem()
    top = X[np.argsort(Y[:, 0])[:5]]
    for i in range(b * q):
        if rng.uniform() < 0.75:
            base = top[rng.integers(0, 5)]
            Xq[i] = base
            Xq[i, CONT] = np.clip(base[CONT] + 0.1 * (HI[CONT] - LO[CONT]) * rng.normal(size=DC),
                                  LO[CONT] + 0.01, HI[CONT] - 0.01)
    Xq = Xq.reshape(b, q, D)
    if npend:       # candidate 0 takes another category than the pending row, in both features
        for blk, lv in zip(BLOCKS, LEVELS):
            k = int(Xp[0, blk].argmax())
            Xq[0, 0, blk] = 0.0
            Xq[0, 0, blk[(k + 1) % lv]] = 1.0
    return Xq, Xp


def reference_models(members):
    X, Y, params, noise, const, ym, ys = problem()
    xc = (X[:, CONT] - LO[CONT]) / (HI[CONT] - LO[CONT])
    c = np.stack([X[:, blk].argmax(1) for blk in BLOCKS], 1)
    j = list(members)
    return mar.MixedModels(xc, c, Y[:, j], params[j], noise[j], const[j], ym[j], ys[j], KIND, LO, HI, CONT, BLOCKS)


@pytest.fixture(scope="module")
def gps():
    X, Y, params, noise, const, ym, ys = problem()
    xc = (X[:, CONT] - LO[CONT]) / (HI[CONT] - LO[CONT])
    c = np.stack([X[:, blk].argmax(1) for blk in BLOCKS], 1).astype(np.int32)
    out = {}
    for members in ((0,), (0, 1)):
        hyp = [MixedGPHyper(params=params[j], noise=float(noise[j]), constant=float(const[j]), y_mean=float(ym[j]),
                            y_std=float(ys[j])) for j in members]
        gp = MixedGPBatch(torch.as_tensor(xc, device="cuda"), torch.as_tensor(c, device="cuda"),
                          torch.as_tensor(Y[:, list(members)], device="cuda"), hyp, KIND)
        out[members] = (gp.set_layout(LO, HI, CONT, BLOCKS), reference_models(members))
    return X, out


SPEC2 = dict(terms=[(0, ops.OBJ_AFFINE, 1.0, A, B, 0.0)],
             constraints=[(1, 1.0, 0.7, 0.05)])           # sigmoid constraint: y1 <= 0.7, eta 0.05


def _build(name, X, gp, Xp):
    from everest_amd.acquisition import QLogEI, QLogNEI, QNEI, QSoboLogEI, QSoboLogNEI

    if name == "QLogEI":
        return QLogEI(gp, X, A, B, S=S, seed=9, X_pending_raw=Xp)
    if name in ("QNEI", "QLogNEI"):
        cls = QNEI if name == "QNEI" else QLogNEI
        return cls(gp, X, X, A, B, S=S, sampler_seed=9, prune_baseline=False, X_pending_raw=Xp)
    if name == "QSoboEI":
        return QSoboLogEI(gp, X, ops.SoboSpec(1, [(0, ops.OBJ_AFFINE, 1.0, A, B, 0.0)]), S=S, seed=9,
                          X_pending_raw=Xp, log=False)
    return QSoboLogNEI(gp, X, X, ops.SoboSpec(2, **SPEC2), S=S, sampler_seed=9, prune_baseline=False,
                       X_pending_raw=Xp)


def _reference(name, acqf, ref, X, Xp, qq):
    """x (b x q x d, requires grad) -> (acq (b), every Cholesky succeeded)."""
    m = ref.m
    z_new = acqf._zq(qq).cpu().reshape(S, qq, m)
    Xt = torch.tensor(X)
    log = name in ("QLogEI", "QLogNEI", "QSoboLogNEI")
    nei = name in ("QNEI", "QLogNEI", "QSoboLogNEI")
    util = sr.Utility(SPEC2["terms"])
    cons = sr.constraints_of(SPEC2["constraints"]) if m == 2 else None

    def no_fallback():
        raise AssertionError("every sample needs a feasible baseline row for this test")

    def forward(x):
        if Xp is not None:
            xp = torch.tensor(Xp)
            x = torch.cat([x, xp.unsqueeze(0).expand(x.shape[0], *xp.shape)], 1)
        if nei:
            Ys, Yb, ok = ref.samples(x, z_new, Xt, acqf.z_base_host())
            if m == 1:
                best = (A * Yb[..., 0] + B).amax(1)
            else:
                best = sr.best_feasible(util(Yb), cons.feasible(Yb), no_fallback)
        else:
            Ys, _, ok = ref.samples(x, z_new)
            mean, _ = ref.joint_posterior(Xt)
            best = (A * mean[:, 0] + B).max().reshape(1).detach()
        if m == 1:
            return nr.scan(A * Ys[..., 0] + B, best, log), ok
        return sr.scan(Ys, util, cons, best, log), ok
    return forward


@pytest.mark.parametrize("q,npend", CASES)
@pytest.mark.parametrize("name", ["QLogEI", "QNEI", "QLogNEI", "QSoboEI", "QSoboLogNEI"])
def test_chain_matches_reference(gps, name, q, npend):
    X, models = gps
    gp, ref = models[(0, 1) if name == "QSoboLogNEI" else (0,)]
    log = name in ("QLogEI", "QLogNEI", "QSoboLogNEI")
    acqf = None
    for b in (1, 5):
        Xq, Xp = candidates(q, npend, b)
        if acqf is None:
            acqf = _build(name, X, gp, Xp)
            if hasattr(acqf, "base_jitter"):
                assert float(torch.as_tensor(acqf.base_jitter).abs().max()) == 0.0      # un-jittered baseline
        Xd = torch.tensor(Xq, device="cuda")
        fwd = acqf.forward(Xd).cpu()
        acq, dX = acqf.forward_backward(Xd)
        acq, dX = acq.cpu(), dX.cpu()
        assert not torch.isnan(acq).any() and torch.isfinite(dX).all()                  # no NaN flag
        assert torch.equal(fwd, acq)
        x = torch.tensor(Xq, requires_grad=True)
        r, ok = _reference(name, acqf, ref, X, Xp, q + npend)(x)
        assert ok, "the reference's un-jittered Cholesky failed"
        r.sum().backward()
        onehot = np.setdiff1d(np.arange(D), CONT)
        assert torch.all(dX[..., onehot] == 0.0) and torch.all(x.grad[..., onehot] == 0.0)
        ev = (acq - r.detach()).abs().max().item()
        eg = (dX - x.grad).abs().max().item()
        print(f"{name} q={q} pending={npend} b={b}: value error {ev:.3e}, gradient error {eg:.3e}, "
              f"acq {acq.numpy().round(6).tolist()}")
        if log:
            assert ev <= 5e-6, (b, ev)
        else:
            assert torch.allclose(acq, r.detach(), rtol=1e-6, atol=1e-10), (b, ev)
        assert torch.allclose(dX, x.grad, rtol=1e-5, atol=1e-8), (b, eg)


def test_torch_autograd_path_runs_on_a_mixed_model(gps):
    """The torch.classes path (QneiAcq over a copy of the model struct's bytes): the same values and
    gradient as forward_backward."""
    X, models = gps
    gp, _ = models[(0,)]
    Xq, _ = candidates(2, 0, 5)
    acqf = _build("QLogNEI", X, gp, None)
    Xd = torch.tensor(Xq, device="cuda")
    acq, dX = acqf.forward_backward(Xd)
    xt = Xd.clone().requires_grad_(True)
    v = acqf(xt)
    v.sum().backward()
    assert torch.allclose(v.detach(), acq, rtol=1e-12, atol=0) and torch.allclose(xt.grad, dX, rtol=1e-12, atol=1e-300)


def test_stationary_entry_points_refuse_a_mixed_model(gps):
    from everest_amd.acquisition import QEI, QNEHVI, QNegIntPosVar

    X, models = gps
    gp, _ = models[(0,)]
    acqf = _build("QLogEI", X, gp, None)
    with pytest.raises(RuntimeError, match="mixed"):
        ops.QnehviPlan(acqf.state, acqf.model, 4, True, "cuda")
    # no workspace size is handed out for a call that will be refused
    import ctypes

    from everest_amd import _native
    lib = _native.load()
    st, md = ctypes.byref(acqf.state), ctypes.byref(acqf.model)
    assert lib.evr_qnehvi_plan_workspace_bytes(st, md, 4, 1) == 0
    assert b"mixed" in lib.evr_last_error()
    g = acqf._g(1)
    assert lib.evr_qng_workspace_doubles(st, st, ctypes.byref(g), md, 4, 1) == 0
    assert lib.evr_qlog_workspace_doubles(st, st, ctypes.byref(g), md, 4, 1) == 0
    assert lib.evr_qnei_workspace_doubles(st, ctypes.byref(g), md, 4, 1) > 0
    for make in (lambda: QEI(gp, X, A, B, S=S), lambda: QNegIntPosVar(gp, X[:4]),
                 lambda: QNEHVI(gp, X, X, [-1.0], None, None, S=S)):
        with pytest.raises(NotImplementedError, match="mixed"):
            make()
