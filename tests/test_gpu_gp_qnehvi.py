"""GPU parity of the GP posterior, MLL gradient and qNEHVI forward/backward against the
torch-CPU oracle on identical inputs and base samples.

Tolerances (north_star): posterior moments 1e-4 relative (we assert 1e-9); qNEHVI values
1e-3 relative (we assert 1e-6); gradients vs oracle autograd 1e-6 relative."""
import numpy as np
import pytest
import torch

from oracle import gp as ogp
from oracle import qnehvi as oq
from tests.helpers import device_gp, make_problem, oracle_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", [0, 3, 2])
@pytest.mark.parametrize("n,d,m", [(30, 3, 2), (256, 6, 1), (100, 6, 5)])
def test_posterior_parity(kind, n, d, m):
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=n + d, lo=-np.ones(d), hi=2 * np.ones(d))
    ost = oracle_states(X, Y, lo, hi, hyp, kind)
    gp = device_gp(X, Y, lo, hi, hyp, kind)
    rng = np.random.default_rng(1)
    Xs = lo + (hi - lo) * rng.uniform(size=(300, d))
    for obs in (False, True):
        mean, var = gp.posterior(torch.tensor(Xs, device="cuda"), observation_noise=obs)
        for j in range(m):
            rm, rv = ogp.posterior(ost[j], torch.tensor((Xs - lo) / (hi - lo)), observation_noise=obs)
            sm, sv = ogp.posterior_scipy(ost[j], torch.tensor((Xs - lo) / (hi - lo)), observation_noise=obs)
            assert np.allclose(rm.numpy(), sm, rtol=1e-9, atol=1e-9)  # oracle self-check
            assert torch.allclose(mean[j].cpu(), rm, rtol=1e-9, atol=1e-9 * ost[j].y_std)
            assert torch.allclose(var[j].cpu(), rv, rtol=1e-7, atol=1e-10 * ost[j].y_std ** 2)


def _post_workgroups(n, nt, B):
    """Workgroups of the 32 x 64-tile posterior projection (evr_gp_posterior's switch: PostCfgW
    from 1024 on, else 32 x 32 tiles)."""
    return -(-nt // 64) * -(-n // 32) * B


@pytest.mark.parametrize("n,d,m,nt,wide", [(257, 6, 4, 1857, True),    # PostCfgW, n and nt odd: scalar loads
                                           (130, 16, 8, 1664, True),   # PostCfgW, paired loads; d = 16: MFMA K_*,
                                                                       # the arrival counters zeroed by the memset
                                           (130, 16, 1, 95, False)])   # PostCfg, scalar loads, d >= 16
def test_posterior_projection_dispatch(n, d, m, nt, wide):
    """post_proj_kernel on either side of its 1024-workgroup switch against the oracle, with the
    bars of test_posterior_parity; 8 test points sit on training rows; a second call is bitwise equal
    (the arrival counters are zeroed again, the last arrival sums in a fixed order)."""
    count = _post_workgroups(n, nt, m)
    assert (count >= 1024) == wide, f"{count} workgroups: the case moved to the other kernel"
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=n + d + nt, lo=-np.ones(d), hi=2 * np.ones(d))
    ost = oracle_states(X, Y, lo, hi, hyp)
    gp = device_gp(X, Y, lo, hi, hyp)
    rng = np.random.default_rng(2)
    Xs = lo + (hi - lo) * rng.uniform(size=(nt, d))
    rows = rng.choice(n, 8, replace=False)
    Xs[rng.choice(nt, 8, replace=False)] = X[rows]
    Xd = torch.tensor(Xs, device="cuda")
    Xo = torch.tensor((Xs - lo) / (hi - lo))
    for obs in (False, True):
        mean, var = gp.posterior(Xd, observation_noise=obs)
        mean2, var2 = gp.posterior(Xd, observation_noise=obs)
        torch.cuda.synchronize()
        assert torch.equal(mean, mean2) and torch.equal(var, var2)
        refs = [ogp.posterior(ost[j], Xo, observation_noise=obs) for j in range(m)]
        em = max(float(((mean[j].cpu() - rm).abs() / (1e-9 * ost[j].y_std + 1e-9 * rm.abs())).max())
                 for j, (rm, _) in enumerate(refs))
        ev = max(float(((var[j].cpu() - rv).abs() / (1e-10 * ost[j].y_std ** 2 + 1e-7 * rv.abs())).max())
                 for j, (_, rv) in enumerate(refs))
        print(f"posterior n={n} d={d} m={m} nt={nt} obs={obs}: mean error / bar {em:.3e}, "
              f"variance error / bar {ev:.3e}")
        for j, (rm, rv) in enumerate(refs):
            assert torch.allclose(mean[j].cpu(), rm, rtol=1e-9, atol=1e-9 * ost[j].y_std)
            assert torch.allclose(var[j].cpu(), rv, rtol=1e-7, atol=1e-10 * ost[j].y_std ** 2)


def test_config2_posterior_1024_sobol_points():
    """BASELINE configs[1]: SingleTaskGP RBF, n_train = 256, d = 6,
    X_train ~ U[0,1]^6 (default_rng(0)), y = DTLZ2(6, 5)'s first objective; hyperparameters
    fitted once (device fit, the reference's fit_gpytorch_mll restatement) and then frozen in
    both models; 1024 scrambled Sobol test points (seed 1).  Mean and variance against the
    oracle posterior (north star: 1e-4 relative; asserted 1e-9 / 1e-7)."""
    from everest_amd.gp import GPBatch, fit_single

    rng = np.random.default_rng(0)
    X = rng.uniform(size=(256, 6))
    from tests.helpers import dtlz2
    y = dtlz2(X, 5)[:, 0]
    dev = torch.device("cuda")
    Xn = torch.tensor(X, device=dev)
    prior = ogp.dim_scaled_lognormal(6)
    h = fit_single(Xn, y, 0, prior, (-4.0, 1.0))
    gp = GPBatch(Xn, torch.tensor(y[:, None], device=dev), [h], 0, torch.zeros(6, device=dev, dtype=torch.float64),
                 torch.ones(6, device=dev, dtype=torch.float64))
    st = ogp.GPState(X=torch.tensor(X), y=torch.tensor((y - h.y_mean) / h.y_std), lengthscale=torch.tensor(h.lengthscale),
                     noise=h.noise, constant=h.constant, y_mean=h.y_mean, y_std=h.y_std, kind=ogp.RBF)
    Xs = torch.quasirandom.SobolEngine(6, scramble=True, seed=1).draw(1024, dtype=torch.float64)
    for obs in (False, True):
        mean, var = gp.posterior(Xs.to(dev), observation_noise=obs)
        rm, rv = ogp.posterior(st, Xs, observation_noise=obs)
        assert torch.allclose(mean[0].cpu(), rm, rtol=1e-9, atol=1e-9 * h.y_std)
        assert torch.allclose(var[0].cpu(), rv, rtol=1e-7, atol=1e-10 * h.y_std ** 2)
        sm, sv = ogp.posterior_scipy(st, Xs, observation_noise=obs)    # independent oracle check
        assert np.allclose(rm.numpy(), sm, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("kind", [0, 3])
def test_mll_value_and_grad(kind):
    from everest_amd.gp import MLLEvaluator

    X, Y, lo, hi, hyp = make_problem(n=80, d=5, m=1, seed=3)
    Xn = torch.tensor((X - lo) / (hi - lo))
    y = torch.tensor(Y[:, 0])
    y = (y - y.mean()) / y.std()
    prior = ogp.dim_scaled_lognormal(5)
    ev = MLLEvaluator(Xn.cuda(), y.numpy(), kind, prior, (-4.0, 1.0))
    x = np.array([3e-3, 0.2, -0.3, 0.1, 0.5, -1.0, 0.8])
    v, g = ev(x)
    t = torch.tensor(x, requires_grad=True)
    ref = ogp.mll_value(Xn, y, t[2:], t[0], t[1], kind, prior)
    ref.backward()
    assert abs(v - ref.item()) < 1e-9 * max(1, abs(ref.item()))
    assert np.allclose(g, t.grad.numpy(), rtol=1e-7, atol=1e-9)


def _matched_qnehvi(n, d, m, S, seed, prune, nprune=64, alpha=0.0):
    from everest_amd.acquisition import QNEHVI

    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=seed)
    ost = oracle_states(X, Y, lo, hi, hyp)
    gp = device_gp(X, Y, lo, hi, hyp)
    obj_a, obj_b = -np.ones(m), np.zeros(m)          # MinimizeObjective, bounds (0, 1)
    ref = -1.1 * np.ones(m)
    objective = oq.Objective(torch.tensor(obj_a), torch.tensor(obj_b))
    Xn = torch.tensor((X - lo) / (hi - lo))
    idx = torch.arange(n)
    zp = oq.base_samples(nprune, n, m, 11)
    if prune:
        idx, _ = oq.prune_baseline(ost, Xn, objective, torch.tensor(ref), zp)
    nb = idx.shape[0]
    zb = oq.base_samples(S, nb, m, 7)
    zn = oq.base_samples(S, nb + 1, m, 7)
    orc = oq.QNEHVI(ost, Xn[idx], objective, torch.tensor(ref), zb, zn[:, nb:nb + 1, :], alpha=alpha)
    dq = QNEHVI(gp, X, X, ref, obj_a, obj_b, S=S, prune_baseline=prune, z_prune=zp, z_base_full=zb,
                z_new_full=zn, prune_samples=nprune, alpha=alpha)
    return X, lo, hi, orc, dq, idx


@pytest.mark.parametrize("n,d,m,S,prune", [(20, 3, 2, 16, False), (40, 4, 3, 32, True), (60, 6, 5, 16, True),
                                           (16, 7, 6, 8, False), (16, 8, 7, 8, True), (12, 9, 8, 8, False)])
def test_qnehvi_forward_backward_parity(n, d, m, S, prune):
    X, lo, hi, orc, dq, idx = _matched_qnehvi(n, d, m, S, seed=n, prune=prune)
    assert dq.nb == idx.shape[0]
    assert np.array_equal(np.sort(dq.base_rows), idx.numpy())
    rng = np.random.default_rng(5)
    Xc = lo + (hi - lo) * rng.uniform(size=(37, d))
    Xc[0] = X[0]                                  # a candidate on top of a training point
    acq, dX = dq.forward_backward(torch.tensor(Xc, device="cuda"))
    xt = torch.tensor(Xc, requires_grad=True)
    ref = orc.forward(((xt - torch.tensor(lo)) / torch.tensor(hi - lo)).unsqueeze(1))
    ref.sum().backward()
    a, r = acq.cpu(), ref.detach()
    # Candidate 0 sits on a baseline point: its conditional variance given f(X_base) is exactly
    # zero, so the psd_safe_cholesky rung (0, 1e-8, 1e-7, ...) chosen for the 1x1 new block is
    # decided by the sign of a ~1e-17 rounding error — in the reference as much as here.  Its
    # value is checked against the north-star 1e-3 tolerance relative to the batch scale.
    assert abs(a[0] - r[0]) <= 1e-3 * r.abs().max()
    assert torch.allclose(a[1:], r[1:], rtol=1e-6, atol=1e-9)
    assert torch.allclose(dX.cpu()[1:], xt.grad[1:], rtol=1e-5, atol=1e-7)
    # total cells equal (same partition algorithm) and per-sample HVI of the device cells
    assert dq.stats.total_cells == sum(c.shape[1] for c in orc.cells)


@pytest.mark.parametrize("n,d,m,alpha", [(40, 4, 3, 0.01), (50, 5, 4, 0.001)])
def test_qnehvi_approximate_partition_parity(n, d, m, alpha):
    """alpha > 0 ([upstream] NondominatedPartitioning(alpha), bofire qnehvi.py:50): the host
    approximate cells through the tiled device scan vs the oracle on its own approximate cells;
    the approximation can only lower the value."""
    X, lo, hi, orc, dq, idx = _matched_qnehvi(n, d, m, 16, seed=n + 1, prune=True, alpha=alpha)
    assert dq.box_path == "host-approx"
    assert dq.stats.total_cells == sum(c.shape[1] for c in orc.cells)
    rng = np.random.default_rng(6)
    Xc = lo + (hi - lo) * rng.uniform(size=(29, d))
    acq, dX = dq.forward_backward(torch.tensor(Xc, device="cuda"))
    xt = torch.tensor(Xc, requires_grad=True)
    r = orc.forward(((xt - torch.tensor(lo)) / torch.tensor(hi - lo)).unsqueeze(1))
    r.sum().backward()
    assert torch.allclose(acq.cpu(), r.detach(), rtol=1e-6, atol=1e-9)
    assert torch.allclose(dX.cpu(), xt.grad, rtol=1e-5, atol=1e-7)
    _, _, _, _, dq0, _ = _matched_qnehvi(n, d, m, 16, seed=n + 1, prune=True)
    assert (acq <= dq0.forward(torch.tensor(Xc, device="cuda")) + 1e-12).all()


def test_qnehvi_large_batch_consistency():
    """Batch size independence (b = 1 vs 1024 in one launch) — a size-free property."""
    X, lo, hi, orc, dq, idx = _matched_qnehvi(64, 6, 5, 32, seed=2, prune=True)
    rng = np.random.default_rng(9)
    Xc = torch.tensor(lo + (hi - lo) * rng.uniform(size=(1024, 6)), device="cuda")
    full = dq.forward(Xc)
    part = torch.cat([dq.forward(Xc[i:i + 1]) for i in range(0, 1024, 97)])
    # the tiling plan (and so the summation order) depends on b: equal up to rounding
    assert torch.allclose(full[::97], part, rtol=1e-12, atol=1e-15)
    assert (full >= 0).all()
    again = dq.forward(Xc)
    assert torch.equal(full, again)              # bitwise reproducible for a fixed batch


@pytest.mark.parametrize("dim,n,seed", [(1, 512, 3), (15, 257, 42), (2560, 2048, 987)])
def test_device_sobol_normal_matches_engine(dim, n, seed):
    """Device Sobol-normal samples vs torch SobolEngine + erfinv on the host (the oracle's
    draw): same scrambled points, erfinv agreeing to a few ulp (glibc vs device erf/exp)."""
    from everest_amd import ops

    ref = oq.draw_sobol_normal_samples(dim, n, seed)                    # n x dim
    z = ops.sobol_normal(n, dim, seed, "cuda").cpu()
    assert z.shape == ref.shape
    # erfinv's condition number grows like exp(z^2/2) in the tails: an ulp of erf() in the
    # Newton steps moves z by ~1e-16 * exp(z^2/2); scale the tolerance accordingly.
    err = (z - ref).abs() / (1.0 + torch.exp(ref * ref / 2))
    assert err.max() < 1e-13, (err.max().item(), (z - ref).abs().max().item())
    assert (z == ref).double().mean() > 0.5, (z == ref).double().mean().item()
    if dim % 5 == 0:                                                      # m x points x n layout
        m = 5
        z1 = ops.sobol_normal(n, dim, seed, "cuda", layout=1, m=m).cpu()
        assert torch.equal(z1, z.view(n, dim // m, m).permute(2, 1, 0))
    zt = ops.sobol_normal(n, dim, seed, "cuda", d0=dim - 1, nd=1).cpu()   # tail dims only
    assert torch.equal(zt[:, 0], z[:, -1])


def test_qnehvi_device_samples_match_host_samples():
    """QNEHVI drawing its own (device) base samples equals the build fed the oracle's host
    draws: same pruned baseline, acquisition values to 1e-10."""
    from everest_amd.acquisition import QNEHVI

    n, d, m, S = 60, 6, 5, 32
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=8)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    auto = QNEHVI(gp, X, X, ref, a, b, S=S, sampler_seed=7, prune_baseline=True, prune_seed=11, prune_samples=256)
    nc = n
    zp = oq.base_samples(256, nc, m, 11)
    nb = auto.nb
    host = QNEHVI(gp, X, X, ref, a, b, S=S, prune_baseline=True, prune_samples=256, z_prune=zp,
                  z_base_full=oq.base_samples(S, nb, m, 7), z_new_full=oq.base_samples(S, nb + 1, m, 7))
    assert np.array_equal(auto.base_rows, host.base_rows)
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(3).uniform(size=(64, d)), device="cuda")
    assert torch.allclose(auto.forward(Xc), host.forward(Xc), rtol=1e-10, atol=1e-13)


def test_qnehvi_compressed_cells_match_explicit_cells():
    """Device box decomposition (64-bit cell keys decoded in the scan) vs the host partition
    (explicit [lo, hi] rows): same cell count, same acquisition values and gradients."""
    from everest_amd.acquisition import QNEHVI

    n, d, m, S = 80, 6, 4, 32
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=21)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    kw = dict(S=S, sampler_seed=3, prune_baseline=True, prune_seed=5, prune_samples=256)
    dev_q = QNEHVI(gp, X, X, ref, a, b, box_device=True, **kw)
    host_q = QNEHVI(gp, X, X, ref, a, b, box_device=False, **kw)
    assert dev_q.box_path.startswith("device") and host_q.box_path == "host"
    assert dev_q.stats.total_cells == host_q.stats.total_cells
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(4).uniform(size=(40, d)), device="cuda")
    a1, g1 = dev_q.forward_backward(Xc)
    a2, g2 = host_q.forward_backward(Xc)
    assert torch.allclose(a1, a2, rtol=1e-12, atol=1e-15)
    assert torch.allclose(g1, g2, rtol=1e-10, atol=1e-13)
    assert torch.allclose(dev_q.forward(Xc), a1, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("npend,prune", [(1, True), (4, True), (3, False)])
def test_qnehvi_pending_parity(npend, prune):
    """X_pending joins the pruned baseline (cache_pending, max_iep = 0): device values and
    gradients vs the oracle over the enlarged baseline with the extended base samples."""
    from everest_amd.acquisition import QNEHVI

    n, d, m, S = 40, 4, 3, 32
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=n + npend)
    ost = oracle_states(X, Y, lo, hi, hyp)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    objective = oq.Objective(torch.tensor(a), torch.tensor(b))
    rng = np.random.default_rng(npend)
    Xp = lo + (hi - lo) * rng.uniform(size=(npend, d))
    Xn = torch.tensor((X - lo) / (hi - lo))
    zp = oq.base_samples(64, n, m, 11)
    idx = torch.arange(n)
    if prune:
        idx, _ = oq.prune_baseline(ost, Xn, objective, torch.tensor(ref), zp)
    nb = idx.shape[0]
    zb, zn = oq.base_samples_pending(S, nb, npend, 1, m, 7)
    Xb = torch.cat([Xn[idx], torch.tensor((Xp - lo) / (hi - lo))], 0)
    orc = oq.QNEHVI(ost, Xb, objective, torch.tensor(ref), zb, zn)
    zfull = torch.cat([zb, zn], 1)
    dq = QNEHVI(gp, X, X, ref, a, b, S=S, prune_baseline=prune, z_prune=zp, z_base_full=zb, z_new_full=zfull,
                prune_samples=64, X_pending_raw=Xp)
    assert dq.nb == nb + npend and dq.n_pending == npend
    assert dq.stats.total_cells == sum(c.shape[1] for c in orc.cells)
    Xc = lo + (hi - lo) * np.random.default_rng(5).uniform(size=(29, d))
    acq, dX = dq.forward_backward(torch.tensor(Xc, device="cuda"))
    xt = torch.tensor(Xc, requires_grad=True)
    r = orc.forward(((xt - torch.tensor(lo)) / torch.tensor(hi - lo)).unsqueeze(1))
    r.sum().backward()
    assert torch.allclose(acq.cpu(), r.detach(), rtol=1e-6, atol=1e-9)
    assert torch.allclose(dX.cpu(), xt.grad, rtol=1e-5, atol=1e-7)
    # the op-by-op chain agrees with the native plan
    assert torch.allclose(dq.forward_ops(torch.tensor(Xc, device="cuda")), acq, rtol=1e-12, atol=1e-15)


def test_qnehvi_pending_device_samples_match_host_samples():
    """Pending rows of the device-drawn base samples come from the (nb+np)*m-dim Sobol draw,
    the new point's from the (nb+np+1)*m-dim one: equal to the oracle's host draws."""
    from everest_amd.acquisition import QNEHVI

    n, d, m, S, npend = 50, 5, 4, 32, 2
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=12)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    Xp = lo + (hi - lo) * np.random.default_rng(2).uniform(size=(npend, d))
    auto = QNEHVI(gp, X, X, ref, a, b, S=S, sampler_seed=7, prune_baseline=True, prune_seed=11, prune_samples=128,
                  X_pending_raw=Xp)
    nb = auto.nb - npend
    zb, zn = oq.base_samples_pending(S, nb, npend, 1, m, 7)
    host = QNEHVI(gp, X, X, ref, a, b, S=S, prune_baseline=True, prune_samples=128,
                  z_prune=oq.base_samples(128, n, m, 11), z_base_full=zb, z_new_full=torch.cat([zb, zn], 1),
                  X_pending_raw=Xp)
    assert np.array_equal(auto.base_rows, host.base_rows)
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(3).uniform(size=(64, d)), device="cuda")
    assert torch.allclose(auto.forward(Xc), host.forward(Xc), rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("npend", [0, 2])
def test_qnehvi_fused_root_matches_split_root(npend):
    """The fused quadratic-form root C (C^T C = Linv^T Linv + G^T G / s^2) reproduces the
    literal [Linv; G] operator: values and gradients agree to rounding."""
    from everest_amd.acquisition import QNEHVI

    n, d, m, S = 80, 5, 4, 64
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=21)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    Xp = lo + (hi - lo) * np.random.default_rng(4).uniform(size=(npend, d)) if npend else None
    kw = dict(S=S, sampler_seed=3, prune_baseline=True, prune_seed=5, prune_samples=256, X_pending_raw=Xp)
    fused = QNEHVI(gp, X, X, ref, a, b, root="fused", **kw)
    split = QNEHVI(gp, X, X, ref, a, b, root="split", **kw)
    assert fused.root == "fused" and split.root == "split" and fused.Rr == split.Rr - split.nb
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(6).uniform(size=(200, d)), device="cuda")
    af, gf = fused.forward_backward(Xc)
    as_, gs = split.forward_backward(Xc)
    assert torch.allclose(af, as_, rtol=1e-9, atol=1e-12)
    assert torch.allclose(gf, gs, rtol=1e-7, atol=1e-10)
