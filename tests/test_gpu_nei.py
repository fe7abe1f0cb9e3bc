"""qNEI / qLogNEI / qLogEI on the MI355X: the improvement scan alone (evr_nei_scan) against
the torch restatement with autograd, the full chain (QNEI / QLogNEI / QLogEI
forward_backward) against tests/nei_reference.py on the same base samples, determinism,
torch autograd, and SoboStrategy end to end with every single-objective acquisition.

Tolerances are the project's bars for the same chain: plain values rtol 1e-6 / atol 1e-10
and gradients rtol 1e-5 / atol 1e-8 (test_qei_joint_batch_parity); log variants 5e-6
absolute in log space and 1e-3 relative gradients per candidate
(test_config3_qlognehvi_values_and_grads_match_oracle).  Every candidate is held."""
import numpy as np
import pytest
import torch

import everest_amd.data_models as dm
from everest_amd import ops, strategies
from everest_amd.benchmarks import DTLZ2
from oracle import gp as ogp
from oracle import qnehvi as oq
from tests import nei_reference as nr

pytestmark = pytest.mark.gpu

A, B = -1.0, 0.0      # MinimizeObjective(w = 1): g = -y


def _sobo_strategy(acquisition_function=None, seed=11):
    """The 25-point, d = 4 Matern SOBO state of test_gpu_strategy._sobo_qei_strategy."""
    bench = DTLZ2(dim=4, num_objectives=2)
    rnd = strategies.map(dm.RandomStrategy(domain=bench.domain, seed=seed))
    exps = bench.f(rnd.ask(25), return_complete=True)
    dom = dm.Domain(inputs=bench.domain.inputs,
                    outputs=dm.Outputs(features=[dm.ContinuousOutput(key="f_0",
                                                                      objective=dm.MinimizeObjective(w=1.0))]))
    spec = dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs, kernel=dm.MaternKernel(nu=2.5))
    kw = {} if acquisition_function is None else {"acquisition_function": acquisition_function}
    s = strategies.map(dm.SoboStrategy(domain=dom, seed=3, surrogate_specs=dm.BotorchSurrogates(surrogates=[spec]),
                                       num_raw_samples=64, num_restarts=2, **kw))
    s.tell(exps[dom.inputs.get_keys() + ["f_0", "valid_f_0"]])
    return s, dom


@pytest.fixture(scope="module")
def state():
    s, dom = _sobo_strategy(dm.qEI(n_mc_samples=128))
    st = s.surrogates.surrogates[0].state
    o = ogp.GPState(X=torch.tensor(st["X"]), y=torch.tensor((st["y"] - st["y_mean"]) / st["y_std"]),
                    lengthscale=torch.tensor(st["lengthscale"]), noise=st["noise"], constant=st["constant"],
                    y_mean=st["y_mean"], y_std=st["y_std"], kind=ogp.MATERN25)
    X_train, _ = s.get_acqf_input_tensors()
    z_prune = oq.base_samples(2048, X_train.shape[0], 1, 5)
    kept = nr.prune_rows([o], torch.tensor(X_train), A, B, z_prune)
    return dict(s=s, o=o, X_train=X_train, z_prune=z_prune, kept=kept)


# ---------------------------------------------------------------------------------------
# the scan alone
# ---------------------------------------------------------------------------------------
def _scan_inputs(S, b, q, seed):
    """Y whose improvements g - best are +-10^u, u uniform in [-9, 3]: (g - best) / tau_relu
    spans -1e9 .. 1e9 (log_fatplus's underflow and linear branches, and everything between)."""
    rng = np.random.default_rng(seed)
    best = torch.tensor(rng.normal(size=S))
    imp = rng.choice([-1.0, 1.0], size=(S, b, q)) * 10.0 ** rng.uniform(-9.0, 3.0, size=(S, b, q))
    imp[0, 0, 0], imp[S - 1, b - 1, q - 1] = -1e3, 1e3
    return imp, best


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("q", [1, 2, 4])
@pytest.mark.parametrize("S", [32, 64, 128])
def test_nei_scan_matches_restatement(S, q, log):
    oa, ob = -1.0, 0.3
    worst = dict(v=0.0, g=0.0)
    for b in (1, 3, 17, 65):
        imp, best_s = _scan_inputs(S, b, q, 1000 * S + 10 * b + q)
        for scalar in (False, True):
            best = best_s[:1].clone() if scalar else best_s
            Y = torch.tensor((imp + best.reshape(-1, 1, 1).numpy() - ob) / oa)      # S x b x q
            for with_gout in (False, True):
                gout = torch.tensor(np.random.default_rng(b).uniform(0.5, 2.0, size=b)) if with_gout else None
                y = Y.clone().requires_grad_(True)
                ref = nr.scan(oa * y + ob, best, log)
                (ref if gout is None else ref * gout).sum().backward()
                flags = torch.zeros(b, dtype=torch.int32)
                flags[b // 2] = 1
                acq, dY = ops.nei_scan(Y.reshape(S, b * q).cuda(), q, best.cuda(), oa, ob, log=log,
                                       tau_relu=nr.TAU_RELU, tau_max=nr.TAU_MAX, flags=flags.cuda(),
                                       gout=None if gout is None else gout.cuda(), backward=True)
                fwd, none = ops.nei_scan(Y.reshape(S, b * q).cuda(), q, best.cuda(), oa, ob, log=log,
                                         tau_relu=nr.TAU_RELU, tau_max=nr.TAU_MAX, flags=flags.cuda())
                acq, dY, fwd = acq.cpu(), dY.cpu().reshape(S, b, q), fwd.cpu()
                ok = flags == 0
                assert none is None and torch.isnan(acq[~ok]).all() and torch.isfinite(acq[ok]).all()
                assert torch.equal(fwd[ok], acq[ok])            # forward-only kernel: the same values
                r, gr = ref.detach(), y.grad
                assert torch.isfinite(dY).all()
                if log:
                    ev = (acq[ok] - r[ok]).abs().max().item() if ok.any() else 0.0
                    eg = ((dY - gr).abs().amax((0, 2)) / gr.abs().amax((0, 2)).clamp_min(1e-300)).max().item()
                    worst["v"], worst["g"] = max(worst["v"], ev), max(worst["g"], eg)
                    assert ev <= 5e-6, (b, scalar, with_gout, ev)
                    assert eg <= 1e-3, (b, scalar, with_gout, eg)
                else:
                    worst["v"] = max(worst["v"], ((acq[ok] - r[ok]).abs() / r[ok].abs().clamp_min(1e-300)).max().item()
                                     if ok.any() else 0.0)
                    worst["g"] = max(worst["g"], (dY - gr).abs().max().item())
                    assert torch.allclose(acq[ok], r[ok], rtol=1e-6, atol=1e-10), (b, scalar, with_gout)
                    assert torch.allclose(dY, gr, rtol=1e-5, atol=1e-8), (b, scalar, with_gout)
    print(f"nei_scan S={S} q={q} log={log}: worst value error {worst['v']:.3e}, gradient error {worst['g']:.3e}")


# ---------------------------------------------------------------------------------------
# the full chain
# ---------------------------------------------------------------------------------------
def _build(state, name, npend, prune, rng):
    from everest_amd.acquisition import QLogEI, QLogNEI, QNEI

    s, X_train = state["s"], state["X_train"]
    Xp = rng.uniform(size=(npend, 4)) if npend else None
    if name == "QLogEI":
        return QLogEI(s.model, X_train, A, B, S=128, seed=9, X_pending_raw=Xp), Xp
    cls = QNEI if name == "QNEI" else QLogNEI
    return cls(s.model, s.model.X_raw, X_train, A, B, S=128, sampler_seed=9, prune_baseline=prune,
               z_prune=state["z_prune"], X_pending_raw=Xp), Xp


def _restatement(state, acqf, name, qq, Xp):
    o = state["o"]
    z_new = acqf._zq(qq).cpu().reshape(128, qq, 1)
    Xpt = None if Xp is None else torch.tensor(Xp)
    if name == "QLogEI":
        return lambda x: nr.log_ei([o], x, acqf.best_f, z_new[..., 0], A, B, X_pending=Xpt)
    Xb = torch.tensor(np.asarray(state["s"].model.X_raw)[acqf.base_rows])
    nei = nr.NEI([o], Xb, A, B, acqf.z_base_host(), z_new, log=name == "QLogNEI", X_pending=Xpt)
    return nei.forward


@pytest.mark.parametrize("q,npend", [(1, 0), (3, 0), (1, 2), (2, 1)])
@pytest.mark.parametrize("name,prune", [("QNEI", True), ("QNEI", False), ("QLogNEI", True), ("QLogNEI", False),
                                        ("QLogEI", False)])
def test_full_chain_matches_restatement(state, name, prune, q, npend):
    rng = np.random.default_rng(q * 10 + npend)
    acqf, Xp = _build(state, name, npend, prune, rng)
    X_train = state["X_train"]
    if name != "QLogEI":
        want = state["kept"].numpy() if prune else np.arange(X_train.shape[0])
        assert np.array_equal(np.asarray(state["s"].model.X_raw)[np.sort(acqf.base_rows)], X_train[want])
    else:
        from everest_amd.acquisition import QEI

        assert acqf.best_f == QEI(state["s"].model, X_train, A, B, S=8).best_f
    Xc = rng.uniform(size=(12, q, 4))
    x = torch.tensor(Xc, requires_grad=True)
    ref = _restatement(state, acqf, name, q + npend, Xp)(x)
    ref.sum().backward()
    acq, dX = acqf.forward_backward(torch.tensor(Xc, device="cuda"))
    acq, dX, r, gr = acq.cpu(), dX.cpu().reshape(12, q, 4), ref.detach(), x.grad
    assert torch.isfinite(acq).all() and torch.isfinite(dX).all()
    assert torch.equal(acqf.forward(torch.tensor(Xc, device="cuda")).cpu(), acq)
    if name == "QNEI":
        print(f"{name} prune={prune} q={q} npend={npend}: max |d acq| {float((acq - r).abs().max()):.3e} "
              f"(max acq {float(r.max()):.3e}), max |d grad| {float((dX - gr).abs().max()):.3e}")
        assert (r > 0).any()
        assert torch.allclose(acq, r, rtol=1e-6, atol=1e-10)
        assert torch.allclose(dX, gr, rtol=1e-5, atol=1e-8)
    else:
        err = (acq - r).abs()
        row = (dX - gr).abs().amax((1, 2)) / gr.abs().amax((1, 2)).clamp_min(1e-300)
        print(f"{name} prune={prune} q={q} npend={npend}: max |d log| {float(err.max()):.3e}, "
              f"max relative gradient error {float(row.max()):.3e}")
        assert (err <= 5e-6).all(), err
        assert (row <= 1e-3).all(), row


def test_forward_backward_is_bitwise_reproducible(state):
    rng = np.random.default_rng(3)
    Xc = torch.tensor(rng.uniform(size=(20, 2, 4)), device="cuda")
    for name in ("QNEI", "QLogNEI", "QLogEI"):
        acqf, _ = _build(state, name, 1, True, rng)
        a1, g1 = acqf.forward_backward(Xc)
        a2, g2 = acqf.forward_backward(Xc)
        assert torch.equal(a1, a2) and torch.equal(g1, g2), name


def test_autograd_equals_forward_backward(state):
    rng = np.random.default_rng(4)
    for name, q, npend in (("QNEI", 2, 0), ("QLogNEI", 1, 1), ("QLogEI", 2, 1)):
        acqf, _ = _build(state, name, npend, True, rng)
        Xc = torch.tensor(rng.uniform(size=(7, q, 4)), device="cuda")
        acq, dX = acqf.forward_backward(Xc)
        x = Xc.clone().requires_grad_(True)
        out = acqf(x)
        out.sum().backward()
        assert torch.equal(out.detach(), acq) and torch.equal(x.grad, dX), name
        w = torch.tensor(rng.uniform(0.5, 2.0, size=7), device="cuda")
        x2 = Xc.clone().requires_grad_(True)
        (acqf(x2) * w).sum().backward()
        _, dXw = acqf.forward_backward(Xc, gout=w)
        assert torch.allclose(x2.grad, dXw, rtol=1e-12, atol=1e-300), name
    flat = torch.tensor(rng.uniform(size=(5, 4)), device="cuda")      # b x d is q = 1
    acqf, _ = _build(state, "QLogNEI", 0, True, rng)
    a, g = acqf.forward_backward(flat)
    assert g.shape == flat.shape and torch.equal(acqf(flat), a)


def test_qnei_operators_equal_forward_backward(state):
    """torch.ops.everest_amd.qnei_forward / qnei_forward_backward / qnei_backward called directly
    on the QneiAcq give forward_backward's values bit for bit (qnei_backward: dX scaled by w)."""
    rng = np.random.default_rng(6)
    for name in ("QNEI", "QLogNEI"):
        acqf, _ = _build(state, name, 0, True, rng)
        Xc = torch.tensor(rng.uniform(size=(5, 2, 4)), device="cuda")
        acq, dX = acqf.forward_backward(Xc)
        tacq = acqf._torch_acq(2)
        assert torch.equal(torch.ops.everest_amd.qnei_forward(tacq, Xc), acq), name
        a2, d2 = torch.ops.everest_amd.qnei_forward_backward(tacq, Xc)
        assert torch.equal(a2, acq) and torch.equal(d2, dX), name
        w = torch.tensor(rng.uniform(0.5, 2.0, size=5), device="cuda")
        assert torch.equal(torch.ops.everest_amd.qnei_backward(tacq, Xc, w), dX * w.view(-1, 1, 1)), name


# ---------------------------------------------------------------------------------------
# SoboStrategy
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("af", [None, "qNEI", "qLogEI"])
def test_sobo_strategy_tell_ask(af):
    from everest_amd.acquisition import QLogEI, QLogNEI, QNEI

    s, dom = _sobo_strategy(None if af is None else getattr(dm, af)())
    keys = dom.inputs.get_keys()
    want = {None: QLogNEI, "qNEI": QNEI, "qLogEI": QLogEI}[af]

    def check(cand, q):
        assert len(cand) == q
        xv = cand[keys].values
        assert ((xv >= 0.0) & (xv <= 1.0)).all()
        acqf, st = s.last_acqf, s.last_ask_stats
        assert type(acqf) is want
        x0 = torch.tensor(np.asarray(st.init_X).reshape(2, q, 4), device="cuda")
        v0 = acqf.forward(x0).cpu()
        vc = acqf.forward(torch.tensor(s._transform(cand).reshape(1, q, 4), device="cuda")).cpu()
        assert torch.isfinite(vc).all() and float(vc[0]) >= float(v0.max()), (vc, v0)

    check(s.ask(1), 1)
    c2 = s.ask(2)
    check(c2, 2)
    c1 = s.ask(1, add_pending=True)
    check(c1, 1)
    assert s.candidates is not None and len(s.candidates) == 1
    c3 = s.ask(1)
    check(c3, 1)
    assert s.last_acqf.n_pending == 1 and not np.allclose(c1[keys].values, c3[keys].values)
    single = s.calc_acquisition(c2[keys])
    joint = s.calc_acquisition(c2[keys], combined=True)
    assert single.shape == (2,) and joint.shape == (1,) and np.isfinite(single).all() and np.isfinite(joint).all()
