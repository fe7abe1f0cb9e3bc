"""GPU: SingleTaskGPSurrogate.cross_validate — all folds fitted in lock-step over a member MLL plan
(gp.fit_folds) and predicted by one masked GPBatch — against the plain sequential loop
(EVR_CV_LOCKSTEP=0: a fresh surrogate per fold, ``_fit`` then ``predict`` twice) and, for two folds,
against ``oracle.gp.fit_gp`` + ``oracle.gp.posterior`` on the CPU.

Domain: DTLZ2(dim=4, num_objectives=2), 23 random experiments plus 0.01 noise, the first output;
experiment 5 lies outside x_1's bounds, so the folds that hold it out normalise with other bounds
than the folds that train on it.

Two fits of one fold are compared with the acceptance rule of
tests/test_gpu_fit.py::test_fit_batch_matches_per_output_fits, unchanged: MLL / n values equal
within 1e-6 max(1, |.|) -> lengthscales to rtol 2e-2 and posterior-mean drift <= 1e-3 y_std;
otherwise the value at most 2 % worse and drift <= 5e-2 y_std.
"""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu
FOLDS, SEED = 4, 3


def _state_hook(surrogate, X_train, y_train, X_test, y_test):
    return copy.deepcopy(surrogate.state)


@pytest.fixture(scope="module")
def setup():
    import everest_amd.data_models as dm
    from everest_amd import strategies, surrogates
    from everest_amd.benchmarks import DTLZ2

    bench = DTLZ2(dim=4, num_objectives=2)
    X = strategies.map(dm.RandomStrategy(domain=bench.domain, seed=7)).ask(23)
    exps = bench.f(X, return_complete=True)
    key = bench.domain.outputs.get_keys()[0]
    exps[key] = exps[key] + 0.01 * np.random.default_rng(1).normal(size=len(exps))
    exps.loc[exps.index[5], "x_1"] = 1.35                       # outside [0, 1]
    exps["labcode"] = [f"L{i}" for i in range(len(exps))]
    spec = dm.SingleTaskGPSurrogate(inputs=bench.domain.inputs,
                                    outputs=dm.Outputs(features=[bench.domain.outputs.get_by_key(key)]))
    return surrogates.SingleTaskGPSurrogate(spec), exps, key


def _run(sur, exps, monkeypatch, lockstep, **kw):
    monkeypatch.setenv("EVR_CV_LOCKSTEP", "1" if lockstep else "0")
    kw.setdefault("folds", FOLDS)
    kw.setdefault("random_state", SEED)
    return sur.cross_validate(exps, hooks={"state": _state_hook}, **kw)


@pytest.fixture(scope="module")
def runs(setup):
    """The lock-step and the sequential cross-validation of the same splits (computed once)."""
    sur, exps, _ = setup
    mp = pytest.MonkeyPatch()
    try:
        lock = _run(sur, exps, mp, True, include_X=True, include_labcodes=True)
        seq = _run(sur, exps, mp, False, include_X=True, include_labcodes=True)
    finally:
        mp.undo()
    return lock, seq


def _mll_and_posterior(sur, state):
    """(MLL / n evaluator, posterior-mean function at normalised points) of one fold's problem."""
    from everest_amd.gp import GPBatch, GPHyper, MLLEvaluator
    from everest_amd.surrogates import map_prior

    Xn = torch.tensor((state["X"] - state["lo"]) / (state["hi"] - state["lo"]), device="cuda")
    d = Xn.shape[1]
    ls_prior = map_prior(sur.kernel.lengthscale_prior, d)
    noise_prior = map_prior(sur.noise_prior, 1)
    yy = (state["y"] - state["y_mean"]) / state["y_std"]
    ev = MLLEvaluator(Xn, yy, state["kind"], ls_prior, noise_prior)
    zero, one = torch.zeros(d, dtype=torch.float64, device="cuda"), torch.ones(d, dtype=torch.float64, device="cuda")
    Xt = torch.tensor(np.random.default_rng(100).uniform(size=(256, d)), device="cuda")

    def value(s):
        return ev(np.r_[s["noise"], s["constant"], np.log(np.expm1(s["lengthscale"]))])[0]

    def mean(s):
        h = GPHyper(lengthscale=s["lengthscale"], noise=s["noise"], constant=s["constant"], y_mean=s["y_mean"],
                    y_std=s["y_std"])
        return GPBatch(Xn, torch.tensor(s["y"][:, None], device="cuda"), [h], s["kind"], zero, one).posterior(Xt)[0][0]

    return value, mean, Xt, (ls_prior, noise_prior)


def _accept(label, vb, vs, ls_b, ls_s, drift):
    """tests/test_gpu_fit.py::test_fit_batch_matches_per_output_fits's rule (b: the fit under
    test, s: the reference fit)."""
    print(f"{label}: MLL/n {vb:.9f} vs {vs:.9f}; lengthscales {np.round(ls_b, 4)} vs {np.round(ls_s, 4)}; "
          f"posterior mean drift {drift:.2e} y_std")
    if abs(vb - vs) <= 1e-6 * max(1.0, abs(vs)):
        assert np.allclose(ls_b, ls_s, rtol=2e-2), label
        assert drift <= 1e-3, (label, drift)
    else:
        assert vb >= vs - 0.02 * max(1.0, abs(vs)), label
        assert drift <= 5e-2, (label, drift)


def _compare_folds(sur, states_b, states_s, label):
    assert len(states_b) == len(states_s)
    for j, (sb, ss) in enumerate(zip(states_b, states_s)):
        for k in ("X", "y", "lo", "hi"):
            assert np.array_equal(sb[k], ss[k]), (j, k)
        assert (sb["y_mean"], sb["y_std"], sb["kind"]) == (ss["y_mean"], ss["y_std"], ss["kind"])
        value, mean, _, _ = _mll_and_posterior(sur, ss)
        drift = float((mean(sb) - mean(ss)).abs().max()) / ss["y_std"]
        _accept(f"{label} fold {j}", value(sb), value(ss), sb["lengthscale"], ss["lengthscale"], drift)


def test_lockstep_matches_sequential(setup, runs):
    sur, exps, key = setup
    (tr_l, te_l, hk_l), (tr_s, te_s, hk_s) = runs
    assert len(tr_l) == len(te_l) == len(tr_s) == FOLDS
    # fold bounds differ from each other: the out-of-bounds experiment is held out by one fold
    his = {tuple(s["hi"]) for s in hk_l["state"]}
    assert len(his) == 2
    _compare_folds(sur, hk_l["state"], hk_s["state"], "lock-step vs sequential")
    seen = []
    for part_l, part_s in ((tr_l, tr_s), (te_l, te_s)):
        for a, b in zip(part_l, part_s):
            assert a.key == b.key == key
            pd.testing.assert_series_equal(a.observed, b.observed)
            assert a.predicted.index.equals(b.predicted.index) and a.predicted.index.equals(a.observed.index)
            assert a.standard_deviation.index.equals(b.standard_deviation.index)
            pd.testing.assert_frame_equal(a.X, b.X)
            pd.testing.assert_series_equal(a.labcodes, b.labcodes)
            assert np.all(np.isfinite(a.predicted.values)) and np.all(a.standard_deviation.values > 0)
    for a in te_l:
        seen += list(a.observed.index)
    assert sorted(seen) == sorted(exps.index)                    # the test folds partition the experiments


def test_matches_cpu_reference(setup, runs):
    """Folds 0 and 3 against oracle.gp.fit_gp / posterior on the CPU, the same rule."""
    from oracle import gp as ogp

    sur, _, _ = setup
    states = runs[0][2]["state"]
    for j in (0, 3):
        s = states[j]
        value, mean, Xt, (ls_prior, noise_prior) = _mll_and_posterior(sur, s)
        Xn = torch.tensor((s["X"] - s["lo"]) / (s["hi"] - s["lo"]))
        st, _ = ogp.fit_gp(Xn, torch.tensor(s["y"]), s["kind"], ls_prior[1:], noise_prior[1:])
        ref = dict(s, lengthscale=st.lengthscale.detach().numpy(), noise=st.noise, constant=st.constant)
        assert abs(st.y_mean - s["y_mean"]) <= 1e-12 * max(1.0, abs(s["y_mean"])) and abs(st.y_std - s["y_std"]) <= 1e-12
        m_ref, _ = ogp.posterior(st, Xt.cpu())
        m_dev = mean(s).cpu()
        drift = float((m_dev - m_ref.detach()).abs().max()) / s["y_std"]
        _accept(f"lock-step vs CPU oracle fold {j}", value(s), value(ref), s["lengthscale"], ref["lengthscale"], drift)


def test_fold_predictions_are_the_fold_surrogates(setup, monkeypatch):
    """A hook returning surrogate.predict(X_test) runs once per fold and gives that fold's test
    CvResult; cross_validate leaves the surrogate's own state alone."""
    sur, exps, key = setup
    sur.fit(exps)
    before = copy.deepcopy(sur.state)
    calls = []

    def hook(surrogate, X_train, y_train, X_test, y_test, tag):
        calls.append((len(X_train), len(X_test), tag))
        assert surrogate is not sur and list(y_test.columns) == [key]
        return surrogate.predict(X_test)

    monkeypatch.setenv("EVR_CV_LOCKSTEP", "1")
    tr, te, out = sur.cross_validate(exps, folds=FOLDS, random_state=SEED, hooks={"p": hook},
                                     hook_kwargs={"p": {"tag": "t"}})
    assert len(calls) == FOLDS == len(out["p"]) and all(c[2] == "t" for c in calls)
    assert sorted(c[1] for c in calls) == [5, 6, 6, 6] and all(c[0] + c[1] == 23 for c in calls)
    for res, pred in zip(te, out["p"]):
        assert res.predicted.index.equals(pred.index)
        # the fold's own GP (its own bounds) and the masked batch member (bounds folded into the
        # lengthscales) are the same model up to rounding
        # lengthscales differ by one rounding (1e-16), the solves magnify it by cond(K) <= n / noise_min
        # = 18 / 1e-4 and the sums by n: <= 1e-9 of |y| ~ 1 on the mean and the variance; the variance is
        # >= noise y_std^2 >= 1e-5, so its square root moves by <= 1e-9 / (2 sd) <= 2e-7
        assert np.abs(res.predicted.values - pred[f"{key}_pred"].values).max() <= 1e-8
        assert np.abs(res.standard_deviation.values - pred[f"{key}_sd"].values).max() <= 1e-6
    for k, v in before.items():
        assert np.array_equal(sur.state[k], v), k
    sur.state, sur.gp = None, None


def test_loo(setup, monkeypatch):
    from everest_amd.diagnostics import RegressionMetricsEnum

    sur, exps, _ = setup
    monkeypatch.setenv("EVR_CV_LOCKSTEP", "1")
    tr, te, _ = sur.cross_validate(exps.iloc[:9], folds=-1)
    assert len(te) == 9 and all(r.n_samples == 1 for r in te) and all(r.n_samples == 8 for r in tr)
    assert te.is_loo and not tr.is_loo
    assert sorted(i for r in te for i in r.observed.index) == sorted(exps.index[:9])
    m = te.get_metrics()
    assert m.shape == (1, 7) and np.all(np.isfinite(m.values)), m
    assert [c for c in m.columns] == [e.name for e in (RegressionMetricsEnum.MAE, RegressionMetricsEnum.MSD,
                                                      RegressionMetricsEnum.R2, RegressionMetricsEnum.MAPE,
                                                      RegressionMetricsEnum.PEARSON, RegressionMetricsEnum.SPEARMAN,
                                                      RegressionMetricsEnum.FISHER)]


def test_native_and_python_drivers_agree(setup, monkeypatch):
    """EVR_FIT_NATIVE=1 and =0 over the member plan: bitwise-equal fold hyperparameters and
    equal evaluation counts (as test_native_fit_rounds_match_python_loop asserts for fit_batch)."""
    from everest_amd.gp import LAST_FIT_STATS

    sur, exps, _ = setup
    out, counts = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("EVR_FIT_NATIVE", mode)
        out[mode] = _run(sur, exps, monkeypatch, True)[2]["state"]
        counts[mode] = (LAST_FIT_STATS.get("driver"), list(LAST_FIT_STATS.get("nfev")))
    assert counts["1"][0] == "native" and counts["0"][0] == "python"
    assert counts["1"][1] == counts["0"][1] and len(counts["1"][1]) == FOLDS, counts
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a["lengthscale"], b["lengthscale"]), (a["lengthscale"], b["lengthscale"])
        assert a["noise"] == b["noise"] and a["constant"] == b["constant"]


def test_chunked_folds(setup, runs, monkeypatch):
    """CV_PLAN_BYTES small enough that the 4 folds run as chunks of 3 + 1: every fold still
    meets the rule against the sequential run."""
    from everest_amd import gp

    sur, exps, _ = setup
    nmax, d = 18, 4                                              # 23 rows in 4 folds: 17 or 18 train rows
    monkeypatch.setattr(gp, "CV_PLAN_BYTES", 3 * gp.plan_member_bytes(nmax, d) + 8)
    assert [len(c) for c in gp.member_chunks(FOLDS, nmax, d)] == [3, 1]
    made = []
    create = gp.MLLBatch.__init__

    def spy(self, Xn, Ys, *a, **kw):
        made.append(tuple(Xn.shape))
        create(self, Xn, Ys, *a, **kw)

    monkeypatch.setattr(gp.MLLBatch, "__init__", spy)
    states = _run(sur, exps, monkeypatch, True)[2]["state"]
    assert made == [(3, nmax, d), (1, nmax, d)], made
    monkeypatch.setattr(gp.MLLBatch, "__init__", create)
    _compare_folds(sur, states, runs[1][2]["state"], "chunked lock-step vs sequential")
