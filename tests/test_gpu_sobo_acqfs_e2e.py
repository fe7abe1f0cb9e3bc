"""SoboStrategy / AdditiveSoboStrategy with qSR, qUCB and qPI end to end on the MI355X: tell,
ask(1), ask(2), calc_acquisition, reproducibility under a seed; QparegoStrategy keeps refusing
the three.

State: 25 points, d = 4, DTLZ2(dim=4, num_objectives=2), Matern-2.5; f_0 Minimize, f_1
MinimizeSigmoid with tp at the median of the observed f_1 (an output constraint for SoboStrategy
and for AdditiveSoboStrategy(use_output_constraints=True))."""
import numpy as np
import pytest
import torch
from pydantic import TypeAdapter

import everest_amd.data_models as dm
from everest_amd import strategies
from everest_amd.benchmarks import DTLZ2

pytestmark = pytest.mark.gpu

_ANY = TypeAdapter(dm.AnyStrategy)

ACQFS = {"qSR": lambda: dm.qSR(n_mc_samples=128), "qUCB": lambda: dm.qUCB(beta=0.5, n_mc_samples=128),
         "qPI": lambda: dm.qPI(tau=1e-2, n_mc_samples=128)}


@pytest.fixture(scope="module")
def problem():
    bench = DTLZ2(dim=4, num_objectives=2)
    rnd = strategies.map(dm.RandomStrategy(domain=bench.domain, seed=11))
    exps = bench.f(rnd.ask(25), return_complete=True)
    f1 = dm.MinimizeSigmoidObjective(w=0.5, steepness=4.0, tp=float(np.median(exps["f_1"].values)))
    dom = dm.Domain(inputs=bench.domain.inputs,
                    outputs=dm.Outputs(features=[dm.ContinuousOutput(key="f_0", objective=dm.MinimizeObjective(w=1.0)),
                                                 dm.ContinuousOutput(key="f_1", objective=f1)]))
    return dom, exps


def _strategy(cls, dom, exps, af, **kw):
    specs = [dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[dom.outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in ("f_0", "f_1")]
    data_model = cls(domain=dom, seed=3, surrogate_specs=dm.BotorchSurrogates(surrogates=specs), num_raw_samples=64,
                     num_restarts=2, acquisition_function=af, **kw)
    # the reference-format JSON round trip is what a user loads
    data_model = _ANY.validate_json(data_model.model_dump_json())
    assert type(data_model) is cls
    s = strategies.map(data_model)
    s.tell(exps[dom.inputs.get_keys() + ["f_0", "f_1", "valid_f_0", "valid_f_1"]])
    return s


def _check(s, cand, q, want):
    keys = s.domain.inputs.get_keys()
    assert len(cand) == q
    xv = cand[keys].values
    assert ((xv >= 0.0) & (xv <= 1.0)).all()
    acqf, st = s.last_acqf, s.last_ask_stats
    assert type(acqf) is want
    # the Boltzmann initial conditions always hold the best raw sample of the ask
    x0 = torch.tensor(np.asarray(st.init_X).reshape(2, q, 4), device="cuda")
    v0 = acqf.forward(x0).cpu()
    vc = acqf.forward(torch.tensor(s._transform(cand).reshape(1, q, 4), device="cuda")).cpu()
    assert torch.isfinite(vc).all() and float(vc[0]) >= float(v0.max()), (vc, v0)
    return float(vc[0])


@pytest.mark.parametrize("name", list(ACQFS))
@pytest.mark.parametrize("kind", ["sobo", "additive", "additive_absorbed"])
def test_strategy_asks_with_reward_acquisitions(problem, kind, name):
    from everest_amd.acquisition import QSoboPI, QSoboSR, QSoboUCB

    dom, exps = problem
    want = {"qSR": QSoboSR, "qUCB": QSoboUCB, "qPI": QSoboPI}[name]
    cls = dm.SoboStrategy if kind == "sobo" else dm.AdditiveSoboStrategy
    kw = {} if kind == "sobo" else {"use_output_constraints": kind == "additive"}
    s, twin = (_strategy(cls, dom, exps, ACQFS[name](), **kw) for _ in range(2))
    keys = dom.inputs.get_keys()
    c1 = s.ask(1)
    _check(s, c1, 1, want)
    acqf = s.last_acqf
    if kind == "additive_absorbed":
        assert acqf.spec.constraints == [] and len(acqf.spec.terms) == 2
    else:
        assert len(acqf.spec.constraints) == 1 and len(acqf.spec.terms) == 1
    if name == "qPI":
        assert acqf.infeasible_cost == 0.0 and acqf.tau == 1e-2 and np.isfinite(acqf.best_f)
    else:
        assert acqf.nonnegative is False
        if kind == "additive_absorbed":
            assert acqf.infeasible_cost == 0.0
        else:
            assert acqf.infeasible_cost > 0.0       # f_0 >= 0 is minimised: u(mu - 6 sigma) goes below zero
        if name == "qUCB":
            assert acqf.beta == 0.5
    assert acqf.S == 128
    c2 = s.ask(2)
    _check(s, c2, 2, want)
    # same seed, same candidates
    t1, t2 = twin.ask(1), twin.ask(2)
    assert np.array_equal(c1[keys].values, t1[keys].values) and np.array_equal(c2[keys].values, t2[keys].values)
    # calc_acquisition builds its own acquisition (the next seeds of the generator): a direct forward of that one
    val = s.calc_acquisition(c1[keys])
    direct = s.last_acqf.forward(torch.tensor(s._transform(c1).reshape(1, 1, 4), device="cuda")).cpu().numpy()
    assert type(s.last_acqf) is want and val.shape == (1,) and np.array_equal(val, direct)
    joint = s.calc_acquisition(c2[keys], combined=True)
    assert joint.shape == (1,) and np.isfinite(joint).all()


def test_infeasible_cost_is_reproducible_and_drawn_first(problem):
    dom, exps = problem
    a, b = (_strategy(dm.SoboStrategy, dom, exps, dm.qSR(n_mc_samples=128)) for _ in range(2))
    acq_a, acq_b = a._get_acqfs(1)[0], b._get_acqfs(1)[0]
    assert acq_a.infeasible_cost == acq_b.infeasible_cost > 0.0
    assert acq_a.sampler_seed == acq_b.sampler_seed
    # qPI draws no RandomStrategy seed: its sampler seed is the generator's first draw, qSR's the second
    c = _strategy(dm.SoboStrategy, dom, exps, dm.qPI(n_mc_samples=128))
    g = torch.Generator().manual_seed(3)
    first = int(torch.randint(1, 1000001, (1,), generator=g).item())
    second = int(torch.randint(0, 1000000, (1,), generator=g).item())
    assert acq_a.sampler_seed == second
    g = torch.Generator().manual_seed(3)
    assert c._get_acqfs(1)[0].sampler_seed == int(torch.randint(0, 1000000, (1,), generator=g).item())
    assert first >= 1


def test_qparego_keeps_refusing_the_reward_acquisitions(problem):
    dom, exps = problem
    bench = DTLZ2(dim=4, num_objectives=2)
    specs = [dm.SingleTaskGPSurrogate(inputs=bench.domain.inputs,
                                      outputs=dm.Outputs(features=[bench.domain.outputs.get_by_key(k)]),
                                      kernel=dm.MaternKernel(nu=2.5)) for k in ("f_0", "f_1")]
    s = strategies.map(dm.QparegoStrategy(domain=bench.domain, seed=3, acquisition_function=dm.qUCB(),
                                          surrogate_specs=dm.BotorchSurrogates(surrogates=specs),
                                          num_raw_samples=64, num_restarts=2))
    s.tell(exps[bench.domain.inputs.get_keys() + ["f_0", "f_1", "valid_f_0", "valid_f_1"]])
    with pytest.raises(NotImplementedError):
        s.ask(1)
