"""The CPU restatement of qNEI / qLogNEI / qLogEI (tests/nei_reference.py) against the
oracle's qEI and against its own limits — no GPU."""
import math

import numpy as np
import torch

from oracle import qnehvi as oq
from tests import nei_reference as nr
from tests.helpers import make_problem, oracle_states


def _state(n=12, d=3, seed=5):
    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=1, seed=seed)
    return X, oracle_states(X, Y, lo, hi, hyp)


def test_plain_q1_constant_incumbent_is_qei():
    X, models = _state()
    S = 32
    z = oq.base_samples(S, 1, 1, 7)                                  # S x 1 x 1
    Xc = torch.tensor(np.random.default_rng(0).uniform(size=(9, 1, 3)))
    best_f = -0.9
    nei = nr.NEI(models, Xc.new_zeros(0, 3), -1.0, 0.0, z.new_zeros(S, 0, 1), z, log=False,
                 best=torch.tensor([best_f], dtype=torch.float64))
    ref = oq.qei(models, Xc, best_f, z[..., 0], a=-1.0, bconst=0.0)
    got = nei.forward(Xc)
    assert (ref > 0).any()
    assert torch.allclose(got, ref, rtol=1e-13, atol=1e-15)
    assert torch.allclose(nr.log_ei(models, Xc, best_f, z[..., 0], -1.0, 0.0, log=False), ref, rtol=1e-13, atol=1e-15)


def test_exp_qlognei_approaches_qnei():
    """Per sample, fatplus(x; t) lies in [x_+, x_+ + t (log 2 + 0.1)] and fatmax over q values
    in [max, max + t log q], so exp(qLogNEI) lies in [qNEI, q^tau_max (qNEI + 0.8 tau_relu)]:
    relative difference <= tau_max log q + 0.8 tau_relu / qNEI (+ second order)."""
    X, models = _state()
    S, q, nb = 64, 2, X.shape[0]
    Xb = models[0].X
    zb = oq.base_samples(S, nb, 1, 3)
    zn = oq.base_samples(S, nb + q, 1, 3)[:, nb:]
    Xc = torch.tensor(np.random.default_rng(1).uniform(size=(24, q, 3)))
    plain = nr.NEI(models, Xb, -1.0, 0.0, zb, zn, log=False).forward(Xc)
    sel = plain >= 1e-3
    assert int(sel.sum()) >= 4, plain
    prev = None
    for tau in (1e-4, 1e-6, 1e-8):
        lg = nr.NEI(models, Xb, -1.0, 0.0, zb, zn, log=True, tau_relu=tau, tau_max=tau).forward(Xc)
        rel = ((lg.exp() - plain).abs() / plain)[sel]
        bound = 1.01 * (tau * math.log(q) + 0.8 * tau / plain[sel]) + 1e-13
        assert (rel <= bound).all(), (tau, rel, bound)
        assert prev is None or float(rel.max()) < prev
        prev = float(rel.max())


def test_fatmax_of_one_element_is_the_element():
    x = torch.tensor([-57.5, -3.0, 0.0, 6.9], dtype=torch.float64)
    assert torch.equal(oq.fatmax(x.unsqueeze(-1), dim=-1, tau=nr.TAU_MAX), x)
    g = torch.tensor([[[0.3]], [[-0.2]]], dtype=torch.float64)       # S = 2, b = 1, q = 1
    best = torch.tensor([0.1, 0.1], dtype=torch.float64)
    want = oq.logmeanexp(oq.fatplus(g[:, :, 0] - 0.1, nr.TAU_RELU).log(), dim=0)
    assert torch.equal(nr.scan(g, best, True), want)


def test_prune_keeps_exactly_the_argmax_rows():
    obj = torch.tensor([[1.0, 2.0, 0.0],
                        [3.0, 1.0, 0.0],
                        [0.0, 5.0, 1.0],
                        [2.0, 1.0, 0.0]], dtype=torch.float64)       # 4 draws x 3 points
    assert nr.prune_inferior_points(obj).tolist() == [0, 1]
    assert nr.prune_inferior_points(obj[:1]).tolist() == [1]
    assert nr.prune_inferior_points(-obj).tolist() == [0, 2]
