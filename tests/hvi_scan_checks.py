"""Shared machinery of the scan-level GPU tests (tests/test_gpu_hvi_wide.py,
tests/test_gpu_hvi_kd.py) — TEST INFRASTRUCTURE ONLY: bare evr_qnehvi_state objects around
device cells, every linear scan path run over the same G, and the comparison with
tests/hvi_reference.Reference under the derived rounding bound (hvi_reference.rounding_factor:
f = 4 (C_max + m) 2^-53 relative plus f times the largest summand, on values and on every
gradient component; tie rows are held on values only)."""
import numpy as np
import torch

from everest_amd import ops
from tests import hvi_reference as hr

F64 = dict(dtype=torch.float64, device="cuda")


def dev_fronts(fronts):
    """S x n x m host fronts -> (O m x n x S, ref) on the device."""
    m = fronts.shape[2]
    return (torch.tensor(np.ascontiguousarray(fronts.transpose(2, 1, 0)), device="cuda"),
            torch.full((m,), hr.REF, **F64))


def bare_state(cells):
    """An evr_qnehvi_state around cells alone: the scan entry points (evr_hvi_forward,
    evr_hvi_forward_backward, evr_hvi_restart_fb) read S, m and the cell / kd fields only, so
    the GP fields are one-element dummies."""
    one = torch.ones(1, **F64)
    st = ops.make_state(0, 0, cells.S, cells.m, one, one, one, one, one, one, one, cells)
    st._keep = (one, cells)      # the struct holds raw pointers into these
    return st


def without_kd(cells):
    return ops.Cells(cells.off, cells.counts, cells.m, keys=cells.keys, pts=cells.pts, rank0=cells.rank0,
                     stride=cells.stride)


def explicit(cells):
    lo, hi = cells.explicit()
    return ops.Cells(cells.off, cells.counts, cells.m, lo=lo, hi=hi)


def candidates_G(Y, b):
    """Y S x B x m host candidates -> G S x m x b on the device (the first b candidates)."""
    return torch.tensor(np.ascontiguousarray(Y[:, :b].transpose(0, 2, 1)), device="cuda")


class Worst:
    """Worst measured error per path, as a fraction of the derived bound and relative."""

    def __init__(self):
        self.w = {}

    def add(self, path, what, err, tol, ref):
        frac = float((err / tol).max()) if err.numel() else 0.0
        nz = ref.abs() > 0
        rel = float((err[nz] / ref[nz].abs()).max()) if nz.any() else 0.0
        k = (path, what)
        f0, r0 = self.w.get(k, (0.0, 0.0))
        self.w[k] = (max(f0, frac), max(r0, rel))

    def report(self, head, f):
        parts = [f"{p} {w}: {fr:.2f} of bound, rel {rl:.1e}" for (p, w), (fr, rl) in sorted(self.w.items())]
        print(f"{head} (bound factor {f:.2e}): " + "; ".join(parts))


def check(path, R, cmax, b, ties, worst, acq=None, dG=None, sval=None, gout=None):
    """One path's outputs for the first b candidates against the reference R."""
    f = hr.rounding_factor(cmax, R.m)
    S = R.S
    if acq is not None:
        a, r = acq.cpu(), R.acq[:b]
        tol = f * r.abs() + f * R.vterm[:, :b].amax(0)
        err = (a - r).abs()
        worst.add(path, "acq", err, tol.clamp_min(1e-300), r)
        assert (err <= tol).all(), (path, b, "acq", err.max().item(), (err / tol.clamp_min(1e-300)).max().item())
    if sval is not None:
        a, r = sval.cpu(), R.sval[:, :b]
        tol = f * r.abs() + f * R.vterm[:, :b]
        err = (a - r).abs()
        worst.add(path, "sval", err, tol.clamp_min(1e-300), r)
        assert (err <= tol).all(), (path, b, "sval", err.max().item())
    if dG is not None:
        go = None if gout is None else gout.cpu()
        g, r = dG.cpu(), R.grad(b, go)
        scale = R.gterm[:, :b] / S * (1.0 if go is None else go.reshape(1, b))
        tol = f * r.abs() + f * scale.unsqueeze(1)
        keep = [c for c in range(b) if c not in ties]
        err = (g - r).abs()[:, :, keep]
        worst.add(path, "dG", err, tol[:, :, keep].clamp_min(1e-300), r[:, :, keep])
        assert (err <= tol[:, :, keep]).all(), (path, b, "dG", err.max().item())
        assert torch.isfinite(g).all()


def run_paths(cells, R, Y, ties, bs, worst, kd_expected, gouts=(False, True)):
    """Every scan path this state admits over the same G; returns the set of paths run."""
    cmax = max(R.c_max, cells.max_cells)
    st_c = bare_state(without_kd(cells))
    st_x = bare_state(explicit(cells))
    st_k = bare_state(cells) if cells.kd is not None else None
    assert (st_k is not None) == kd_expected
    ran = set()
    for b in bs:
        G = candidates_G(Y, b)
        for with_gout in gouts:
            gout = torch.linspace(0.5, 2.0, b, **F64) if with_gout else None
            for name, st in (("tiled-keys", st_c), ("tiled-explicit", st_x), ("kd2", st_k)):
                if st is None:
                    continue
                acq, dG = ops.hvi_forward_backward(st, G, b, None, gout)
                check(name, R, cmax, b, ties, worst, acq=acq, dG=dG, gout=gout)
                ran.add(name)
        for name, st in (("fwd-tiled", st_c), ("fwd-kd", st_k)):
            if st is not None:
                check(name, R, cmax, b, ties, worst, acq=ops.hvi_forward(st, G, b))
                ran.add(name)
        if st_k is not None and ops.hvi_restart_fb_applies(st_k, b):
            sval, dG = ops.hvi_restart_fb(st_k, G, b)
            check("restart", R, cmax, b, ties, worst, acq=ops.mean_over_samples(sval), dG=dG, sval=sval)
            ran.add("restart")
        else:
            assert st_k is None or b > 32 or not ops.hvi_restart_fb_applies(st_k, 1)
    torch.cuda.synchronize()
    return ran


def sorted_cells(lo, hi):
    a = np.concatenate([lo, hi], axis=1)
    return a[np.lexsort(a.T[::-1])]


def assert_cells_equal_host(cells, fronts):
    """Offsets and per-sample cell sets of the device decomposition equal the native host
    partition's, bit for bit."""
    m = fronts.shape[2]
    lo_h, hi_h, off_h = ops.box_decompose(fronts, hr.REF * np.ones(m), None, 4, layout="sij")
    off_d = cells.off.cpu().numpy()
    assert np.array_equal(off_d, off_h)
    lo_d, hi_d = (t.cpu().numpy() for t in cells.explicit())
    for s in range(fronts.shape[0]):
        a = slice(off_h[s], off_h[s + 1])
        assert np.array_equal(sorted_cells(lo_h[a], hi_h[a]), sorted_cells(lo_d[a], hi_d[a]))


_REFS = {}


def reference(key, fronts, b):
    """(Y, tie rows, Reference) of a front set, computed once per module run."""
    if key not in _REFS:
        m = fronts.shape[2]
        Y, ties = hr.batch(fronts, hr.REF * np.ones(m), b, seed=sum(map(ord, str(key))))
        _REFS[key] = (Y, ties, hr.Reference(fronts, hr.REF * np.ones(m), Y))
    return _REFS[key]
