"""GPU: the hypervolume chain (box_device.hip -> cells_kd.hip -> hvi.hip) at scan level
against a CPU reference built another way (tests/hvi_reference.py: the oracle's Pareto filter,
local-upper-bound cells and autograd), at m = 6, 7, 8, at saturated key fields and around the
size limits where the decomposition and the scans disagree.

Tolerance (derived, see hvi_reference.rounding_factor): every summand is a product of m
nonnegative clipped lengths, so no sum cancels and two correctly rounded evaluations differ by
at most ~2 (C_max + m) 2^-53 relative; the tests allow f = 4 (C_max + m) 2^-53 relative plus
f times the largest summand absolute, on values and on every gradient component alike.  The
two tie rows of hvi_reference.candidates (on a front point / on a cell bound) are held on
values only; no other row is excused anywhere."""
import warnings

import numpy as np
import pytest
import torch

from everest_amd import ops
from tests import hvi_reference as hr
from tests import hvi_scan_checks as sc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------
# m = 6, 7, 8 (and the known-good m = 5 as control)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,S,kd", [(6, 16, 8, True), (7, 16, 8, True), (8, 12, 8, True), (8, 24, 4, True),
                                      (8, 32, 2, False), (5, 30, 8, True)])
def test_scans_match_reference_wide(m, n, S, kd):
    """bd kernels, cells_kd_kernel<M, u32> and hvi_tiled<M> (keyed and explicit), hvi_kd2<M> +
    hvi_reduce_fb<8 / 16> (b = 1, 7, 32, 65), hvi_kdw<M> (b <= 32; launch bounds change at
    M = 8) and the forward-only scans at M = 5 (control), 6, 7, 8 on sphere fronts, gout absent
    and non-uniform.  (8, 24, 4) runs the kd path near its 8192-cell limit; (8, 32, 2) exceeds
    it, so the pipeline must not build kd groups and only the dense tiled scans run."""
    fronts = hr.sphere(S, n, m, seed=100 * m + n)
    Y, ties, R = sc.reference(("sphere", m, n, S), fronts, 65)
    O, ref = sc.dev_fronts(fronts)
    cells, built = ops.box_decompose_kd_device(O, ref, want_kd=True)
    assert built == kd and ops.kd_supported(cells) == kd
    assert np.array_equal(cells.counts, np.asarray(R.counts))          # same partition algorithm
    if (n, S) == (24, 4):
        assert 4096 < cells.max_cells <= 8192        # two-level bitonic sort buffer, near the kd limit
    assert (cells.max_cells <= 8192) == kd
    sc.assert_cells_equal_host(cells, fronts)
    worst = sc.Worst()
    ran = sc.run_paths(cells, R, Y, ties, (1, 7, 32, 65), worst, kd)
    want = {"tiled-keys", "tiled-explicit", "fwd-tiled"} | ({"kd2", "fwd-kd", "restart"} if kd else set())
    assert ran == want
    assert (R.acq > 0).sum() > 32 and (R.acq[[1, 2, 4]] == 0).all()
    worst.report(f"hvi wide m={m} n={n} S={S} cells<={cells.max_cells}", hr.rounding_factor(max(R.c_max, cells.max_cells), m))


# ---------------------------------------------------------------------------------------
# key-field saturation
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,j0,j1,fb", [(8, 246, 0, 1, 8), (8, 246, 6, 7, 8), (7, 503, 0, 6, 9), (6, 1012, 2, 5, 10),
                                          (6, 1016, 2, 5, 10)])
def test_key_fields_saturated(m, n, j0, j1, fb):
    """CellKey<M> at the largest point count its fields hold (n = 2^FB - 2 - m, FB = 8, 9, 10
    bits at M = 8, 7, 6): staircase fronts in the first / last objectives (field 0 carries a
    rank, the others point indices) make every index up to the field's top appear in cells
    while the cell count stays small.  cells_kd_kernel<M, u32> (stride < 1023 throughout),
    hvi_tiled<M>, hvi_kd2<M>, hvi_kdw<M> at b = 7 and 32.  The limit at M = 6 is n = 1016
    (2^10 - 2 - 6); n = 1012, four rows short of it, is kept as the case this test was asked
    for, and only there one point more still fits."""
    from everest_amd import acquisition

    S = 2
    top = (1 << fb) - 2 - m
    assert n == top or (m, n) == (6, 1012)
    assert ops.box_device_supported(n, m) and not ops.box_device_supported(top + 1, m)
    assert ops.box_device_supported(n + 1, m) == (n < top)
    fronts = hr.staircase(S, n, m, j0, j1, seed=n + j0)
    Y, ties, R = sc.reference(("stair", m, n, j0, j1), fronts, 32)
    O, ref = sc.dev_fronts(fronts)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        cells, path = acquisition._decompose(O, ref)
    assert path == "device+kd" and not rec
    sc.assert_cells_equal_host(cells, fronts)
    # all n points are nondominated, so every point index defines some cell bound: the keys
    # use n distinct indices, up to the top of the field's range
    keys = cells.keys.cpu().numpy().view(np.uint64)
    off = cells.off.cpu().numpy()
    rank0 = cells.rank0.cpu().numpy().reshape(S, -1)
    fm = np.uint64((1 << fb) - 1)
    for s in range(S):
        kk = keys[off[s]:off[s + 1]]
        used = set(rank0[s][((kk >> np.uint64(fb * (m - 1))) & fm).astype(np.int64)].tolist())
        for j in range(1, m):
            used |= set(((kk >> np.uint64(fb * (m - 1 - j))) & fm).astype(np.int64).tolist())
        assert len(used) >= n and n - 1 <= max(used) <= (1 << fb) - 2
    worst = sc.Worst()
    ran = sc.run_paths(cells, R, Y, ties, (7, 32), worst, True)
    assert {"tiled-keys", "tiled-explicit", "kd2", "restart"} <= ran
    assert (R.acq > 0).sum() > 16
    worst.report(f"hvi saturated m={m} n={n} ({j0},{j1}) cells<={cells.max_cells}",
                 hr.rounding_factor(max(R.c_max, cells.max_cells), m))
    # one point more does not fit the key: the host partition takes over, with its warning
    O1, ref1 = sc.dev_fronts(hr.staircase(S, top + 1, m, j0, j1, seed=n + j0))
    with pytest.warns(RuntimeWarning, match="exceed the device box decomposition's limits"):
        cells1, path1 = acquisition._decompose(O1, ref1)
    assert path1 == "host" and cells1.keys is None and cells1.lo is not None


# ---------------------------------------------------------------------------------------
# limit windows: the decomposition accepts more points than the scans' point table holds
# ---------------------------------------------------------------------------------------
def _scan_max_n(m):
    """Largest n whose point table (stride n + m rows of m doubles + one int) fits the scans'
    64 KB (hvi.hip, hvi_check_state)."""
    return 65536 // (8 * m + 4) - m


def _box_max_n(m):
    """Largest n the device box decomposition accepts (evr_box_device_limits: LDS and key width)."""
    lo, hi = 1, 1 << 17
    assert ops.box_device_supported(lo, m) and not ops.box_device_supported(hi, m)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.box_device_supported(mid, m) else (lo, mid)
    return lo


@pytest.mark.parametrize("where", ["scan_max", "scan_max+1", "inner", "box_max", "box_max+1"])
@pytest.mark.parametrize("m,n_inner", [(2, 3300), (3, 2400), (5, 1500)])
def test_limit_windows_never_raise(m, n_inner, where):
    """Between the scans' point-table bound and the decomposition's own limit (n = 1485..1677
    at m = 5) _decompose must hand the scans cells they accept: the device path up to the
    scans' bound (hvi_kd2<M> / hvi_tiled<M, keyed> at the largest stride they take), the host
    partition with its RuntimeWarning beyond (hvi_tiled<M, explicit>).  Whatever box_path
    says, the evaluation returns the reference's values and never raises."""
    from everest_amd import acquisition

    S, b = 2, 4
    n_scan, n_box = _scan_max_n(m), _box_max_n(m)
    assert n_scan < n_inner <= n_box, (n_scan, n_box)
    n = {"scan_max": n_scan, "scan_max+1": n_scan + 1, "inner": n_inner, "box_max": n_box,
         "box_max+1": n_box + 1}[where]
    assert ops.hvi_scan_supported(n_scan + m, m) and not ops.hvi_scan_supported(n_scan + 1 + m, m)
    base = hr.sphere(S, 12, m, seed=40 + m)
    fronts = hr.with_dominated(base, n, seed=n)
    Y, ties, R = sc.reference(("window", m), base, b)        # padding is dominated: the same reference
    assert not ties
    O, ref = sc.dev_fronts(fronts)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        cells, path = acquisition._decompose(O, ref)
    if n <= n_scan:
        assert path == "device+kd" and not rec
    else:
        assert path == "host" and any(issubclass(w.category, RuntimeWarning) for w in rec)
    assert np.array_equal(cells.counts, np.asarray(R.counts))
    st = sc.bare_state(cells)
    G = sc.candidates_G(Y, b)
    worst = sc.Worst()
    acq, dG = ops.hvi_forward_backward(st, G, b)
    sc.check(path, R, cells.max_cells, b, ties, worst, acq=acq, dG=dG)
    sc.check(path + " fwd", R, cells.max_cells, b, ties, worst, acq=ops.hvi_forward(st, G, b))
    if ops.hvi_restart_fb_applies(st, b):
        sval, dG2 = ops.hvi_restart_fb(st, G, b)
        sc.check("restart", R, cells.max_cells, b, ties, worst, acq=ops.mean_over_samples(sval), dG=dG2, sval=sval)
    torch.cuda.synchronize()
    assert R.acq[0] > 0 and R.acq[3] > 0
    worst.report(f"hvi window m={m} n={n} {path}", hr.rounding_factor(cells.max_cells, m))


def test_explicit_device_box_in_the_window_surfaces_the_scan_limit():
    """box_device=True is taken at its word inside the window (m = 5, n = 1500): the device
    decomposition runs, and the first linear evaluation is refused by the host-side
    point-table check of evr_hvi_forward_backward (hvi_check_state) with its LDS message,
    before any launch — the limit surfaces as it does for the decomposition's own limits."""
    from everest_amd import acquisition

    m, n, S, b = 5, 1500, 2, 4
    assert ops.box_device_supported(n, m) and not ops.hvi_scan_supported(n + m, m)
    fronts = hr.with_dominated(hr.sphere(S, 12, m, seed=40 + m), n, seed=n)
    O, ref = sc.dev_fronts(fronts)
    cells, path = acquisition._decompose(O, ref, box_device=True)
    assert path.startswith("device") and cells.keys is not None and cells.stride == n + m
    G = torch.zeros(S, m, b, **sc.F64)
    with pytest.raises(RuntimeError, match="exceeds the LDS budget"):
        ops.hvi_forward_backward(sc.bare_state(cells), G, b)
