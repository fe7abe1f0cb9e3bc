"""GPU: kd-ordered cell groups and the sparse three-level HVI scan (cells_kd.hip,
hvi.hip::hvi_kd) against the tiled dense scan on the same compressed cells, and the kd
index invariants (every cell kept exactly once, group minima, sorted lower bounds)."""
import numpy as np
import pytest
import torch

from tests.helpers import device_gp, make_problem

pytestmark = pytest.mark.gpu


def _pair(n, d, m, S, seed, prune=True):
    from everest_amd.acquisition import QNEHVI

    X, Y, lo, hi, hyp = make_problem(n=n, d=d, m=m, seed=seed)
    gp = device_gp(X, Y, lo, hi, hyp)
    a, b, ref = -np.ones(m), np.zeros(m), -1.1 * np.ones(m)
    kw = dict(S=S, sampler_seed=seed + 1, prune_baseline=prune, prune_seed=seed + 2, prune_samples=256,
              box_device=True)
    kd = QNEHVI(gp, X, X, ref, a, b, kd_scan=True, **kw)
    dense = QNEHVI(gp, X, X, ref, a, b, kd_scan=False, **kw)
    return kd, dense, lo, hi, d


@pytest.mark.parametrize("n,d,m,S,b", [(120, 6, 5, 64, 200), (60, 4, 3, 32, 65), (40, 3, 2, 16, 1),
                                       (200, 6, 5, 128, 64)])
def test_kd_scan_matches_tiled_scan(n, d, m, S, b):
    kd, dense, lo, hi, d = _pair(n, d, m, S, seed=n + m)
    assert kd.box_path == "device+kd" and dense.box_path == "device"
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(b).uniform(size=(b, d)), device="cuda")
    a1, g1 = kd.forward_backward(Xc)
    a2, g2 = dense.forward_backward(Xc)
    assert torch.allclose(a1, a2, rtol=1e-12, atol=1e-15)
    assert torch.allclose(g1, g2, rtol=1e-10, atol=1e-13)
    assert torch.allclose(kd.forward(Xc), a1, rtol=1e-13, atol=1e-16)
    a3, g3 = kd.forward_backward(Xc)
    assert torch.equal(a1, a3) and torch.equal(g1, g3)          # bitwise reproducible


def test_kd_scan_gout_and_sample_grad():
    """dG of the sparse scan (with an upstream gradient) equals the tiled scan's."""
    from everest_amd import ops

    kd, dense, lo, hi, d = _pair(100, 5, 4, 48, seed=5)
    b = 90
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(9).uniform(size=(b, d)), device="cuda")
    Kx = kd.gp.cross(Xc)
    R = ops.gemm(kd.M, Kx)
    G, L22, flags = ops.qnehvi_samples(kd.state, R, b)
    gout = torch.linspace(0.5, 2.0, b, dtype=torch.float64, device="cuda")
    a1, d1 = ops.hvi_forward_backward(kd.state, G, b, flags, gout)
    a2, d2 = ops.hvi_forward_backward(dense.state, G, b, flags, gout)
    assert torch.allclose(a1, a2, rtol=1e-12, atol=1e-15)
    assert torch.allclose(d1, d2, rtol=1e-10, atol=1e-14)


def test_kd2_bench_size_matches_tiled_scan():
    """BASELINE configs[2] size (DTLZ2 n=512, d=6, m=5, S=256, b=512): the sparse scan equals
    the tiled dense scan over the same compressed cells, and repeats bitwise."""
    import bench
    from everest_amd import ops

    dev = torch.device("cuda", 0)
    X, Y, gp, hypers, acqf, _, _ = bench.build_state(512, 6, 5, 256, dev)
    assert acqf.box_path == "device+kd"
    dense = ops.make_state(acqf.n, acqf.nb, acqf.S, acqf.m, gp.const, gp.ym, gp.ys, gp.kxx, acqf.zq, acqf.obj_a,
                           acqf.obj_b, ops.Cells(acqf.cells.off, acqf.cells.counts, acqf.m, keys=acqf.cells.keys,
                                                 pts=acqf.cells.pts, rank0=acqf.cells.rank0,
                                                 stride=acqf.cells.stride))
    b = 512
    Xc = bench.candidates(b, 6, seed=2, device=dev)
    R, P = ops.qnehvi_project(acqf.state, acqf.M, gp.cross(Xc), b)
    G, L22, flags = ops.qnehvi_samples_norms(acqf.state, R, P, b)
    a1, g1 = ops.hvi_forward_backward(acqf.state, G, b, flags)
    a2, g2 = ops.hvi_forward_backward(dense, G, b, flags)
    assert torch.allclose(a1, a2, rtol=1e-12, atol=1e-15)
    assert torch.allclose(g1, g2, rtol=1e-10, atol=1e-13)
    a3, g3 = ops.hvi_forward_backward(acqf.state, G, b, flags)
    assert torch.equal(a1, a3) and torch.equal(g1, g3)
    assert (a1 > 0).sum() > b // 2


def _assert_kd_index_invariants(cells):
    """Every cell kept exactly once in the kd order, padding, group minima, ascending lower
    bounds, and lower bounds recovered through the rank index."""
    g = cells.kd
    m = cells.m
    off = cells.off.cpu().numpy()
    goff = g.goff.cpu().numpy()
    keys = cells.keys.cpu().numpy().view(np.uint64)
    gkeys = g.keys.cpu().numpy().view(np.uint64)
    # the kd keys carry the point index in field 0 where the cell keys carry its rank
    fb = 16 if m <= 4 else (12 if m == 5 else 64 // m)
    sh, fm = np.uint64(fb * (m - 1)), np.uint64((1 << fb) - 1)
    rank0 = cells.rank0.cpu().numpy().reshape(cells.S, -1)
    rank = g.rank.cpu().numpy().view(np.uint16).reshape(-1, m, 16)
    box = g.box.cpu().numpy().view(np.uint16).reshape(-1, 8)
    sv = g.sorted_lo.cpu().numpy()
    for s in range(cells.S):
        C = off[s + 1] - off[s]
        assert goff[s + 1] - goff[s] == (C + 15) // 16
        kk = keys[off[s]:off[s + 1]]
        idx = rank0[s][((kk >> sh) & fm).astype(np.int64)].astype(np.uint64)
        mine = np.sort((kk & ~(fm << sh)) | (idx << sh))
        got = gkeys[goff[s] * 16: goff[s] * 16 + C]
        assert np.array_equal(np.sort(got), mine)                   # a permutation of the cells
        r = rank[goff[s]:goff[s + 1]]                               # groups x m x 16
        flat = r.transpose(0, 2, 1).reshape(-1, m)
        assert (flat[C:] == 0x7FFF).all() and (flat[:C] < 0x7FFF).all()
        assert np.array_equal(box[goff[s]:goff[s + 1], :m], r.min(axis=2))
        assert (box[goff[s]:goff[s + 1], m:] == 0).all()             # slots beyond m always pass
        assert (sv[s][:, 1:] >= sv[s][:, :-1]).all()                 # ascending per objective
    # lower bounds recovered through the rank index equal the decoded cells
    lo_x, _ = cells.explicit()
    lo_x = lo_x.cpu().numpy()
    s = 0
    C = off[1]
    flat = rank[goff[0]:goff[1]].transpose(0, 2, 1).reshape(-1, m)[:C]
    lo_rank = np.stack([sv[0, j, flat[:, j]] for j in range(m)], 1)
    assert np.array_equal(np.sort(lo_rank, axis=0), np.sort(lo_x[:C], axis=0))


def test_kd_index_invariants():
    kd, dense, lo, hi, d = _pair(150, 6, 5, 32, seed=2)
    _assert_kd_index_invariants(kd.cells)


def _kd_order_raw(cells, max_cells):
    """evr_cells_kd_order_device on cells with the given max_cells: it sizes the LDS sort
    buffer and picks the sort-key layout (u32 when max_cells < 8192 and stride < 1023, else
    u64); the kernel sorts by each sample's own count."""
    from everest_amd import ops

    S, m, stride = cells.S, cells.m, cells.stride
    dev = cells.off.device
    ng = (cells.counts + 15) // 16
    goff_h = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(ng, out=goff_h[1:])
    G = int(goff_h[-1])
    goff = torch.as_tensor(goff_h.astype(np.int32)).to(dev)
    keys = torch.zeros(G * 16, dtype=torch.int64, device=dev)
    rank = torch.zeros(G * m * 16, dtype=torch.int16, device=dev)
    box = torch.zeros(G * 8, dtype=torch.int16, device=dev)
    sorted_lo = torch.zeros(S, m, stride, dtype=torch.float64, device=dev)
    ops.call("evr_cells_kd_order_device", ops._stream(), S, m, stride, cells.off.data_ptr(), goff.data_ptr(),
             int(max_cells), cells.keys.data_ptr(), cells.pts.data_ptr(), cells.rank0.data_ptr(), keys.data_ptr(),
             rank.data_ptr(), box.data_ptr(), sorted_lo.data_ptr())
    return keys, rank, box, sorted_lo


@pytest.mark.parametrize("which", ["m5", "m8"])
def test_kd_u64_sort_keys_equal_u32_bitwise(which):
    """cells_kd_kernel<M, unsigned long long> against cells_kd_kernel<M, unsigned int> on the
    same cells (M = 5: the state of test_kd_index_invariants; M = 8: sphere n = 12, S = 8):
    max_cells = 8192 selects the u64 layout and sizes the LDS for 8192 keys (within the
    kernel's 96 KB since stride m 10 + 16 <= 32 KB), the true max_cells the u32 layout.  Both
    orders are the same, so keys, ranks, group minima and sorted lower bounds are equal bit
    for bit."""
    from everest_amd import ops
    from tests import hvi_reference as hr

    if which == "m5":
        cells = _pair(150, 6, 5, 32, seed=2)[0].cells
    else:
        fr = hr.sphere(8, 12, 8, seed=812)
        O = torch.tensor(np.ascontiguousarray(fr.transpose(2, 1, 0)), device="cuda")
        cells, built = ops.box_decompose_kd_device(O, torch.full((8,), hr.REF, dtype=torch.float64, device="cuda"))
        assert built
    assert cells.max_cells < 8192 and cells.stride < 1023                 # u32 by itself
    assert cells.stride * cells.m * 10 + 16 <= 32 * 1024 and ops.kd_supported(cells)
    assert which == "m5" or cells.max_cells > 1024                        # whole-buffer and wave sorts both run
    k32 = _kd_order_raw(cells, cells.max_cells)
    k64 = _kd_order_raw(cells, 8192)
    for a, b in zip(k32, k64):
        assert torch.equal(a, b)
    g = cells.kd                                                          # what the pipeline built
    for a, b in zip(k64, (g.keys, g.rank, g.box, g.sorted_lo)):
        assert torch.equal(a.reshape(-1), b.reshape(-1)[:a.numel()])


@pytest.mark.parametrize("m,n,S", [(3, 1100, 2), (2, 1100, 4)])
def test_kd_u64_sort_keys_natural(m, n, S):
    """stride = n + m >= 1023, so evr_box_kd_pipeline sorts with cells_kd_kernel<M, unsigned
    long long> by itself (M = 3: ~870 cells per sample; M = 2: ~95): box_path device+kd, the
    index invariants, and hvi_kd2<M> / hvi_kdw<M> / hvi_tiled<M> against the CPU reference at
    b = 20 within the derived rounding bound (tests/test_gpu_hvi_wide.py)."""
    from everest_amd import acquisition, ops
    from tests import hvi_reference as hr
    from tests import hvi_scan_checks as sc

    fronts = hr.sphere(S, n, m, seed=n + m)
    assert n + m >= 1023
    O, ref = sc.dev_fronts(fronts)
    cells, path = acquisition._decompose(O, ref)
    assert path == "device+kd" and cells.kd is not None and cells.stride == n + m
    _assert_kd_index_invariants(cells)
    Y, ties, R = sc.reference(("u64", m, n, S), fronts, 20)
    assert np.array_equal(cells.counts, np.asarray(R.counts))
    worst = sc.Worst()
    ran = sc.run_paths(cells, R, Y, ties, (20,), worst, True)
    assert {"kd2", "restart", "tiled-keys", "fwd-kd"} <= ran
    worst.report(f"hvi u64 kd keys m={m} n={n} S={S} cells<={cells.max_cells}",
                 hr.rounding_factor(max(R.c_max, cells.max_cells), m))


@pytest.mark.parametrize("n,d,m,S,b", [(120, 6, 5, 256, 20), (60, 4, 3, 256, 7), (40, 3, 2, 512, 1),
                                       (200, 6, 5, 512, 32), (90, 5, 4, 256, 16), (80, 4, 1, 1024, 3)])
def test_restart_fused_scan_equals_three_launch_chain(n, d, m, S, b):
    """The one-launch restart scan (hvi_kdw: one wave per candidate) against hvi_thresholds +
    hvi_kd2 + hvi_reduce_fb on the same samples, in its own summation order to 1e-12; acq =
    mean of the per-sample values to 1e-12; bitwise reproducible."""
    from everest_amd import ops

    kd, dense, lo, hi, d = _pair(n, d, m, S, seed=n + 5 * m)
    assert ops.hvi_restart_fb_applies(kd.state, b)
    assert not ops.hvi_restart_fb_applies(kd.state, 33) and not ops.hvi_restart_fb_applies(dense.state, b)
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(b + 2).uniform(size=(b, d)), device="cuda")
    R, P = ops.qnehvi_project(kd.state, kd.M, kd.gp.cross(Xc), b)
    G, L22, flags = ops.qnehvi_samples_norms(kd.state, R, P, b)
    a1, d1 = ops.hvi_forward_backward(kd.state, G, b, flags)
    sval, d2 = ops.hvi_restart_fb(kd.state, G, b)
    torch.cuda.synchronize()
    a2 = ops.mean_over_samples(sval)
    assert torch.allclose(d2, d1, rtol=1e-12, atol=1e-15 * d1.abs().max().item())
    assert torch.allclose(a2, a1, rtol=1e-12, atol=1e-300)
    assert torch.isfinite(a1).all() and (b < 7 or (a1 > 0).any())
    sval2, d3 = ops.hvi_restart_fb(kd.state, G, b)
    assert torch.equal(sval, sval2) and torch.equal(d2, d3)      # bitwise reproducible


def test_restart_wave_scan_long_term_lists():
    """hvi_kdw on candidates dominating most of the front (hundreds of terms per sample and
    candidate: many 64-term rounds and list remainders) against the three-launch chain, and
    batch-invariant bitwise (a candidate's result depends on its own cells only: the first 9
    candidates alone equal their values in the batch of 32)."""
    from everest_amd import ops

    kd, dense, lo, hi, d = _pair(240, 6, 5, 256, seed=11, prune=False)
    b = 32
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(3).uniform(size=(b, d)), device="cuda")
    R, P = ops.qnehvi_project(kd.state, kd.M, kd.gp.cross(Xc), b)
    G, L22, flags = ops.qnehvi_samples_norms(kd.state, R, P, b)
    G = G + 3.0
    a1, d1 = ops.hvi_forward_backward(kd.state, G, b, flags)
    sval, d2 = ops.hvi_restart_fb(kd.state, G, b)
    assert torch.allclose(d2, d1, rtol=1e-12, atol=1e-15 * d1.abs().max().item())
    assert torch.allclose(ops.mean_over_samples(sval), a1, rtol=1e-12)
    G9 = G.reshape(kd.S, -1, b)[:, :, :9].contiguous()
    sval9, d9 = ops.hvi_restart_fb(kd.state, G9, 9)
    assert torch.equal(sval9, sval.reshape(kd.S, b)[:, :9])
    assert torch.equal(d9, d2.reshape(kd.S, -1, b)[:, :, :9])


@pytest.mark.parametrize("b", [20, 32, 7])
def test_restart_wave_scan_is_batch_invariant(b):
    """hvi_kdw: a candidate's per-sample value and gradient depend on its own terms only, so
    they are bitwise the same in any batch — the property that makes a restart batch sharded
    over ranks evaluate exactly as on one rank."""
    from everest_amd import ops

    kd, dense, lo, hi, d = _pair(120, 6, 5, 256, seed=31)
    Xc = torch.tensor(lo + (hi - lo) * np.random.default_rng(b).uniform(size=(b, d)), device="cuda")
    R, P = ops.qnehvi_project(kd.state, kd.M, kd.gp.cross(Xc), b)
    G, _, _ = ops.qnehvi_samples_norms(kd.state, R, P, b)
    sval, dG = ops.hvi_restart_fb(kd.state, G, b)
    h = b // 2
    for lo_i, hi_i in ((0, h), (h, b)):
        Gs = G[:, :, lo_i:hi_i].contiguous()
        sv, dg = ops.hvi_restart_fb(kd.state, Gs, hi_i - lo_i)
        assert torch.equal(sv, sval[:, lo_i:hi_i]) and torch.equal(dg, dG[:, :, lo_i:hi_i])
