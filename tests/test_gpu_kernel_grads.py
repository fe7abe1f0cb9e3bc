"""GPU: the GP gradient, MLL-term and posterior-finalize kernels alone, through everest_amd.ops,
against the plain long-double reference (tests/gp_kernel_reference.py, itself checked on the CPU
by tests/test_gp_kernel_reference.py) at every dispatch edge:

* evr_kernel_cross_grad: kcross_grad_kernel<8|16|32|64> (4 / 8 / 2 / 2 outputs per round, so B
  with a full and a remainder chunk), the row split (300 x 65: 38 splits of 8 rows, so the
  reducer's clamped second round, and a 4-row last split; 300 x 4096: 32 splits of 10 rows, the
  last 2 of them empty; 100 x 4096: 13 splits of 8), the optional shift / scale / outputscale
  pointers, mixed per-output families, zero distances.
* evr_kernel_lengthscale_grad: kls_grad_kernel<8> (four columns per lane and round), <16> (one),
  kls_grad_block_kernel<32|64> (n = 513: the third j round of 256 threads), colsum_kernel.
* evr_gp_mll_terms, evr_gp_posterior_finalize.

Bar of the two gradients: |got - ref| <= 1e-12 * S elementwise, S the reference's sum of the
absolute values of the same terms (the project's bar for exact-arithmetic restatements,
tests/test_gpu_linalg.py).  Worst-case rounding of B * n1 <= 2700 fused terms is about 3e-13 S.
"""
import math

import numpy as np
import pytest
import torch

from tests import gp_kernel_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIXED = [0, 3, 1, 2, 3]
MAXRATIO = {}


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _kinds(kind, B):
    # B <= 5: the list of the fit tests, [0, 3, 1, 2, 3][:B]; cycled above that
    return (MIXED * 3)[:B] if kind == "mixed" else [kind] * B


def _code(kind, B):
    from everest_amd.gp import kind_code

    return kind_code(_kinds(kind, B))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXRATIO):
        print(f"max |err| / S  {k}: {MAXRATIO[k]:.3e}")


def _note(label, err, S):
    ok = S > 0
    r = float((err[ok] / S[ok]).max()) if ok.any() else 0.0
    MAXRATIO[label] = max(MAXRATIO.get(label, 0.0), r)
    print(f"{label}: max |err| / S = {r:.3e}")
    return r


# ---------------------------------------------------------------------------------------
# evr_kernel_cross_grad
# ---------------------------------------------------------------------------------------
CROSS_ROWS = [  # instantiation, dims, B (full + remainder chunk), (n1, n2), the shape with all five kinds
    # B = 7: a remainder chunk of three outputs (B = 5 leaves one), so that an output of a partial
    # chunk other than its first is there to be lost or mixed up
    (8, (1, 8), (1, 7, 5), [(1, 1), (9, 65), (300, 65), (37, 130)], (300, 65)),
    (16, (9, 16), (3, 9), [(17, 64), (300, 65)], (300, 65)),
    (32, (17, 32), (1, 3), [(9, 65), (300, 65)], (300, 65)),
    (64, (33, 64), (3,), [(7, 1), (300, 65)], (300, 65)),
]
NORMS = ("none", "side2", "both")


def _cross_cases():
    out = []
    for inst, dims, Bs, shapes, full in CROSS_ROWS:
        i = 0
        for d in dims:
            for B in Bs:
                for shp in shapes:
                    kinds = [0, 1] + ([2, 3, "mixed"] if shp == full and B == Bs[-1] else [])
                    for kind in kinds:
                        # each of the three normalisations and outputscale present / absent comes
                        # round within any six consecutive cases of an instantiation
                        out.append(pytest.param(inst, d, B, shp[0], shp[1], kind, NORMS[i % 3], (i // 3) % 2 == 0,
                                                id=f"k{inst}-d{d}-B{B}-{shp[0]}x{shp[1]}-kind{kind}-{NORMS[i % 3]}"
                                                   f"-os{int((i // 3) % 2 == 0)}"))
                        i += 1
    # the column-tile count caps the row splits here: 13 splits at n1 = 100, 32 at n1 = 300 with the
    # last 2 of them empty (test_cross_row_splits)
    out.append(pytest.param(8, 2, 1, 100, 4096, 0, "side2", False, id="k8-d2-B1-100x4096-kind0-side2-os0"))
    out.append(pytest.param(8, 2, 1, 300, 4096, 0, "side2", False, id="k8-d2-B1-300x4096-kind0-side2-os0"))
    return out


def _row_split(n1, n2):
    """kcross_nsplit's formula: the number of row splits, the rows of each, the number of trailing
    splits with no row (i0 >= n1: they still write zeros to their slice of the partials, which the
    reducer sums) and the rows of the last split that has any."""
    cdiv = lambda a, b: -(-a // b)
    ns = max(1, min(cdiv(2048, cdiv(n2, 64)), cdiv(n1, 8)))
    rows_per = cdiv(n1, ns)
    empty = sum(1 for s in range(ns) if s * rows_per >= n1)
    last = n1 - (ns - empty - 1) * rows_per
    return ns, rows_per, empty, last


def test_cross_row_splits():
    """The shapes reach the row-split edges they are there for; a retuned kcross_nsplit then
    fails here instead of silently moving a case off its edge."""
    assert _row_split(300, 65) == (38, 8, 0, 4)         # > 32 splits: the reducer's second round; ragged last split
    assert _row_split(300, 4096) == (32, 10, 2, 10)     # splits 30 and 31 start at rows 300 and 310
    assert _row_split(100, 4096) == (13, 8, 0, 4)
    assert _row_split(1, 1) == (1, 1, 0, 1) and _row_split(7, 1) == (1, 7, 0, 7)
    shapes = {(p.values[3], p.values[4]) for p in _cross_cases()}
    assert {(300, 65), (300, 4096), (100, 4096)} <= shapes
    assert any(_row_split(*shp)[2] >= 2 for shp in shapes)


def test_cross_case_list_covers_every_option():
    """Every instantiation sees the three normalisations, outputscale present and absent, all
    five kind settings, and its full and remainder output chunks."""
    seen = {}
    for p in _cross_cases():
        inst, d, B, n1, n2, kind, norm, use_os = p.values
        s = seen.setdefault(inst, dict(norm=set(), os=set(), kind=set(), B=set()))
        s["norm"].add(norm), s["os"].add(use_os), s["kind"].add(kind), s["B"].add(B)
    for inst, dims, Bs, _, _ in CROSS_ROWS:
        s = seen[inst]
        assert s["norm"] == set(NORMS) and s["os"] == {True, False}
        assert s["kind"] == {0, 1, 2, 3, "mixed"} and s["B"] >= set(Bs)


@pytest.mark.parametrize("inst,d,B,n1,n2,kind,norm,use_os", _cross_cases())
def test_kernel_cross_grad(inst, d, B, n1, n2, kind, norm, use_os):
    from everest_amd import ops

    assert inst == (8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64)
    rng = np.random.default_rng(100000 * d + 1000 * B + 7 * n1 + n2 + 13 * len(str(kind)))
    X1 = rng.uniform(-1, 2, (n1, d))
    X2 = rng.uniform(-1, 2, (n2, d))
    if n1 == 300:
        X2[[3, 17, 31, 50, 64]] = X1[[0, 7, 150, 296, 299]]      # zero distances, the last split's rows too
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    G = rng.normal(size=(B, n1, n2))
    os_ = rng.uniform(0.5, 2.0, B) if use_os else None
    shift, scale = -np.ones(d), np.full(d, 1.0 / 3.0)
    s1 = (shift, scale) if norm == "both" else (None, None)
    s2 = (shift, scale) if norm != "none" else (None, None)
    if norm == "side2":            # the product's call: X1 the normalised training inputs, X2 raw
        X1 = (X1 - shift) * scale
    kinds = _kinds(kind, B)
    want, S = ref.cross_grad(X1, X2, ls, G, kinds, *s1, *s2, os_)
    args = (_t(X1), _t(X2), _t(ls), _t(G), _code(kind, B), _t(s1[0]), _t(s1[1]), _t(s2[0]), _t(s2[1]), _t(os_))
    # a freed block of NaN of the size of the partials, for the caching allocator to hand to the op
    # as its workspace: a slice that a block (an empty split's, say) left unwritten then shows
    dirty = torch.full((_row_split(n1, n2)[0] * n2 * d,), float("nan"), dtype=torch.float64, device=DEV)
    del dirty
    got = ops.kernel_cross_grad(*args)
    again = ops.kernel_cross_grad(*args)
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g))
    err = np.abs(g.astype(ref.LD) - want)
    _note(f"kcross_grad_kernel<{inst}>", err, S)
    assert np.all(err <= ref.LD(1e-12) * S), float((err / np.maximum(S, ref.LD(1e-300))).max())


# ---------------------------------------------------------------------------------------
# evr_kernel_lengthscale_grad
# ---------------------------------------------------------------------------------------
LS_ROWS = [  # label, dims, n, the n with all five kind settings
    ("kls_grad_kernel<8>", (1, 8), (1, 3, 5, 64, 257, 300), 300),
    ("kls_grad_kernel<16>", (9, 16), (5, 130, 257), 130),
    ("kls_grad_block_kernel<32>", (17, 32), (1, 130, 257, 513), 130),
    ("kls_grad_block_kernel<64>", (33, 64), (1, 130, 257, 513), 130),
]


def _ls_cases():
    out = []
    for label, dims, ns, full in LS_ROWS:
        for d in dims:
            for j, n in enumerate(ns):
                # kinds 0 and 1 at every (d, n), B = 1 and 3 swapped between them from one n to the
                # next; n = 513 at the widest d of a kernel keeps B = 1 (the reference's cost)
                for kind, B in ((0, (1, 3)[j % 2]), (1, (3, 1)[j % 2])):
                    if n == 513 and d in (32, 64):
                        B = 1
                    out.append(pytest.param(label, d, n, B, kind, id=f"{label}-d{d}-n{n}-B{B}-kind{kind}"))
                if n == full:
                    for kind, B in ((2, 1), (3, 3), ("mixed", 5)):
                        out.append(pytest.param(label, d, n, B, kind, id=f"{label}-d{d}-n{n}-B{B}-kind{kind}"))
    return out


@pytest.mark.parametrize("label,d,n,B,kind", _ls_cases())
def test_kernel_lengthscale_grad(label, d, n, B, kind):
    from everest_amd import ops

    rng = np.random.default_rng(7919 * d + 31 * n + B)
    X = rng.uniform(-1, 2, (n, d))
    if n >= 64:
        X[[n - 1, n - 2, 40, 33]] = X[[0, 1, 2, 3]]              # 4 duplicated rows (distinct at n = 64)
    ls = rng.uniform(0.3, 1.2, (B, d)) * math.sqrt(d)
    W = rng.normal(size=(B, n, n))                               # not symmetric
    want, S = ref.lengthscale_grad(X, ls, W, _kinds(kind, B))
    args = (_t(X), _t(ls), _t(W), _code(kind, B))
    got = ops.kernel_lengthscale_grad(*args)
    again = ops.kernel_lengthscale_grad(*args)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                               # fixed-order sums: bitwise reproducible
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g))
    err = np.abs(g.astype(ref.LD) - want)
    _note(label, err, S)
    assert np.all(err <= ref.LD(1e-12) * S), float((err / np.maximum(S, ref.LD(1e-300))).max())


# ---------------------------------------------------------------------------------------
# evr_gp_mll_terms
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 33, 257])
def test_mll_terms(n, B):
    from everest_amd import ops

    rng = np.random.default_rng(50 * n + B)
    # a well-conditioned lower factor: diagonal in [0.5, 2] (logs of both signs), small off-diagonal
    L = np.tril(rng.normal(size=(B, n, n)) / math.sqrt(4 * n), -1)
    L[:, np.arange(n), np.arange(n)] = rng.uniform(0.5, 2.0, (B, n))
    Linv = np.tril(np.linalg.inv(L))                             # upper triangle exactly zero
    r, alpha = rng.normal(size=(B, n)), rng.normal(size=(B, n))
    want, S = ref.mll_terms(L, Linv, r, alpha)
    got = ops.mll_terms(_t(L), _t(Linv), _t(r), _t(alpha)).cpu().numpy()
    err = np.abs(got.astype(ref.LD) - want)
    _note("mll_terms_kernel", err, S)
    assert np.all(err <= ref.LD(1e-12) * S), (err / S).astype(np.float64)


# ---------------------------------------------------------------------------------------
# evr_gp_posterior_finalize
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("nt", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 16, 49, 64, 65, 113])
def test_posterior_finalize(n, nt, noise):
    from everest_amd import ops

    B = 2
    rng = np.random.default_rng(1000 * n + nt)
    R = rng.normal(size=(B, n + 1, nt)) / math.sqrt(2 * n)       # sum_i R_i^2 about 1/2
    R[:, n] = np.abs(R[:, n])
    # every term of the mean positive: its relative bar is then the bar against the absolute term sum
    c, ym, ys = rng.uniform(0.1, 1.0, B), rng.uniform(1.0, 4.0, B), rng.uniform(0.5, 4.0, B)
    kxx = np.array([1.0, 1.7])
    nz = np.array([0.03, 0.2]) if noise else None
    mean_w, var_w, ss = ref.posterior_finalize(R, c, ym, ys, kxx, nz)
    mean, var = ops.posterior_finalize(_t(R), _t(c), _t(ym), _t(ys), _t(kxx), _t(nz))
    mean, var = mean.cpu().numpy().astype(ref.LD), var.cpu().numpy().astype(ref.LD)
    em = np.abs(mean - mean_w) / np.abs(mean_w)
    # kxx - sum R^2 (+ noise) recovered from the variance; its bar is relative to kxx + sum R^2 (+ noise)
    ys2 = (np.asarray(ys, dtype=ref.LD) ** 2)[:, None]
    nzl = 0 if nz is None else np.asarray(nz, dtype=ref.LD)[:, None]
    ev = np.abs(var / ys2 - var_w / ys2) / (np.asarray(kxx, dtype=ref.LD)[:, None] + ss + nzl)
    print(f"posterior_finalize n={n} nt={nt}: mean rel {float(em.max()):.2e}, var core {float(ev.max()):.2e}")
    MAXRATIO["posterior_finalize mean"] = max(MAXRATIO.get("posterior_finalize mean", 0.0), float(em.max()))
    MAXRATIO["posterior_finalize var"] = max(MAXRATIO.get("posterior_finalize var", 0.0), float(ev.max()))
    assert np.all(em <= 1e-14)
    assert np.all(ev <= 1e-12)
