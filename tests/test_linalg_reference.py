"""CPU: the plain long-double reference of the dense primitives (tests/linalg_reference.py)
checked against 40-digit mpmath at n = 12, and the inputs of tests/test_gpu_linalg_reference.py
checked for room: LAPACK (torch.linalg.cholesky_ex, solve_triangular, matmul on the CPU) factors
every one of them without jitter and stays under one quarter of each bar the device is held to.
The quarter is a condition on the inputs, not a tolerance of the device: it shows that a correct
float64 algorithm has ample room under the bars.  Measured largest ratios at n >= 15: Cholesky
0.13 gamma(n + 1), solve 0.20 gamma(n), inverse 0.07 n u.  For n <= 3 LAPACK is held to the bar
itself (QUARTER_FROM_N in the reference module says why a quarter cannot be promised there)."""
import numpy as np
import pytest
import torch

from tests import linalg_reference as ref

LD = ref.LD
N = 12
# a long-double sum of k products of float64 values is off by at most k 2^-64 of the sum of the
# absolute values (first order): the ratios agree with the 40-digit ones to that, three orders
# below the bars (gamma(k) ~ k 2^-53) they are compared with
LD_EPS = LD(2) ** -64


def _mp():
    import mpmath as mp

    mp.mp.dps = 40
    return mp


def _mpm(mp, a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _mabs(mp, M):
    return M.apply(abs)


def _mp_ratio(mp, E, S, mask=None):
    best = mp.mpf(0)
    for i in range(E.rows):
        for j in range(E.cols):
            if mask is None or mask(i, j):
                best = max(best, abs(E[i, j]) / S[i, j])
    return best


def _case():
    A = ref.spectrum(N, 4, 5)
    L = torch.linalg.cholesky(A)
    return A, L


def _close(ld_value, mp_value, k):
    return abs(float(ld_value) - float(mp_value)) <= float(2 * k * LD_EPS)


def test_chol_residual_matches_mpmath():
    mp = _mp()
    A, L = _case()
    Am, Lm = _mpm(mp, A), _mpm(mp, L)
    E, S = Lm * Lm.T - Am, _mabs(mp, Lm) * _mabs(mp, Lm).T
    got = ref.chol_residual(A, L)
    assert got.ratio > 0 and _close(got.ratio, _mp_ratio(mp, E, S), N)
    assert _close(got.err / got.scale, got.ratio, 1)
    rows = [0, 5, 11]
    sub = ref.chol_residual(A, L, rows)
    assert _close(sub.ratio, _mp_ratio(mp, E, S, lambda i, j: i in rows), N) and sub.ratio <= got.ratio
    # only A's lower triangle is read
    An = A.clone()
    An[torch.triu(torch.ones(N, N, dtype=torch.bool), 1)] = float("nan")
    assert ref.chol_residual(An, L).ratio == got.ratio
    # a wrong element is seen at its own scale, however small next to the rest
    Lb = L.clone()
    Lb[7, 2] *= 1 + 1e-12
    assert ref.chol_residual(A, Lb).ratio > 10 * ref.gamma(N + 1)
    # a non-zero upper triangle enters the product; NaN gives NaN
    Lu = L.clone()
    Lu[2, 9] = 1e-9
    assert ref.chol_residual(A, Lu).ratio > 1e3 * ref.gamma(N + 1)
    Lu[2, 9] = float("nan")
    assert np.isnan(ref.chol_residual(A, Lu).ratio)
    assert np.isnan(ref.chol_residual(A, Lu, rows=[2]).ratio)


def test_zero_scale_needs_zero_error():
    eye = np.eye(3)
    assert ref.chol_residual(eye, eye).ratio == 0
    A = eye.copy()
    A[2, 0] = 1e-300
    assert ref.chol_residual(A, eye).ratio == np.inf
    assert ref.gemm_error(1.0, np.zeros((2, 3)), np.ones((3, 2)), 0.0, None, np.zeros((2, 2))).ratio == 0
    assert ref.gemm_error(1.0, np.zeros((2, 3)), np.ones((3, 2)), 0.0, None, np.full((2, 2), 1e-300)).ratio == np.inf


@pytest.mark.parametrize("transpose", [False, True])
def test_trsm_residual_matches_mpmath(transpose):
    mp = _mp()
    _, L = _case()
    g = torch.Generator().manual_seed(3)
    B = torch.randn(N, 5, generator=g, dtype=torch.float64) * torch.logspace(-8, 8, 5, dtype=torch.float64)
    X = torch.linalg.solve_triangular(ref.op(L, transpose), B, upper=transpose)
    Tm = _mpm(mp, L).T if transpose else _mpm(mp, L)
    Xm, Bm = _mpm(mp, X), _mpm(mp, B)
    want = _mp_ratio(mp, Tm * Xm - Bm, _mabs(mp, Tm) * _mabs(mp, Xm))
    got = ref.trsm_residual(L, X, B, transpose)
    assert got.ratio > 0 and _close(got.ratio, want, N)
    # the strict upper triangle of L is not read
    Lj = L + torch.triu(torch.full((N, N), float("nan"), dtype=torch.float64), 1)
    assert ref.trsm_residual(Lj, X, B, transpose).ratio == got.ratio
    Xb = X.clone()
    Xb[4, 0] *= 1 + 1e-12                     # the smallest column (scaled by 1e-8)
    assert ref.trsm_residual(L, Xb, B, transpose).ratio > 10 * ref.gamma(N)


def test_tri_inv_matches_mpmath():
    mp = _mp()
    _, L = _case()
    Lm = _mpm(mp, L)
    Xm = mp.inverse(Lm)
    Sm = _mabs(mp, Xm) * _mabs(mp, Lm) * _mabs(mp, Xm)
    Xr = ref.tri_inv_ld(L)
    S = ref.tri_inv_scale(L, Xr)
    for i in range(N):
        for j in range(N):
            if j > i:
                assert Xr[i, j] == 0 and S[i, j] == 0
                continue
            # forward substitution in long double: N 2^-64 |X||L||X| (the bound the device is held
            # to at 2^-53)
            assert abs(mp.mpf(float(Xr[i, j])) + mp.mpf(float(Xr[i, j] - LD(float(Xr[i, j])))) - Xm[i, j]) \
                <= 2 * N * mp.mpf(float(LD_EPS)) * Sm[i, j]
            assert abs(float(S[i, j]) - float(Sm[i, j])) <= 1e-15 * float(Sm[i, j])
    X = torch.linalg.solve_triangular(L, torch.eye(N, dtype=torch.float64), upper=False)
    want = _mp_ratio(mp, _mpm(mp, X) - Xm, Sm, lambda i, j: j <= i)
    got, upper_zero = ref.tri_inv_error(L, X)
    assert upper_zero and got.ratio > 0 and _close(got.ratio, want, 2 * N)
    again, _ = ref.tri_inv_error(L, X, ref=(Xr, S))
    assert again.ratio == got.ratio
    Xu = X.clone()
    Xu[3, 8] = 1e-300
    assert ref.tri_inv_error(L, Xu)[1] is False
    Xb = X.clone()
    Xb[9, 1] *= 1 + 1e-12
    assert ref.tri_inv_error(L, Xb)[0].ratio > 10 * N * ref.U


@pytest.mark.parametrize("beta", [0.0, -0.5])
def test_gemm_error_matches_mpmath(beta):
    mp = _mp()
    A, B, C0 = ref.gemm_operands(7, 5, N, 1, False, False)
    A, B, C0 = A[0], B[0], C0[0]
    C = 1.5 * (A @ B) + beta * C0
    Rm = mp.mpf(1.5) * _mpm(mp, A) * _mpm(mp, B) + mp.mpf(beta) * _mpm(mp, C0)
    Sm = mp.mpf(1.5) * _mabs(mp, _mpm(mp, A)) * _mabs(mp, _mpm(mp, B)) + abs(mp.mpf(beta)) * _mabs(mp, _mpm(mp, C0))
    want = _mp_ratio(mp, _mpm(mp, C) - Rm, Sm)
    C0n = torch.full_like(C0, float("nan")) if beta == 0 else C0      # beta = 0: C0 does not enter
    got = ref.gemm_error(1.5, A, B, beta, C0n, C)
    assert got.ratio > 0 and _close(got.ratio, want, N + 3)
    Cb = C.clone()
    Cb[int(torch.argmin(C.abs().sum(1))), 0] *= 1 + 1e-12            # the smallest row
    assert ref.gemm_error(1.5, A, B, beta, C0n, Cb).ratio > 10 * ref.gamma(N + 3)
    Cb[0, 0] = float("nan")
    assert np.isnan(ref.gemm_error(1.5, A, B, beta, C0n, Cb).ratio)


def test_builders_are_seeded_float64_and_symmetric():
    for f in (lambda s: ref.spectrum(17, 8, s), lambda s: ref.rbf_clustered(17, 1e-6, s), lambda s: ref.graded(17, s)):
        A = f(0)
        assert A.dtype == torch.float64 and torch.equal(A, A.T) and torch.equal(A, f(0)) and not torch.equal(A, f(1))
    ev = torch.linalg.eigvalsh(ref.spectrum(64, 8))
    assert 0.5e8 < float(ev[-1] / ev[0]) < 2e8
    d = torch.diagonal(ref.graded(64))
    assert float(d.max() / d.min()) > 1e20
    rows = ref.residual_rows(1025)
    assert len(rows) == 96 == len(set(rows.tolist())) and {0, 63, 64, 1023, 1024} <= set(rows.tolist())


# ---------------------------------------------------------------------------------------
# the GPU tests' inputs leave a correct float64 algorithm a factor 4
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.CHOL_SMALL_N + (130,) + ref.CHOL_MID_N + (ref.CHOL_BIG_N,))   # 130: the strided calls
def test_lapack_factors_inputs_within_a_quarter(n):
    A = ref.chol_inputs(n)
    L, info = torch.linalg.cholesky_ex(A)
    assert info.eq(0).all()
    eye = torch.eye(n, dtype=torch.float64)
    X = torch.linalg.solve_triangular(L, eye.expand_as(L), upper=False)
    rows = ref.residual_rows(n) if n == ref.CHOL_BIG_N else None
    for b, name in enumerate(ref.chol_classes(n)):
        room = 4 if n >= ref.QUARTER_FROM_N else 1      # n <= 3: see QUARTER_FROM_N
        c = ref.chol_residual(A[b], L[b], rows).ratio / ref.gamma(n + 1)
        e, upper_zero = ref.tri_inv_error(L[b], X[b])
        cols = min(n, 64)     # the solve's residual on the first 64 columns of the identity
        s = ref.trsm_residual(L[b], X[b, :, :cols], eye[:, :cols], False).ratio / ref.gamma(n)
        print(f"n={n} {name}: LAPACK chol {float(c):.3f} inverse {float(e.ratio / (n * ref.U)):.3f} solve {float(s):.3f}")
        assert upper_zero
        assert room * c <= 1 and room * e.ratio <= n * ref.U and room * s <= 1, (n, name)


@pytest.mark.parametrize("n", [130, 200, 513])
def test_lapack_factors_well_conditioned_inputs(n):
    """The matrix of the info tests (and of the lower-triangle-only test at 513 next to the
    ill-conditioned classes)."""
    A = ref.well_conditioned(n)
    L, info = torch.linalg.cholesky_ex(A)
    assert int(info) == 0 and 4 * ref.chol_residual(A, L).ratio <= ref.gamma(n + 1)
    if n == 130:   # the second member of the lower-triangle-only test (513: among chol_inputs)
        A = ref.rbf_clustered(n, 1e-4)
        L, info = torch.linalg.cholesky_ex(A)
        assert int(info) == 0 and 4 * ref.chol_residual(A, L).ratio <= ref.gamma(n + 1)


@pytest.mark.parametrize("n,nrhs,transpose", [(n, r, False) for n, r in ref.TRSM_N_CASES]
                         + [(n, r, True) for n, r in ref.TRSM_T_CASES])
def test_lapack_solves_inputs_within_a_quarter(n, nrhs, transpose):
    L, B = ref.trsm_inputs(n, nrhs)
    X = torch.linalg.solve_triangular(ref.op(L, transpose), B, upper=transpose)
    for b in range(2):
        assert 4 * ref.trsm_residual(L[b], X[b], B[b], transpose).ratio <= ref.gamma(n), (n, nrhs, b)


@pytest.mark.parametrize("n", [65, 513])
def test_lapack_inverts_inputs_within_a_quarter(n):
    L, _ = ref.trsm_inputs(n, 1)
    X = torch.linalg.solve_triangular(L, torch.eye(n, dtype=torch.float64).expand_as(L), upper=False)
    for b in range(2):
        e, upper_zero = ref.tri_inv_error(L[b], X[b])
        assert upper_zero and 4 * e.ratio <= n * ref.U


def test_cpu_matmul_within_a_quarter():
    worst = 0.0
    for M, Nn, K, batch, ta, tb, alpha, beta in ref.GEMM_SHAPES:
        A, B, C0 = ref.gemm_operands(M, Nn, K, min(batch, 2), ta, tb)
        C = alpha * (ref.op(A, ta) @ ref.op(B, tb)) + beta * C0
        for b in range(C.shape[0]):
            r = float(ref.gemm_error(alpha, ref.op(A[b], ta), ref.op(B[b], tb), beta, C0[b], C[b]).ratio
                      / ref.gamma(K + 3))
            worst = max(worst, r)
            assert 4 * r <= 1, (M, Nn, K, ta, tb, r)
    print("CPU matmul: largest ratio to gamma(K + 3)", worst)
