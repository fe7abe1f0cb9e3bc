/*
 * everest_amd — MI355X-native (gfx950) GP-surrogate + qNEHVI hot path of BoFire.
 *
 * C-ABI drop-in boundary.  Plain pointers and sizes only; every device pointer is an
 * HBM allocation owned by the caller (torch tensors in the Python host layer); every
 * entry point enqueues on the given HIP stream (hipStream_t passed as void*) and returns
 * 0 on success, non-zero on error with the message in evr_last_error().  Layouts are
 * row-major float64 unless stated.
 *
 * The reference (experimental-design/everest = BoFire) has no FFI: its hot path hands
 * control to BoTorch/GPyTorch from Python.  Each entry point below names the reference
 * call site whose [upstream] arithmetic it replaces (paths relative to the reference root).
 */
#ifndef EVEREST_AMD_H
#define EVEREST_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define EVR_VERSION 1

/* kernel families: bofire/kernels/mapper.py:31-69 (RBFKernel, MaternKernel nu) */
#define EVR_KERNEL_RBF 0
#define EVR_KERNEL_MATERN05 1
#define EVR_KERNEL_MATERN15 2
#define EVR_KERNEL_MATERN25 3
/* one family per output (heterogeneous ModelListGP members, bofire/surrogates/
 * botorch_surrogates.py:79-128): EVR_KERNEL_MIXED | kind_j << (5 + 2 j), j < 13, wherever an
 * entry point takes `kind` together with a batch of outputs */
#define EVR_KERNEL_MIXED 16

int evr_version(void);
const char* evr_last_error(void);
int evr_device_arch(int device, char* buf, int buflen);
int evr_stream_sync(void* stream);

/* ---- kernel-matrix assembly ---------------------------------------------------------
 * K[b][i][j] = outputscale[b] * k( ||(x1n_i - x2n_j) / ls[b]|| ) (+ diag_add[b] if i==j)
 * x1n = (X1 - shift1) * scale1, x2n = (X2 - shift2) * scale2 per column (NULL = identity),
 * X1: n1 x d, X2: n2 x d, ls: B x d, K: B x n1 x n2 (ld n2).
 * Replaces gpytorch RBFKernel/MaternKernel forward under the Normalize input transform
 * called from bofire/surrogates/single_task_gp.py:48-66 and every posterior() call
 * (bofire/strategies/predictives/botorch.py:180; bofire/surrogates/botorch.py:27,33). */
int evr_kernel_matrix(void* stream, int kind, int B, int n1, int n2, int d,
                      const double* X1, const double* shift1, const double* scale1,
                      const double* X2, const double* shift2, const double* scale2,
                      const double* lengthscales, const double* outputscale,
                      const double* diag_add, double* K);

/* dX2[c][k] = sum_b sum_i G[b][i][c] * dK_b(x1_i, x2_c)/dX2[c][k]  (chain through shift2/scale2)
 * G: B x n1 x n2.  Backward of the cross-covariance for the acquisition gradient
 * (autograd inside gen_candidates_scipy, bofire/strategies/predictives/botorch.py:384-405). */
int evr_kernel_cross_grad(void* stream, int kind, int B, int n1, int n2, int d,
                          const double* X1, const double* shift1, const double* scale1,
                          const double* X2, const double* shift2, const double* scale2,
                          const double* lengthscales, const double* outputscale,
                          const double* G, double* dX2, double* work);
/* doubles of `work` evr_kernel_cross_grad needs (row-split partials); work NULL = allocate */
long long evr_kernel_cross_grad_workspace_doubles(int n1, int n2, int d);

/* MLL gradient pieces for the exact GP fit (fit_gpytorch_mll,
 * bofire/surrogates/single_task_gp.py:70-71):
 * gls[b][k] = sum_{i,j} W[b][i][j] * dK_b[i][j]/d ls[b][k]   (W symmetric, X normalized);
 * work: B*n*d doubles (per-row partials, summed in fixed order -> bitwise reproducible). */
int evr_kernel_lengthscale_grad(void* stream, int kind, int B, int n, int d, const double* X,
                                const double* lengthscales, const double* W, double* gls,
                                double* work);
/* out[b][0..4] = {2 sum log L_ii, r.alpha, ||Linv||_F^2 (= tr K^-1), sum alpha, sum alpha^2}
 * — the scalar terms of the exact MLL and of its noise/constant gradients. */
int evr_gp_mll_terms(void* stream, int B, int n, const double* L, const double* Linv,
                     const double* r, const double* alpha, double* out);

/* ---- mixed continuous / categorical kernel ([upstream] BoTorch MixedSingleTaskGP, built by
 * bofire/surrogates/mixed_single_task_gp.py:46-112) --------------------------------------
 *   K(x, x') = s_sum (k_c(r1) + s_cat h1) + s_prod k_c(r2) h2
 *   r_t^2 = sum_k ((xc_k - xc'_k) / ls_t,k)^2                              t = 1, 2
 *   h_t   = exp(-(1 / nc) sum_f [c_f != c'_f] / lam_t,f)   (CategoricalKernel, ARD over the features)
 * k_c: one family 0..3 (kind) for every member, with the d2 < 1e-30 convention of the
 * continuous kernels.  Inputs, shared by the B members: Xc (n x dc, normalised continuous
 * columns) and C (n x nc, int32 category codes).  Member b reads params + b P,
 * P = 2 dc + 2 nc + 3: [ls1 (dc) | ls2 (dc) | lam1 (nc) | lam2 (nc) | s_sum | s_cat | s_prod].
 * Supported: 1 <= dc <= 32, 1 <= nc <= 8 (any cardinality); anything else is an error.
 *
 * K: B x n1 x n2; diag_add (B, or NULL) is added where i == j (meaningful for the train
 * matrix only).  Explicit differences, no distance expansion.  Every entry is computed from an
 * expression that does not depend on the order of its two points (no tile is mirrored): with
 * X2 = X1 the result is bitwise symmetric, and the train matrix is the cross call's. */
int evr_mixed_kernel_matrix(void* stream, int kind, int B, int n1, int n2, int dc, int nc, const double* X1c,
                            const int* C1, const double* X2c, const int* C2, const double* params,
                            const double* diag_add, double* K);
/* g[b][p] = sum_{i,j} W[b][i][j] dK_b[i][j] / dparams_p for all P parameters in one pass over W
 * (B x n x n, need not be symmetric).  work: B*n*P doubles (per-row partials, summed in a
 * fixed order: bitwise reproducible).  A wave per row up to dc = 16 (instantiations for
 * dc <= 8 and dc <= 16), a workgroup per row above. */
int evr_mixed_kernel_param_grad(void* stream, int kind, int B, int n, int dc, int nc, const double* Xc, const int* C,
                                const double* params, const double* W, double* g, double* work);
/* Candidate split: raw transformed rows X (rows x d, continuous columns and one-hot blocks) ->
 * Xc (rows x dc) = (X[:, cont_idx[k]] - shift[cont_idx[k]]) * scale[cont_idx[k]] (shift / scale
 * d-wide, the Normalize bounds; exactly that subtraction and product) and Cc (rows x nc, int32):
 * per block [cat_start[f], cat_start[f] + cat_len[f]) the arg-max, the first on ties
 * ([upstream] OneHotToNumeric).  cont_idx / cat_start / cat_len: device int arrays. */
int evr_mixed_split(void* stream, int rows, int d, int dc, int nc, const double* X, const double* shift,
                    const double* scale, const int* cont_idx, const int* cat_start, const int* cat_len,
                    double* Xc, int* Cc);
/* X-gradient of the mixed cross-covariance K(train, candidates): given G = dK (B x n x rows),
 *   dXc[j][k] = sum_b sum_i G[b][i][j] (s_sum k_c'(r1^2) (xc_jk - xc_ik) / ls1_k^2
 *                                      + s_prod h2(i, j) k_c'(r2^2) (xc_jk - xc_ik) / ls2_k^2)
 * (k_c' the families' derivative factor with the d2 < 1e-30 convention; the s_sum s_cat h1 term
 * does not depend on x), written into the d-wide dX (rows x d) as dX[j][cont_idx[k]] =
 * dXc[j][k] * scale[cont_idx[k]]; every other column (the one-hot blocks: the arg-max has no
 * gradient) is set to exactly 0.  A row split into partials and a fixed-order reduction: no
 * atomics, bitwise reproducible.  work: evr_mixed_kernel_cross_grad_workspace_doubles(n, rows,
 * dc) doubles (NULL = allocate).  Instantiations for dc <= 8, <= 16, <= 32. */
long long evr_mixed_kernel_cross_grad_workspace_doubles(int n, int rows, int dc);
int evr_mixed_kernel_cross_grad(void* stream, int kind, int B, int n, int rows, int d, int dc, int nc,
                                const double* Xc, const int* C, const double* X2c, const int* C2,
                                const double* params, const double* scale, const int* cont_idx, const double* G,
                                double* dX, double* work);

/* ---- dot-product kernels ([upstream] gpytorch LinearKernel / PolynomialKernel behind
 * bofire/data_models/surrogates/linear.py and polynomial.py) --------------------------------
 * Functions of the Gram matrix G = X1n X2n^T of the normalised inputs (evr_gemm_f64, transB):
 *   power = 0        k = theta g                 theta = the variance v
 *   power = p in 1..8  k = (g + theta)^p         theta = the offset c
 * theta: B doubles, one per member.  Powers are formed by repeated multiplication in one fixed
 * order, never through pow(): t = g + theta, r_1 = t, r_{k+1} = r_k t, k = r_p; the theta
 * derivative is g (power 0), exactly 1 (p = 1) and (double)p r_{p-1} (p >= 2).  The kernels are
 * not stationary: the prior variance k(x, x) = theta |x|^2 or (|x|^2 + theta)^p depends on x.
 * A power outside 0..8 is an error.
 *
 * K[b][i][j] = f(G[i][j]; theta_b) (+ diag_add[b] where i == j; diag_add may be NULL).  G: n1 x n2,
 * shared by the members; K: B x n1 x n2.  G and K must not alias.  Element-wise, so a symmetric G
 * gives a bitwise symmetric K.  n1 n2 = 0 returns 0 without a launch; n1 n2 < 2^31. */
int evr_dot_kernel_apply(void* stream, int power, int B, int n1, int n2, const double* G, const double* theta,
                         const double* diag_add, double* K);
/* g[b] = sum_{i,j} W[b][i][j] df/dtheta(G[i][j]; theta_b) in one pass over W (B x n x n, need not be
 * symmetric) and G (n x n).  work: B*n doubles (per-row partials, summed in a fixed order: no
 * atomics, bitwise reproducible). */
int evr_dot_kernel_theta_grad(void* stream, int power, int B, int n, const double* G, const double* theta,
                              const double* W, double* g, double* work);
/* Whole posterior in one call, on the model of evr_gp_posterior: the test rows are normalised
 * ((X - shift) * scale per column, exactly that subtraction and product; NULL = identity), the
 * cross Gram Xn Xt^T, evr_dot_kernel_apply, R = M K* with M = [Linv; alpha^T] (B x (n+1) x n), and
 *   mean[b][t] = ym[b] + ys[b] (c[b] + R[b][n][t])
 *   var[b][t]  = ys[b]^2 (k_b(x_t, x_t) - sum_{i<n} R[b][i][t]^2 + noise_add[b])
 * with k_b(x_t, x_t) from the test point's own normalised row (|x_t|^2 summed in column order).
 * R's columns are reduced in a fixed order.  Xn: n x d normalised training rows, X: nt x d raw.
 * work: evr_dot_gp_posterior_workspace_doubles(B, n, nt, d) doubles, 16-byte aligned.  nt = 0
 * returns 0 without a launch. */
long long evr_dot_gp_posterior_workspace_doubles(int B, int n, int nt, int d);
int evr_dot_gp_posterior(void* stream, int power, int B, int n, int nt, int d, const double* Xn, const double* X,
                         const double* shift, const double* scale, const double* theta, const double* M,
                         const double* c, const double* ym, const double* ys, const double* noise_add, double* mean,
                         double* var, double* work);

/* Native MLL plan for the GP fit: B exact GPs sharing the normalised inputs Xn (n x d,
 * device, must outlive the plan) with standardised targets Y (B x n, device, copied).  One
 * evr_mll_plan_eval is one hipGraph launch computing, per member b, with params (host) =
 * [lengthscales (B x d) | noise (B) | constant (B)]:
 *   out (host) = [terms (B x 5) as evr_gp_mll_terms | gls (B x d) as
 *                 evr_kernel_lengthscale_grad with W = alpha alpha^T - K^-1 | info (B)]
 * for K = k(Xn, Xn; ls_b) + noise_b I (psd_safe_cholesky attempt 0: a member with
 * info != 0 needs the jitter ladder, i.e. the unfused path).  Replaces the per-evaluation
 * op chain of the ExactMarginalLogLikelihood closure inside [upstream] fit_gpytorch_mll
 * (bofire/surrogates/single_task_gp.py:70-71). */
typedef struct evr_mll_plan evr_mll_plan;
int evr_mll_plan_create(void* stream, int kind, int B, int n, int d, const double* Xn, const double* Y,
                        evr_mll_plan** out);
int evr_mll_plan_eval(void* stream, evr_mll_plan* plan, const double* params, double* out);
void evr_mll_plan_destroy(evr_mll_plan* plan);

/* The lock-step fit of the plan's B members in native code (gp.fit_batch: one L-BFGS-B per
 * output over -MLL / n with the gpytorch priors, [upstream] fit_gpytorch_mll ->
 * scipy L-BFGS-B, bofire/surrogates/single_task_gp.py:70-71).  Member b: runs[b] an
 * evr_lbfgsb of dimension d + 2 over x = [noise, constant, raw lengthscales (softplus)],
 * task[b] its current task (EVR_LBFGSB_FG: x[b] is to be evaluated; 0: finished), f / g the
 * last evaluation it was given, nit / nfev / status as scipy's driver loop counts them
 * (status 0 converged, 1 iteration / evaluation limit, 2 abnormal line search, 3 error).
 * params (B x (d + 2), the plan's layout) carries the members' last evaluated parameters
 * across calls.  prior: ls (fam, a, b), noise (fam, a, b) with fam 0 none, 1 LogNormal,
 * 2 Gamma, 3 Normal.  Runs rounds (one plan evaluation of every member with task FG, then
 * each one's L-BFGS-B steps) until every member has finished (*pending = 0), or a round in
 * which an evaluated member's attempt-0 factor failed or its terms are not finite: then
 * nothing of that round is consumed and *pending = 1 (the caller evaluates that round
 * through the jitter ladder and hands the results to evr_lbfgsb_advance). */
int evr_mll_fit_rounds(void* stream, evr_mll_plan* plan, void** runs, int* task, double* x, double* f, double* g,
                       int* nit, int* nfev, int* status, int maxiter, int maxfun, const double* prior, double* params,
                       int* pending);
/* Host-only.  ll / n and its gradient in x = [noise, constant, raw lengthscales] per member
 * (B x (d + 2)), the ExactMarginalLogLikelihood with the hyperparameter priors (prior as in
 * evr_mll_fit_rounds) divided by n, from the plan's terms (B x 5) and lengthscale-gradient
 * pieces gls (B x d): the closure of fit_gpytorch_mll (bofire/surrogates/single_task_gp.py:70-71)
 * after the device work; evr_mll_fit_rounds applies the same code. */
int evr_mll_assemble(int B, int n, int d, const double* prior, const double* x, const double* terms,
                     const double* gls, double* ll, double* g);
/* ---- member form: B GPs on their own training rows (the folds of a cross-validation) -----
 * Member b has its own normalised inputs Xb[b] (n x d, device; Xb is B x n x d) of which the
 * first nvalid[b] <= n rows are real and the rest padding (finite values, zeros by
 * convention).  Its train matrix is padded with the identity:
 *   K[b][i][j] = k(|(x_bi - x_bj) / ls_b|) + diag_add[b] [i == j]      i, j < nvalid[b]
 *              = [i == j] exactly                                       otherwise,
 * so chol(K[b]) is the member's own factor with an identity block, and with r = 0 on the
 * padded rows alpha is 0 there, W = alpha alpha^T - K^-1 is exactly 0 off the diagonal of the
 * padded rows / columns, log det, r.alpha, sum alpha and sum alpha^2 are the member's own, and
 * tr K^-1 is its own plus the pad count n - nvalid[b].  kind: one family 0..3; the dispatch
 * (VALU differences for d < 16, MFMA distance expansion for 16 <= d <= 64) and the arithmetic
 * of the valid block are evr_kernel_matrix's for the symmetric train matrix. */
int evr_kernel_matrix_members(void* stream, int kind, int B, int n, int d, const double* Xb, const int* nvalid,
                              const double* lengthscales, const double* diag_add, double* K);
/* evr_kernel_lengthscale_grad with member b reading Xb[b] (same instantiations and summation
 * order).  No nvalid: with the padding above W is exactly 0 off the diagonal of the padded rows
 * and columns (a finite dK/dls times 0), and a diagonal entry has distance 0, i.e. dK/dls = 0. */
int evr_kernel_lengthscale_grad_members(void* stream, int kind, int B, int n, int d, const double* Xb,
                                        const double* lengthscales, const double* W, double* gls, double* work);
/* evr_mll_plan_create for members: Xb (B x n x d, device, must outlive the plan), Y (B x n,
 * device, copied; entries of padded rows ignored), nvalid (B, host, copied).  The plan is
 * evaluated by evr_mll_plan_eval / evr_mll_fit_rounds as any other; r is 0 on padded rows, the
 * reported tr K^-1 has the pad count subtracted, and evr_mll_fit_rounds scales member b by its
 * own nvalid[b]: every reported term is the member's own GP's. */
int evr_mll_plan_create_members(void* stream, int kind, int B, int n, int d, const double* Xb, const double* Y,
                                const int* nvalid, evr_mll_plan** out);
/* evr_mll_assemble with member b's own size nvalid[b] (host) for the -n/2 log 2 pi term and the
 * 1 / n scaling. */
int evr_mll_assemble_members(int B, const int* nvalid, int d, const double* prior, const double* x,
                             const double* terms, const double* gls, double* ll, double* g);
/* ---- scaled kernel: k = sigma^2 k_base (gpytorch ScaleKernel around RBF / Matérn) ------------
 * The MLL gradient pieces of the lengthscales and of the outputscale sigma^2 in one pass over W:
 *   out = [gls (B x d) | gos (B)],
 *   gls[b][k] = sigma^2_b sum_ij W[b][i][j] dk_base[i][j] / d ls[b][k]   (dK/dls = sigma^2 dk_base/dls)
 *   gos[b]    = sum_ij W[b][i][j] k_base[i][j]                           (dK/dsigma^2 = k_base)
 * evr_kernel_lengthscale_grad's dispatch, lane order and row partials, one column wider; k_base and
 * its derivative factor come from one exponential per pair.  outputscale: B doubles.
 * work: B*n*(d+1) doubles (per-row partials, summed in a fixed order: no atomics, bitwise
 * reproducible). */
int evr_kernel_hyper_grad(void* stream, int kind, int B, int n, int d, const double* X, const double* lengthscales,
                          const double* outputscale, const double* W, double* out, double* work);
/* Member form.  Unlike the lengthscale pieces, gos is not blind to the identity padding (a padded
 * row has W_ii = -1 and k_base(0) = 1), so the sums run over the member's own rows and columns
 * i, j < nvalid[b] only (nvalid: B ints, device): every piece is the member's own GP's. */
int evr_kernel_hyper_grad_members(void* stream, int kind, int B, int n, int d, const double* Xb, const int* nvalid,
                                  const double* lengthscales, const double* outputscale, const double* W, double* out,
                                  double* work);
/* evr_kernel_matrix_members with K = outputscale[b] k_base + diag_add[b] I on the member's real
 * block; the padding stays the identity. */
int evr_kernel_matrix_members_scaled(void* stream, int kind, int B, int n, int d, const double* Xb, const int* nvalid,
                                     const double* lengthscales, const double* outputscale, const double* diag_add,
                                     double* K);
/* MLL plans of the scaled kernel.  evr_mll_plan_eval reads params = [ls (B x d) | noise (B) |
 * constant (B) | outputscale (B)] and writes out = [terms (B x 5) | gls (B x d) | gos (B) |
 * info (B)] (gls, gos as evr_kernel_hyper_grad).  evr_mll_plan_eval, evr_mll_fit_rounds and
 * evr_mll_plan_destroy take either kind of plan; for a scaled plan evr_mll_fit_rounds' member
 * dimension is d + 3, x = [noise, constant, raw lengthscales, raw outputscale] (softplus), params
 * is B x (d + 3), and prior has nine entries: ls, noise, outputscale x (family, a, b). */
int evr_mll_plan_create_scaled(void* stream, int kind, int B, int n, int d, const double* Xn, const double* Y,
                               evr_mll_plan** out);
int evr_mll_plan_create_scaled_members(void* stream, int kind, int B, int n, int d, const double* Xb, const double* Y,
                                       const int* nvalid, evr_mll_plan** out);
/* Host-only.  evr_mll_assemble[_members] for the scaled kernel: x is B x (d + 3), g likewise, prior
 * has nine entries; the outputscale prior is evaluated on sigma^2 = softplus(raw) and
 * g[d + 2] = (gos / 2 + d log prior / d sigma^2) sigmoid(raw) / n. */
int evr_mll_assemble_scaled(int B, int n, int d, const double* prior, const double* x, const double* terms,
                            const double* gls, const double* gos, double* ll, double* g);
int evr_mll_assemble_scaled_members(int B, const int* nvalid, int d, const double* prior, const double* x,
                                    const double* terms, const double* gls, const double* gos, double* ll, double* g);
/* One member's L-BFGS-B after its evaluation at x (f, g): scipy's driver loop up to the next
 * evaluation request or the end (the state machine evr_mll_fit_rounds applies). */
int evr_lbfgsb_advance(void* run, double f, const double* g, double* x, int* task, int* nit, int* nfev,
                       int* status, int maxiter, int maxfun);

/* ---- dense float64 linear algebra --------------------------------------------------- */
int evr_gemm_f64(void* stream, int transA, int transB, int M, int N, int K, double alpha,
                 const double* A, int lda, long long strideA, const double* B, int ldb,
                 long long strideB, double beta, double* C, int ldc, long long strideC, int batch);

/* Batched Cholesky with [upstream] linear_operator psd_safe_cholesky semantics: plain
 * attempt, then total diagonal jitter jitter0*10^(t-1) for t = 1..max_tries.  info[b] = 0
 * on success; otherwise member b is still not p.d. after the last attempt (NotPSDError) and
 * info[b] = k + 1, k the first pivot of that attempt that is not positive (NaN included):
 * LAPACK potrf's index.  L of a failed member is unspecified.  A and L must not alias.
 * Only the lower triangle of A (j <= i) is read: the strict upper triangle may hold anything,
 * NaN included.  L's strict upper triangle is written as zeros.  lda / ldl >= n; the
 * elements of each row from column n to ld - 1 and the gaps between batch members
 * (stride >= n * ld) are neither read nor written.
 * Replaces the Cholesky behind GPyTorch exact inference (K + sigma^2 I), the qNEHVI
 * baseline root (bofire/strategies/predictives/qnehvi.py:46, cache_root=True) and the
 * prune-sampling root (qnehvi.py:44, prune_baseline=True). */
int evr_cholesky(void* stream, int batch, int n, const double* A, int lda, long long strideA,
                 double* L, int ldl, long long strideL, double jitter0, int max_tries,
                 double* jitter_used, int* info);

/* evr_cholesky plus L^-1 (Linv) from the same blocked pass (diagonal-block inverses are
 * by-products of the factorisation).  A, L and Linv must not alias.  Linv is lower
 * triangular with an exactly zero strict upper triangle; info and the operand layout as for
 * evr_cholesky (Linv of a failed member is unspecified). */
int evr_cholesky_inverse(void* stream, int batch, int n, const double* A, int lda, long long strideA,
                         double* L, int ldl, long long strideL, double* Linv, int ldi,
                         long long strideI, double jitter0, int max_tries, double* jitter_used,
                         int* info);

/* In-place B <- L^-1 B (transpose=0) or L^-T B (transpose=1); L lower, n x n; B n x nrhs. */
int evr_trsm_lower(void* stream, int batch, int n, int nrhs, const double* L, int ldl,
                   long long strideL, int transpose, double* B, int ldb, long long strideB);
int evr_tri_inv_lower(void* stream, int batch, int n, const double* L, int ldl, long long strideL,
                      double* Linv, int ldi, long long strideI);

/* ---- GP posterior --------------------------------------------------------------------
 * Given R[b] = [Linv_b; alpha_b^T] * K(Xtr, Xtest)  ((n+1) x nt per output, ld nt):
 * mean[b][t] = ym[b] + ys[b]*(c[b] + R[b][n][t]);
 * var[b][t]  = ys[b]^2 * (kxx[b] - sum_{i<n} R[b][i][t]^2 + noise_add[b]).
 * Replaces [upstream] GPyTorch exact prediction (fast_pred_var covar cache) + Standardize
 * untransform, called at bofire/strategies/predictives/botorch.py:180 and
 * bofire/surrogates/botorch.py:27-33. */
int evr_gp_posterior_finalize(void* stream, int B, int n, int nt, const double* R,
                              const double* c, const double* ym, const double* ys,
                              const double* kxx, const double* noise_add,
                              double* mean, double* var);

/* Whole posterior in one call: K_x = k(Xn, normalize(X)) (kernel_matrix), then the moments
 * of R = M K_x (M = [Linv; alpha^T], B x (n+1) x n) without storing R: per 32-row tile sums
 * of squares, finalised as above by each column tile's last-arriving workgroup.  work:
 * evr_gp_posterior_workspace_doubles(B, n, nt) doubles (K_x, the row-tile partials, the mean
 * row and the arrival counters), 16-byte aligned, contents irrelevant on entry. */
long long evr_gp_posterior_workspace_doubles(int B, int n, int nt);
int evr_gp_posterior(void* stream, int B, int n, int nt, int d, int kind, const double* Xn, const double* X,
                     const double* shift, const double* scale, const double* lengthscales, const double* M,
                     const double* c, const double* ym, const double* ys, const double* kxx,
                     const double* noise_add, double* mean, double* var, double* work);

/* ---- qNEHVI (q = 1) -----------------------------------------------------------------
 * Replaces [upstream] qNoisyExpectedHypervolumeImprovement.forward/backward as built at
 * bofire/strategies/predictives/qnehvi.py:39-52 (cached-Cholesky sampling + box-cell HVI).
 * Per output j the precomputed operator M_j = [Linv; G; H^T; alpha^T] (rows Rr =
 * n + nb + S + 1; n + nb + 1 with no_h) has been applied to k(Xtr, x): R_j = M_j K_x
 * (Rr x b, ld b). */
typedef struct {
  int n, nb, S, m;          /* train points, pruned baseline, MC samples, objectives */
  const double* c;          /* m: constant mean (standardized space) */
  const double* ym;         /* m: Standardize mean */
  const double* ys;         /* m: Standardize std */
  const double* kxx;        /* m: prior variance k(x,x) */
  const double* zq;         /* S x m: base samples of the new point */
  const double* obj_a;      /* m: objective g_j = a_j*y_j + b_j */
  const double* obj_b;      /* m */
  /* box-decomposition cells (maximisation space), AoS per cell, ragged per sample */
  const double* cell_lo;    /* total_cells x m */
  const double* cell_hi;    /* total_cells x m (may be +inf) */
  const int* cell_off;      /* S + 1 */
  int max_cells;            /* max_s (cell_off[s+1] - cell_off[s]) — host-known, sizes the launch */
  /* compressed cells (device box decomposition, evr_box_pack_keys_device): when cell_keys is
   * not NULL the scan rebuilds every cell from its 64-bit key of defining-point indices and
   * the sample's point table, and cell_lo / cell_hi are not read. */
  const unsigned long long* cell_keys; /* total_cells */
  const double* cell_pts;   /* S x pts_stride x m: minimisation-space points, then m dummies */
  const int* cell_rank0;    /* S x pts_stride: point index of rank r (key field 0) */
  int pts_stride;           /* rows per sample of cell_pts / cell_rank0 */
  /* kd-ordered cell groups (evr_cells_kd_order_device, needs the compressed cells above):
   * when grp_off is not NULL the scan runs the sparse group -> cell -> term filter */
  const int* grp_off;                  /* S + 1: group offsets, 16 cells per group */
  const unsigned long long* grp_keys;  /* grp_off[S]*16 cell keys in kd order (field 0: point index) */
  const unsigned short* grp_rank;      /* grp_off[S] x m x 16 per-cell lower-bound ranks (0x7FFF pad) */
  const unsigned short* grp_box;       /* grp_off[S] x 8: per-group minimum rank per objective */
  const double* sorted_lo;             /* S x m x pts_stride ascending lower-bound values */
  int max_groups;                      /* max_s (grp_off[s+1] - grp_off[s]) */
  /* optional scan statistics (nullable, device): [0] += passing (candidate, group) pairs,
   * [1] += exact (cell, candidate) terms evaluated, [2] += (candidate, group) tests,
   * [3] += (candidate, 16-group chunk) entries passing the chunk pre-filter (hvi_kd2) */
  unsigned long long* scan_counters;
  /* 0: M = [Linv; G; H^T; alpha^T] (qNEHVI).  1: M carries no H^T rows (Rr = n + nb + 1) and
   * the samples have no baseline term, y_s = mu + L22 zq_s — qEHVI, where the cells come
   * from the observed Pareto front instead of per-sample baseline draws (nb = 0). */
  int no_h;
  /* 1: log-space scan (qLogNEHVI / qLogEHVI, fat = True): acq = logmeanexp_s logsumexp_cells
   * sum_j fatmin(log fatplus(y_j - l_j; tau_relu), log(min(u_j, 1e10) - l_j); tau_max), dense
   * over every cell; needs the explicit cells cell_lo / cell_hi (keys and kd groups unused). */
  int log_hvi;
  double tau_relu, tau_max;
} evr_qnehvi_state;

/* samples: G[s][j][c] = g_j(mu_j + h_js + L22_j zq[s][j]); aux L22: m x b; flags: m x b
 * (0 ok, 1 new-block Cholesky failed after 6 jitter tries). */
int evr_qnehvi_samples(void* stream, const evr_qnehvi_state* st, int b, const double* R,
                       double* G, double* L22, int* flags);
/* Workspace (doubles) the HVI scan needs for b candidates (per-(sample, cell-chunk)
 * partials); backward != 0 sizes it for evr_hvi_backward / evr_hvi_forward_backward. */
long long evr_hvi_workspace_doubles(const evr_qnehvi_state* st, int b, int backward);
/* acq[c] = mean_s HVI_s(G[s][:, c]) over the cells of sample s (register-tiled cell x
 * candidate scan, deterministic two-stage reduction); acq[c] = NaN where flags (m x b,
 * from evr_qnehvi_samples, nullable) report a failed new-point Cholesky block. */
int evr_hvi_forward(void* stream, const evr_qnehvi_state* st, int b, const double* G,
                    const int* flags, double* work, double* acq);
/* acq[c] = mean_s partial[s][c] */
int evr_mean_over_samples(void* stream, int S, int b, const double* partial, double* acq);
/* dG[s][j][c] = gout[c]/S * dHVI_s/dg_j (torch min/clamp_min/prod subgradients; gout NULL = 1) */
int evr_hvi_backward(void* stream, const evr_qnehvi_state* st, int b, const double* G,
                     const double* gout, double* work, double* dG);
/* One fused scan: acq (as evr_hvi_forward, NaN on flags) and dG (as evr_hvi_backward). */
int evr_hvi_forward_backward(void* stream, const evr_qnehvi_state* st, int b, const double* G,
                             const int* flags, const double* gout, double* work, double* acq,
                             double* dG);
/* Restart-batch scan (kd cells, b <= 32) in one launch (hvi_kdw: one wave per sample and
 * candidate): what evr_hvi_forward_backward (gout = NULL) computes, in the wave's own
 * summation order.  sval (S x b) holds the per-sample HVI values, acq = their mean
 * (evr_mean_over_samples; the plan folds it into the dX reduction).  _applies: 1 when the
 * state / batch qualifies. */
int evr_hvi_restart_fb_applies(const evr_qnehvi_state* st, int b);
/* 0 if the linear scans accept compressed cells whose point tables have `stride` rows (the
 * bound every evr_hvi_* entry checks: the table is staged in LDS), else 3.  A caller asks
 * before it chooses the device box decomposition (stride = n + m). */
int evr_hvi_scan_limits(int stride, int m);
int evr_hvi_restart_fb(void* stream, const evr_qnehvi_state* st, int b, const double* G, double* sval,
                       double* dG);
/* gR_j (Rr x b): gradient w.r.t. R_j given dG (chains objective, sampling, L22 ladder) */
int evr_qnehvi_samples_backward(void* stream, const evr_qnehvi_state* st, int b, const double* R,
                                const double* L22, const double* dG, double* gR);

/* Fused projection path (qnehvi_proj.hip), replacing gemm + evr_qnehvi_samples +
 * evr_qnehvi_samples_backward + gemm^T:
 * evr_qnehvi_project: R_j = M_j Kx_j (M: m x Rr x n, Kx: m x n x b, R: m x Rr x b) and the
 *   per-64-row-tile partial sums of squares norms (m x evr_qnehvi_norms_rows(st) x 2 x b).
 * evr_qnehvi_samples_norms: G, L22, flags as evr_qnehvi_samples, from R's sample / mean rows
 *   and the partial norms.
 * evr_qnehvi_project_backward: dKx_j = M_j^T gR_j (n x b per output) with gR generated in
 *   the K loop from R, L22 and dG (never written to memory).
 * `work` (split-K partials, gR coefficients): the *_workspace_doubles size, NULL = allocate. */
int evr_qnehvi_norms_rows(const evr_qnehvi_state* st);
int evr_qnehvi_project(void* stream, const evr_qnehvi_state* st, int b, const double* M, const double* Kx,
                       double* R, double* norms, double* work);
long long evr_qnehvi_project_workspace_doubles(const evr_qnehvi_state* st, int b);
int evr_qnehvi_samples_norms(void* stream, const evr_qnehvi_state* st, int b, const double* R,
                             const double* norms, double* G, double* L22, int* flags);
int evr_qnehvi_project_backward(void* stream, const evr_qnehvi_state* st, int b, const double* M,
                                const double* R, const double* L22, const double* dG, double* dKx,
                                double* work);
long long evr_qnehvi_project_backward_workspace_doubles(const evr_qnehvi_state* st, int b);

/* Native evaluation plan of the whole qNEHVI chain (qnehvi_plan.hip): K_x, fused projection,
 * samples, HVI scan (+ backward: projection^T with generated gR, cross-covariance gradient)
 * in one call, every intermediate carved from `work`, optionally captured into a hipGraph
 * (use_graph) and replayed by evr_qnehvi_plan_run.  X: b x d raw (transformed) candidates;
 * acq: b; dX: b x d (backward).  The plan copies *st / *md; the buffers they and X / work /
 * acq / dX point to must outlive the plan.
 * Replaces one [upstream] qNoisyExpectedHypervolumeImprovement forward (+ autograd backward)
 * call of gen_candidates_scipy (bofire/strategies/predictives/botorch.py:384-405). */
typedef struct {
  int n, d, kind;              /* training points, input dims, EVR_KERNEL_* */
  const double* Xn;            /* n x d normalized training inputs */
  const double* lengthscales;  /* m x d */
  const double* shift;         /* d: Normalize lower bounds (candidates arrive raw) */
  const double* scale;         /* d: 1 / (upper - lower) */
  const double* M;             /* m x (n + nb + S + 1) x n forward operator [Linv; G; H^T; alpha^T] */
  /* Mixed continuous / categorical model (evr_mixed_kernel_matrix's kernel); all zero = the
   * stationary model above.  With mixed != 0, Xn and lengthscales are not read; candidates still
   * arrive as raw d-wide rows (one-hot blocks for the categoricals) and are split on the device
   * (evr_mixed_split).  Only the chains of evr_qnei_eval / evr_qsobo_eval / evr_qparego_eval /
   * evr_qreward_eval / evr_qmult_eval take a mixed model; every other entry point that reads
   * this struct fails with an evr_last_error. */
  int mixed, dc, nc;           /* flag, continuous columns (1..32), categorical features (1..8) */
  const double* Xc;            /* n x dc normalised continuous training columns */
  const int* C;                /* n x nc training category codes */
  const double* params;        /* m x (2 dc + 2 nc + 3): [ls1 | ls2 | lam1 | lam2 | s_sum | s_cat | s_prod] */
  const int* cont_idx;         /* dc: column of X holding continuous column k */
  const int* cat_start;        /* nc: first column of categorical feature f's one-hot block */
  const int* cat_len;          /* nc: levels (columns) of that block */
} evr_qnehvi_model;
typedef struct evr_qnehvi_plan evr_qnehvi_plan;
long long evr_qnehvi_plan_workspace_bytes(const evr_qnehvi_state* st, const evr_qnehvi_model* md, int b,
                                          int backward);
int evr_qnehvi_plan_create(void* stream, const evr_qnehvi_state* st, const evr_qnehvi_model* md, int b,
                           int backward, const double* X, void* work, double* acq, double* dX, int use_graph,
                           evr_qnehvi_plan** out);
/* The b <= 32 (restart-batch) pieces of the plan chain, exposed op by op for measurement and
 * parity tests (qnehvi_small.hip): small_forward R, P (16-row norm tiles) from Kx; small_samples
 * G, L22, flags from them; small_backward dX (b x d, the cross-covariance gradient fused) from
 * R, L22, dG and the candidates X.  workspace_doubles(which = 0: P, 1: dXp). */
int evr_qnehvi_small_applies(const evr_qnehvi_state* st, int b, int d);
long long evr_qnehvi_small_workspace_doubles(const evr_qnehvi_state* st, int b, int d, int which);
int evr_qnehvi_small_forward(void* stream, const evr_qnehvi_state* st, const evr_qnehvi_model* md, int b,
                             const double* Kx, double* R, double* P);
int evr_qnehvi_small_samples(void* stream, const evr_qnehvi_state* st, int b, const double* R, const double* P,
                             double* G, double* L22, int* flags);
int evr_qnehvi_small_backward(void* stream, const evr_qnehvi_state* st, const evr_qnehvi_model* md, int b,
                              const double* X, const double* R, const double* L22, const double* dG, double* dXp,
                              double* dX);
int evr_qnehvi_plan_run(void* stream, evr_qnehvi_plan* plan);
/* One evaluation at host x (b x d): out (host) = [acq (b) | dX (b x d, backward plans)].
 * Runs a second graph [copy-in from fine-grained pinned memory, the chain, copy-out + a
 * completion word] and spins on that word: no blit copies and no stream synchronise per
 * evaluation (the hot loop of evr_qnehvi_plan_minimize; botorch's per-evaluation
 * forward+backward of gen_candidates_scipy's objective). */
int evr_qnehvi_plan_eval_host(void* stream, evr_qnehvi_plan* plan, const double* x, double* out);
void evr_qnehvi_plan_destroy(evr_qnehvi_plan* plan);

/* ---- acquisition restarts: native L-BFGS-B ------------------------------------------
 * Restatement of the bound-constrained L-BFGS-B (v3.0: Cauchy point, direct primal
 * subspace step with projection / backtracking, More-Thuente line search) that
 * scipy.optimize.minimize(method="L-BFGS-B") runs inside [upstream] botorch
 * gen_candidates_scipy, called by optimize_acqf from
 * bofire/strategies/predictives/botorch.py:384-405 (box bounds, no linear constraints).
 * Host-only.  Reverse communication: evr_lbfgsb_start returns EVR_LBFGSB_FG with the
 * (projected) x to evaluate; evr_lbfgsb_step(f, g at x) returns the next task and x.
 * m: corrections (scipy maxcor 10), factr = ftol / eps (1e7), pgtol (1e-5), maxls (20). */
#define EVR_LBFGSB_FG 1
#define EVR_LBFGSB_NEW_X 2
#define EVR_LBFGSB_CONV_PGTOL 3
#define EVR_LBFGSB_CONV_FACTR 4
#define EVR_LBFGSB_ABNORMAL 5
#define EVR_LBFGSB_ERROR 6
typedef struct evr_lbfgsb evr_lbfgsb;
int evr_lbfgsb_create(int n, int m, const double* lb, const double* ub, double factr, double pgtol, int maxls,
                      evr_lbfgsb** out);
int evr_lbfgsb_start(evr_lbfgsb* h, const double* x0, double* x);
int evr_lbfgsb_step(evr_lbfgsb* h, double f, const double* g, double* x);
void evr_lbfgsb_stats(const evr_lbfgsb* h, int* nit, int* nfev, double* f, double* pgnorm);
void evr_lbfgsb_destroy(evr_lbfgsb* h);

/* Hit-and-run sampler over {x : A x <= b} (rows x d, row-major), moving in x0 + span(N)
 * (N: d x k, row-major; k = d and N = I without equality constraints).  x0 must be
 * interior.  n_burnin + n * n_thinning steps from x0; every n_thinning-th step after the
 * burn-in is written to out (n x d).  Step i draws its variates 2k + 1 from a counter-based
 * SplitMix64 stream at counters i (2k + 1) + j: k Box-Muller normals (cos branch) for the
 * direction, one uniform for the point on the chord.  Host-only.
 * Replaces [upstream] HitAndRunPolytopeSampler / sample_q_batches_from_polytope, called by
 * optimize_acqf under linear constraints (bofire/strategies/predictives/botorch.py:384-405)
 * and by RandomStrategy (bofire/strategies/random.py:300-326). */
int evr_hit_and_run(int d, int rows, const double* A, const double* b, int k, const double* N,
                    const double* x0, long long n, unsigned long long seed, long long n_burnin,
                    long long n_thinning, double* out);

/* One joint restart problem driven natively on a backward plan: minimise
 * -sum_r acq(x_r) over the b restarts of `plan` in the box [lb, ub] (b*d host arrays each)
 * from x0 (b*d host), with scipy's wrapper rules (stop after maxiter iterations or more
 * than maxfun evaluations).  Each evaluation is one evr_qnehvi_plan_eval_host on `stream`,
 * with no Python in the loop.  Outputs (host): x (b*d,
 * clipped to the box), acq (b) at x, info[4] = {iterations, evaluations, status (0
 * converged, 1 iteration/evaluation limit, 2 abnormal line search), last task}.
 * Returns EVR_ERR_NOTPSD when an evaluation yields NaN (a new-point posterior block not
 * p.d. after the jitter ladder: [upstream] NotPSDError). */
#define EVR_ERR_NOTPSD 7
int evr_qnehvi_plan_minimize(void* stream, evr_qnehvi_plan* plan, const double* x0, const double* lb,
                             const double* ub, int maxiter, int maxfun, double factr, double pgtol, int m,
                             int maxls, double* x, double* acq, int* info);

/* ---- general qNEHVI / qEHVI evaluation (qnehvi_general.hip) ---------------------------
 * q >= 1 joint candidate batches (inclusion-exclusion over the 2^q - 1 subsets of the q
 * points), objectives over selected model outputs (Maximize / Minimize: a*y + b;
 * CloseToTarget: -|y - t|^e) and output constraints c(y) = sign*(y_out - thr) <= 0 weighted
 * by exp(sum logsigmoid(-c/eta)).  Replaces [upstream] qNoisyExpectedHypervolumeImprovement /
 * qExpectedHypervolumeImprovement forward + backward with q = candidate_count
 * (bofire/strategies/predictives/botorch.py:385), objective = get_multiobjective_objective
 * (bofire/utils/torch_tools.py:699-727, callables :384-402) and constraints / eta from
 * get_output_constraints (torch_tools.py:258-381, passed at
 * bofire/strategies/predictives/qnehvi.py:28-48 and mobo.py:50-86).
 * Model side: `stm` (m = model outputs; operator M / R layout as for q = 1, zq unused) and
 * `md`; scan side: `sth` (m = m_obj objectives, the cells, log_hvi = 0).  X: (b*q) x d raw
 * candidates, point i of candidate c at row c*q + i; acq: b; dX (NULL = forward only):
 * (b*q) x d; gout (nullable, b) weights the backward.  The objective / constraint arrays are
 * HOST arrays (copied into the launch); zq (S x q x m_model) is on the device. */
#define EVR_OBJ_AFFINE 0
#define EVR_OBJ_CLOSE_TO_TARGET 1
#define EVR_QNG_MAX_Q 12
typedef struct {
  int q;                    /* points per candidate, 1..8 */
  int m_obj;                /* objectives, 1..8 */
  const int* obj_out;       /* m_obj: model output index */
  const int* obj_kind;      /* m_obj: EVR_OBJ_* */
  const double* obj_p0;     /* m_obj: a (affine) / target (close-to-target) */
  const double* obj_p1;     /* m_obj: b (affine) / exponent (close-to-target) */
  int n_con;                /* output constraints, 0..16 */
  const int* con_out;       /* n_con: model output index */
  const double* con_sign;   /* n_con: c = sign*(y - thr) */
  const double* con_thr;
  const double* con_eta;    /* n_con: sigmoid temperature (BoFire: 1/steepness) */
  const double* zq;         /* device, S x q x m_model: base samples of the q new points */
} evr_qn_general;
long long evr_qng_workspace_doubles(const evr_qnehvi_state* stm, const evr_qnehvi_state* sth,
                                    const evr_qn_general* g, const evr_qnehvi_model* md, int b, int backward);
int evr_qng_eval(void* stream, const evr_qnehvi_state* stm, const evr_qnehvi_state* sth, const evr_qn_general* g,
                 const evr_qnehvi_model* md, int b, const double* X, const double* gout, double* work,
                 double* acq, double* dX);
/* Log-space general evaluation ([upstream] qLogExpectedHypervolumeImprovement._compute_log_qehvi,
 * fat = True; qLogNEHVI / qLogEHVI, MoboStrategy's default, bofire/strategies/predictives/
 * mobo.py:47-90): as evr_qng_eval, with `sth` carrying EXPLICIT cells (cell_lo / cell_hi /
 * cell_off) and tau_relu / tau_max; per cell the q-subset areas are combined in log space
 * (log fatplus improvements, fat-min over the subset's points and with the log cell lengths,
 * log feasibilities summed over the subset, odd minus even sizes by logdiffexp), logsumexp
 * over the cells, logmeanexp over the samples. */
long long evr_qlog_workspace_doubles(const evr_qnehvi_state* stm, const evr_qnehvi_state* sth, const evr_qn_general* g,
                                     const evr_qnehvi_model* md, int b, int backward);
int evr_qlog_eval(void* stream, const evr_qnehvi_state* stm, const evr_qnehvi_state* sth, const evr_qn_general* g,
                  const evr_qnehvi_model* md, int b, const double* X, const double* gout, double* work,
                  double* acq, double* dX);
/* Objectives of baseline / prune samples (Y: m_model x n x S plus mu: m_model x n, nullable)
 * with hard feasibility: O[k][i][s] = g_k(y), or ref[k] where any constraint c > 0
 * ([upstream] prune_inferior_points_multi_objective and the qNEHVI baseline partitions drop
 * infeasible samples).  g->q / g->zq unused. */
int evr_objective_general(void* stream, int m_model, int n, int S, const evr_qn_general* g, const double* Y,
                          const double* mu, const double* ref, double* O);
/* Objective values and smoothed feasibility weights of model-output rows (Y: m_model x n,
 * output-major) through the per-point function the general scan applies to every MC sample:
 * G[k][i] = g_k(y_i) (get_objective_callable, bofire/utils/torch_tools.py:384-402) and
 * W[i] = exp(sum_c logsigmoid(-c(y_i) / eta_c)) ([upstream] compute_smoothed_feasibility_indicator
 * over the constrained_objective2botorch callables, torch_tools.py:258-337; W = 1 without
 * constraints).  g->q / g->zq unused. */
int evr_objective_weights(void* stream, int m_model, int n, const evr_qn_general* g, const double* Y, double* G,
                          double* W);

/* ---- single-objective improvement scan: qNEI / qLogNEI / qLogEI (nei_scan.hip) ----------
 * The step between the joint samples Y of q-point candidates and dY for one output with the
 * affine objective g = a*y + b ([upstream] qNoisyExpectedImprovement, qLogNoisyExpected-
 * Improvement, qLogExpectedImprovement as called from bofire/strategies/predictives/
 * sobo.py:51-90):
 *   plain (log = 0): acq_c = mean_s max_i (g(y_sci) - best_s)_+
 *   log   (log = 1): acq_c = logmeanexp_s fatmax_i(log fatplus(g(y_sci) - best_s; tau_relu); tau_max)
 * Y: S x (b*q), point i of candidate c at column c*q + i.  best: device, S values
 * (best_stride = 1: the per-sample incumbent of qNEI / qLogNEI) or one value (best_stride =
 * 0: the scalar best_f of qLogEI / qEI).  flags (nullable, b ints): acq_c = NaN where set.
 * dY (nullable = forward only): d(sum_c gout_c acq_c)/dY, S x (b*q); gout (nullable, b) = 1.
 * Plain mode uses the subgradients of evr_qei / evr_qng_eval (strict improvement, first
 * arg-max).  Forward and backward are ONE launch; results are bitwise reproducible. */
int evr_nei_scan(void* stream, int q, int log, int S, int b, const double* Y, const double* best,
                 int best_stride, double obj_a, double obj_b, double tau_relu, double tau_max,
                 const int* flags, const double* gout, double* acq, double* dY);
typedef struct {
  int log;              /* 0: qNEI (plain), 1: qLogNEI / qLogEI */
  double tau_relu;      /* log mode: fatplus temperature ([upstream] TAU_RELU = 1e-6) */
  double tau_max;       /* log mode: fatmax temperature ([upstream] logei.TAU_MAX = 1e-2) */
  const double* best;   /* device: incumbent(s) in objective space */
  int best_stride;      /* 1: S per-sample values, 0: one value */
} evr_nei;
/* Full evaluation modelled on evr_qng_eval: kernel matrix -> projection R = M K_x -> q x q
 * Gram / jittered Cholesky / joint samples -> evr_nei_scan -> (dX != NULL) analytic backward.
 * stm: single-output model-side state (m = 1; n, nb, S, no_h, c, ym, ys, kxx; cells unused);
 * g: q (1..EVR_QNG_MAX_Q), ONE affine objective on output 0, no constraints, zq (device,
 * S x q).  X: (b*q) x d raw candidates; acq: b; dX: (b*q) x d. */
long long evr_qnei_workspace_doubles(const evr_qnehvi_state* stm, const evr_qn_general* g,
                                     const evr_qnehvi_model* md, int b, int backward);
int evr_qnei_eval(void* stream, const evr_qnehvi_state* stm, const evr_qn_general* g, const evr_qnehvi_model* md,
                  const evr_nei* nei, int b, const double* X, const double* gout, double* work, double* acq,
                  double* dX);

/* ---- scalarised single-objective scan with output constraints (sobo_scan.hip) -----------
 * The step between the joint samples Y of q-point candidates and dY for a utility over several
 * model outputs, u(y) = sum_t w_t g_t(y[out_t]) (1..EVR_SOBO_MAX_TERMS terms), and 0..16 output
 * constraints c(y) = sign*(y[out] - thr) <= 0 with temperature eta ([upstream]
 * SampleReducingMCAcquisitionFunction._apply_constraints as reached from BoFire's SoboStrategy /
 * AdditiveSoboStrategy, bofire/strategies/predictives/sobo.py:42-222: the feasibility weighs
 * every (sample, point) BEFORE the reduction over the q points):
 *   plain (log = 0): acq_c = mean_s max_i [ (u_sci - best_s)_+ * exp(sum_c logsigmoid(-c/eta)) ]
 *   log   (log = 1): acq_c = logmeanexp_s fatmax_i [ log fatplus(u_sci - best_s; tau_relu)
 *                                                    + sum_c log_fatmoid(-c/eta) ; tau_max ]
 * Term kinds: EVR_OBJ_AFFINE (p0*y + p1), EVR_OBJ_CLOSE_TO_TARGET (-|y - p0|^p1),
 * EVR_OBJ_SIGMOID (1/(1+exp(-p0*(y-p1))); p0 = +steepness for MaximizeSigmoid, -steepness for
 * MinimizeSigmoid) and EVR_OBJ_TARGET (sig(p0*(y-(p1-p2))) * (1 - sig(p0*(y-(p1+p2)))); p0 =
 * steepness, p1 = target, p2 = tolerance) — the callables of bofire/utils/torch_tools.py:403-450.
 * Y / dY: S x m_model x (b*q), Y[s][j][c*q + i] (the layout of the joint samples of
 * evr_qng_eval).  flags (nullable, m_model x b ints): acq_c = NaN where any output's flag is
 * set.  best / best_stride, gout and the plain-mode subgradients (strict improvement, first
 * arg-max of the weighted value) are as in evr_nei_scan.  dY (nullable = forward only) is
 * written in full: outputs no term or constraint reads get zeros.  The term / constraint arrays
 * are HOST arrays (copied into the launch); best is on the device.  Forward and backward are
 * ONE launch; results are bitwise reproducible. */
#define EVR_OBJ_SIGMOID 2
#define EVR_OBJ_TARGET 3
#define EVR_SOBO_MAX_TERMS 8
typedef struct {
  int log;                  /* 0: plain (qNEI / qEI), 1: log (qLogNEI / qLogEI) */
  double tau_relu;          /* log mode: fatplus temperature */
  double tau_max;           /* log mode: fatmax temperature */
  const double* best;       /* device: incumbent(s) in utility space */
  int best_stride;          /* 1: S per-sample values, 0: one value */
  int n_term;               /* 1..EVR_SOBO_MAX_TERMS */
  const int* term_out;      /* n_term: model output index */
  const int* term_kind;     /* n_term: EVR_OBJ_* */
  const double* term_w;     /* n_term: weight in the sum */
  const double* term_p0;
  const double* term_p1;
  const double* term_p2;    /* n_term: read by EVR_OBJ_TARGET only */
  int n_con;                /* 0..16 */
  const int* con_out;
  const double* con_sign;
  const double* con_thr;
  const double* con_eta;
} evr_sobo;
int evr_sobo_scan(void* stream, int q, int m_model, int S, int b, const evr_sobo* sb, const double* Y,
                  const int* flags, const double* gout, double* acq, double* dY);
/* Full evaluation modelled on evr_qng_eval with the scan above in place of subsets / HVI /
 * combine: kernel matrix over the m model outputs -> projection -> q x q Gram / jittered
 * Cholesky / joint samples per (candidate, output) -> evr_sobo_scan -> (dX != NULL) analytic
 * backward.  stm: model-side state (m = model outputs 1..8; cells unused); g: q and zq (device,
 * S x q x m) only — its objective / constraint fields are not read.  X: (b*q) x d raw
 * candidates; acq: b; dX: (b*q) x d. */
long long evr_qsobo_workspace_doubles(const evr_qnehvi_state* stm, const evr_qn_general* g,
                                      const evr_qnehvi_model* md, int b, int backward);
int evr_qsobo_eval(void* stream, const evr_qnehvi_state* stm, const evr_qn_general* g, const evr_qnehvi_model* md,
                   const evr_sobo* sb, int b, const double* X, const double* gout, double* work, double* acq,
                   double* dX);

/* ---- augmented Chebyshev scalarisation scan with output constraints (parego_scan.hip) ------
 * The step between the joint samples Y of q-point candidates and dY for the qParEGO utility
 * over several model outputs (2..EVR_SOBO_MAX_TERMS terms),
 *   t_k(y) = A_k * g_k(y[out_k]) + B_k,   u(y) = min_k t_k(y) + alpha * sum_k t_k(y),
 * ([upstream] get_chebyshev_scalarization as reached from BoFire's QparegoStrategy,
 * bofire/strategies/predictives/qparego.py:30-140; weights, normalisation bounds and signs are
 * folded into A_k > 0 and B_k by the caller) and 0..16 output constraints as in evr_sobo_scan.
 * The reductions over the q points and the samples, Y / dY, flags, best / best_stride, gout and
 * the plain-mode subgradients are exactly those of evr_sobo_scan.  Term kinds: EVR_OBJ_AFFINE
 * (p0*y + p1) and EVR_OBJ_CLOSE_TO_TARGET (-|y - p0|^p1) only.  Backward: the slope of u with
 * respect to t_k is alpha + [k == k*], k* the FIRST arg-min (lowest term index on ties); dY is
 * written in full, outputs nothing reads get exact zeros.  The term / constraint arrays are HOST
 * arrays (copied into the launch); best is on the device.  Refused: n_term < 2, any other term
 * kind, A_k <= 0, alpha < 0, eta <= 0, an output index outside the model.  Forward and backward
 * are ONE launch; no atomics; results are bitwise reproducible. */
typedef struct {
  int log;                  /* 0: plain (qNEI / qEI), 1: log (qLogNEI / qLogEI) */
  double tau_relu;          /* log mode: fatplus temperature */
  double tau_max;           /* log mode: fatmax temperature */
  const double* best;       /* device: incumbent(s) in utility space */
  int best_stride;          /* 1: S per-sample values, 0: one value */
  double alpha;             /* augmentation weight (>= 0; [upstream] 0.05) */
  int n_term;               /* 2..EVR_SOBO_MAX_TERMS */
  const int* term_out;      /* n_term: model output index */
  const int* term_kind;     /* n_term: EVR_OBJ_AFFINE or EVR_OBJ_CLOSE_TO_TARGET */
  const double* term_p0;
  const double* term_p1;
  const double* term_a;     /* n_term: scale A_k > 0 */
  const double* term_b;     /* n_term: shift B_k */
  int n_con;                /* 0..16 */
  const int* con_out;
  const double* con_sign;
  const double* con_thr;
  const double* con_eta;
} evr_parego;
int evr_parego_scan(void* stream, int q, int m_model, int S, int b, const evr_parego* pg, const double* Y,
                    const int* flags, const double* gout, double* acq, double* dY);
/* Full evaluation: evr_qsobo_eval's chain (same stm / g / md / X / work / acq / dX semantics)
 * with evr_parego_scan in place of evr_sobo_scan. */
long long evr_qparego_workspace_doubles(const evr_qnehvi_state* stm, const evr_qn_general* g,
                                        const evr_qnehvi_model* md, int b, int backward);
int evr_qparego_eval(void* stream, const evr_qnehvi_state* stm, const evr_qn_general* g, const evr_qnehvi_model* md,
                     const evr_parego* pg, int b, const double* X, const double* gout, double* work, double* acq,
                     double* dX);

/* ---- reward scans qSR / qUCB / qPI with output constraints (reward_scan.hip) ---------------
 * The step between the joint samples Y of q-point candidates and dY for the three
 * single-objective acquisitions that are not an improvement over a per-sample incumbent, over
 * the utility u(y) = sum_t w_t g_t(y[out_t]) and the constraints of evr_sobo_scan (same term
 * kinds, same tables).  W = exp(sum_c logsigmoid(-c/eta)) (plain sigmoid; 1 without constraints).
 * Restated from memory of BoTorch (parity-unpinned):
 *   reward ([upstream] ConstrainedMCObjective / apply_constraints, as bofire/strategies/
 *   predictives/sobo.py:130-145, 192-205 builds it): r = (u + M) W - M with constraints, r = u
 *   without; M = infeasible_cost >= 0.
 *   EVR_REWARD_SR  ([upstream] qSimpleRegret):         acq_c = mean_s max_i r_sci
 *   EVR_REWARD_UCB ([upstream] qUpperConfidenceBound): acq_c = mean_s max_i (rbar_ci + k |r_sci - rbar_ci|),
 *                  rbar_ci = mean_s r_sci, k = ucb_scale = sqrt(beta pi / 2)
 *   EVR_REWARD_PI  ([upstream] qProbabilityOfImprovement, constraints applied to the non-negative
 *                  acquisition): acq_c = mean_s max_i [ sigmoid((u_sci - best[0]) / tau) W_sci ]
 * All maxima take the first arg-max; sgn(0) = 0 in qUCB's adjoint (at S = 1 every difference is
 * exactly zero).  Y / dY, flags, gout as in evr_sobo_scan; dY (nullable = forward only) is
 * written in full with exact zeros for outputs nothing reads.  The term / constraint arrays are
 * HOST arrays; best is on the device (one double, read in PI mode only).  Refused: what
 * evr_sobo_scan refuses, an unknown mode, a negative or non-finite ucb_scale (UCB), tau <= 0
 * (PI), infeasible_cost < 0 (SR / UCB).  Forward and backward are ONE launch each (qUCB walks Y
 * two / three times inside it); no atomics; results are bitwise reproducible. */
#define EVR_REWARD_SR 0
#define EVR_REWARD_UCB 1
#define EVR_REWARD_PI 2
typedef struct {
  int mode;                 /* EVR_REWARD_* */
  double ucb_scale;         /* UCB: k = sqrt(beta pi / 2) >= 0 */
  double tau;               /* PI: temperature > 0 */
  const double* best;       /* device: one double, the incumbent in utility space (PI only) */
  double infeasible_cost;   /* SR / UCB: M >= 0, read when n_con > 0 */
  int n_term;               /* 1..EVR_SOBO_MAX_TERMS */
  const int* term_out;
  const int* term_kind;
  const double* term_w;
  const double* term_p0;
  const double* term_p1;
  const double* term_p2;
  int n_con;                /* 0..16 */
  const int* con_out;
  const double* con_sign;
  const double* con_thr;
  const double* con_eta;
} evr_reward;
int evr_reward_scan(void* stream, int q, int m_model, int S, int b, const evr_reward* rw, const double* Y,
                    const int* flags, const double* gout, double* acq, double* dY);
/* Full evaluation: evr_qsobo_eval's chain (same stm / g / md / X / work / acq / dX semantics)
 * with evr_reward_scan in place of evr_sobo_scan. */
long long evr_qreward_workspace_doubles(const evr_qnehvi_state* stm, const evr_qn_general* g,
                                        const evr_qnehvi_model* md, int b, int backward);
int evr_qreward_eval(void* stream, const evr_qnehvi_state* stm, const evr_qn_general* g, const evr_qnehvi_model* md,
                     const evr_reward* rw, int b, const double* X, const double* gout, double* work, double* acq,
                     double* dX);

/* ---- multiplicative / multiplicative-additive utility scan (mult_scan.hip) ------------------
 * The step between the joint samples Y of q-point candidates and dY for the utility
 *   u(y) = [ prod_{k factor} g_k(y[out_k]) ** w_k ] * [ 1 + sum_{a addend} w_a * g_a(y[out_a]) ]
 * of BoFire's MultiplicativeSoboStrategy (no addends) and MultiplicativeAdditiveSoboStrategy
 * (bofire/utils/torch_tools.py:662-675, 730-806; bofire/strategies/predictives/sobo.py:225-284),
 * without output constraints.  ** is C pow: a negative base is real with an integer-valued
 * exponent and NaN with any other.  Term kinds and their p0 / p1 / p2: the four EVR_OBJ_* of
 * evr_sobo.  The reductions over the q points and the samples are evr_sobo_scan's at n_con = 0;
 * Y / dY, flags, best / best_stride, gout and the plain-mode subgradients are evr_sobo_scan's.
 * Backward: d u / d g_k = w_k pow(g_k, w_k - 1) * prod_{s != k} g_s ** w_s * A, d u / d g_a =
 * w_a * P (A the bracket, P the product); the product of the others is formed from the others,
 * never by division, so an exactly zero factor keeps the slope of the rest.  dY is written in
 * full, outputs nothing reads get exact zeros.  A candidate with a NaN utility in any (sample,
 * point) gets acq = NaN (its dY columns are unspecified); the others are unaffected.  The table
 * arrays are HOST arrays (copied into the launch); best is on the device.  Refused: table sizes
 * outside the limits, an output index outside the model, an unknown kind, a weight that is not
 * finite or (factor) below 1, tau <= 0 in log mode, best_stride not 0 or 1.  Forward and backward
 * are ONE launch; no atomics; results are bitwise reproducible, and the forward-only launch gives
 * the bits of the backward one. */
typedef struct {
  int log;                  /* 0: plain (qNEI / qEI), 1: log (qLogNEI / qLogEI) */
  double tau_relu;          /* log mode: fatplus temperature */
  double tau_max;           /* log mode: fatmax temperature */
  const double* best;       /* device: incumbent(s) in utility space */
  int best_stride;          /* 1: S per-sample values, 0: one value */
  int n_fac;                /* >= 0; 1 <= n_fac + n_add <= EVR_SOBO_MAX_TERMS */
  const int* fac_out;       /* n_fac: model output index */
  const int* fac_kind;      /* n_fac: EVR_OBJ_* */
  const double* fac_w;      /* n_fac: exponent, finite and >= 1 */
  const double* fac_p0;
  const double* fac_p1;
  const double* fac_p2;     /* read by EVR_OBJ_TARGET only */
  int n_add;                /* >= 0 */
  const int* add_out;
  const int* add_kind;
  const double* add_w;      /* n_add: weight in the bracket, finite */
  const double* add_p0;
  const double* add_p1;
  const double* add_p2;
} evr_mult;
int evr_mult_scan(void* stream, int q, int m_model, int S, int b, const evr_mult* mt, const double* Y,
                  const int* flags, const double* gout, double* acq, double* dY);
/* Full evaluation: evr_qsobo_eval's chain (same stm / g / md / X / work / acq / dX semantics)
 * with evr_mult_scan in place of evr_sobo_scan. */
long long evr_qmult_workspace_doubles(const evr_qnehvi_state* stm, const evr_qn_general* g,
                                      const evr_qnehvi_model* md, int b, int backward);
int evr_qmult_eval(void* stream, const evr_qnehvi_state* stm, const evr_qn_general* g, const evr_qnehvi_model* md,
                   const evr_mult* mt, int b, const double* X, const double* gout, double* work, double* acq,
                   double* dX);

/* ---- negative integrated posterior variance (ActiveLearningStrategy) --------------------
 * The per-candidate step of [upstream] qNegIntegratedPosteriorVariance as built by
 * bofire/strategies/predictives/active_learning.py:16-66 (restated from memory, parity-unpinned).
 * Per output j < B and candidate c < b of q joint points (point i at column c*q + i):
 *   G = C^T C,  A = k_j(X_c, X_c) - Vx^T Vx + noise_j I,
 *   acq[c] = - sum_j coef_j (v0_j - tr(A^-1 G) / N).
 * C: B x N x (b*q) posterior cross-covariances to the N integration points; Vx: B x ldv x (b*q),
 * rows 0..n-1 of each output used (ldv >= n: rows 0..n-1 of R = M K_x pass with ldv = n + 1);
 * X: b x q x d raw candidates with lo / inv_range (d), ls (B x d) and the kind code for the self
 * block; noise, coef, v0: B.  flags[c] != 0: a pivot of some output's q x q Cholesky was <= 0.
 * Backward (dC, dVx, dXself all non-NULL, or all NULL): dC like C, dVx B x n x (b*q), dXself
 * b x q x d (the slope through k_j(X_c, X_c), outputs summed in order), each weighted by gout
 * (nullable, b).  No atomics; b = 0 returns 0 without a launch. */
int evr_nipv_reduce(void* stream, int q, int B, int n, int N, int b, int d, int kind, const double* C,
                    const double* Vx, int ldv, const double* X, const double* lo, const double* inv_range,
                    const double* ls, const double* noise, const double* coef, const double* v0,
                    const double* gout, double* acq, int* flags, double* dC, double* dVx, double* dXself);

/* The PyTorch-ROCm operators torch.ops.everest_amd.qnehvi_*(everest_amd/csrc/torch_ops.cpp)
 * take a torch.classes.everest_amd.QnehviAcq: it copies the evr_qnehvi_state /
 * evr_qnehvi_model / evr_qn_general structs, holds references to the device tensors they
 * point into, and caches one plan per batch size (no raw addresses cross the boundary). */

/* ---- qEI (q = 1, single output) -----------------------------------------------------
 * R = [Linv; alpha^T] K(Xtr, x) ((n+1) x b).  acq[c] = mean_s (a*(mu + sd*z_s) + b - best_f)_+
 * with sd from psd_safe_cholesky (3 tries) of the posterior variance; gR (nullable) =
 * d acq / d R for the analytic backward; flags[c] = 1 if the jitter ladder failed.
 * Replaces [upstream] qExpectedImprovement (bofire/strategies/predictives/sobo.py:51-90). */
int evr_qei(void* stream, int n, int b, int S, const double* R, double c, double ym, double ys,
            double kxx, const double* z, double obj_a, double obj_b, double best_f, double* acq,
            double* gR, int* flags);

/* ---- Pareto / pruning ---------------------------------------------------------------
 * O: m x n x S (objective samples, layout [j][i][s]).  For every sample s and point i:
 * nd = not dominated (maximisation) & (O > ref all) [& first of duplicates if dedup].
 * mask (S x n bytes, may be NULL); counts (n ints, may be NULL) += nd.
 * Replaces prune_inferior_points_multi_objective (qnehvi.py:44) and the per-sample
 * Pareto filter of _pad_batch_pareto_frontier. */
int evr_pareto_mask(void* stream, int S, int n, int m, const double* O, const double* ref,
                    int dedup, unsigned char* mask, int* counts);

/* Elementwise objective on a sample tensor: O[j][i][s] = a_j*(Y[j][i][s] + mu[j][i]) + b_j */
int evr_objective_affine(void* stream, int m, int n, int S, const double* Y, const double* mu,
                         const double* a, const double* b, double* O);
/* X[b][e] *= alpha[b] for e < per (per-output variance scaling s_y^2 of covariances) */
int evr_scale_batched(void* stream, int B, long long per, const double* alpha, double* X);
/* E[b][r][idx[r]] += val[b] (adds the baseline row selection P to E, nb x n per output) */
int evr_add_selection(void* stream, int B, int nb, int n, const int* idx, const double* val, double* E);

/* ---- host box decomposition ----------------------------------------------------------
 * Exact partition of the non-dominated region above ref into disjoint boxes, per MC sample
 * (FastNondominatedPartitioning, alpha = 0, qnehvi.py:50; Lacour et al. 2017 local upper
 * bounds).  Host memory.  obj: element (s, i, j) at obj[s*ss + i*si + j*sj]; mask (S x n,
 * nullable) selects the candidate points (Pareto filter is re-applied on the host). */
typedef struct evr_cells evr_cells;
int evr_box_decompose(int S, int n, int m, const double* obj, long long ss, long long si,
                      long long sj, const unsigned char* mask, const double* ref, int num_threads,
                      evr_cells** out);
/* alpha > 0 (finite) with m > 2: the approximate partition of [upstream] BoTorch
 * NondominatedPartitioning(alpha) (bofire/strategies/predictives/qnehvi.py:50 passes the data
 * model's alpha, bofire/data_models/strategies/predictives/qnehvi.py:19); alpha = 0 or m <= 2
 * is the exact partition above. */
int evr_box_decompose_approx(int S, int n, int m, const double* obj, long long ss, long long si,
                             long long sj, const unsigned char* mask, const double* ref, double alpha,
                             int num_threads, evr_cells** out);
long long evr_cells_total(const evr_cells* c);
int evr_cells_copy(const evr_cells* c, double* lo, double* hi, int* off);
void evr_cells_free(evr_cells* c);

/* ---- device box decomposition (same partition as evr_box_decompose) --------------------
 * One workgroup per sample; obj is m x n x S on the device (objective values, maximisation),
 * ref (m) on the device.  Every LUB is a 64-bit key of defining-point indices, cap keys per
 * sample (power of two).  status[s] = 1 if sample s overflowed cap (retry with a larger
 * cap).  counts[s] = number of non-empty cells.  evr_box_pack_keys_device then packs the
 * sorted keys at off[s] (cells ordered by first lower bound) with the per-sample point tables
 * pts (S x (n+m) x m) and rank0 (S x (n+m)) -> evr_qnehvi_state.cell_keys / cell_pts /
 * cell_rank0, pts_stride n+m.  evr_cells_from_keys expands them into explicit lo / hi rows.
 * evr_box_device_limits returns 0 if (n, m) fits the kernel (LDS, key width), else 3. */
int evr_box_device_limits(int n, int m, int* max_points, long long* lds_bytes);
long long evr_box_device_workspace_bytes(int S, int n, int m, int cap);
int evr_box_decompose_device(void* stream, int S, int n, int m, const double* obj, const double* ref,
                             int cap, void* work, int* counts, int* status);
int evr_box_pack_keys_device(void* stream, int S, int n, int m, int cap, const void* work,
                             const int* off, int max_cells, unsigned long long* keys, double* pts,
                             int* rank0);
int evr_cells_from_keys(void* stream, int S, int m, int stride, const int* off, int max_cells,
                        const unsigned long long* keys, const double* pts, const int* rank0,
                        double* lo, double* hi);

/* ---- kd ordering of compressed cells for the sparse HVI scan -------------------------
 * Per sample (one workgroup each): rank tables of the point rows per objective, a kd split
 * order of the cells (median split on the objective of largest rank spread, leaves of 16),
 * then per group of 16 cells: the keys (okeys, goff[S]*16), the cells' lower-bound ranks
 * (ork, goff[S] x m x 16 u16, 0x7FFF padding), the group's minimum rank per objective (ogb,
 * goff[S] x 8 u16) and per sample the ascending lower-bound values (osv, S x m x stride).
 * goff[s] = sum_{s'<s} ceil(counts[s'] / 16).  evr_cells_kd_limits returns 0 if max_cells /
 * stride fit the kernel (LDS sort buffer), else 3 (the tiled scan is used then).
 * Replaces nothing in the reference: an MI355X-side index over the [upstream]
 * FastNondominatedPartitioning cells (bofire/strategies/predictives/qnehvi.py:50). */
/* evr_box_decompose_device + evr_box_pack_keys_device + evr_cells_kd_order_device in one host
 * call with one synchronisation (the per-sample counts): outputs sized by the caller for the
 * capacity (keys S*cap; okeys 16*G, ork 16*m*G, ogb 8*G with G = S*cap/16 + S; off / goff S+1);
 * info[0] = 1: a sample overflowed cap (rerun with a larger cap), info[1] = 1: kd order built,
 * info[2] = largest per-sample count; counts_host[s] = cells of sample s.  Replaces the
 * reference's host-side partition + cell list (bofire/strategies/predictives/qnehvi.py:39-52
 * -> [upstream] FastNondominatedPartitioning) for the sparse scan in one step. */
int evr_box_kd_pipeline(void* stream, int S, int n, int m, const double* obj, const double* ref, int cap,
                        void* work, int* counts_dev, int* status_dev, int* off_dev, int* goff_dev,
                        unsigned long long* keys, double* pts, int* rank0, int want_kd, unsigned long long* okeys,
                        unsigned short* ork, unsigned short* ogb, double* osv, int* counts_host, int* info);
int evr_cells_kd_limits(int stride, int m, int max_cells, long long* lds_bytes);
int evr_cells_kd_order_device(void* stream, int S, int m, int stride, const int* off, const int* goff,
                              int max_cells, const unsigned long long* keys, const double* pts,
                              const int* rank0, unsigned long long* okeys, unsigned short* ork,
                              unsigned short* ogb, double* osv);

/* ---- quasi-MC base samples -------------------------------------------------------------
 * Replaces [upstream] draw_sobol_normal_samples / torch.quasirandom.SobolEngine(scramble=True)
 * as called by the qNEHVI samplers (bofire/strategies/predictives/qnehvi.py:39-52, seed from
 * the strategy RNG bofire/strategies/predictives/botorch.py:86).
 * evr_sobol_scramble (host): V (dim x 30 int64, in/out) holds the unscrambled direction
 * numbers and receives SobolEngine(dim, scramble=True, seed).sobolstate; shift (dim) receives
 * .shift.  evr_sobol_normal (device): normal samples of points 0..n-1, dims [d0, d0+nd):
 * layout 0 -> out[k*nd + t]; layout 1 -> out[(o*np + p)*n + k] with t = p*m + o, np = nd/m. */
int evr_sobol_scramble(int dim, unsigned long long seed, long long* V, long long* shift);
/* The same for dimensions [d0, d0 + nd) of the dim-dimensional engine only: V (nd x 30) and
 * shift (nd) hold those dimensions (the stream is still drawn through dimension d0 + nd - 1;
 * the per-dimension work is skipped for the others). */
int evr_sobol_scramble_range(int dim, unsigned long long seed, int d0, int nd, long long* V, long long* shift);
/* The same in two steps: generate a seed's raw stream once (evr_sobol_stream_words(dim)
 * words cover every draw of up to dim dimensions; the draws of one seed at different
 * dimension counts are prefixes of the same stream), then scramble dimension ranges of any
 * dim it covers.  Lets the host start the stream before the dimension count is known. */
typedef struct evr_sobol_stream evr_sobol_stream;
long long evr_sobol_stream_words(int dim);
int evr_sobol_stream_create(unsigned long long seed, long long nwords, evr_sobol_stream** out);
int evr_sobol_scramble_stream(const evr_sobol_stream* st, int dim, int d0, int nd, long long* V, long long* shift);
void evr_sobol_stream_destroy(evr_sobol_stream* st);
int evr_sobol_normal(void* stream, int n, int nd, int d0, const long long* V, const long long* shift,
                     int layout, int m, double* out);

#ifdef __cplusplus
}
#endif
#endif /* EVEREST_AMD_H */
