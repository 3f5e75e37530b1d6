/* C ABI of the MI355X-native GP-MPC solve path (gfx950).
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point names the
 * reference interface it replaces (file:line in amacati/gp-mpc).  All device pointers are
 * plain HIP device allocations (e.g. torch tensors' data_ptr()); host pointers are noted.
 * Calls are asynchronous on the given stream (NULL = default stream) unless noted.
 * No C++ exceptions cross this boundary; every call returns a gpmpc_status and
 * gpmpc_last_error() describes the last failure of the calling thread.
 *
 * Threading: one handle per GPU/process, driven by one host thread at a time
 * (the reference drives one acados solver from one Python thread, gpmpc/gpmpc.py:105-107).
 * Streams: every call queues its work on its stream argument.  The handle's device state is
 * shared by all of them, so each call that takes the handle and a stream ends by recording a
 * handle-owned event on its stream, and a call on a different stream first makes its stream wait
 * for that event (hipStreamWaitEvent: no host synchronisation, and the previous stream may already
 * be gone).  Consecutive calls on one handle therefore run in the order they were made, whatever
 * their streams: a reader (gpmpc_gp_predict, gpmpc_gp_mean_grad, the gpmpc_get_* copies) sees what
 * the calls before it wrote, and an update queued after it waits until it has read.  gpmpc_plant_step,
 * which closes every step of a control loop, defers its record until a call arrives on another stream
 * (on one stream the record would only cost a dispatch gap): its stream must still exist then.  Two calls stand
 * outside the rule because they touch nothing of the handle on the device: gpmpc_gp_posterior takes
 * no handle, and gpmpc_preprocess carries its model parameters by value; their buffers are the
 * caller's to order.  (tests/stream_order_util.py lists every stream-taking call under one of the two.)
 * gpmpc_gp_inducing takes no stream: it is a synchronous builder in the class of gpmpc_gp_reserve, with no
 * device input of the caller's, and it keeps the rule on a stream the handle owns, which waits for the
 * handle's event first and carries the record when the call returns, its work completed.
 * gpmpc_rollout takes no stream either and keeps the rule the same way: its launches run on that stream of the
 * handle's, behind the handle's last call whatever stream that was on, and the stream is drained before the call
 * returns.  Unlike gpmpc_gp_inducing it has device inputs of the caller's, and they are the caller's to order:
 * x0_dev and u_dev must be complete when the call is made; the outputs are complete when it returns.
 * gpmpc_rollout_lin follows the same rule as gpmpc_rollout in every respect (cov0_dev is one more input of the caller's).
 * gpmpc_rollout_sample does too: xref_dev and xi_dev are further inputs of the caller's, complete when the call is
 * made, and K is read on the host before the call returns.
 * The library reads no environment variables: every option is an explicit call.
 */
#ifndef GPMPC_MI355X_H
#define GPMPC_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpmpc_handle gpmpc_handle;

typedef enum {
    GPMPC_OK = 0,
    GPMPC_ERR_ARG = -1,     /* invalid argument / shape */
    GPMPC_ERR_HIP = -2,     /* HIP runtime error (message in gpmpc_last_error) */
    GPMPC_ERR_STATE = -3,   /* call out of order (e.g. solve before set_model) */
    GPMPC_ERR_NOMEM = -4
} gpmpc_status;

/* Model ids (gpmpc/models.py MODEL_*). */
enum { GPMPC_MODEL_QUAD2D = 0, GPMPC_MODEL_QUAD3D = 1, GPMPC_MODEL_CARTPOLE = 2 };

/* Per-instance solver status codes, identical to acados (asserted in {0,2} at
 * gpmpc/gpmpc.py:365 and gpmpc/mpc.py:185).  An obs outside the stage-0 state box
 * (gpmpc/gpmpc.py:288,296,309-310; gpmpc/mpc.py:141,145,157-158) by more than the inequality
 * tolerance makes the QP infeasible: GPMPC_QP_FAILURE, as acados reports it.  After a failed
 * solve (NAN or QP_FAILURE) the instance keeps its previous iterate, its multipliers restart
 * from zero and its next solve runs untightened (no poisoning of later steps).
 * GPMPC_NAN: a non-finite value (NaN or Inf) in anything the NLP residuals read -- the stored
 * iterate, the dynamics at it, the multipliers, the tightened bounds -- at the iteration that
 * meets it, or a non-finite iterate after a full step.  A non-finite STORED iterate (a
 * gpmpc_set_iterate from a gpmpc_rollout that returned NaN, say) therefore ends the solve at
 * iteration 0 with GPMPC_NAN whatever the other terms are.  The iterate is kept like any failed
 * solve's, which here means it stays non-finite -- and every later solve of the instance ends the
 * same way -- until gpmpc_set_iterate or gpmpc_reset(reset_iterate = 1) replaces it, and u0 is
 * the kept iterate's first input (NaN when that is where the NaN sits). */
enum { GPMPC_SUCCESS = 0, GPMPC_NAN = 1, GPMPC_MAXITER = 2, GPMPC_MINSTEP = 3, GPMPC_QP_FAILURE = 4 };

/* Create a solver for `max_batch` independent instances of model `model_id` with horizon
 * `horizon` on HIP device `device`.
 * Replaces: AcadosOcpSolver(ocp, json) construction at gpmpc/gpmpc.py:105-107 and
 * gpmpc/mpc.py:58 (code generation + compile there; nothing to compile here). */
gpmpc_status gpmpc_create(int32_t model_id, int32_t horizon, int32_t max_batch, int32_t device, gpmpc_handle** out);
void gpmpc_destroy(gpmpc_handle* h);
const char* gpmpc_last_error(void);

/* OCP definition (host arrays, float64).
 * Replaces: setup_acados_model / setup_acados_optimizer / setup_acados_constraints,
 * gpmpc/gpmpc.py:166-320 (and gpmpc/mpc.py:65-163).
 *   params      prior parameters in the model's order (gpmpc/models.py param_vector)
 *   x_lo..u_hi  box bounds (gpmpc/gpmpc.py:242-246)
 *   q_diag, r_diag  LINEAR_LS weights W = blkdiag(Q,R), W_e = Q (gpmpc/gpmpc.py:233-234)
 *   u_eq        input reference (ref_action, gpmpc/gpmpc.py:54)
 *   uh          upper bound of h = A[x;u] - b - t: -1e-8 GPMPC (gpmpc.py:309-314), +1e-8 MPC
 *   cost_scaling 1: stage costs scaled by dt, terminal by 1 (acados time-step scaling) */
gpmpc_status gpmpc_set_model(gpmpc_handle* h, const double* params, int32_t n_params, double dt,
                             const double* x_lo, const double* x_hi, const double* u_lo, const double* u_hi,
                             const double* q_diag, const double* r_diag, const double* u_eq, double uh,
                             int32_t cost_scaling);

/* Periodic reference trajectory (host, shape (nx, L) row-major like the reference's
 * traj array).  Replaces: GPMPC.reference_trajectory, gpmpc/gpmpc.py:509-514. */
gpmpc_status gpmpc_set_reference(gpmpc_handle* h, const double* traj_nx_by_L, int32_t L);

/* SQP / QP options.  Reference: nlp_solver_max_iter = 25 (gpmpc/gpmpc.py:262); acados
 * default NLP tolerances 1e-6.  The QP options belong to the batched IPM: qp_max_iter 50
 * (acados qp_solver_iter_max), qp_tol 1e-6 by default -- the OCP leaves the QP tolerances unset,
 * and acados' SQP then passes its NLP tolerances on to the QP solver. */
gpmpc_status gpmpc_set_options(gpmpc_handle* h, int32_t max_iter, double tol_stat, double tol_eq,
                               double tol_ineq, double tol_comp, int32_t qp_max_iter, double qp_tol, double qp_mu0);

/* Load GP `gp_id` (host arrays).
 *   Mean:      inputs X [n][d] (d <= 3) and weights alpha [n]: m(z) = sf2 sum_i alpha_i e(z, X_i).
 *              Exact GP: alpha = K^-1 y (gpytorch_predict2casadi, gpmpc/gp.py:72-85).
 *              FITC: X = inducing inputs, alpha = posterior weights (gpmpc/gpmpc.py:175-187,377-400).
 *   Variance:  training inputs Xv [nv][d] (NULL -> Xv = X, nv = n) and Linv = inverse Cholesky
 *              factor of K(Xv,Xv) + noise I [nv][nv] (row-major lower; NULL -> no variance).
 *              The reference takes the variance from the exact GP even in FITC mode
 *              (gpmpc/gpmpc.py:441-445).
 *   lengthscale (isotropic), outputscale, noise: ScaleKernel(RBFKernel()) + Gaussian likelihood. */
gpmpc_status gpmpc_set_gp(gpmpc_handle* h, int32_t gp_id, int32_t n, int32_t d, const double* X,
                          const double* alpha, int32_t nv, const double* Xv, const double* Linv,
                          double lengthscale, double outputscale, double noise);

/* LOVE variance for the constraint tightening (replaces GaussianProcess predictive variance
 * under gpytorch.settings.fast_pred_var, gpmpc/gpmpc.py:442-444): R [n][r] row-major with
 * R R^T ~ (K(Xv,Xv) + noise I)^-1 (a rank-r Lanczos root, gpmpc/gp.py love_root); the tightening
 * variance becomes outputscale - ||R^T k(z, Xv)||^2 + noise.  n must equal the GP's nv,
 * 1 <= r <= 256.  R = NULL restores the exact variance; gpmpc_set_gp clears the root.
 * gpmpc_gp_predict / gpmpc_gp_posterior stay exact. */
gpmpc_status gpmpc_set_gp_variance_root(gpmpc_handle* h, int32_t gp_id, int32_t n, int32_t r, const double* R);

/* Appending training rows on the device (no refactorisation, no host round trip): for an exact GP
 * uploaded with Linv, a block of m <= 16 new rows is one bordered Cholesky update of (L^-1)^T and
 * alpha = K^-1 y (csrc/gp_append.hip), with the hyperparameters unchanged.  The MFMA tile pack of
 * the mean rows (tW lane order as gpmpc_set_gp builds it: for row i = 16t + r, lane group r % 4,
 * register r / 4, columns [alpha, alpha (x - xbar)]) is rewritten for every row, centred on the
 * xbar gpmpc_set_gp computed: the centring is algebraically exact for any xbar and only conditions
 * the exponent, so xbar is not moved.
 *
 * Make room for up to `capacity` training rows of GP gp_id (after gpmpc_set_gp; contents kept;
 * synchronous setup call).  gpmpc_set_gp resets the capacity to the uploaded size. */
gpmpc_status gpmpc_gp_reserve(gpmpc_handle* h, int32_t gp_id, int32_t capacity);

/* Append m >= 1 training rows (device: Xnew [m][d], ynew [m]) to GP gp_id on `stream`: blocks of
 * up to 16 rows, each one bordered-Cholesky update; no host synchronisation.
 * accepted_dev: device int32 [ceil(m/16)], 1 / 0 per block, may be NULL.  A block with a
 * non-finite input or target, or whose Schur complement has a pivot that is not finite and
 * positive, is written as inert rows (zero input, zero weight, zero factor row and column, like
 * padding: they add nothing to any mean or variance, now or after later appends) and reports 0;
 * the old weights are left alone and the row count advances either way.
 * Refused, with the GP unchanged: n + m above the capacity (GPMPC_ERR_ARG); GP not set, set
 * without Linv, a FITC upload (Xv != X), or a LOVE root installed -- it belongs to the old
 * training set, drop it first with gpmpc_set_gp_variance_root(R = NULL), or rebuild it afterwards with
 * gpmpc_gp_love_root (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_append(gpmpc_handle* h, int32_t gp_id, int32_t m, const double* Xnew_dev,
                             const double* ynew_dev, int32_t* accepted_dev, void* stream);

/* Remove the m oldest training rows (rows 0 .. m-1; row j + m becomes row j) of GP gp_id on
 * `stream`, the counterpart of gpmpc_gp_append for a bounded, moving training set (the reference
 * only ever grows its data set, stacking each epoch's samples onto it before a refit,
 * scripts/run_gp_mpc.py:115-120; here "drop m, append m" keeps the size fixed while the loop runs).  Blocks of up to 16 rows, each one
 * rank-m update of (L^-1)^T and of alpha = K^-1 y with no stored targets (csrc/gp_drop.hip): no
 * refactorisation, no host synchronisation, nothing read back; hyperparameters, xbar and the
 * capacity are unchanged, gpmpc_gp_size reports the new count.  Inert rows (rejected append
 * blocks) may be among the dropped and the kept rows; kept ones stay inert.
 * ok_dev: device int32 [ceil(m/16)], may be NULL; 1 when every pivot of the block's update was
 * finite and positive, else 0.  After a 0 the contents of the GP are unspecified (nothing is
 * accessed out of bounds, but means and variances are meaningless): upload it again with
 * gpmpc_set_gp before it is used.
 * Refused, with the GP unchanged: m < 1 or m >= n, at least one row stays (GPMPC_ERR_ARG); GP not
 * set, set without Linv, a FITC upload (Xv != X), a LOVE root installed (drop it first with
 * gpmpc_set_gp_variance_root(R = NULL), or rebuild it afterwards with gpmpc_gp_love_root), or no
 * gpmpc_gp_reserve since gpmpc_set_gp -- the update writes the factor into the second buffer a reserve allocates (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_drop_oldest(gpmpc_handle* h, int32_t gp_id, int32_t m, int32_t* ok_dev, void* stream);

/* Remove the m training rows idx_dev names (device int32 [m], indices into the rows as they are when the call is
 * made) of GP gp_id on `stream`: gpmpc_gp_drop_oldest for an arbitrary set, to take out an outlier, a row whose
 * target is no longer trusted, or the rows gpmpc_gp_redundant chose.  The kept rows keep their order; row counts,
 * xbar, capacity and hyperparameters behave as after gpmpc_gp_drop_oldest, and the linearisation cache is invalidated.
 * One launch sorts the set ascending into scratch of the GP; then blocks of up to 16 rows are taken from the highest
 * indices down (so no block shifts the rows of the blocks after it), each a rank-m update of (L^-1)^T and alpha
 * through the kept-row map (csrc/gp_drop.hip): no refactorisation, no host synchronisation, nothing read back.
 * Indices that are not m distinct values in 0 .. n-1 cannot be refused without a read-back, so the call stays well
 * defined: the rows dropped are the distinct indices in range, and while these are fewer than m the lowest rows not
 * yet among them are added; ok_dev then reads 0 and the GP is valid.
 * dropped_dev: device int32 [m], may be NULL; the rows actually dropped, ascending (the caller who keeps the
 * targets needs it).  ok_dev: device int32 [1], may be NULL; 1 when the indices were m distinct values in range and
 * every pivot of every block was finite and positive.  After a 0 caused by a pivot the contents of the GP are
 * unspecified but every access stayed in bounds, as for gpmpc_gp_drop_oldest.  Inert rows may be among the dropped
 * and the kept rows (a zero on the diagonal of M[D,D] / P[D,D] reads as 1); kept ones stay inert.
 * Refused, with the GP unchanged: m < 1, m >= n or idx_dev NULL (GPMPC_ERR_ARG); what gpmpc_gp_drop_oldest refuses
 * of the GP's state (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_drop_rows(gpmpc_handle* h, int32_t gp_id, int32_t m, const int32_t* idx_dev,
                                int32_t* dropped_dev, int32_t* ok_dev, void* stream);

/* Factorise GP gp_id again from scratch on `stream`, from what the device already holds: the
 * handle's own training inputs, the caller's device targets y_dev [n] (float64, the targets of the
 * GP's n current rows in row order; n as gpmpc_gp_size reports it, inert rows included) and the
 * hyperparameters passed in.  With the current hyperparameters it refreshes a factor that appends
 * and drops have let drift; with new ones it applies a hyperparameter refit.  No host
 * synchronisation, nothing read back, nothing allocated (csrc/gp_refactor.hip: a blocked Cholesky
 * factorisation and triangular inverse in 16-wide panels, 2 ceil(n/16) + 4 launches).  Afterwards
 * the GP is what gpmpc_set_gp would have produced for (X, y, lengthscale, outputscale, noise):
 * (L^-1)^T of k(X,X) + noise I at the stride it had, alpha = K^-1 y, and the MFMA tile pack
 * rewritten in full (its input part depends on the lengthscale); xbar, n and the capacity are
 * unchanged.  Inert rows (rejected append blocks, recognised by the zero on the old factor's
 * diagonal) take part as identity rows and stay inert; their y_dev entries are never read into a
 * sum and may be anything, NaN included.
 * ok_dev: device int32 [1], may be NULL; 1 when every target of a live row is finite and every
 * pivot was finite and positive, else 0.  After a 0 the contents of the GP are unspecified (nothing
 * is accessed out of bounds): upload it again with gpmpc_set_gp before it is used.
 * Refused, with the GP unchanged: y_dev NULL or a hyperparameter that is not finite and positive
 * (GPMPC_ERR_ARG); GP not set, set without Linv, a FITC upload (Xv != X), a LOVE root installed
 * (drop it first with gpmpc_set_gp_variance_root(R = NULL), or rebuild it afterwards with
 * gpmpc_gp_love_root), or no gpmpc_gp_reserve since gpmpc_set_gp -- the work space is the second factor buffer and scratch a reserve allocates
 * (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_refactor(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double lengthscale,
                               double outputscale, double noise, int32_t* ok_dev, void* stream);

/* The exact marginal log likelihood per live row of GP gp_id as the handle holds it, and its gradient
 * with respect to (lengthscale, outputscale, noise), on `stream`: out_dev [4] (device, float64) =
 * {MLL / n_live, d/d lengthscale, d/d outputscale, d/d noise} (the ExactMarginalLogLikelihood
 * convention; inert rows are not counted).  y_dev [n]: the targets of the GP's n current rows in row
 * order, as gpmpc_gp_refactor takes them.  Everything comes from the handle's state (csrc/gp_fit.hip):
 * log det from the diagonal of (L^-1)^T, alpha from the rows, K^-1 = L^-T L^-1 tile by tile on f64 MFMA
 * for tr((alpha alpha^T - K^-1) dK/dtheta).  After appends and drops it is the likelihood of the factor
 * as it has drifted.  Asynchronous, nothing read back; nothing of the GP changes.
 * Refused: y_dev or out_dev NULL (GPMPC_ERR_ARG); every state refusal of gpmpc_gp_refactor, an installed
 * LOVE root among them (drop it first, or rebuild it afterwards with gpmpc_gp_love_root)
 * (GPMPC_ERR_STATE; gpmpc_gp_reserve also allocates this call's scratch). */
gpmpc_status gpmpc_gp_mll(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double* out_dev, void* stream);

/* Fit the hyperparameters of GP gp_id on the device: Adam (lr, torch.optim.Adam's defaults) on
 * -MLL / n_live over the raw parameters (lengthscale = softplus(raw[0]), outputscale =
 * softplus(raw[1]), noise = 1e-6 + softplus(raw[2])), at most max_iter iterations, ended early after
 * the step at which |previous loss - loss| < 1e-3.  Iteration t factorises at the raw parameters
 * of iteration t - 1 (gpmpc_gp_refactor's kernels), evaluates loss and gradient (gpmpc_gp_mll's) and
 * steps; parameters, moments and flags stay on the device, and the host reads the flags once per 8
 * queued iterations.  THE CALL SYNCHRONISES `stream`: it returns after the GP has been refactorised
 * at the fitted hyperparameters, bit for bit as gpmpc_gp_refactor(y_dev, those hyperparameters) leaves
 * it, and the handle's hyperparameters are the fitted ones.
 * raw: host [3], in: the start, out: the fitted raw parameters.  iters_out, ok_out: host, may be NULL;
 * the iterations run and 1 for success.  hist_dev: device [max_iter][4] or NULL; row t - 1 receives
 * (loss before step t, raw after it), rows past the iterations run are not written.
 * Failure (a target of a live row, a pivot, a loss or a gradient that is not finite): *ok_out = 0, raw
 * is left as passed in, and the GP is refactorised at the hyperparameters it had; if that
 * refactorisation fails too (the targets), its contents are unspecified as after gpmpc_gp_refactor's 0.
 * Refused, with the GP unchanged: y_dev or raw NULL, a raw value or lr that is not finite, lr <= 0,
 * max_iter < 1 (GPMPC_ERR_ARG); every state refusal of gpmpc_gp_refactor, an installed LOVE root among
 * them (drop it first, or rebuild it afterwards with gpmpc_gp_love_root) (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_fit(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double lr, int32_t max_iter, double* raw,
                          int32_t* iters_out, int32_t* ok_out, double* hist_dev, void* stream);

/* Build the LOVE variance root of GP gp_id on the device and install it, as
 * gpmpc_set_gp_variance_root would install the host's: Lanczos with full reorthogonalisation (two
 * passes) on Khat = k(X, X) + noise I, generated on the device from the handle's own rows and current
 * hyperparameters, from the start vector q0_dev [n] (device, float64; the library draws no random
 * numbers).  It restates GaussianProcess.love_root (gpmpc/gp.py), its breakdown rule
 * |v| <= 1e-12 max |alpha| included, up to the last step: instead of the eigendecomposition of the
 * tridiagonal matrix T the root is R = Q C^-T with T = C C^T, C lower bidiagonal -- R R^T = Q T^-1 Q^T
 * is the same matrix, and only it reaches the variance (csrc/gp_love.hip).  The root's rank is at most
 * min(rank, live rows), 1 <= rank <= 256.  Inert rows (rejected append blocks, recognised by the zero
 * on the factor's diagonal) take no part: their q0_dev entries are never read into a sum and may be
 * anything, NaN included, and their rows of the root are exact zeros.  The result depends on the inputs
 * alone, bit for bit (every sum has a fixed order).
 * THE CALL SYNCHRONISES `stream` (the host needs the final rank).  rank_out, ok_out: host, may be
 * NULL; the installed root's rank and 1, or 0 and 0 when a pivot of C was not finite and positive (or no
 * row is live): then the handle is unchanged, a root installed before included.
 * Refused, with the GP unchanged: q0_dev NULL or rank outside 1..256 (GPMPC_ERR_ARG); GP not set, set
 * without Linv, a FITC upload (Xv != X), or no gpmpc_gp_reserve since gpmpc_set_gp -- Khat is built in
 * the second factor buffer and the Lanczos vectors in scratch a reserve allocates (GPMPC_ERR_STATE).
 * An installed root is no obstacle: it is replaced on success. */
gpmpc_status gpmpc_gp_love_root(gpmpc_handle* h, int32_t gp_id, int32_t rank, const double* q0_dev,
                                int32_t* rank_out, int32_t* ok_out, void* stream);

/* The installed LOVE root of GP gp_id: its rows n (the variance GP's training rows) and its rank r,
 * either may be NULL; with R_dev non-NULL (device, float64 [n][r] row-major, unpadded) the root is
 * copied on `stream`.  GPMPC_ERR_STATE when no root is installed. */
gpmpc_status gpmpc_get_gp_variance_root(gpmpc_handle* h, int32_t gp_id, int32_t* n, int32_t* r,
                                        double* R_dev, void* stream);

/* Build the FITC inducing-point mean of GP gp_id on the device and install it as the mean the solver reads,
 * as gpmpc_set_gp(X = S, alpha = w, Xv = training rows) would: from the handle's own n training rows X
 * (n as gpmpc_gp_size reports it, inert rows included), its current hyperparameters, the caller's device
 * targets y_dev [n] (float64, in row order, as gpmpc_gp_refactor takes them) and the inducing rows
 * S = X[idx], idx_dev [M] a device int32 array, 1 <= M <= n.  It restates gpmpc/gpmpc.py:392-397 in the
 * factored form (csrc/gp_fitc.hip), jitter >= 0 an absolute value added to the diagonal of K_ss (0: the
 * reference's own formula):
 *   K_ss + jitter I = L L^T,  V = L^-1 k(S, X),  Gamma_i = outputscale + noise - |V[:, i]|^2,
 *   B = I + V Gamma^-1 V^T = C C^T,  w = L^-T B^-1 V Gamma^-1 y
 * so that the mean at z is sum_j w_j k(z, S_j), k carrying the outputscale.  Inert rows (rejected append
 * blocks, recognised by the zero on the factor's diagonal) take no part: their Gamma^-1 is 0 and their
 * y_dev entries are never read into a sum and may be anything, NaN included.  Distinct indices are the
 * caller's responsibility (with jitter 0 a duplicate fails its pivot).  The result depends on the inputs
 * alone, bit for bit (every sum has a fixed order).
 * The FITC mean is an overlay on the exact GP, which stays in the handle beside it (rows with alpha, the
 * tile pack, the factor, the capacity): gpmpc_gp_size keeps reporting the training rows,
 * gpmpc_gp_predict / gpmpc_gp_mean_grad return the FITC mean with the exact variance, the tightening
 * variance and a LOVE root are untouched.  The tile pack of the inducing rows is centred on the xbar the
 * GP already has.  M = 0 with idx_dev = NULL removes the overlay and restores the exact mean (no
 * synchronisation; y_dev, jitter and ok_out are ignored; M = 0 with idx_dev non-NULL is GPMPC_ERR_ARG).
 * gpmpc_set_gp clears the overlay; gpmpc_set_gp_variance_root and gpmpc_gp_love_root leave it alone.
 * While it is installed gpmpc_gp_append, _drop_oldest, _refactor, _mll, _fit and gpmpc_gp_reserve are
 * refused (GPMPC_ERR_STATE): the overlay belongs to the old training set; drop it first with M = 0, or
 * rebuild it afterwards.
 * With M >= 1 THE CALL SYNCHRONISES `stream` (the host reads the status).  ok_out: host, may be NULL; 1
 * on success, 0 when a pivot of L or C or a live row's Gamma is not finite and positive, a live target is
 * not finite, or an index names an inert row or lies outside 0 .. n-1: then the handle is unchanged, a
 * FITC mean installed before included.  The work space depends on M: the call allocates it and the handle
 * keeps it for a later call of the same or a smaller M (GPMPC_ERR_NOMEM, handle unchanged, when it cannot).
 * Refused, with the GP unchanged: y_dev or idx_dev NULL with M >= 1, M outside 1 .. n, jitter negative or
 * not finite (GPMPC_ERR_ARG); GP not set, set without Linv, a FITC upload (Xv != X), or no
 * gpmpc_gp_reserve since gpmpc_set_gp -- V is built in the second factor buffer (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_fitc(gpmpc_handle* h, int32_t gp_id, int32_t M, const int32_t* idx_dev, const double* y_dev,
                           double jitter, int32_t* ok_out, void* stream);

/* The FITC mean gpmpc_gp_fitc installed for GP gp_id: *M (host, may be NULL) its inducing rows, 0 when none
 * is installed; with idx_dev / w_dev non-NULL (device, int32 [M] / float64 [M]) the inducing indices and
 * the weights are copied on `stream`. */
gpmpc_status gpmpc_get_gp_fitc(gpmpc_handle* h, int32_t gp_id, int32_t* M, int32_t* idx_dev, double* w_dev,
                               void* stream);

/* Choose the FITC inducing rows of GP gp_id on the device, by the kernel instead of a random draw (the
 * reference's np_random.choice, gpmpc/gpmpc.py:387): up to M of the GP's n training rows, picked greedily by
 * residual prior variance, which is a pivoted partial Cholesky factorisation of the prior covariance k(X, X)
 * of the handle's own rows at its current hyperparameters (csrc/gp_observe.hip).  The likelihood noise is not
 * in it: K_ss has none.
 *   d_i = outputscale for every live row.  For t = 0 .. M-1: the score s_i = d_i / outputscale of the open
 *   rows; the pick j_t is the largest finite score above tol, ties to the lower index, and when there is none
 *   the selection stops with count = t; else l_t[i] = (k(x_i, x_j) - sum_{s<t} l_s[i] l_s[j]) / sqrt(d_j) and
 *   d_i -= l_t[i]^2 for every live row, and row j closes.
 * Step 0 is an exact tie (every score is 1.0): the lowest live index is picked.  Inert rows (rejected append
 * blocks, recognised by the zero on the factor's diagonal) are closed from the start, never picked and in no
 * sum.  Outputs: idx_dev (device int32 [M]) the picks in pick order, then -1 up to M; gain_dev (device float64
 * [M], may be NULL) the scores s_j at which they were picked, then NaN; resid_dev (device float64 [n], may be
 * NULL) the final d_i = outputscale - k(x_i, S) K_ss^-1 k(S, x_i), 0 for an inert row (plus the noise it is
 * FITC's Gamma_i); count_out (host, may be NULL) the number of picks.  The first k picks and gains of a call
 * with M are those of a call with M = k, and every output is fixed bit for bit by the inputs (every sum has a
 * fixed order: 16 parts of fixed extent added as a balanced tree; no atomics).
 * tol = 0 takes M rows whatever their gain, while a positive pivot is left; below a gain of about 1e-12 the
 * gains are rounding noise, and so is the order of the picks.  With tol > 0 the diagonal of the Cholesky factor
 * of K_ss in pick order is sqrt(gain x outputscale), so gpmpc_gp_fitc(idx = the picks, M = count, jitter = 0)
 * has pivots bounded below by sqrt(tol x outputscale), and near-copies of a picked row are never picked.
 * THE CALL IS SYNCHRONOUS and takes no stream (see "Streams" above): the host needs count before it can call
 * gpmpc_gp_fitc.  Its launches, one for the start state and one per pick, run on a stream of the handle's own
 * behind the handle's last call; the count is read back every 64 picks and nothing more is queued after a
 * stop, which changes no output.  The output buffers must be idle when the call is made (work queued on them
 * in the caller's streams is not waited for); they are complete when it returns.  Nothing of the GP changes, and
 * the call allocates no device memory: the l columns [M][capacity] go into the second factor buffer and the rest
 * into scratch gpmpc_gp_reserve allocates (the handle's stream, the one the overlapped steps of gpmpc_solve use, is
 * created on first use).  An installed LOVE root or FITC mean is no obstacle: gpmpc_gp_love_root
 * and gpmpc_gp_fitc had finished with the second factor buffer when they returned and keep nothing in it.
 * Refused, with nothing written: M outside 1 .. n, tol negative or not finite, idx_dev NULL (GPMPC_ERR_ARG);
 * GP not set, set without Linv, a FITC upload (Xv != X), or no gpmpc_gp_reserve since gpmpc_set_gp
 * (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_inducing(gpmpc_handle* h, int32_t gp_id, int32_t M, double tol, int32_t* idx_dev,
                               double* gain_dev, double* resid_dev, int32_t* count_out);

/* Training rows of GP gp_id (inert rows included; with a FITC mean installed by gpmpc_gp_fitc still the
 * training rows, not the inducing ones) and its capacity; either may be NULL. */
gpmpc_status gpmpc_gp_size(gpmpc_handle* h, int32_t gp_id, int32_t* n, int32_t* capacity);

/* Enable (1) / disable (0) the GP residual in the dynamics: 0 = nominal MPC
 * (gpmpc/mpc.py, prior dynamics only). */
gpmpc_status gpmpc_use_gp(gpmpc_handle* h, int32_t enabled);

/* Constraint tightening (gpmpc/gpmpc.py:425-498): inverse_cdf (gpmpc.py:63-65) and the
 * prior LQR closed loop: Ad [nx][nx], Bd [nx][nu], K [nu][nx] (gpmpc.py:500-507).
 * enabled = 0 disables tightening (nominal MPC).  Builds the H-term gain table of the covariance
 * recursion on the host and copies it to the device (synchronous; a setup call). */
gpmpc_status gpmpc_set_tightening(gpmpc_handle* h, int32_t enabled, double inverse_cdf, const double* Ad,
                                  const double* Bd, const double* K);

/* Input map of GP gp_id's tightening variance: indices src[0..d) into z = [x; u] (d = the
 * GP's input dimension).  The default is the reference's map, which evaluates GP g at
 * z[:, gp_idx[g]] with gp_idx indexing the GP-input space (gpmpc/gpmpc.py:59 vs 437-444,
 * reproduced for quad3d); passing the GP's own dynamics inputs (gpmpc/gpmpc.py:173)
 * evaluates the variance where the mean is evaluated. */
gpmpc_status gpmpc_set_var_inputs(gpmpc_handle* h, int32_t gp_id, const int32_t* src, int32_t d);

/* Forget the previous solution for instances [0, batch): the next solve runs without
 * tightening (GPMPC.reset, gpmpc/gpmpc.py:109-111).  reset_iterate = 1 also zeroes the
 * warm-start iterate and multipliers (acados_solver.reset(), gpmpc/mpc.py:62; and the fresh
 * AcadosOcpSolver GPMPC.reset builds after new GPs, gpmpc/gpmpc.py:97-108). */
gpmpc_status gpmpc_reset(gpmpc_handle* h, int32_t batch, int32_t reset_iterate, void* stream);

/* Set the warm-start iterate (device arrays x [B][H+1][nx], u [B][H][nu]); multipliers zeroed.
 * The next solve starts from exactly this guess (GPMPC_TUNE_SHIFT does not move it). */
gpmpc_status gpmpc_set_iterate(gpmpc_handle* h, int32_t batch, const double* x_dev, const double* u_dev, void* stream);

/* One batched control step: GPMPC.select_action(obs) for every instance
 * (gpmpc/gpmpc.py:334-368): tightening from the stored previous solution, SQP to
 * convergence warm-started from it, store the new solution.
 *   x0      [B][nx]  initial states (obs)                                   (device)
 *   tstep   [B]      reference index per instance (traj_step)               (device)
 *   u0      [B][nu]  first input (return value of select_action)            (device, out)
 *   status  [B]      acados status code                                     (device, out)
 *   sqp_iter, qp_iter [B]  SQP iterations / total IPM iterations            (device, out, may be NULL)
 *   res     [B][4]   final NLP residuals stat, eq, ineq, comp               (device, out, may be NULL)
 * When the SQP launch needs more than one round of workgroups (more instances than the device
 * holds at once) and the step has a variance launch, half of the step's work runs on a handle-owned
 * side stream forked from and joined back into `stream` (results bit-identical;
 * gpmpc_set_tuning(GPMPC_TUNE_OVERLAP, 0) turns it off): work queued on `stream` after the call
 * still sees the whole step complete. */
gpmpc_status gpmpc_solve(gpmpc_handle* h, int32_t batch, const double* x0, const int32_t* tstep, double* u0,
                         int32_t* status, int32_t* sqp_iter, int32_t* qp_iter, double* res, void* stream);

/* Copy the current solution (x_prev / u_prev, gpmpc/gpmpc.py:366-367) into device arrays
 * x [B][H+1][nx], u [B][H][nu]; tight [B][H+1][nx+nu] receives the last tightening
 * magnitudes (icdf*sqrt(var)) if non-NULL. */
gpmpc_status gpmpc_get_solution(gpmpc_handle* h, int32_t batch, double* x_dev, double* u_dev, double* tight_dev,
                                void* stream);

/* Copy the GP variances the last tightening used (the variance kernel's output at the previous
 * solution, likelihood noise included, gpmpc/gpmpc.py:437-445) into var [B][H][n_gp] (device).
 * Diagnostic / parity surface: the values the constraint tightening consumed.  GPMPC_ERR_STATE
 * when the last gpmpc_solve ran no variance launch (first step after a reset, tightening or GPs
 * off): there are no such values; GPMPC_ERR_ARG when batch exceeds that launch's batch. */
gpmpc_status gpmpc_get_variance(gpmpc_handle* h, int32_t batch, double* var_dev, void* stream);

/* GP posterior at P points Z [P][d] (device): mean [P] and/or variance [P] (either may be
 * NULL; variance needs Linv).  with_noise = 1 adds the likelihood noise
 * (gp.likelihood(gp(z)), gpmpc/gpmpc.py:444).  GaussianProcess.predict() of the build. */
gpmpc_status gpmpc_gp_predict(gpmpc_handle* h, int32_t gp_id, const double* Z, int32_t P, double* mean,
                              double* var, int32_t with_noise, void* stream);

/* GP mean and its input gradient at P points Z [P][d] (device): mean [P], grad [P][d] (either
 * may be NULL), through the MFMA tile sums the SQP linearisation uses (sqp_kernel.hip
 * gp_tiles).  Replaces the casadi mean export gpytorch_predict2casadi (gpmpc/gp.py:72-85) and
 * the CasADi AD of it inside setup_acados_model (gpmpc/gpmpc.py:189-209). */
gpmpc_status gpmpc_gp_mean_grad(gpmpc_handle* h, int32_t gp_id, const double* Z, int32_t P, double* mean,
                                double* grad, void* stream);

/* Handle-free GP posterior (GaussianProcess.predict() of the build): GP data already on the
 * device in the kernel layout -- rows [npad][4] = (x0, x1, x2 zero padded, alpha) and
 * linvT [npad][npad] = (L^-1)^T zero padded (NULL -> mean only), npad = n rounded up to 16.
 * Replaces the gpytorch posterior of gpmpc/gpmpc.py:441-445 and the casadi mean export
 * gpmpc/gp.py:72-85. */
gpmpc_status gpmpc_gp_posterior(int32_t n, int32_t d, int32_t npad, const double* rows, const double* linvT,
                                double lengthscale, double outputscale, double noise, const double* Z, int32_t P,
                                double* mean, double* var, int32_t with_noise, void* stream);

/* Synthetic plant: x_next = RK4(prior-form dynamics with `params`, no GP) for B instances,
 * tstep += 1 if tstep != NULL (crazyflow env.step replacement, scripts/run_gp_mpc.py:59).
 * params (host) is read before the call returns and travels to the kernel by value: a queued launch
 * integrates with the parameters of its own call, whatever later calls pass on any stream.  No
 * host synchronisation, whether the parameters change or not. */
gpmpc_status gpmpc_plant_step(gpmpc_handle* h, int32_t batch, const double* params, const double* x,
                              const double* u, double* x_next, int32_t* tstep, void* stream);

/* Open-loop rollout of the model the MPC plans with: P trajectories of T steps, one launch
 * (csrc/sqp_kernel.hip rollout_kernel).  x0_dev [P][nx] and u_dev [P][T][nu] are device inputs; x_dev
 * [P][T+1][nx] is the device output: row 0 a copy of x0, row k+1 one RK4 step of length dt from (x_k, u_k)
 * (the RK4 of the build, gpmpc/gpmpc.py:204-209, over the residual dynamics of gpmpc/gpmpc.py:171-199).
 *   with_gp = 1  the prior at gpmpc_set_model's parameters plus the GP means as the solver reads them (the
 *                handle's tile packs: a FITC mean installed by gpmpc_gp_fitc or uploaded by gpmpc_set_gp is the
 *                one used), evaluated at z[gp_src_g] at each of the four RK4 substages: the discrete map of the
 *                SQP's multiple-shooting constraint.
 *   with_gp = 0  the GP means are zero: the nominal MPC's model.  Nothing of the GPs is read, none needs to be set.
 * With with_gp = 0 the states are the bits of T chained gpmpc_plant_step calls at the same parameters.
 * var_dev [P][T][n_gp], may be NULL: the exact posterior variance without likelihood noise of GP g at
 * z_k[gp_src_g], z_k = [x_k; u_k], k = 0 .. T-1, by the launch behind gpmpc_gp_predict(with_noise = 0) on the
 * finished trajectory and bit-identical to that call on those inputs (a LOVE root is ignored, a FITC overlay does
 * not change it).  Allowed with with_gp = 0: the uncertainty along a prior rollout.
 * What is computed for a trajectory depends on its own inputs and the handle only: the same (x0, u) gives the same
 * bits whatever P is and wherever it sits in the batch, and the first k+1 rows of a T-step rollout are the bits of
 * a k-step rollout.  A non-finite state or input makes that trajectory's later rows non-finite and touches no other
 * trajectory; nothing is refused on the device.
 * THE CALL IS SYNCHRONOUS and takes no stream (see "Streams" above).  The gathered variance inputs (P T points) are
 * scratch of the handle, allocated inside the call and kept for a later call of the same or a smaller size; if the
 * allocation fails the call returns GPMPC_ERR_NOMEM and the handle is unchanged.
 * Refused with nothing written: P < 1, T < 1, x0_dev, u_dev or x_dev NULL, with_gp not 0 or 1, P (T+1) nx not
 * representable in int32 (GPMPC_ERR_ARG); a call before gpmpc_set_model, with_gp = 1 while the handle's GPs are
 * off (gpmpc_use_gp(0), or a GP of the model not set), var_dev with a GP not set or set without Linv
 * (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_rollout(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                           int32_t with_gp, double* x_dev, double* var_dev);

/* gpmpc_rollout with the Jacobians of every step and, on request, the state covariance along the trajectory
 * (csrc/sqp_kernel.hip rollout_lin_kernel, csrc/rollout_cov.hip).  P, T, x0_dev, u_dev, with_gp, x_dev and var_dev
 * are gpmpc_rollout's: x_dev and var_dev receive the bits that call writes (the same RK4 statements and tile sums,
 * the same gather and variance launches; the variance carries no likelihood noise and ignores a LOVE root).
 *   A_dev [P][T][nx][nx], B_dev [P][T][nx][nu], row-major: A_k = dx_{k+1}/dx_k and B_k = dx_{k+1}/du_k, the exact
 *     derivative of the RK4 step at (x_k, u_k): the tangent recursion dk_s = J_s[:, :nx] (E + c_s dt dk_{s-1}) +
 *     [0, J_s[:, nx:]] over the four substages, J_s the Jacobian of the residual dynamics with the GP input gradient
 *     sf2/ell^2 (S_{1+d} - (z_d - xbar_d) S0) taken from the tile pass that yields the mean (a GP whose input is a
 *     control is evaluated at substage 0 only).  With with_gp = 0 means and gradients are zero and nothing of the
 *     GPs is read.
 *   cov_dev [P][T+1][nx][nx], may be NULL: Sigma_0 = cov0_dev [P][nx][nx] (NULL: zero; taken as given, the caller
 *     keeps it symmetric), Sigma_{k+1} = Phi_k Sigma_k Phi_k^T + Bd diag(q_k) Bd^T with Phi_k = A_k + B_k K (K a
 *     HOST array [nu][nx], row-major; NULL: the open loop, Phi_k = A_k), Bd the identity columns of the model's
 *     uncertain dimensions and q_k[j] = dt^2 sum_g W_{j,g}(x_k, u_k) (var_g,k + with_noise noise_g), W the
 *     tightening's variance weights (quad3d's literal cos(phi) sin(theta)^2 included).  This is the tightening's
 *     recursion (gpmpc/gpmpc.py:425-498) with the learned model's own A_k, B_k along the trajectory in place of the
 *     prior's constant Ad, Bd.  THE NOISE ENTERS ONCE (with_noise = 1), not twice as in the reference's tightening,
 *     whose variance already includes it before cov_noise adds it again.  K is read before the call returns and
 *     travels by value.  Every Sigma_k equals its transpose bit for bit (one triangle is computed and mirrored), and
 *     every sum has a fixed order.  var_dev may be NULL with cov_dev given: the variances then go to scratch of the
 *     handle.
 * Independence as for gpmpc_rollout: a trajectory's x, A, B, var and cov depend on its own (x0, u, cov0) and the
 * handle only, whatever P is and wherever it sits in the batch; the first k rows of A and B and the first k+1 rows
 * of cov of a T-step call are those of a k-step call; a non-finite input poisons only its own trajectory.
 * THE CALL IS SYNCHRONOUS and takes no stream (see "Streams" above).  Scratch (the gathered variance inputs, and the
 * variances when var_dev is NULL) is the handle's, allocated before anything is queued and kept; if the allocation
 * fails the call returns GPMPC_ERR_NOMEM and the handle is unchanged.
 * Refused with nothing written: everything gpmpc_rollout refuses; also A_dev or B_dev NULL, with_noise not 0 or 1,
 * a non-finite entry of K, P T nx nx not representable in int32 (GPMPC_ERR_ARG); var_dev or cov_dev with a GP not
 * set or set without Linv (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_rollout_lin(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                               int32_t with_gp, double* x_dev, double* A_dev, double* B_dev, double* var_dev,
                               const double* K, const double* cov0_dev, int32_t with_noise, double* cov_dev);

/* One closed-loop sample per trajectory of the future the learned model believes in: gpmpc_rollout with the input
 * recomputed from a feedback law at every step and a draw of every GP's residual added to its mean, one launch for
 * the whole horizon (csrc/sqp_kernel.hip rollout_sample_kernel).  P, T, x0_dev, with_gp and x_dev are gpmpc_rollout's;
 * u_dev [P][T][nu] holds the NOMINAL inputs.  For step k = 0 .. T-1 of a trajectory:
 *   applied input  v_c = u_nom,k[c], then for j ascending v_c = fma(K[c][j], x_k[j] - xref_k[j], v_c); with clip = 1
 *                  u_k[c] = v_c < u_lo[c] ? u_lo[c] : (v_c > u_hi[c] ? u_hi[c] : v_c) with gpmpc_set_model's input box
 *                  (a NaN stays a NaN), else u_k[c] = v_c.  K is a HOST array [nu][nx], row-major, read before the
 *                  call returns (it travels by value), or NULL for no feedback; xref_dev [P][T+1][nx] is the feedback
 *                  reference, row k read at step k (row T is not read), NULL if and only if K is NULL.
 *   variance       var_{g,k}: the exact posterior variance of GP g without likelihood noise at z_k[gp_src_g],
 *                  z_k = [x_k; u_k] with the APPLIED input: the quantity gpmpc_gp_predict(with_noise = 0) computes (inert
 *                  rows inert, a LOVE root ignored, a FITC overlay not changing it), evaluated inside the step loop
 *                  and only when xi_dev or var_dev is given.  The sums run in another order than that call's, so the
 *                  two agree to rounding, not bit for bit.
 *   disturbance    e_g = sqrt(fmax(var_{g,k} + with_noise noise_g, 0)) xi[k][g]: one draw of GP g's residual, held
 *                  over the step.  xi_dev [P][T][n_gp] holds the caller's standard-normal draws (the library draws
 *                  none), NULL for no disturbance.
 *   state          x_{k+1}: gpmpc_rollout's RK4 step with mean_g(z at the substage) + e_g in place of the mean at every
 *                  substage (a control-only GP is evaluated at substage 0 alone; with_gp = 0: the means are zero and
 *                  the value is e_g).  The draw so passes through the model's own df/dgm, with its sign and its
 *                  correlation across state rows; the diagonal dt^2 W (var + noise) of gpmpc_rollout_lin's cov_dev and
 *                  of the tightening is its first-order marginal.
 * x_dev [P][T+1][nx] receives the states, uapp_dev [P][T][nu] (may be NULL) the applied inputs, var_dev [P][T][n_gp]
 * (may be NULL) the variances.
 * With xi_dev = NULL, K = NULL and clip = 0, x_dev receives gpmpc_rollout's bits: the draw is then not in the
 * arithmetic at all (it is not multiplied by zero).  A trajectory's outputs depend on its own inputs and the handle
 * only, whatever P is and wherever it sits in the batch; the first k+1 rows of a T-step call are those of a k-step
 * call; a non-finite input poisons its own trajectory only; every sum has a fixed order, there are no atomics, and
 * nothing is refused on the device.
 * THE CALL IS SYNCHRONOUS and takes no stream (see "Streams" above).  It needs no scratch and allocates nothing.
 * Refused with nothing written: everything gpmpc_rollout refuses of P, T, x0_dev, u_dev, x_dev and with_gp; also
 * with_noise or clip not 0 or 1, exactly one of K and xref_dev given, a non-finite entry of K (GPMPC_ERR_ARG); a call
 * before gpmpc_set_model, with_gp = 1 with the GPs off or a GP unset, xi_dev or var_dev with a GP not set or set
 * without Linv (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_rollout_sample(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                                  const double* xref_dev, const double* K, int32_t clip, const double* xi_dev,
                                  int32_t with_gp, int32_t with_noise, double* x_dev, double* uapp_dev,
                                  double* var_dev);

/* GP training rows from transitions, on the device: GPMPC.preprocess_data of the build (the reference's
 * gpmpc/gpmpc.py:113-151) for the handle's model, csrc/gp_observe.hip.  x_dev [P][nx], u_dev [P][nu] and
 * xnext_dev [P][nx] are P transitions; output row r comes from transition pick_dev[r], r = 0 .. m-1 (pick_dev
 * NULL: from transition r, and then m <= P).  inputs_dev [m][sum d_g] and targets_dev [m][n_gp], row-major, have
 * the shapes and the column order preprocess_data returns; either may be NULL, not both.  The inputs are copies of
 * z[gp_src_g], z = [x; u].  The targets start from x_dot = (x_next - x) / dt_diff: for quad2d and quad3d the thrust
 * target is sqrt(sum of the squared velocity components of x_dot, `gravity` added to the z-component) minus
 * (a u_0 + b), and the rate targets are x_dot_j - f_j(x, u); cartpole's two targets are its two acceleration
 * residuals.  f is the prior dynamics (csrc/models.h, zero GP means) at the parameters gpmpc_set_model was given,
 * not the plant's.  dt_diff and gravity are the caller's: the reference's literals 1/60 and 9.81 for quad3d, the
 * model's dt and gravity otherwise.
 * One kernel launch on `stream`, no host synchronisation, nothing of the handle changes.  A pick outside 0 .. P-1
 * reads nothing and gives a row of NaN; a non-finite transition propagates as NaN or Inf, nothing is refused on
 * the device.
 * Refused: P < 1, m < 1, a NULL transition array, both outputs NULL, pick_dev NULL with m > P, dt_diff not finite
 * and positive, gravity not finite (GPMPC_ERR_ARG); a call before gpmpc_set_model (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_preprocess(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev,
                              const double* xnext_dev, int32_t m, const int32_t* pick_dev, double dt_diff,
                              double gravity, double* inputs_dev, double* targets_dev, void* stream);

/* The m of P points z_i = [x_i; u_i] (device, x_dev [P][nx], u_dev [P][nu]) where the GPs are least certain:
 * score s_i = max over the GPs g of var_g(z_i[gp_src_g]) / outputscale_g, var_g the exact posterior variance
 * without likelihood noise over GP g's training rows.  The inputs are gathered as gpmpc_preprocess gathers them
 * and the variance is the launch behind gpmpc_gp_predict(with_noise = 0), so the scores are bit-identical to that
 * call on those inputs, divided by the outputscale; a LOVE root and a FITC mean are ignored, as gpmpc_gp_predict
 * ignores them.  A NaN among a point's variances makes its score NaN, and so does a non-finite value among its GP
 * inputs (what the variance launch returns for such a point is unspecified).
 * pick_dev (device int32 [m]) receives the indices of the m largest scores in decreasing order; ties go to the
 * lower index, and a score that is not finite ranks after every finite one, again lower index first.  The rank
 * is counted (rank_i = the number of points that beat i, O(P^2) comparisons), so every output is fixed bit for
 * bit.  score_dev (device float64 [P]) receives the scores, may be NULL.  The picks are the m most uncertain
 * points one by one: no account is taken of redundancy among them, and near-duplicates may all be picked;
 * gpmpc_gp_select below conditions every candidate on the picks before it and so picks no near-duplicates.
 * Asynchronous on `stream`, no host synchronisation; the first call allocates the handle's scratch for max_batch
 * points, a synchronous setup step like gpmpc_gp_reserve.
 * Refused: P < 1, P > max_batch, m < 1, m > P, NULL x_dev, u_dev or pick_dev (GPMPC_ERR_ARG); a GP of the model
 * not set, or set without Linv (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_informative(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev, int32_t m,
                                  int32_t* pick_dev, double* score_dev, void* stream);

/* Greedy conditional-variance selection: m of the P candidates z_i = [x_i; u_i] (device, as above) such that each
 * pick is the candidate the GPs are least certain about once the picks before it are taken as observed.  This is a
 * pivoted partial Cholesky of the candidates' posterior covariance.  For each GP g, from the exact factor the handle
 * holds: v_g,i = L_g^-1 k_g(X_g, z_i) and d_g,i = outputscale_g - |v_g,i|^2, the latter the variance launches of
 * gpmpc_gp_informative (the same bits).  Then for t = 0 .. m-1:
 *   score    s_i = max_g d_g,i / outputscale_g over the candidates not yet picked, NaN for a candidate with a
 *            non-finite GP input or a NaN variance (gpmpc_gp_informative's rule);
 *   pick     j_t = the largest finite score, ties to the lower index: pick_dev[t] = j_t, gain_dev[t] = s_{j_t}.  When
 *            no finite candidate is left the remaining picks are the non-finite ones in index order, with gain NaN,
 *            and they condition nothing;
 *   condition, per GP: p = d_g,j + noise_g,
 *            l_g,t[i] = (k_g(z_i, z_j) - v_g,i . v_g,j - sum_{s<t} l_g,s[i] l_g,s[j]) / sqrt(p),
 *            d_g,i -= l_g,t[i]^2 for every i.  A p that is not finite and positive skips GP g for this pick and
 *            clears ok_dev[0], which is otherwise written as 1.
 * So step 0 is gpmpc_gp_informative's top pick and score, bit for bit, and afterwards the d_g,i are the posterior
 * variances (without noise) of a GP with the picked rows appended.  pick_dev: device int32 [m].  gain_dev (device
 * float64 [m]), resid_dev (device float64 [n_gp][P]: the final d_g,i; the entry of a non-finite candidate is
 * unspecified) and ok_dev (device int32 [1]) may be NULL.  Every output is fixed bit for bit by the inputs (fixed
 * summation orders, no atomics), and what is computed for a candidate depends on its own inputs and the GPs only:
 * duplicated candidates carry equal bits.  A LOVE root and a FITC mean are ignored, inert rows take no part, nothing
 * of the GPs changes.
 * Asynchronous on `stream`, no host synchronisation: the variance launches, one launch that stores V for every GP,
 * one for the start state and one per pick.  The handle's scratch (V at the GPs' capacity, the l columns
 * [n_gp][256][max_batch]) is allocated by the first call and again when a capacity has grown, a synchronous setup
 * step like gpmpc_gp_reserve; if that fails the call returns GPMPC_ERR_NOMEM and the handle is unchanged.
 * Refused: as gpmpc_gp_informative, and m > 256 (GPMPC_ERR_ARG). */
gpmpc_status gpmpc_gp_select(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev, int32_t m,
                             int32_t* pick_dev, double* gain_dev, double* resid_dev, int32_t* ok_dev, void* stream);

/* The m training rows the handle's GPs would miss least, one after the other: greedy backward selection, the mirror
 * of gpmpc_gp_select for the rows that leave a full window.  Every GP of the model must be set exactly with Linv, and
 * all must hold the same n rows.  With M_g = L_g^-1 and the precision P_g = M_g^T M_g, 1 / P_g,ii - noise_g is row
 * i's latent leave-one-out variance, what the other rows still say about x_i, and deleting row j turns P_g into
 * P_g[k,k] - P_g[k,j] P_g[j,k] / P_g,jj: a pivoted partial Cholesky of P_g, whose entries are inner products of rows
 * of (L_g^-1)^T.  Start from p_g,i = |linvT_g[i]|^2; a row inert in GP g has p = 0, its term below is 0 and it takes
 * no part in g's conditioning.  Then for t = 0 .. m-1:
 *   score    s_i = max_g (1 / p_g,i - noise_g) / outputscale_g over the rows not yet picked;
 *   pick     j_t = the smallest score, ties to the lower index (the older row leaves first), a score that is not
 *            finite after every finite one: pick_dev[t] = j_t, score_dev[t] = s_{j_t};
 *   condition, every GP in which j is live: c_g,t[i] = (P_g,ij - sum_{s<t} c_g,s[i] c_g,s[j]) / sqrt(p_g,j),
 *            p_g,i -= c_g,t[i]^2 for every i.  A p_g,j that is not finite and positive skips GP g for this pick and
 *            clears ok_dev[0], which is otherwise written as 1.
 * The score of the remaining rows never decreases from pick to pick.  pick_dev: device int32 [m]; score_dev (device
 * float64 [m]) and ok_dev (device int32 [1]) may be NULL.  Every output is fixed bit for bit by the inputs: each
 * inner product is split over 16 parts of fixed extent added as a balanced tree, no atomics.  A LOVE root and a FITC
 * mean are ignored, nothing of the GPs changes.
 * Asynchronous on `stream`, no host synchronisation: one launch for the start state and one per pick.  The handle's
 * scratch (the c columns [n_gp][m][capacity], p and the per-block bests) is allocated by the first call and again
 * when a capacity or m has grown, a synchronous setup step like gpmpc_gp_reserve; if that fails the call returns
 * GPMPC_ERR_NOMEM and the handle is unchanged.
 * Refused: m < 1, m >= n, m > 256, pick_dev NULL (GPMPC_ERR_ARG); a GP not set, set without Linv or a FITC upload,
 * GPs that differ in their row count (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_redundant(gpmpc_handle* h, int32_t m, int32_t* pick_dev, double* score_dev, int32_t* ok_dev,
                                void* stream);

/* gpmpc_preprocess followed by an append of the m rows to every GP of the handle, in one stream-ordered call:
 * the rows are staged per GP (X_g [m][d_g], y_g [m]) in scratch of the handle, which holds max_batch rows and is
 * allocated on first use (a synchronous setup step), and appended by gpmpc_gp_append's own launches.  With
 * evict_oldest = 1 and n + m above the capacity, exactly the excess is dropped first from every GP by
 * gpmpc_gp_drop_oldest's launches; at least one old row stays.  Afterwards the GPs are bit-identical to
 * gpmpc_preprocess, a slice of its outputs' columns per GP, gpmpc_gp_drop_oldest where needed and
 * gpmpc_gp_append, GP after GP, on the same handle state.  inputs_dev and targets_dev as for gpmpc_preprocess,
 * here both may be NULL: they are copies for the caller, who keeps the targets (the handle stores none).
 * accepted_dev: device int32 [n_gp][ceil(m/16)], per GP as gpmpc_gp_append reports; dropped_ok_dev: device int32
 * [n_gp][max(ceil(excess/16), 1)], per GP as gpmpc_gp_drop_oldest reports, 1 where nothing was dropped; both may
 * be NULL.  A row of NaN (a pick out of range, a non-finite transition) makes its block inert and reports 0, as
 * gpmpc_gp_append defines it.  No host synchronisation.
 * Refused before any GP changes: what gpmpc_preprocess refuses of its transitions, picks, dt_diff and gravity,
 * m > max_batch, n + m above the capacity without evict_oldest, an excess >= n with it (GPMPC_ERR_ARG); a call
 * before gpmpc_set_model, what gpmpc_gp_append refuses of any GP of the model -- not set, set without Linv, a FITC
 * upload, a LOVE root or a FITC mean installed --, where rows must be dropped no gpmpc_gp_reserve, and GPs that
 * differ in their row count or capacity (GPMPC_ERR_STATE). */
gpmpc_status gpmpc_gp_observe(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev,
                              const double* xnext_dev, int32_t m, const int32_t* pick_dev, double dt_diff,
                              double gravity, int32_t evict_oldest, double* inputs_dev, double* targets_dev,
                              int32_t* accepted_dev, int32_t* dropped_ok_dev, void* stream);

/* Launch shape of the SQP kernel (no reference counterpart: the reference solves one instance).
 *   waves     0 = auto: one wavefront per instance, or -- for the models whose stage fits one MFMA
 *             tile (quad2d, cartpole) -- four per instance when batch <= the device's compute units
 *             and two when batch <= twice that, so the SIMDs that would idle take the GP tile sums;
 *             1 / 2 / 4 force a count for quad2d / cartpole.  quad3d always runs four: it accepts
 *             0 or 4 and rejects any other count (GPMPC_ERR_ARG), so a setting never silently
 *             does nothing.
 * Results are identical up to floating-point rounding; a performance option. */
gpmpc_status gpmpc_set_launch(gpmpc_handle* h, int32_t waves);

/* What gpmpc_solve would run for `batch` instances with the current options (host, no device
 * work): waves per instance of the SQP launch, and overlapped = 1 when a step with a variance
 * launch runs as two overlapped halves (see gpmpc_solve).  With overlapped = 1 the profiling
 * events of gpmpc_kernel_times bracket the costlier half's variance launch ("variance") and the
 * span from its end to the join of both halves' SQP launches ("SQP", which also contains the
 * cheaper half's variance launch): spans of the step, not per-kernel durations.  overlapped = 2:
 * the tail boost of GPMPC_TUNE_TAIL applies (two SQP launches side by side, the "SQP" events
 * bracketing both; `waves` is then the other instances' one). */
gpmpc_status gpmpc_get_launch_info(gpmpc_handle* h, int32_t batch, int32_t* waves, int32_t* overlapped);

/* Horizon segments of the Newton solves gpmpc_solve would run for `batch` instances (host, no
 * device work): 1 = one wave runs each recursion over the whole horizon; 2 or 3 = the
 * segment-parallel solve of GPMPC_TUNE_SEG (two segments on two waves per instance, three on four). */
gpmpc_status gpmpc_get_launch_segments(gpmpc_handle* h, int32_t batch, int32_t* segments);

/* Performance switches (no reference counterpart; every output is bit-identical or identical up
 * to rounding whichever value is set, GPMPC_TUNE_SHIFT excepted -- A/B measurement knobs, all on
 * their default after gpmpc_create).  gpmpc_set_tuning(h, option, value):
 *   GPMPC_TUNE_LIN_CACHE   1 (default): the first SQP iteration of a step reads the stored
 *                          iterate's linearisation; 0: recompute it (bit-identical)
 *   GPMPC_TUNE_ORDER       1 (default): a launch needing more than one round of workgroups runs
 *                          its instances by decreasing previous cost; 0: instance order; 2: rank
 *                          every launch (bit-identical)
 *   GPMPC_TUNE_OVERLAP     1 (default): overlapped halves for multi-round steps; 0: sequential
 *   GPMPC_TUNE_VAR_SPLIT   0 (default): automatic; 1: one wave per 16-point tile of the
 *                          triangular variance kernel; 4: its four-wave column split
 *   GPMPC_TUNE_EVENT_FENCE 0 (default): profiling events without the system-scope fence;
 *                          1: default (fenced) events
 *   GPMPC_TUNE_SEG         1 (default): segment-parallel Newton solves when a launch runs two or
 *                          four waves per instance (quad2d, cartpole): the horizon's two (two
 *                          waves) or three (four waves) segments are factorised and swept on
 *                          different waves at once and joined by a chain over the boundaries;
 *                          0: one wave runs the whole recursion; identical up to rounding
 *   GPMPC_TUNE_TAIL        -1 (default): automatic, K = the SIMDs the launch leaves free (4 x CUs - B,
 *                          so 0 at B = 4 x CUs); 0: off; K > 0: fixed.  A step whose SQP launch gives
 *                          every instance one wave in one round of workgroups (quad2d, cartpole; batch
 *                          between 2 and 4 x CUs, waves automatic, segments on) runs its K costliest
 *                          instances (by the cost of their previous solve) as two-wave segment solves
 *                          on the caller's stream, beside the other instances' one-wave launch on a
 *                          second stream; identical up to rounding (each instance's arithmetic is that of
 *                          its launch shape).  The SQP profiling events then bracket both launches
 *   GPMPC_TUNE_SEG_PIVOT   10 (default): the segment solve's boundary chain refuses a pivot below
 *                          10^-value x Ph's largest diagonal entry and redoes that Newton solve as
 *                          the one-segment recursion; -1: refuses every pivot (every segment solve
 *                          takes that fallback: a test of it)
 *   GPMPC_TUNE_SHIFT       0 (default): every solve starts from the stored iterate and multipliers
 *                          at the same stage index; 1: one-stage shifted warm start.  An instance
 *                          whose previous gpmpc_solve ended good (status 0 or 2) at reference index
 *                          t and whose tstep now equals (t + 1) mod L starts its SQP from stage
 *                          min(k + 1, last) of the stored x, u, dynamics and bound multipliers (the
 *                          terminal stage duplicated, not rolled out), the window its reference has
 *                          moved to.  Every other instance -- first solve, after gpmpc_reset or
 *                          gpmpc_set_iterate, after a failed solve, a repeated or jumped tstep --
 *                          runs exactly as with 0.  Only the SQP's start point moves: the tightening,
 *                          its variance launch and gpmpc_get_solution read the unshifted stored
 *                          solution, so each step's NLP is unchanged.  Outputs are NOT identical up
 *                          to rounding under this option: the converged solution agrees with the
 *                          unshifted one to the solver tolerance and the iteration path (sqp_iter,
 *                          qp_iter, a status-2 iterate) differs.  A shifted solve recomputes its
 *                          first linearisation (the cache holds no row for the duplicated last
 *                          stage).  Any other value: GPMPC_ERR_ARG
 *   GPMPC_TUNE_VAR_TRIM    1 (default): the one-wave triangular variance kernel (N <= 256) carries a
 *                          last 16-column tile with at most 8 real columns (N mod 16 in 1..8 for
 *                          every GP of the launch) on one or two four-column MFMA quads and skips
 *                          that tile's zero rows; 0: the whole padded tile is multiplied.  The
 *                          skipped products are exact zeros; the variances agree to rounding (the
 *                          order of additions differs) */
enum {
    GPMPC_TUNE_LIN_CACHE = 0,
    GPMPC_TUNE_ORDER = 1,
    GPMPC_TUNE_OVERLAP = 2,
    GPMPC_TUNE_VAR_SPLIT = 3,
    GPMPC_TUNE_EVENT_FENCE = 4,
    GPMPC_TUNE_SEG = 5,
    GPMPC_TUNE_TAIL = 6,
    GPMPC_TUNE_SEG_PIVOT = 7,
    GPMPC_TUNE_SHIFT = 8,
    GPMPC_TUNE_VAR_TRIM = 9
};
gpmpc_status gpmpc_set_tuning(gpmpc_handle* h, int32_t option, int32_t value);

/* Optional device buffer [max_batch][H+1] (float64) receiving, on every gpmpc_solve, the stage
 * costs of each instance's new solution: the acados LINEAR_LS cost 1/2 ||y_k - y_ref,k||^2_W with
 * W = blkdiag(Q, R) scaled by dt on stages 0..H-1 and W_e = Q unscaled on stage H
 * (gpmpc/gpmpc.py:231-239, gpmpc/mpc.py:101-102, acados cost_scaling), y_k = [x_k; u_k],
 * y_ref,k = [reference window; u_eq].  Their sum is the objective value acados reports ("cost").
 * A solve that ends with any status other than 0 or 2 (a failed solve: its x, u hold the previous
 * solution) writes NaN.  NULL disables (default). */
gpmpc_status gpmpc_set_cost_buffer(gpmpc_handle* h, void* cost_dev);

/* Kernel timing with HIP events recorded on the solve stream around the variance kernel
 * and the SQP kernel of every gpmpc_solve while enabled.  gpmpc_kernel_times synchronises
 * on the recorded events, returns the summed milliseconds and launch counts, and clears them.
 * gpmpc_kernel_time_list returns the per-launch milliseconds instead (host arrays of capacity
 * `cap`; n_var / n_sqp receive the counts, at most cap are written) and clears them.
 * Replaces the perf_counter around select_action, scripts/run_gp_mpc.py:55-57. */
gpmpc_status gpmpc_set_profiling(gpmpc_handle* h, int32_t enabled);
gpmpc_status gpmpc_kernel_times(gpmpc_handle* h, double* var_ms, int32_t* n_var, double* sqp_ms, int32_t* n_sqp);
gpmpc_status gpmpc_kernel_time_list(gpmpc_handle* h, int32_t cap, double* var_ms, int32_t* n_var, double* sqp_ms,
                                    int32_t* n_sqp);

/* Diagnostic builds (-DGPMPC_TIMING) only: device buffer [max_batch][12] (uint64) receiving
 * per-phase shader-clock cycles of each instance's last solve; NULL disables. */
gpmpc_status gpmpc_set_timing_buffer(gpmpc_handle* h, void* timing_dev);

/* Optional device buffer [max_batch][GPMPC_STATS_SLOTS] (int64) of running solver statistics,
 * accumulated by the SQP kernel on every gpmpc_solve: [0] SQP iterations, [1] QP (IPM) iterations, [2 + s] number
 * of solves that ended with status s (0..4), [7] largest SQP iteration count of one solve,
 * [8] largest QP iteration total of one solve, [9] linearisations computed (the first SQP
 * iteration of a step reads the stored iterate's linearisation when it is valid), [10] the
 * instance's solve time inside the SQP kernel in s_memrealtime ticks (the 100 MHz constant clock:
 * 10 ns; from the instance's first to its last instruction, summed over solves), [11] the last
 * solve's time in ticks (the slot holds the start stamp while the solve runs).  The slowest instance's time against the kernel's duration is the
 * latency-bound figure of bench.py's roofline block.  The caller
 * zeroes it; NULL disables (default).  `slots` is the caller's row stride in int64: it must
 * equal GPMPC_STATS_SLOTS (a buffer laid out for another slot count is rejected, not
 * overrun).
 * Replaces reading acados' per-solve "sqp_iter" / "qp_iter" / status stats in a host loop. */
enum { GPMPC_STATS_SLOTS = 12 };
gpmpc_status gpmpc_set_stats_buffer(gpmpc_handle* h, void* stats_dev, int32_t slots);

/* LDS bytes one instance's workgroup needs (capacity planning / tests). */
int64_t gpmpc_lds_bytes(int32_t model_id, int32_t horizon);

/* Build provenance (host, static string): "src=<sha256 of the library's sources, 16 hex digits>
 * git=<commit at build time>[+dirty] kind=<product|timing>".  The Python binding recomputes the
 * source hash from the tree and refuses an in-tree library built from other sources. */
const char* gpmpc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
