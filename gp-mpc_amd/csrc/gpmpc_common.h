// Shared host/device definitions for the MI355X GP-MPC solve path.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

namespace gpmpc {

constexpr int kMaxGP = 4;       // GPs per model (quad3d: 3)
constexpr int kMaxGPDim = 3;    // inputs per GP (packed rows are 4 doubles: x0,x1,x2,alpha)
constexpr int kMaxNX = 12;
constexpr int kMaxNU = 4;
constexpr int kMaxH = 63;       // one lane per stage 0..H (64-lane wavefront)
constexpr int kPhases = 15;  // diagnostic phase slots (GPMPC_TIMING builds; sqp_kernel.hip TPHASE)
constexpr int kMaxParams = 16;
constexpr int kStatsSlots = 12;  // per-instance solver statistics (gpmpc_set_stats_buffer, = GPMPC_STATS_SLOTS)
// Floor of the IPM's slacks after a step (HPIPM's t_min; oracle/cpu_ref.cpp has the same).  With a
// bound active, the 0.995 steps can take a slack to 1e-14 while the other QP residuals are still above
// a 1e-11 tolerance; Sigma = lam / s then passes 1e12, the Riccati recursion cancels every digit of the
// cost-to-go, Huu loses definiteness and a feasible QP ends as status 4.
constexpr double kSlackMin = 1e-12;

enum ModelId : int32_t { kQuad2D = 0, kQuad3D = 1, kCartpole = 2 };

// acados status codes (acados_c/ocp_nlp_interface.h) -- gpmpc/gpmpc.py:365
enum SolveStatus : int32_t { kSuccess = 0, kNaN = 1, kMaxIter = 2, kMinStep = 3, kQPFailure = 4 };

// One GP replica in device memory.
struct GPDev {
    const double* rows;   // [n][4]: mean inputs (d <= 3, zero padded) + weight alpha = K^-1 y (gpmpc/gp.py:84-85)
                          //         (FITC: inducing inputs + posterior weights, gpmpc/gpmpc.py:377-400)
    const double* vrows;  // [nv][4]: training inputs of the variance GP (== rows for an exact GP)
    const double* linvT;  // [npad][npad] row-major (L^-1)^T, L = chol(K); NULL -> no variance
    // MFMA tile pack of the mean rows (the SQP linearisation's GP sums, sqp_kernel.hip gp_tiles):
    //   tX[t][16][4]     rows [(x_i - xbar)/ell^2 (zero padded to 3 dims), c|x_i - xbar|^2],
    //                    c = -1/(2 ell^2); rows past n are zero
    //   tW[t][4][4][4]   for lane group g and output column j: {W[i][j], i = 16t+g+4r, r = 0..3},
    //                    W[i] = [alpha_i, alpha_i (x_i - xbar)]
    const double* tX;
    const double* tW;
    int32_t ntile;
    double xbar[3];       // centre of the mean rows (the RBF kernel is shift invariant)
    int32_t n;
    int32_t nv;
    int32_t d;
    // LOVE root (gpytorch fast_pred_var, gpmpc/gpmpc.py:442-444): [npad][vroot_cols] row-major,
    // R R^T ~ (K + sn2 I)^-1; when set, the variance is sf2 - ||R^T k||^2 instead of the exact
    // triangular form (set only in the tightening's variance launch).  NULL: exact.
    const double* vroot;
    int32_t vroot_cols;   // padded to 16
    int32_t vroot_rank;   // the root's columns before padding
    double inv_ell2;      // 1 / lengthscale^2 (isotropic RBF, gpmpc/gp.py:34)
    double sf2;           // outputscale
    double sn2;           // likelihood noise (gpmpc/gp.py:31)
};

// Everything the per-step kernels need, passed by value.
struct ProblemDev {
    int32_t model;
    int32_t nx, nu, H;
    int32_t n_gp;
    int32_t use_gp;           // 0: nominal MPC (gpmpc/mpc.py)
    double dt;
    double cost_scale;        // acados cost_scaling for stages 0..H-1 (time step), 1 for terminal
    double uh;                // h <= uh: -1e-8 GPMPC (gpmpc.py:309-314), +1e-8 MPC (mpc.py:157-162)
    double params[kMaxParams];
    double x_lo[kMaxNX], x_hi[kMaxNX], u_lo[kMaxNU], u_hi[kMaxNU];
    double q[kMaxNX], r[kMaxNU], u_eq[kMaxNU];
    // reference trajectory (nx, L) column-major by time: traj[t * nx + i]   (gpmpc.py:509-514)
    const double* traj;
    int32_t traj_len;
    // tightening (gpmpc.py:425-498)
    int32_t tighten;
    double icdf;
    double Acl[kMaxNX * kMaxNX];   // A_d + B_d K_lqr (the four-term update of gpmpc.py:489-495)
    double K[kMaxNU * kMaxNX];     // K_lqr
    // diag of Sigma_k and K Sigma_k K^T as a convolution of the per-stage GP noise (Sigma_0 = 0,
    // Sigma_{k+1} = Acl Sigma_k Acl^T + Bd D_k Bd^T with D_k diagonal):
    //   tgain[m][v][q] = (Acl^m Bd)_{vq}^2 (v < nx),  (K Acl^m Bd)_{v-nx,q}^2 (v >= nx),  m = 0..H-1
    const double* tgain;
    // SQP / QP options (gpmpc.py:257-263; acados default tolerances)
    int32_t max_iter, qp_max_iter;
    double tol_stat, tol_eq, tol_ineq, tol_comp, qp_tol, qp_mu0;
    // linearisation cache generation: bumped by every host call that changes what the
    // linearisation depends on (iterate, GPs, model parameters, GP switch); 0 disables the cache
    int32_t lin_gen;
    // launch shape of the SQP kernel: waves per instance (0: auto -- four when batch <= n_cu for the
    // single-tile models, sqp_kernel.hip sqp_waves)
    int32_t waves;
    int32_t n_cu;             // compute units of the device (set by gpmpc_create)
    // cost-ordered dispatch (StateDev::order): on when a launch has more instances than the
    // device holds at once (gpmpc_set_tuning GPMPC_TUNE_ORDER: 0 off, 2 ranks every launch)
    int32_t order_dispatch;
    // segment-parallel Newton solves when the launch runs two or four waves per instance (single-tile
    // models; gpmpc_set_tuning GPMPC_TUNE_SEG)
    int32_t seg;
    // the boundary chain's pivot threshold relative to Ph's largest diagonal entry (gpmpc_set_tuning
    // GPMPC_TUNE_SEG_PIVOT): below it the solve falls back to the one-segment recursion
    double seg_piv_rel;
    // one-stage shifted warm start (gpmpc_set_tuning GPMPC_TUNE_SHIFT): an instance whose previous
    // solve ended good at reference index t_prev starts this one, at tstep = t_prev + 1 (mod
    // traj_len), from the stored iterate and multipliers moved up one stage (StateDev::t_prev)
    int32_t shift;
    GPDev gp[kMaxGP];
};

// Per-instance state owned by the handle (acados keeps the same in its memory).
struct StateDev {
    double* x;        // [B][H+1][nx] iterate / previous solution (x_prev)
    double* u;        // [B][H][nu]
    double* pi;       // [B][H][nx]  dynamics multipliers
    double* lam;      // [B][H+1][2*nb] bound multipliers (lower | upper), nb = nx+nu
    int32_t* has_prev;   // [B] previous solution valid -> tighten (gpmpc.py:432-433)
    const double* var;   // [B][H][n_gp] GP variances at the previous solution (incl. noise)
    double* tight;       // [B][H+1][2*nb] tightening values (state lo|hi, input lo|hi), optional
    // Linearisation of the stored iterate (x, u above): [B][H][nx][nb+1], per stage the rows of
    // [A_k B_k | F_k] with F_k = RK4(x_k, u_k), written by the step that produced the iterate.
    // The next step's first SQP iteration linearises at exactly that iterate (acados keeps it as
    // the initial guess), so it reads the rows instead of recomputing them when lin_tag[b] equals
    // ProblemDev::lin_gen.  Optional (NULL: always recompute).
    double* lin;
    int32_t* lin_tag;    // [B]
    // Cost-ordered dispatch.  cost[b]: the work of instance b's last solve, SQP iterations and IPM
    // iterations weighted by their measured cycle ratio (written by every SQP launch, optional;
    // in-kernel timestamps cost the single-wave kernel 48 B/lane of scratch).  order[blockIdx.x] = instance: when a launch needs more than one
    // round of workgroups (config 5: 512 instances, one per CU), launch_sqp fills order[] with the
    // instances by decreasing previous cost, so the dispatcher starts the slowest instances first
    // and the fast ones fill in behind them (longest-processing-time-first; an instance's cost
    // barely changes from one control step to the next).  NULL: identity.
    const int32_t* order;
    uint32_t* cost;      // [B]
    // rank of this launch's first workgroup in order[] (a launch over ranks first .. first + grid - 1:
    // the two halves of an overlapped step, capi.hip gpmpc_solve); 0 otherwise
    int32_t first;
    // reference index (tstep mod traj_len) of the instance's last solve when it ended good, -1 after
    // a failed one, a reset or gpmpc_set_iterate: the eligibility test of ProblemDev::shift.  [B]
    int32_t* t_prev;
};

struct StepIO {
    const double* x0;        // [B][nx]
    const int32_t* tstep;    // [B] reference index
    double* u0;              // [B][nu] out
    int32_t* status;         // [B] out
    int32_t* sqp_iter;       // [B] out
    int32_t* qp_iter;        // [B] out, total IPM iterations
    double* res;             // [B][4] out, final NLP residuals (stat, eq, ineq, comp)
    unsigned long long* timing;  // [B][kPhases] phase cycles (GPMPC_TIMING builds only), may be null
    long long* stats;            // [B][kStatsSlots] sqp iters, qp iters (sums), status 0..4 counts,
                                 // max sqp iters, max qp iters per solve, linearisations
                                 // computed, the instance's solve time in s_memrealtime ticks
                                 // (sum; the last solve's); may be null
};

// Arguments of the GP posterior kernel (gp_kernels.hip).
struct PostArgs {
    // points: either dense Z[P][ldz] (first d columns), or gathered from the solver state
    const double* Z;
    int32_t ldz;
    const double* sx;     // state x [B][H+1][nx]
    const double* su;     // state u [B][H][nu]
    int32_t H, nx, nu, ngp, gp_index;
    int32_t src[3];       // var input map into z = [x; u] (gpmpc.py:437-444)
    int32_t P;            // number of points
    int32_t d;
    int32_t with_noise;
    double* mean;         // [P] or null
    double* var;          // var[p * var_stride + var_off] or null
    int32_t var_stride, var_off;
    // gathered points only: point p is stage p % H of the instance of rank first + p / H in order[]
    // (var row: that instance's), or of instance p / H when order is null
    const int32_t* order;
    int32_t first;
};

// var row of point p (see PostArgs::order)
__device__ __forceinline__ size_t post_row(const PostArgs& a, int p) {
    if (a.order == nullptr) return (size_t)p;
    const int r = p / a.H;
    return (size_t)a.order[a.first + r] * a.H + (p - r * a.H);
}

// exp(x) for the RBF kernel, total on x <= 0 (-inf included): Cody-Waite reduction x = n ln2 + r,
// |r| <= ln2/2, degree-11 Chebyshev fit of exp on [-ln2/2, ln2/2] (mpmath chebyfit, fit error
// 3.2e-18; max relative error of this f64 evaluation 1 ulp on a 2e5-point grid), scale by 2^n.
// n comes from the magic-number rounding t = x log2(e) + 1.5 2^52 (one fma; the low word of t is
// n in two's complement) and 2^n is applied by an integer add to the exponent field of p, so the
// f64 work is 15 operations instead of 17 (rint, cvt and ldexp gone).  The argument is clamped
// first, so that n >= -1022 always: without a clamp the low word of t wraps below
// -2^31 ln2 = -1.49e9 (a query 1.1e4 lengthscales from a training row) and the exponent add returns
// huge or negative values.  The clamp is one 32-bit integer operation on the high word of x
// (exp_rbf_clamp: a negative double's magnitude grows with its high word read as unsigned), in
// place of the integer max(n, -1022) the scaling had before, so the operation count is the same.
// It heads the dependent chain, where that max sat beside it: the headline benchmark measured
// 0.7 % slower with it (2.790 -> 2.769 M), and 1.2 % slower with an f64 max(x, -1022 ln2) instead.
// An argument whose high word exceeds kExpRbfHiMin, i.e. x < -708.39648 (-inf and negative NaNs
// included), takes that high word and keeps its low word: it lands in [-708.39698, -708.39648],
// where n = -1022 and p < 1, and gives about 2^-1022 (2.2e-308) instead of a denormal or 0.
// Every x >= -708.39648, which includes all x >= -1022 ln2 = -708.39642, is untouched and gives
// what the routine gave before, bit for bit; below exp(-708.2) the result is under 3e-308 but not
// correctly rounded.
// No overflow / positive-NaN guards: the argument is -0.5 q/ell^2 (or its centred expansion, which
// can round a few ulp above 0).
constexpr unsigned kExpRbfHiMin = 0xC086232Cu;   // high word of -708.396484375 (one step past -1022 ln2's)
__device__ __forceinline__ double exp_rbf_clamp(double x) {
    return __hiloint2double((int)min((unsigned)__double2hiint(x), kExpRbfHiMin), __double2loint(x));
}
__device__ __forceinline__ double exp_rbf(double x) {
    constexpr double kMagic = 6755399441055744.0;   // 1.5 * 2^52
    x = exp_rbf_clamp(x);
    const double t = fma(x, 1.4426950408889634, kMagic);
    const double n = t - kMagic;
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 2.5110037605963777e-08;
    p = fma(p, r, 2.763263963904103e-07);
    p = fma(p, r, 2.755724091857897e-06);
    p = fma(p, r, 2.4801485482328494e-05);
    p = fma(p, r, 0.00019841269890047113);
    p = fma(p, r, 0.0013888888952314775);
    p = fma(p, r, 0.008333333333319601);
    p = fma(p, r, 0.0416666666664881);
    p = fma(p, r, 0.1666666666666668);
    p = fma(p, r, 0.5000000000000019);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return __hiloint2double(__double2hiint(p) + (__double2loint(t) << 20), __double2loint(p));
}

// exp_rbf of K independent arguments, written step by step across the K values.  One wave
// issues an f64 VALU operation every ~5.5 cycles whether or not it depends on the previous one,
// but a dependent one waits ~7.3 (tools/probe_f64.hip): the compiler schedules back-to-back
// exp_rbf calls as K serial 15-deep chains (124 cycles per exp), the interleaved form runs at
// the issue rate (94 cycles per exp with K = 8).  Same operations, same results as exp_rbf.
template <int K>
__device__ __forceinline__ void exp_rbf_n(double (&x)[K]) {
    constexpr double kMagic = 6755399441055744.0;   // 1.5 * 2^52
    constexpr double c[12] = {2.5110037605963777e-08, 2.763263963904103e-07, 2.755724091857897e-06,
                              2.4801485482328494e-05, 0.00019841269890047113, 0.0013888888952314775,
                              0.008333333333319601, 0.0416666666664881, 0.1666666666666668,
                              0.5000000000000019, 1.0, 1.0};
    double t[K], r[K], p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = exp_rbf_clamp(x[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = fma(x[k], 1.4426950408889634, kMagic);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = fma(t[k] - kMagic, -6.93147180369123816490e-01, x[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = fma(t[k] - kMagic, -1.90821492927058770002e-10, r[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = fma(c[0], r[k], c[1]);
#pragma unroll
    for (int i = 2; i < 12; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = fma(p[k], r[k], c[i]);
#pragma unroll
    for (int k = 0; k < K; ++k)
        x[k] = __hiloint2double(__double2hiint(p[k]) + (__double2loint(t[k]) << 20), __double2loint(p[k]));
}

// sum over the 16 lanes of a DPP row (lanes 16i .. 16i + 15), left in each of them (the variance kernels of
// gp_kernels.hip and sqp_kernel.hip rollout_sample_kernel: the squared norms over the column lanes)
__device__ __forceinline__ double dpp_row_sum(double v) {
    auto mv = [](double x, auto ctrl) {
        const long long b = __double_as_longlong(x);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, decltype(ctrl)::value, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), decltype(ctrl)::value, 0xf, 0xf, false);
        return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    };
    v += mv(v, std::integral_constant<int, 0x128>{});   // row_ror:8
    v += mv(v, std::integral_constant<int, 0x124>{});   // row_ror:4
    v += mv(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
    v += mv(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
    return v;
}

// Up to kMaxGP posterior evaluations in one launch (grid.y = GP).
struct PostBatch {
    GPDev g[kMaxGP];
    PostArgs a[kMaxGP];
    int32_t npad[kMaxGP];
    int32_t n;
    // points of the whole step when this launch is one part of it (the overlapped halves): the
    // kernel choice follows the step, so both halves use the kernel a single launch would (0: P)
    int32_t step_points;
    // triangular variance kernel's column split (GPMPC_TUNE_VAR_SPLIT): 0 automatic, 1 or 4 forced
    int32_t var_split;
    // 1: the triangular variance kernel multiplies its ragged last column tile in full
    // (GPMPC_TUNE_VAR_TRIM = 0); 0: on four-column quads where at most 8 of its columns are real
    int32_t var_full;
};

// One block of m <= 16 rows appended to an exact GP (gp_append.hip; gpmpc_gp_append fills it per block).
struct GPAppend {
    double* rows;         // [>= npad][4], GPDev::rows (rows past n0 are zero)
    double* tX;           // GPDev::tX / tW (capacity-sized regions)
    double* tW;
    double* linvT;        // [npad][npad], the factor at the stride this block leaves it with
    int32_t npad;         // n0 + m rounded up to 16
    int32_t n0;           // rows before the block
    int32_t m;            // rows of the block
    int32_t d;
    double xbar[3];       // the tile pack's centre (unchanged by appends)
    double inv_ell2, sf2, sn2;
    const double* Xnew;   // [m][d] (device)
    const double* ynew;   // [m]
    // scratch of the GP: W^T [16][ldw], per-tile means at X_b [ntile][16], L_b^-1 [16][16], beta [16],
    // the block's status (1 accepted, 0 written as inert rows)
    double* wt;
    int32_t ldw;
    double* pmean;
    double* lbinv;
    double* beta;
    int32_t* flag;
    int32_t* accepted;    // the caller's status word of this block, may be null
};

// One block of m <= 16 oldest rows dropped from an exact GP (gp_drop.hip; gpmpc_gp_drop_oldest fills it
// per block).  The factor moves from src to dst (the GP's two factor buffers); rows / tX / tW are read
// in place and their shifted successors written to a staging region the caller copies back.
struct GPDrop {
    const double* src;    // [npad0][npad0], the factor before the block
    double* dst;          // [npad1][npad1], the factor after it: written in full, zeros included
    const double* rows;   // GPDev::rows / tX before the block
    const double* tX;
    double* srows;        // staging: rows [npad1][4], tX [npad1/16][64], tW [npad1/16][64]
    double* stX;
    double* stW;
    int32_t npad0;        // n0 rounded up to 16
    int32_t npad1;        // n0 - m rounded up to 16
    int32_t n0;           // rows before the block
    int32_t m;            // rows dropped (m < n0)
    int32_t d;
    double xbar[3];       // the tile pack's centre (unchanged by drops)
    // scratch of the GP: V^T [16][ldv], M21 g [ldv], E_T and D_T [npad1/16][16][16] each, the block's
    // status (1: every pivot finite and positive)
    double* vt;
    int32_t ldv;
    double* w;
    double* et;
    double* dt;
    int32_t* flag;
    int32_t* ok;          // the caller's status word of this block, may be null
    // gpmpc_gp_drop_rows only (null: the m oldest rows).  didx: the block's m rows, ascending, indices into the rows
    // before the block (device); w then holds M[:, D] g over all npad0 old rows.  acc: the call's running status
    // (gp_drop_prep_kernel starts it); ok then receives acc & flag, one word for the whole call.
    const int32_t* didx;
    int32_t* acc;
};

// The row set of gpmpc_gp_drop_rows (gp_drop.hip), made ascending on the device: the distinct indices of idx within
// 0 .. n-1, filled up to m with the lowest rows not among them.  acc = 1 when idx held m distinct indices in range.
struct GPDropPrep {
    const int32_t* idx;   // [m] the caller's indices (device)
    int32_t n, m;         // 1 <= m < n
    int32_t* mask;        // [n] scratch
    int32_t* sorted;      // [m] the rows dropped, ascending
    int32_t* dropped;     // [m] the caller's copy, may be null
    int32_t* acc;
};

// Rows per workgroup of the pick loop that GPRedundant, GPSelect and GPInducing below run (gp_pick.h): the unit of
// their nblk and of the scratch layouts capi.hip carves for them
constexpr int kPickBlock = 16;
// Greedy backward selection of the m rows the GPs would miss least (gp_drop.hip; gpmpc_gp_redundant fills it): a
// pivoted partial Cholesky of the precisions P_g = M_g^T M_g, whose entries are inner products of rows of linvT.
constexpr int kRedundantMaxPicks = 256;
struct GPRedundantGP {
    const double* linvT;  // [npad][npad]
    double* ccol;         // [m][ldn]: c_t[i]
    int32_t npad;
    double sf2, sn2;
};
struct GPRedundant {
    int32_t n, m, n_gp;
    int32_t ldn;          // stride of the per-row arrays (>= n)
    int32_t nblk;         // ceil(n / kPickBlock)
    GPRedundantGP g[kMaxGP];
    double* p;            // [2][n_gp][ldn]: step t reads half t & 1 and writes the other
    int32_t* state;       // [ldn]: 1 picked
    double* bval;         // [2][nblk]: each block's smallest finite score among its unpicked rows
    int32_t* bidx;        // [2][nblk][2]: its index (INT_MAX: none), the block's lowest unpicked row with a non-finite score
    int32_t* pick;        // [m]
    double* score;        // [m] or null
    int32_t* ok;          // [1] or null
};

// A from-scratch factorisation of an exact GP from its device-resident rows (gp_refactor.hip;
// gpmpc_gp_refactor fills it).  Khat and its factor are built in A, the GP's spare factor buffer; the
// live one receives (L^-1)^T in full, zeros included, at the stride it has.
struct GPRefactor {
    double* rows;         // [>= npad][4], GPDev::rows: inputs read, rows[.][3] rewritten
    double* tX;           // GPDev::tX / tW (capacity-sized regions), rewritten for the new lengthscale
    double* tW;
    double* linvT;        // [npad][npad], the live factor: its diagonal is read for the inert mask first
    double* A;            // [npad][npad] work space (the second factor buffer)
    const double* y;      // [n] targets in row order (device); inert rows' entries are not read into sums
    int32_t npad;         // n rounded up to 16 (unchanged)
    int32_t n;
    int32_t d;
    double xbar[3];       // the tile pack's centre (unchanged)
    double inv_ell2, sf2, sn2;   // the hyperparameters the GP is left with
    // scratch of the GP: L_kk^-1 [npad/16][16][16], w = L^-1 y [npad], the targets with the inert rows'
    // zeroed [npad], the inert mask [npad], the status
    double* dinv;
    double* w;
    double* ym;
    int32_t* mask;
    int32_t* flag;
    int32_t* ok;          // the caller's status word, may be null
};

// The marginal log likelihood of an exact GP and its gradient from the factor the handle holds, and the
// hyperparameter fit built on it (gp_fit.hip; gpmpc_gp_mll and gpmpc_gp_fit fill it).  Nothing of the GP
// is written through it.
struct GPFit {
    const double* rows;   // [>= npad][4], GPDev::rows: inputs and alpha = rows[.][3]
    const double* linvT;  // [npad][npad], the live factor (a zero on its diagonal: an inert or padding row)
    const double* y;      // [n] targets in row order (device); inert rows' entries are not read into sums
    int32_t npad;
    int32_t n;
    double* part;         // [nt (nt + 1) / 2][3], nt = npad / 16: the tiles' partial sums, tile (I, J) at I (I + 1) / 2 + J
    double* state;        // the fit-state block (kFit* below)
};
// The fit-state block, in doubles: raw parameters, Adam's moments, its step count (= iterations done),
// the last loss, the stop and fail flags, the constrained hyperparameters the next factorisation reads
// {1 / ell^2, sf2, sn2, ell} and the last evaluation {MLL / n_live, d/d ell, d/d sf2, d/d sn2}
enum : int { kFitRaw = 0, kFitM = 3, kFitV = 6, kFitStep = 9, kFitLast = 10, kFitStop = 11, kFitFail = 12,
             kFitHyp = 16, kFitOut = 20, kFitDoubles = 24 };

// The LOVE variance root of an exact GP built on the device (gp_love.hip; gpmpc_gp_love_root fills it): Lanczos
// with full reorthogonalisation on Khat, generated into A, and the bidiagonal root of its tridiagonal matrix.
// Nothing of the GP is written through it.
constexpr int kLoveMaxRank = 256;
struct GPLove {
    const double* rows;   // [>= npad][4], GPDev::rows: the inputs
    const double* linvT;  // [npad][npad], the live factor (a zero on its diagonal: an inert or padding row)
    double* A;            // [npad][npad] work space (the second factor buffer): Khat in full
    const double* q0;     // [n] the start vector (device); inert rows' entries are not read into sums
    int32_t npad;         // n rounded up to 16
    int32_t n;
    int32_t ld;           // the padded capacity: stride of Qt's columns
    int32_t rank;         // the rank asked for, 1 .. kLoveMaxRank (the iterations stop at min(rank, live rows))
    double inv_ell2, sf2, sn2;
    // scratch of the GP: Q transposed [kLoveMaxRank][ld], v [ld], the inert mask [ld], the parts of alpha_j
    // [ld / 16], of Q^T v (two buffers, [ceil(ld / 64)][256] each), of |v|^2 [ceil(ld / 64)] and of the live-row
    // count [ceil(ld / 256)], alpha, beta, the bidiagonal factor's diagonal and subdiagonal [kLoveMaxRank] each
    // and the state words (kLove* below)
    double* qt;
    double* v;
    int32_t* mask;
    double* apart;
    double* cpa;
    double* cpb;
    double* npart;
    double* ipart;
    double* alpha;
    double* beta;
    double* cd;
    double* lsub;
    int32_t* state;
};
// The state words: finished (kernels queued later do nothing), the root's rank m, 1 when every pivot was finite
// and positive, the iteration cap min(rank, live rows), the live rows
enum : int { kLoveDone = 0, kLoveM = 1, kLoveOk = 2, kLoveKmax = 3, kLoveLive = 4, kLoveInts = 8 };

// The FITC inducing-point mean of an exact GP built on the device (gp_fitc.hip; gpmpc_gp_fitc fills it): the
// weights of the M inducing rows S = X[idx] from the training rows, the targets and the current hyperparameters.
// Nothing of the GP is written through it: the result goes to staged rows and tiles the caller installs.
struct GPFitc {
    const double* rows;   // [>= npad][4], the training rows (the slot's exact rows): the inputs
    const double* linvT;  // [npad][npad], the live factor (a zero on its diagonal: an inert or padding row)
    const double* y;      // [n] targets in row order (device); inert rows' entries are not read into sums
    const int32_t* idx;   // [M] the inducing rows' indices (device)
    double* V;            // [mpad][npad] work space (the second factor buffer): L^-1 k(S, X)
    int32_t npad;         // n rounded up to 16
    int32_t n;
    int32_t mpad;         // M rounded up to 16
    int32_t M;
    int32_t d;
    double xbar[3];       // the tile pack's centre (the GP's own)
    double inv_ell2, sf2, sn2, jitter;
    // work space of the call: K_ss + jitter I and L, then B and C [mpad][mpad]; (L^-1)^T and (C^-1)^T [mpad][mpad]
    // each; the diagonal tiles' inverses [mpad/16][256]; Gamma^-1 and Gamma^-1 y [npad] each; u, p, q [mpad] each;
    // the inert mask of the training rows [npad], the padding mask of the inducing rows [mpad], the status
    double* A;
    double* lt1;
    double* lt2;
    double* dinv;
    double* ginv;
    double* t;
    double* u;
    double* p;
    double* q;
    int32_t* lmask;
    int32_t* smask;
    int32_t* flag;
    // staged result: rows [mpad][4] (inputs, weight), tX, tW [mpad/16][64] each, the indices [mpad]
    double* srows;
    double* stX;
    double* stW;
    int32_t* sidx;
};

// Transitions (x, u, x_next) turned into GP training rows (gp_observe.hip; gpmpc_preprocess, gpmpc_gp_informative
// and gpmpc_gp_observe fill it): output row r comes from transition pick[r] (r when pick is null).  Every output may
// be null; with targets, Xg and yg all null, xnext is not read (the inputs alone: gpmpc_gp_informative).
struct GPObserve {
    int32_t model;
    double params[kMaxParams];   // the prior's (ProblemDev::params)
    int32_t P, m;                // transitions, output rows
    const double* x;             // [P][nx]
    const double* u;             // [P][nu]
    const double* xnext;         // [P][nx]
    const int32_t* pick;         // [m] or null; an entry outside 0 .. P-1 reads nothing and gives a NaN row
    double dt_diff, gravity;
    double* inputs;              // [m][sum d_g]
    double* targets;             // [m][n_gp]
    double* Xg[kMaxGP];          // per GP [m][d_g]: the same values, contiguous (what gpmpc_gp_append reads)
    double* yg[kMaxGP];          // per GP [m]
};

// Launchers (sqp_kernel.hip, gp_kernels.hip, gp_append.hip, gp_drop.hip, gp_refactor.hip, gp_fit.hip, gp_love.hip,
// gp_fitc.hip, gp_observe.hip; what the six before the last share, the tile pack's layout included, is in gp_tile.h).
hipError_t launch_gp_observe(const GPObserve& a, hipStream_t stream);
// score[i] = max_g var[g * ldv + i] / sf2[g] over n_gp GPs (a NaN among them gives NaN), and NaN for a point with a
// non-finite GP input (the variance kernels' exponential is defined for finite arguments only: what they return for
// such a point is unspecified); then pick[rank_i] = i for rank_i < m, rank_i the number of points that beat i: a
// finite score beats a non-finite one, a larger finite one a smaller, and otherwise the lower index wins.
struct GPRank {
    const double* Z;      // [P][ldz] the points' gathered GP inputs
    int32_t ldz;
    const double* var;    // [n_gp][ldv]
    int32_t ldv, n_gp;
    double sf2[kMaxGP];
    int32_t P, m;
    double* score;        // [P] scratch
    double* score_out;    // [P] the caller's copy, may be null
    int32_t* pick;        // [m]
};
hipError_t launch_gp_score_rank(const GPRank& a, hipStream_t stream);
// Greedy conditional-variance selection of m of P candidates (gp_observe.hip; gpmpc_gp_select fills it): a pivoted
// partial Cholesky of the candidates' posterior covariance, every GP conditioned on each pick observed with its
// likelihood noise.  var0 holds the start variances d_g,i (the variance launches' own output); everything else is
// scratch of the handle.  Candidate i's entries of V, of the l columns and of d lie at [.][i] with stride ldp, so the
// pick loop reads them coalesced over the candidates.
constexpr int kSelectMaxPicks = 256;
struct GPSelectGP {
    const double* rows;   // GPDev::vrows [>= npad][4]
    const double* linvT;  // [npad][npad]
    double* Vt;           // [npad][ldp]: Vt[c][i] = (L^-1 k(X, z_i))_c
    double* lcol;         // [kSelectMaxPicks][ldp]: l_t[i]
    int32_t npad, nv, d;
    int32_t zcol;         // the GP's first column in the gathered inputs
    double c, sf2, sn2;   // c = -1 / (2 ell^2)
};
struct GPSelect {
    int32_t P, m, n_gp;
    int32_t ldp;          // stride of the per-candidate arrays (>= P)
    int32_t nblk;         // ceil(P / kPickBlock)
    const double* Z;      // [P][ldz] the candidates' gathered GP inputs
    int32_t ldz;
    const double* var0;   // [n_gp][ldv]
    int32_t ldv;
    GPSelectGP g[kMaxGP];
    double* d;            // [2][n_gp][ldp]: step t reads half t & 1 and writes the other
    int32_t* state;       // [ldp]: bit 0 picked, bit 1 a non-finite GP input
    double* bval;         // [2][nblk]: each block's best finite score among its unpicked candidates
    int32_t* bidx;        // [2][nblk][2]: its index (INT_MAX: none), the block's lowest unpicked non-finite candidate
    int32_t* pick;        // [m]
    double* gain;         // [m] or null
    double* resid;        // [n_gp][P] or null
    int32_t* ok;          // [1] or null
};
// V for every GP (one launch), the start state, then one launch per pick
hipError_t launch_gp_select(const GPSelect& a, hipStream_t stream);
// Greedy choice of up to M of a GP's n training rows as FITC inducing rows (gp_observe.hip; gpmpc_gp_inducing fills
// it): a pivoted partial Cholesky of the prior covariance k(X, X), no likelihood noise, that ends when no open row's
// residual prior variance exceeds tol sf2.  The grid runs over the training rows; everything but the outputs is
// scratch of the GP.
struct GPInducing {
    const double* rows;   // [>= npad][4], the training rows (the slot's exact rows): the inputs
    const double* linvT;  // [npad][npad], the live factor: only its diagonal is read (zero: an inert row)
    double* lcol;         // [M][ld]: l_t[i] (the second factor buffer)
    int32_t npad, n, M, d;
    int32_t ld;           // the padded capacity: stride of the l columns and of d
    int32_t nblk;         // ceil(n / kPickBlock)
    double c, sf2, tol;   // c = -1 / (2 ell^2)
    double* dd;           // [2][ld]: step t reads half t & 1 and writes the other
    int32_t* state;       // [ld]: bit 0 closed (picked or inert), bit 1 inert
    double* bval;         // [2][nblk]: each block's best score among its open rows
    int32_t* bidx;        // [2][nblk]: its index (INT_MAX: none)
    int32_t* flag;        // the state words (kInd* below)
    int32_t* idx;         // [M]: the picks, then -1
    double* gain;         // [M] or null: the scores at which they were picked, then NaN
    double* resid;        // [n] or null: the final d
};
// The state words: stopped, as step t reads it at [t & 1] and leaves it at [(t + 1) & 1]; the picks made (-1 while
// the selection runs: the stopping step or step M - 1 writes it)
enum : int { kIndStop = 0, kIndCount = 2, kIndInts = 4 };
// the start state and the outputs' tails; pick t (nothing once the state says stopped)
hipError_t launch_gp_inducing_begin(const GPInducing& a, hipStream_t stream);
hipError_t launch_gp_inducing_step(const GPInducing& a, int t, hipStream_t stream);
hipError_t launch_gp_append(const GPAppend& a, hipStream_t stream);
hipError_t launch_gp_drop(const GPDrop& a, hipStream_t stream);
hipError_t launch_gp_drop_prep(const GPDropPrep& a, hipStream_t stream);
// the start values and bests, then one launch per pick
hipError_t launch_gp_redundant(const GPRedundant& a, hipStream_t stream);
hipError_t launch_gp_refactor(const GPRefactor& a, hipStream_t stream);
// Its pieces, which the fit's iterations queue around a Khat built from device-resident hyperparameters:
// the status word set to 1 and the inert mask / masked targets; the 2 nt panel and update launches on a
// Khat already in A (linvT zeroed); w, alpha, rows[.][3], tX / tW and the caller's status word
hipError_t launch_gp_refactor_begin(const GPRefactor& a, hipStream_t stream);
hipError_t launch_gp_refactor_factor(const GPRefactor& a, hipStream_t stream);
hipError_t launch_gp_refactor_solve(const GPRefactor& a, hipStream_t stream);
// {1 / ell^2, sf2, sn2, ell} into state[kFitHyp ..]; then {MLL / n_live and its gradient} into out[4]
hipError_t launch_gp_fit_set_hyp(double* state, double inv_ell2, double sf2, double sn2, hipStream_t stream);
hipError_t launch_gp_fit_eval(const GPFit& f, double* out, hipStream_t stream);
// The fit: the state block from the raw start; one iteration (factorise at state's hyperparameters through
// `a`, evaluate, Adam step with the early-stop rule; hist: [max_iter][4] or null, row = the step taken)
hipError_t launch_gp_fit_init(double* state, const double* raw, hipStream_t stream);
hipError_t launch_gp_fit_iteration(const GPRefactor& a, const GPFit& f, double lr, double* hist_dev, hipStream_t stream);
// The LOVE root: the state, mask, Khat and q_0; iteration j (six launches; nothing once the state says done);
// the root R [npad][rp] of rank m from the finished state (R is zeroed first)
hipError_t launch_gp_love_begin(const GPLove& a, hipStream_t stream);
hipError_t launch_gp_love_iteration(const GPLove& a, int j, hipStream_t stream);
hipError_t launch_gp_love_root(const GPLove& a, int m, double* R, int rp, hipStream_t stream);
// The FITC mean: everything from the status word set to 1 to the staged rows and tiles (the caller reads the status)
hipError_t launch_gp_fitc(const GPFitc& a, hipStream_t stream);
// count < 0: the whole batch; else ranks first .. first + count - 1 of order[] (launch_sqp_order)
hipError_t launch_sqp(const ProblemDev& P, const StateDev& S, const StepIO& io, int batch, hipStream_t stream,
                      int first = 0, int count = -1);
hipError_t launch_sqp_order(const StateDev& S, int batch, hipStream_t stream);
bool sqp_overlap_ok(const ProblemDev& P, int batch);
bool sqp_tail_ok(const ProblemDev& P, int batch);   // GPMPC_TUNE_TAIL applies (gpmpc_solve)
int sqp_tail_spare(const ProblemDev& P, int batch);  // its automatic K: SIMDs the one-wave launch leaves free
int sqp_launch_waves(const ProblemDev& P, int batch);   // waves per instance launch_sqp would use
int sqp_launch_segments(const ProblemDev& P, int batch);   // horizon segments of its Newton solves
size_t sqp_lds_bytes(int model, int H);
int model_unc_dims(int model, int32_t* unc);   // the model's uncertain state dims (Bd columns), returns their count
hipError_t launch_stage_cost(const ProblemDev& P, const double* x, const double* u, const int32_t* tstep,
                             const int32_t* status, double* cost, int B, hipStream_t stream);
hipError_t launch_gp_mean_grad(const GPDev& g, const double* Z, int P, double* mean, double* grad, hipStream_t stream);
// An open-loop rollout of the model (sqp_kernel.hip rollout_kernel; gpmpc_rollout fills it), by value like the plant's
// parameters: P trajectories of T steps from x0 under u.  gp[] is read by the GP variant only.
struct RolloutArgs {
    double params[kMaxParams];   // the prior's (ProblemDev::params)
    double dt;
    int32_t P, T;                // P (T + 1) nx fits an int32
    const double* x0;            // [P][nx]
    const double* u;             // [P][T][nu]
    double* x;                   // [P][T+1][nx]
    GPDev gp[kMaxGP];
};
hipError_t launch_rollout(int model, const RolloutArgs& a, bool with_gp, hipStream_t stream);
// Z [P T][D]: the GP inputs z_k[gp_src_g] along x [P][T+1][nx], u [P][T][nu], D = sum of the GPs' dimensions
hipError_t launch_rollout_inputs(int model, const double* x, const double* u, int P, int T, double* Z, hipStream_t stream);
// The same rollout with the Jacobians of every step (sqp_kernel.hip rollout_lin_kernel; gpmpc_rollout_lin fills it):
// A [P][T][nx][nx] and B [P][T][nx][nu], row-major, the exact derivative of the RK4 step at (x_k, u_k).
struct RolloutLinArgs {
    RolloutArgs r;
    double* A;
    double* B;
};
hipError_t launch_rollout_lin(int model, const RolloutLinArgs& a, bool with_gp, hipStream_t stream);
// A closed-loop sample of the rollout (sqp_kernel.hip rollout_sample_kernel; gpmpc_rollout_sample fills it), by value:
// per step the applied input u_k = clip(u_nom,k + K (x_k - xref_k)), every GP's exact variance at z_k[gp_src_g] with
// that input, one draw e_g = sqrt(max(var_g + noise_g, 0)) xi_g of its residual, and rollout_kernel's RK4 step with
// mean_g + e_g in place of the mean at every substage.
struct RolloutSampleGP {         // what the variance reads of GPDev (the exact rows and their factor)
    const double* vrows;         // [nv][4]
    const double* linvT;         // [npad][npad]
    int32_t nv, npad;
    double inv_ell2, sf2;
};
struct RolloutSampleArgs {
    RolloutArgs r;               // r.u: the nominal inputs
    const double* xref;          // [P][T+1][nx], read when closed
    const double* xi;            // [P][T][n_gp] standard-normal draws, or null (no disturbance)
    double* uapp;                // [P][T][nu] the applied inputs, or null
    double* var;                 // [P][T][n_gp], or null
    int32_t closed, clip;
    double K[kMaxNU * kMaxNX];   // [nu][nx] row-major
    double u_lo[kMaxNU], u_hi[kMaxNU];
    double noise[kMaxGP];        // with_noise * sn2_g
    RolloutSampleGP vg[kMaxGP];  // read when xi or var is given
};
hipError_t launch_rollout_sample(int model, const RolloutSampleArgs& a, bool with_gp, hipStream_t stream);
// The state covariance along a finished rollout (rollout_cov.hip; gpmpc_rollout_lin fills it), by value:
//   S_0 = cov0 or zero,  S_{k+1} = Phi_k S_k Phi_k^T + Bd diag(q_k) Bd^T,  Phi_k = A_k + B_k K (A_k: open loop),
//   q_k[j] = dt^2 sum_g W_{j,g}(x_k, u_k) (var[p][k][g] + noise[g])     (Model::var_weights, Bd = Model::unc)
struct RolloutCovArgs {
    double dt;
    int32_t P, T;
    int32_t closed;              // K is read (0: Phi_k = A_k)
    double K[kMaxNU * kMaxNX];   // [nu][nx] row-major
    double noise[kMaxGP];        // with_noise * sn2_g
    const double* x;             // [P][T+1][nx]
    const double* u;             // [P][T][nu]
    const double* A;             // [P][T][nx][nx]
    const double* B;             // [P][T][nx][nu]
    const double* var;           // [P][T][n_gp]
    const double* cov0;          // [P][nx][nx] or null
    double* cov;                 // [P][T+1][nx][nx]
};
hipError_t launch_rollout_cov(int model, const RolloutCovArgs& a, hipStream_t stream);
hipError_t launch_gp_post(const GPDev& g, int npad, const PostArgs& a, bool from_state, hipStream_t stream,
                          int var_full = 0);   // PostBatch::var_full
hipError_t launch_gp_post_batch(const PostBatch& pb, bool from_state, hipStream_t stream);
struct PlantParams {   // gpmpc_plant_step's parameter vector, a kernel argument (entries past the model's are 0)
    double v[kMaxParams];
};
hipError_t launch_plant(int model, const PlantParams& params, double dt, const double* x, const double* u, double* xn,
                        int32_t* tstep, int B, hipStream_t stream);

}  // namespace gpmpc
