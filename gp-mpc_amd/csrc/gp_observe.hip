// GP training rows from transitions on the device (gpmpc_preprocess, gpmpc_gp_informative, gpmpc_gp_observe): the
// device restatement of GPMPC.preprocess_data (gpmpc/gpmpc.py, the reference's gpmpc/gpmpc.py:113-151) and the
// counting rank of the points' variance scores.  One thread per output row; nothing here synchronises the host.
// Below them the greedy conditional-variance selection (gpmpc_gp_select): the V kernel and the pick loop; and the
// greedy choice of a GP's FITC inducing rows among its own training rows (gpmpc_gp_inducing): the same pick loop
// (gp_pick.h) over a grid of the rows, with an end by tolerance.
#include "gp_pick.h"
#include "gp_tile.h"
#include "gpmpc_common.h"
#include "models.h"

#include <cmath>

namespace gpmpc {

namespace {

constexpr int kObserveThreads = 64;

// Row r of the outputs from transition pick[r]: the GP inputs z[gp_src_g] of z = [x; u] in GP order, and per GP the
// target.  x_dot = (x_next - x) / dt_diff; the quadrotors' thrust target is the norm of x_dot's velocity components
// with gravity added to the z-component, minus the prior thrust map a u_0 + b; their rate targets and cartpole's two
// targets are x_dot_j - f_j(x, u) with f the prior (Model<ID>::f at zero GP means).
template <int ID>
__global__ void gp_observe_kernel(const GPObserve a) {
    using M = Model<ID>;
    constexpr int NX = M::NX, NU = M::NU, NGP = M::NGP;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.m) return;
    const int src = a.pick != nullptr ? a.pick[r] : r;
    const bool live = src >= 0 && src < a.P;   // (an index outside the transitions reads nothing)
    const bool want_y = a.targets != nullptr || a.yg[0] != nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double z[NX + NU], y[NGP];
#pragma unroll
    for (int i = 0; i < NX + NU; ++i) z[i] = nan;
#pragma unroll
    for (int g = 0; g < NGP; ++g) y[g] = nan;
    if (live) {
#pragma unroll
        for (int i = 0; i < NX; ++i) z[i] = a.x[(size_t)src * NX + i];
#pragma unroll
        for (int i = 0; i < NU; ++i) z[NX + i] = a.u[(size_t)src * NU + i];
    }
    if (live && want_y) {
        double xd[NX], f[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) xd[i] = (a.xnext[(size_t)src * NX + i] - z[i]) / a.dt_diff;
        const double gm[kMaxGP] = {0.0, 0.0, 0.0, 0.0};
        M::f(a.params, z, z + NX, gm, f);
        if constexpr (ID == kQuad2D) {
            const double vz = xd[3] + a.gravity;
            y[0] = sqrt(xd[1] * xd[1] + vz * vz) - (a.params[0] * z[NX] + a.params[1]);
            y[1] = xd[5] - f[5];
        } else if constexpr (ID == kQuad3D) {
            const double vz = xd[5] + a.gravity;
            y[0] = sqrt(xd[1] * xd[1] + xd[3] * xd[3] + vz * vz) - (a.params[0] * z[NX] + a.params[1]);
            y[1] = xd[6] - f[6];
            y[2] = xd[7] - f[7];
        } else {
            y[0] = xd[1] - f[1];
            y[1] = xd[3] - f[3];
        }
    }
    int D = 0;
#pragma unroll
    for (int g = 0; g < NGP; ++g) D += M::gp_dim[g];
    int col = 0;
#pragma unroll
    for (int g = 0; g < NGP; ++g) {
        const int d = M::gp_dim[g];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < d) {
                const double v = z[M::gp_src[g][k]];
                if (a.inputs != nullptr) a.inputs[(size_t)r * D + col + k] = v;
                if (a.Xg[g] != nullptr) a.Xg[g][(size_t)r * d + k] = v;
            }
        }
        col += d;
        if (a.targets != nullptr) a.targets[(size_t)r * NGP + g] = y[g];
        if (a.yg[g] != nullptr) a.yg[g][r] = y[g];
    }
}

__global__ void gp_score_kernel(const GPRank a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P) return;
    double s = a.var[i] / a.sf2[0];
    for (int g = 1; g < a.n_gp; ++g) {
        const double t = a.var[(size_t)g * a.ldv + i] / a.sf2[g];
        if (t > s || t != t) s = t;   // (a NaN stays: nothing compares above it)
    }
    bool finite = true;
    for (int k = 0; k < a.ldz; ++k) finite = finite && isfinite(a.Z[(size_t)i * a.ldz + k]);
    if (!finite) s = __longlong_as_double(0x7ff8000000000000ll);
    a.score[i] = s;
    if (a.score_out != nullptr) a.score_out[i] = s;
}

// rank_i = #{j : s_j beats s_i}, a permutation of 0 .. P-1, so every slot of pick below m is written exactly once
__global__ void gp_rank_kernel(const GPRank a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P) return;
    const double si = a.score[i];
    const bool fi = isfinite(si);
    int rank = 0;
    for (int j = 0; j < a.P; ++j) {
        const double sj = a.score[j];
        const bool fj = isfinite(sj);
        bool beats;
        if (fi != fj) beats = fj;
        else if (fi && sj != si) beats = sj > si;
        else beats = j < i;
        rank += beats ? 1 : 0;
    }
    if (rank < a.m) a.pick[rank] = i;
}

// ---------------------------------------------------------------------------- greedy selection (gpmpc_gp_select)
// V_g = K_ZX L_g^-T for the P candidates and every GP of the model (grid.y), contracted as gp_post_kernel contracts
// it: one wave = 16 candidates, the A operand's kernel values generated on the fly (one exp per lane per K-step), the
// 16-row panels of (L^-1)^T staged in LDS for the workgroup's four waves, only the upper triangle loaded and
// multiplied, column groups of kSelCT tiles looped for npad > 256.  The accumulator tiles are stored, transposed:
// Vt[column][candidate], the layout the pick loop reads coalesced over its candidates.
constexpr int kSelWaves = 4;
constexpr int kSelCT = 16;
constexpr int kSelStride = 16 * (kSelCT | 1);   // odd number of tiles per LDS row, as gp_post_kernel's

// k(z, z') of two inputs of d columns, the operations of the variance kernels' kernel value
__device__ __forceinline__ double select_rbf(int d, double c, double sf2, const double* zi, const double* zj) {
    double q = 0.0;
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) {
        const int k = dd < d ? dd : 0;   // (nothing is read past the GP's own columns)
        const double df = (dd < d) ? zj[k] - zi[k] : 0.0;
        q = fma(df, df, q);
    }
    return sf2 * exp_rbf(c * q);
}
// k_g(z, z') of two gathered candidates
__device__ __forceinline__ double select_kernel_value(const GPSelectGP& g, const double* zi, const double* zj) {
    return select_rbf(g.d, g.c, g.sf2, zi, zj);
}

__global__ __launch_bounds__(64 * kSelWaves) void gp_select_v_kernel(const GPSelect a) {
    __shared__ __attribute__((aligned(16))) double panel[16 * kSelStride];
    const GPSelectGP g = a.g[blockIdx.y];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int p0 = (blockIdx.x * kSelWaves + wave) * 16;
    const int p = min(p0 + lc, a.P - 1);   // (a lane past the end repeats the last candidate and stores nothing)
    double z[3];
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) z[dd] = (dd < g.d) ? a.Z[(size_t)p * a.ldz + g.zcol + dd] : 0.0;
    const double4* rows = reinterpret_cast<const double4*>(g.rows);
    const int ntile = g.npad / 16;
    for (int t0 = 0; t0 < ntile; t0 += kSelCT) {
        const int tn = min(kSelCT, ntile - t0);
        const int npan = t0 + tn;   // K rows below 16 (t0 + tn): the upper triangle
        f64x4 acc[kSelCT];
#pragma unroll
        for (int t = 0; t < kSelCT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int pan = 0; pan < npan; ++pan) {
            const int lt0 = max(pan - t0, 0), w = 16 * (tn - lt0);
            __syncthreads();   // the previous panel has been read
            for (int e = tid; e < 16 * w; e += 64 * kSelWaves) {
                const int row = e / w, col = e - row * w;
                panel[row * kSelStride + 16 * lt0 + col] = g.linvT[(size_t)(16 * pan + row) * g.npad + 16 * (t0 + lt0) + col];
            }
            double kv[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int i = 16 * pan + 4 * ks + kq;
                const double4 r = rows[i < g.nv ? i : 0];
                const double xr[3] = {r.x, r.y, r.z};
                double q = 0.0;
#pragma unroll
                for (int dd = 0; dd < 3; ++dd) {
                    const double df = (dd < g.d) ? xr[dd] - z[dd] : 0.0;
                    q = fma(df, df, q);
                }
                const double e = g.sf2 * exp_rbf(g.c * q);
                kv[ks] = i < g.nv ? e : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const double* brow = panel + (4 * ks + kq) * kSelStride + lc;
#pragma unroll
                for (int t = 0; t < kSelCT; ++t)
                    if (t >= lt0 && t < tn)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[ks], brow[16 * t], acc[t], 0, 0, 0);
            }
        }
        // acc[t][r] = V[candidate p0 + kq + 4r][column 16 (t0 + t) + lc]
#pragma unroll
        for (int t = 0; t < kSelCT; ++t) {
            if (t < tn) {
                double* col = g.Vt + (size_t)(16 * (t0 + t) + lc) * a.ldp;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pr = p0 + kq + 4 * r;
                    if (pr < a.P) col[pr] = acc[t][r];
                }
            }
        }
    }
}

// gp_score_kernel's score of candidate i from the variances d[g * ldd + i]
__device__ __forceinline__ double select_score(const GPSelect& a, const double* d, size_t ldd, int i, bool bad_input) {
    double s = d[i] / a.g[0].sf2;
    for (int g = 1; g < a.n_gp; ++g) {
        const double t = d[(size_t)g * ldd + i] / a.g[g].sf2;
        if (t > s || t != t) s = t;   // (a NaN stays: nothing compares above it)
    }
    return bad_input ? __longlong_as_double(0x7ff8000000000000ll) : s;
}

// The start state: d = the variance launches' output, the non-finite inputs marked, each block's best, ok = 1.
// One wave = 64 / kPickBlock candidate blocks.
__global__ __launch_bounds__(64) void gp_select_init_kernel(const GPSelect a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < a.P;
    PickBest b = pick_none();
    if (valid) {
        for (int g = 0; g < a.n_gp; ++g) a.d[(size_t)g * a.ldp + i] = a.var0[(size_t)g * a.ldv + i];
        bool finite = true;
        for (int k = 0; k < a.ldz; ++k) finite = finite && isfinite(a.Z[(size_t)i * a.ldz + k]);
        a.state[i] = finite ? 0 : 2;
        b = pick_candidate(select_score(a, a.var0, a.ldv, i, !finite), i, true);
    }
    b = pick_group_best<kPickLargest>(b);
    const int blk = i / kPickBlock;
    if (threadIdx.x % kPickBlock == 0 && blk < a.nblk) pick_store_best<true>(a.bval, a.bidx, blk, b);
    if (i == 0 && a.ok != nullptr) a.ok[0] = 1;
}

// Pick t of the pick loop: the workgroup's kPickBlock candidates of every GP conditioned on j_t.  The inner product is
// v_i . v_j + sum_s l_s[i] l_s[j]: part q takes the column tiles [q nt / 16, (q + 1) nt / 16) of V (nt = npad / 16)
// and the l columns s = q, q + 16, .. .  The split depends on npad and t only.  One step reads all of V once: with few
// candidates per workgroup and the loads of four columns in flight the launch is spread over P / kPickBlock
// workgroups instead of waiting on one chain of dependent loads.
__global__ __launch_bounds__(kPickThreads) void gp_select_step_kernel(const GPSelect a, const int t) {
    __shared__ double sval[kPickThreads];
    __shared__ int sidx[kPickThreads], snf[kPickThreads];
    __shared__ double part[kPickParts][kPickBlock];
    const int tid = threadIdx.x;
    const int cur = t & 1, nxt = cur ^ 1;
    const PickBest best = pick_reduce_blocks<kPickLargest, true>(a.bval, a.bidx, a.nblk, cur, sval, sidx, snf);
    const bool fin = best.idx != kPickNone;   // a finite candidate is left; else the non-finite ones in index order
    const int j = fin ? best.idx : best.nf;
    const double gain = best.val;
    if (j < 0 || j >= a.P) return;   // (m <= P leaves a candidate for every pick; uniform)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (blockIdx.x == 0 && tid == 0) {
        a.pick[t] = j;
        if (a.gain != nullptr) a.gain[t] = fin ? gain : nan;
    }
    const int ci = tid % kPickBlock, kp = tid / kPickBlock;
    const int i = blockIdx.x * kPickBlock + ci;
    const bool valid = i < a.P;
    const int ii = valid ? i : a.P - 1;
    const size_t ldp = a.ldp;
    double score = 0.0;
    for (int gi = 0; gi < a.n_gp; ++gi) {
        const GPSelectGP& g = a.g[gi];
        const double* din = a.d + ((size_t)cur * a.n_gp + gi) * ldp;
        double* dout = a.d + ((size_t)nxt * a.n_gp + gi) * ldp;
        const double pv = din[j] + g.sn2;
        const bool good = fin && isfinite(pv) && pv > 0.0;   // (uniform over the workgroup)
        if (fin && !good && blockIdx.x == 0 && tid == 0 && a.ok != nullptr) a.ok[0] = 0;
        double l = 0.0;
        if (good) {
            const int ntile = g.npad / 16;
            const int c0 = 16 * (kp * ntile / kPickParts), c1 = 16 * ((kp + 1) * ntile / kPickParts);
            const double* vi = g.Vt + ii;
            const double* vj = g.Vt + j;
            double acc = 0.0;
            for (int c = c0; c < c1; c += 4) {   // (whole tiles: c1 - c0 is a multiple of 16)
                double x[4], y[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[k] = vi[(size_t)(c + k) * ldp];
                    y[k] = vj[(size_t)(c + k) * ldp];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = fma(x[k], y[k], acc);
            }
            for (int s = kp; s < t; s += kPickParts)
                acc = fma(g.lcol[(size_t)s * ldp + ii], g.lcol[(size_t)s * ldp + j], acc);
            part[kp][ci] = acc;
            __syncthreads();
            if (kp == 0) {
                const double k = select_kernel_value(g, a.Z + (size_t)ii * a.ldz + g.zcol, a.Z + (size_t)j * a.ldz + g.zcol);
                l = (k - pick_tree(part, ci)) / sqrt(pv);
            }
            __syncthreads();
        }
        if (kp == 0 && valid) {
            g.lcol[(size_t)t * ldp + i] = l;
            const double dn = din[i] - l * l;
            dout[i] = dn;
            if (a.resid != nullptr && t == a.m - 1) a.resid[(size_t)gi * a.P + i] = dn;
            const double sg = dn / g.sf2;
            if (gi == 0 || sg > score || sg != sg) score = sg;
        }
    }
    if (kp == 0) {   // (the first kPickBlock lanes of wave 0)
        PickBest nb = pick_none();
        if (valid) {
            int st = a.state[i];
            if (i == j) a.state[i] = st = st | 1;
            nb = pick_candidate((st & 2) ? nan : score, i, !(st & 1));
        }
        nb = pick_group_best<kPickLargest>(nb);
        if (tid == 0) pick_store_best<true>(a.bval, a.bidx, (size_t)nxt * a.nblk + blockIdx.x, nb);
    }
}

// ------------------------------------------------------------------ greedy inducing rows (gpmpc_gp_inducing)
// The same pick loop over a GP's own training rows with the prior covariance: d_i = sf2 at the start, no V, no noise,
// an end as soon as no open row's score d_i / sf2 exceeds tol, and so no use for a row whose score is not finite: the
// blocks' bests keep one index (kNf = false).  The grid runs over the n rows and the history grows to M columns (2000
// at the large quad3d size, against gp_select's 256), so what gp_select_step_kernel reads straight from memory inside
// its sum, the pivot row l_s[j], is staged here: it is a gather over the columns (stride ld), the same for every row
// of the workgroup, and read from memory inside the sum it doubles the loads of the dependent loop with lines of which
// 8 bytes are used.  Each chunk of kPickThreads columns is gathered once, one column per thread and all in flight
// together, into LDS, where the kPickBlock rows of a part read one address (a broadcast) and a wave's four parts four
// consecutive ones; the rows' own entries are loaded kPickParts at a time ahead of their sums.

// The start state: d = sf2 and open for a live row, 0 and closed for an inert one (a zero on the factor's diagonal),
// each block's best (every live score is exactly 1: the lowest live index wins), the outputs' tails (-1, NaN) in
// full, the state words.  One wave = 64 / kPickBlock row blocks.
__global__ __launch_bounds__(64) void gp_inducing_init_kernel(const GPInducing a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < a.n;
    PickBest b = pick_none();
    if (valid) {
        const bool live = a.linvT[(size_t)i * a.npad + i] != 0.0;
        a.dd[i] = live ? a.sf2 : 0.0;
        a.state[i] = live ? 0 : 3;
        b = pick_candidate(a.sf2 / a.sf2, i, live);
        if (i < a.M) {
            a.idx[i] = -1;
            if (a.gain != nullptr) a.gain[i] = __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    b = pick_group_best<kPickLargest>(b);
    const int blk = i / kPickBlock;
    if (threadIdx.x % kPickBlock == 0 && blk < a.nblk) pick_store_best<false>(a.bval, a.bidx, blk, b);
    if (i == 0) {
        a.flag[kIndStop] = 0;
        a.flag[kIndCount] = -1;
    }
}

// Pick t.  When the selection has stopped, or stops here (no open row with a finite score above tol), the workgroup
// leaves the stop for the next launch, the count and the residuals, and returns, uniformly.  Otherwise its rows form
// l_t: part q sums the columns s = q, q + 16, .. in order.
__global__ __launch_bounds__(kPickThreads) void gp_inducing_step_kernel(const GPInducing a, const int t) {
    __shared__ double sval[kPickThreads];
    __shared__ int sidx[kPickThreads];
    __shared__ double lj[kPickThreads];
    __shared__ double part[kPickParts][kPickBlock];
    const int tid = threadIdx.x;
    const int cur = t & 1, nxt = cur ^ 1;
    const bool first = blockIdx.x == 0 && tid == 0;
    if (a.flag[kIndStop + cur] != 0) {   // (written by the launch before this one; uniform)
        if (first) a.flag[kIndStop + nxt] = 1;
        return;
    }
    const PickBest best = pick_reduce_blocks<kPickLargest, false>(a.bval, a.bidx, a.nblk, cur, sval, sidx, nullptr);
    const int j = best.idx;
    const double gain = best.val;
    const int ci = tid % kPickBlock, kp = tid / kPickBlock;
    const int i = blockIdx.x * kPickBlock + ci;
    const bool valid = i < a.n;
    const int ii = valid ? i : a.n - 1;
    const size_t ld = a.ld;
    const double* din = a.dd + (size_t)cur * ld;
    double* dout = a.dd + (size_t)nxt * ld;
    if (j < 0 || j >= a.n || !(gain > a.tol)) {   // the end: count = t (uniform; a score kept as a best is finite)
        if (first) {
            a.flag[kIndStop + nxt] = 1;
            a.flag[kIndCount] = t;
        }
        if (kp == 0 && valid && a.resid != nullptr) a.resid[i] = din[i];
        return;
    }
    if (first) {
        a.idx[t] = j;
        if (a.gain != nullptr) a.gain[t] = gain;
        a.flag[kIndStop + nxt] = 0;
        if (t == a.M - 1) a.flag[kIndCount] = a.M;
    }
    const double pv = din[j];   // (= gain sf2 > 0)
    double acc = 0.0;
    for (int s0 = 0; s0 < t; s0 += kPickThreads) {
        const int cnt = min(kPickThreads, t - s0);
        __syncthreads();   // the previous chunk has been read
        lj[tid] = tid < cnt ? a.lcol[(size_t)(s0 + tid) * ld + j] : 0.0;
        double x[kPickParts];
#pragma unroll
        for (int k = 0; k < kPickParts; ++k) {
            const int q = kp + kPickParts * k;
            x[k] = q < cnt ? a.lcol[(size_t)(s0 + q) * ld + ii] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPickParts; ++k) {
            const int q = kp + kPickParts * k;
            if (q < cnt) acc = fma(x[k], lj[q], acc);
        }
    }
    part[kp][ci] = acc;
    __syncthreads();
    if (kp == 0) {   // (the first kPickBlock lanes of wave 0)
        PickBest nb = pick_none();
        if (valid) {
            const double r = pick_tree(part, ci);
            int st = a.state[i];
            const double k = select_rbf(a.d, a.c, a.sf2, a.rows + (size_t)i * 4, a.rows + (size_t)j * 4);
            const double l = (st & 2) ? 0.0 : (k - r) / sqrt(pv);
            a.lcol[(size_t)t * ld + i] = l;
            const double dn = din[i] - l * l;
            dout[i] = dn;
            if (a.resid != nullptr && t == a.M - 1) a.resid[i] = dn;
            if (i == j) a.state[i] = st = st | 1;
            nb = pick_candidate(dn / a.sf2, i, !(st & 1));
        }
        nb = pick_group_best<kPickLargest>(nb);
        if (tid == 0) pick_store_best<false>(a.bval, a.bidx, (size_t)nxt * a.nblk + blockIdx.x, nb);
    }
}

}  // namespace

static bool inducing_args_ok(const GPInducing& a) {
    return a.n >= 1 && a.M >= 1 && a.M <= a.n && a.n <= a.ld && a.n <= a.npad && a.npad >= 16 && a.npad % 16 == 0 &&
           a.nblk == (a.n + kPickBlock - 1) / kPickBlock && a.d >= 1 && a.d <= 3 && a.idx != nullptr;
}

hipError_t launch_gp_inducing_begin(const GPInducing& a, hipStream_t stream) {
    if (!inducing_args_ok(a)) return hipErrorInvalidValue;
    GP_LAUNCH(gp_inducing_init_kernel, dim3((a.n + 63) / 64), dim3(64), stream, a);
    return hipSuccess;
}

hipError_t launch_gp_inducing_step(const GPInducing& a, int t, hipStream_t stream) {
    if (!inducing_args_ok(a) || t < 0 || t >= a.M) return hipErrorInvalidValue;
    GP_LAUNCH(gp_inducing_step_kernel, dim3(a.nblk), dim3(kPickThreads), stream, a, t);
    return hipSuccess;
}

hipError_t launch_gp_select(const GPSelect& a, hipStream_t stream) {
    if (a.P < 1 || a.m < 1 || a.m > a.P || a.m > kSelectMaxPicks || a.P > a.ldp || a.n_gp < 1 || a.n_gp > kMaxGP ||
        a.nblk != (a.P + kPickBlock - 1) / kPickBlock)
        return hipErrorInvalidValue;
    for (int g = 0; g < a.n_gp; ++g)
        if (a.g[g].npad < 16 || a.g[g].npad % 16 != 0 || a.g[g].nv > a.g[g].npad) return hipErrorInvalidValue;
    GP_LAUNCH(gp_select_v_kernel, dim3((a.P + 16 * kSelWaves - 1) / (16 * kSelWaves), a.n_gp), dim3(64 * kSelWaves), stream, a);
    GP_LAUNCH(gp_select_init_kernel, dim3((a.P + 63) / 64), dim3(64), stream, a);
    for (int t = 0; t < a.m; ++t) GP_LAUNCH(gp_select_step_kernel, dim3(a.nblk), dim3(kPickThreads), stream, a, t);
    return hipSuccess;
}

hipError_t launch_gp_observe(const GPObserve& a, hipStream_t stream) {
    const dim3 grid((a.m + kObserveThreads - 1) / kObserveThreads), block(kObserveThreads);
    switch (a.model) {
        case kQuad2D: hipLaunchKernelGGL(gp_observe_kernel<kQuad2D>, grid, block, 0, stream, a); break;
        case kQuad3D: hipLaunchKernelGGL(gp_observe_kernel<kQuad3D>, grid, block, 0, stream, a); break;
        case kCartpole: hipLaunchKernelGGL(gp_observe_kernel<kCartpole>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_gp_score_rank(const GPRank& a, hipStream_t stream) {
    const dim3 grid((a.P + kObserveThreads - 1) / kObserveThreads), block(kObserveThreads);
    hipLaunchKernelGGL(gp_score_kernel, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gp_rank_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace gpmpc
