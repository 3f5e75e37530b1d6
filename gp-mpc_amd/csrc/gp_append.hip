// Appending training rows to an exact GP on the device (gpmpc_gp_append): one bordered Cholesky
// update per block of m <= 16 new rows (X_b, y_b), hyperparameters unchanged.  With n rows, inverse
// factor L^-1 (stored transposed, GPDev::linvT) and weights alpha = K^-1 y:
//
//   K_b = k(X, X_b)                         n x m
//   W   = L^-1 K_b                          n x m    (W^T = K_b^T L^-T: the variance kernels' contraction)
//   S   = k(X_b, X_b) + sn2 I - W^T W       m x m
//   L_b = chol(S), L_b^-1
//   R   = -L_b^-1 (W^T L^-1)                m x n    new rows of L^-1; the diagonal block is L_b^-1
//   beta = L_b^-1 (y_b - K_b^T alpha)
//   alpha <- [alpha + R^T beta ; L_b^-T beta]
//
// Three launches per block, on the caller's stream:
//   gp_append_w_kernel     W^T (16 x n) on v_mfma_f64_16x16x4_f64: one wave per 16-column tile, the
//                          block's points the 16-row A operand with its kernel values generated on the
//                          fly (exp_rbf), the zero triangle of L^-T skipped; plus each tile's share of
//                          the posterior mean at X_b (K_b^T alpha).
//   gp_append_chol_kernel  one wave: Gram matrix W^T W (MFMA, four accumulators added in a fixed order),
//                          the per-tile means added in tile order, S, its Cholesky factor, L_b^-1, beta,
//                          the guard, and the block's own rows (rows, tX, tW, diagonal block of linvT).
//   gp_append_r_kernel     R = -L_b^-1 (W^T L^-1) on the same MFMA, one wave per 16-column tile: the new
//                          columns of linvT, and rows[.][3] and the tW pack of every old row.
// No sum crosses waves except through memory in a fixed order; no floating-point atomics.
//
// Guard.  The block is accepted when X_b, y_b and the mean at X_b are finite and every pivot of S is
// finite and positive.  Otherwise nothing is written but the status: the block's rows stay what rows
// past n always are (zero inputs, zero weight, zero linvT row and column), so they contribute nothing
// to any mean or variance, now or after later appends (their W row and their R column are exact zeros).
//
// The tile pack stays centred on the xbar gpmpc_set_gp computed: the centring is algebraically exact
// for any xbar and only conditions the exponent.
#include "gp_tile.h"

namespace gpmpc {

constexpr int kAppWaves = 4;   // column tiles per workgroup (one wave each, no LDS)

// W^T[p][j] = sum_{i <= j} k(xb_p, x_i) linvT[i][j], tile t = columns 16t .. 16t + 15, K rows < 16 (t + 1)
__global__ __launch_bounds__(64 * kAppWaves) void gp_append_w_kernel(GPAppend a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * kAppWaves + wave;
    const int nt = (a.n0 + 15) / 16;
    if (t >= nt) return;   // wave-uniform
    const int lc = lane & 15, kq = lane >> 4;
    const bool pvalid = lc < a.m;
    double z[3];
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) z[dd] = (dd < a.d) ? a.Xnew[(size_t)(pvalid ? lc : 0) * a.d + dd] : 0.0;
    const double c = -0.5 * a.inv_ell2;
    const double4* rows = reinterpret_cast<const double4*>(a.rows);
    const double* bcol = a.linvT + 16 * t + lc;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    double msum = 0.0;
    for (int pan = 0; pan <= t; ++pan) {
        double4 rw[4];
        double b[4], kv[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int i = 16 * pan + 4 * ks + kq;
            rw[ks] = rows[i];
            b[ks] = bcol[(size_t)i * a.npad];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {   // four independent exps
            const double d0 = rw[ks].x - z[0], d1 = rw[ks].y - z[1], d2 = rw[ks].z - z[2];
            const double e = rbf_raw(c, a.sf2, d0, d1, d2);
            kv[ks] = pvalid ? e : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[ks], b[ks], acc, 0, 0, 0);
            if (pan == t) msum = fma(kv[ks], rw[ks].w, msum);   // this tile's rows of K_b^T alpha
        }
    }
    // acc[r] = W^T[point kq + 4r][column 16t + lc]
#pragma unroll
    for (int r = 0; r < 4; ++r) a.wt[(size_t)(kq + 4 * r) * a.ldw + 16 * t + lc] = acc[r];
    msum += __shfl_xor(msum, 16);
    msum += __shfl_xor(msum, 32);
    if (kq == 0) a.pmean[(size_t)t * 16 + lc] = msum;
}

// One wave: S = k(X_b, X_b) + sn2 I - W^T W, L_b = chol(S), L_b^-1, beta, the guard, the block's rows.
__global__ __launch_bounds__(64) void gp_append_chol_kernel(GPAppend a) {
    __shared__ double S[16][17], Li[16][17], xb[16][4], res[16], bet[16], gam[16];
    const int lane = threadIdx.x;
    const int lc = lane & 15, kq = lane >> 4;
    const int nt = (a.n0 + 15) / 16;
    const int m = a.m;
    // the block's points; finite inputs and targets
    bool fin = true;
    double yv = 0.0;
    if (lane < 16) {
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) {
            const double v = (lane < m && dd < a.d) ? a.Xnew[(size_t)lane * a.d + dd] : 0.0;
            fin = fin && isfinite(v);
            xb[lane][dd] = v;
        }
        xb[lane][3] = 0.0;
        yv = lane < m ? a.ynew[lane] : 0.0;
        fin = fin && isfinite(yv);
        // mean at X_b: the tiles' shares in tile order
        double mu = 0.0;
        for (int t = 0; t < nt; ++t) mu += a.pmean[(size_t)t * 16 + lane];
        fin = fin && isfinite(mu);
        res[lane] = lane < m ? yv - mu : 0.0;
    }
    // Gram matrix G = W^T W over the old rows
    const f64x4 gw = gram16(a.wt + (size_t)lc * a.ldw + 4 * kq, nt);
    __syncthreads();
    const double c = -0.5 * a.inv_ell2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = kq + 4 * r, q = lc;   // G[p][q]
        const double d0 = xb[p][0] - xb[q][0], d1 = xb[p][1] - xb[q][1], d2 = xb[p][2] - xb[q][2];
        const double kbb = rbf_raw(c, a.sf2, d0, d1, d2) + (p == q ? a.sn2 : 0.0);
        S[p][q] = (p < m && q < m) ? kbb - gw[r] : (p == q ? 1.0 : 0.0);
        Li[p][q] = 0.0;
    }
    __syncthreads();
    bool ok = __all(fin);
    ok = chol16<true>(S, nullptr, lane) && ok;   // (measured against the LDS pivot: profiles/r13)
    inv_lower16(S, Li, lane);   // L_b^-1
    __syncthreads();
    if (lane < 16) {   // beta = L_b^-1 (y_b - mean)
        double s = 0.0;
        for (int q = 0; q <= lane; ++q) s = fma(Li[lane][q], res[q], s);
        bet[lane] = s;
    }
    __syncthreads();
    if (lane < 16) {   // the block's weights L_b^-T beta
        double s = 0.0;
        for (int p = lane; p < 16; ++p) s = fma(Li[p][lane], bet[p], s);
        gam[lane] = s;
        ok = ok && isfinite(s);
    }
    ok = __all(ok);
    if (lane == 0) {
        *a.flag = ok ? 1 : 0;
        if (a.accepted) *a.accepted = ok ? 1 : 0;
    }
    if (!ok) return;   // inert rows: what rows past n already are
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = kq + 4 * r, q = lc;
        a.lbinv[p * 16 + q] = Li[p][q];
        // diagonal block: row n0 + p of L^-1 is column n0 + p of linvT
        if (q <= p && p < m) a.linvT[(size_t)(a.n0 + q) * a.npad + a.n0 + p] = Li[p][q];
    }
    if (lane < 16) a.beta[lane] = bet[lane];
    if (lane < m) {
        const int i = a.n0 + lane;
        const TileSlot slot = tile_slot(i);
        double xc[3];
        tile_centre(xc, xb[lane][0], xb[lane][1], xb[lane][2], a.xbar, a.d);
        const double al = gam[lane];
        double* row = a.rows + (size_t)i * 4;
        row[0] = xb[lane][0];
        row[1] = xb[lane][1];
        row[2] = xb[lane][2];
        row[3] = al;
        tile_write_x(a.tX, slot, xc, a.inv_ell2, c);
        tile_write_w(a.tW, slot, al, xc);
    }
}

// R = -L_b^-1 T, T[q][i] = sum_{k >= i} W^T[q][k] linvT[i][k]; tile t = old rows 16t .. 16t + 15
__global__ __launch_bounds__(64 * kAppWaves) void gp_append_r_kernel(GPAppend a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * kAppWaves + wave;
    const int nt = (a.n0 + 15) / 16;
    if (t >= nt) return;        // wave-uniform
    if (*a.flag == 0) return;   // rejected block: the old weights are left alone
    const int lc = lane & 15, kq = lane >> 4;
    const int i = 16 * t + lc;
    // lane (lc, kq) takes K indices 16 pan + 4 kq + j: one double4 of its linvT row and of W^T per panel
    const double* brow = a.linvT + (size_t)i * a.npad + 4 * kq;
    const double* arow = a.wt + (size_t)lc * a.ldw + 4 * kq;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int pan = t; pan < nt; ++pan) {   // rows k < 16t of L^-1 have zeros in these columns
        const double4 bv = *reinterpret_cast<const double4*>(brow + 16 * pan);
        const double4 av = *reinterpret_cast<const double4*>(arow + 16 * pan);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, acc, 0, 0, 0);
    }
    // acc[r] = T[q = kq + 4r][i]: the B operand of K-step r when A is -L_b^-1[p][kq + 4r]
    f64x4 racc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
        racc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.lbinv[lc * 16 + kq + 4 * r], acc[r], racc, 0, 0, 0);
    // racc[r] = R[p = kq + 4r][i]: column n0 + p of linvT, row i
    double da = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = kq + 4 * r;
        if (p < a.m && i < a.n0) a.linvT[(size_t)i * a.npad + a.n0 + p] = racc[r];
        da = fma(racc[r], a.beta[p], da);
    }
    da += __shfl_xor(da, 16);
    da += __shfl_xor(da, 32);
    if (kq == 0 && i < a.n0) {   // alpha_i += (R^T beta)_i; its tile-pack entries
        const double4 rw = reinterpret_cast<const double4*>(a.rows)[i];
        const double al = rw.w + da;
        a.rows[(size_t)i * 4 + 3] = al;
        double xc[3];
        tile_centre(xc, rw.x, rw.y, rw.z, a.xbar, a.d);
        tile_write_w(a.tW, tile_slot(t, lc), al, xc);
    }
}

hipError_t launch_gp_append(const GPAppend& a, hipStream_t stream) {
    if (a.m < 1 || a.m > 16 || a.n0 < 1 || a.npad % 16 != 0 || a.n0 + a.m > a.npad || a.ldw < a.npad)
        return hipErrorInvalidValue;
    const int nt = (a.n0 + 15) / 16;
    const int blocks = (nt + kAppWaves - 1) / kAppWaves;
    GP_LAUNCH(gp_append_w_kernel, dim3(blocks), dim3(64 * kAppWaves), stream, a);
    GP_LAUNCH(gp_append_chol_kernel, dim3(1), dim3(64), stream, a);
    GP_LAUNCH(gp_append_r_kernel, dim3(blocks), dim3(64 * kAppWaves), stream, a);
    return hipSuccess;
}

}  // namespace gpmpc
