// Dropping the oldest training rows of an exact GP on the device (gpmpc_gp_drop_oldest): one update
// per block of m <= 16 rows, hyperparameters unchanged.  With n rows, K + sn2 I = L L^T, M = L^-1
// (stored transposed, GPDev::linvT: row j of linvT is column j of M) and alpha = (K + sn2 I)^-1 y;
// index 1 the m dropped rows, index 2 the n2 = n - m kept ones:
//
//   L11 = M11^-1                      m x m
//   V   = -M21 L11 (= L22^-1 L21)     n2 x m;  V^T = -L11^T linvT[0:m][m:n]
//   K22 + sn2 I = L22 (I + V V^T) L22^T   =>   M' = C^-1 M22,  C = chol(I + V V^T)
//
// a rank-m update of the trailing factor (I + V V^T >= I: every pivot below is >= 1 in exact
// arithmetic).  C is block-semiseparable, so C^-1 is applied per 16-row tile T of the kept rows with
// no recurrence through the result (p: the kept rows before the tile, B = M22):
//
//   G_T = I_m + V_p^T V_p,  E_T = V_T G_T^-1,  D_T = chol(I_16 + E_T V_T^T)^-1,  S_T = V_p^T B_p
//   M'_T = D_T (B_T - E_T S_T)
//
// M' is lower triangular: column tile J visits only the row tiles T >= J, S starting from zero.
// Weights, with no stored y:  P11 = M[:, 0:m]^T M[:, 0:m] (a Gram matrix of m rows of linvT),
// g = P11^-1 alpha_1, alpha' = alpha_2 - M22^T (M21 g).
//
// Three launches per block, on the caller's stream:
//   gp_drop_head_kernel   one workgroup: M11 (masked) and L11, P11 (MFMA Gram loop), its Cholesky
//                         factor and g; then V^T (16 x npad') and the vector M21 g over all columns.
//   gp_drop_tile_kernel   one wave per 16-row tile T: G_T by an MFMA Gram loop over the prefix of
//                         V^T (each wave sums its own prefix, in column order), its Cholesky factor,
//                         E_T, and D_T (16 x 16 Cholesky factor and inverse in LDS).
//   gp_drop_apply_kernel  one wave per 16-column tile J of M' on v_mfma_f64_16x16x4_f64, looping over
//                         T >= J with S in accumulators: it reads B from the old factor buffer and
//                         writes M' (and exact zeros above the diagonal and in the padding) to the
//                         other buffer at the new stride; the same pass forms alpha' and writes the
//                         shifted rows / tX / tW of its 16 rows to a staging region, which
//                         gpmpc_gp_drop_oldest then copies over the live ones (the shift overlaps
//                         its source, so nothing is moved in place).
// No sum crosses waves except through memory in a fixed order; no floating-point atomics.
//
// Inert rows (rejected append blocks: zero row and column of M, zero input, zero weight).  In the
// dropped block such a row puts a zero on the diagonal of M11 and of P11, which is treated as 1: its
// column of M21 and its alpha are exact zeros, so it drops out.  Among the kept rows it has a zero V
// row and a zero B row and column and stays inert without special code.
//
// Guard.  The block's status is 1 when every pivot (the diagonal of M11, the Cholesky factors of
// P11, of every G_T and of every I + E_T V_T^T) was finite and positive; otherwise 0, and the GP's
// contents are unspecified (every access stays in bounds whatever the values).
//
// The tile pack stays centred on the xbar gpmpc_set_gp computed (tX is moved, tW rewritten).
#include "gp_tile.h"

namespace gpmpc {

constexpr int kDropWaves = 4;   // column tiles per workgroup of the apply kernel (one wave each, no LDS)

// One workgroup of 256: L11, P11 and g on its first wave, then V^T and M21 g over all columns.
__global__ __launch_bounds__(256) void gp_drop_head_kernel(GPDrop a) {
    __shared__ double A[16][17], Li[16][17], P[16][17], gv[16], tmp[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int m = a.m, n2 = a.n0 - a.m;
    {   // M11 padded with the identity; an inert row's zero diagonal reads as 1
        const int p = tid >> 4, q = tid & 15;
        double v = (p == q) ? 1.0 : 0.0;
        if (p < m && q <= p) {
            v = a.src[(size_t)q * a.npad0 + p];
            if (p == q && v == 0.0) v = 1.0;
        }
        A[p][q] = v;
        Li[p][q] = 0.0;
    }
    if (wave == 0) {
        // P11 = Gram matrix of rows 0 .. m-1 of linvT
        const f64x4 g = gram16(a.src + (size_t)lc * a.npad0 + 4 * kq, a.npad0 / 16, lc < m);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = kq + 4 * r, q = lc;
            double v = g[r];
            if (p >= m || q >= m) v = (p == q) ? 1.0 : 0.0;
            if (p == q && v == 0.0) v = 1.0;
            P[p][q] = v;
        }
    }
    __syncthreads();
    bool ok = true;
    for (int j = 0; j < 16; ++j) ok = ok && isfinite(A[j][j]) && A[j][j] > 0.0;
    inv_lower16(A, Li, tid);   // L11 = M11^-1
    ok = chol16(P, tmp, tid) && ok;
    if (tid == 0) {   // g = P11^-1 alpha_1
        for (int i = 0; i < 16; ++i) {
            double s = i < m ? a.rows[(size_t)i * 4 + 3] : 0.0;
            for (int k = 0; k < i; ++k) s = fma(-P[i][k], tmp[k], s);
            tmp[i] = s / P[i][i];
        }
        for (int i = 15; i >= 0; --i) {
            double s = tmp[i];
            for (int k = i + 1; k < 16; ++k) s = fma(-P[k][i], gv[k], s);
            gv[i] = s / P[i][i];
        }
        *a.flag = ok ? 1 : 0;
    }
    __syncthreads();
    // column i of the kept rows: V^T[.][i] = -L11^T linvT[0:m][m + i] and (M21 g)_i; zero past n2
    for (int i = tid; i < a.npad1; i += 256) {
        double col[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) col[b] = (b < m && i < n2) ? a.src[(size_t)b * a.npad0 + m + i] : 0.0;
        double ws = 0.0;
#pragma unroll
        for (int b = 0; b < 16; ++b) ws = fma(col[b], gv[b], ws);
        a.w[i] = ws;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            double s = 0.0;
#pragma unroll
            for (int b = p; b < 16; ++b) s = fma(Li[b][p], col[b], s);
            a.vt[(size_t)p * a.ldv + i] = p < m ? -s : 0.0;
        }
    }
}

// One wave per 16-row tile T of the kept rows: G_T, E_T = V_T G_T^-1, D_T = chol(I + E_T V_T^T)^-1
__global__ __launch_bounds__(64) void gp_drop_tile_kernel(GPDrop a) {
    __shared__ double G[16][17], VT[16][17], E[16][17], F[16][17], D[16][17], tmp[16];
    const int lane = threadIdx.x, T = blockIdx.x;
    const int lc = lane & 15, kq = lane >> 4;
    const f64x4 g = gram16(a.vt + (size_t)lc * a.ldv + 4 * kq, T);   // over the kept rows before the tile
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = kq + 4 * r, q = lc;
        G[p][q] = g[r] + (p == q ? 1.0 : 0.0);
        VT[p][q] = a.vt[(size_t)p * a.ldv + 16 * T + q];   // V^T[p][row q of the tile]
        D[p][q] = 0.0;
    }
    __syncthreads();
    bool ok = chol16(G, tmp, lane);
    if (lane < 16) {   // row `lane` of E_T: G e = v by forward and backward substitution
        for (int i = 0; i < 16; ++i) {
            double s = VT[i][lane];
            for (int k = 0; k < i; ++k) s = fma(-G[i][k], E[lane][k], s);
            E[lane][i] = s / G[i][i];
        }
        for (int i = 15; i >= 0; --i) {
            double s = E[lane][i];
            for (int k = i + 1; k < 16; ++k) s = fma(-G[k][i], E[lane][k], s);
            E[lane][i] = s / G[i][i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // F = I + E_T V_T^T
        const int p = kq + 4 * r, q = lc;
        double s = (p == q) ? 1.0 : 0.0;
        for (int k = 0; k < 16; ++k) s = fma(E[p][k], VT[k][q], s);
        F[p][q] = s;
    }
    __syncthreads();
    ok = chol16(F, tmp, lane) && ok;
    inv_lower16(F, D, lane);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = kq + 4 * r, q = lc;
        a.et[(size_t)T * 256 + p * 16 + q] = E[p][q];
        a.dt[(size_t)T * 256 + p * 16 + q] = D[p][q];
    }
    if (!ok && lane == 0) *a.flag = 0;
}

// Column tile J of M' (columns c = 16J .. 16J + 15: rows of the new factor buffer), T = J .. nt - 1:
//   M'_T = D_T (B_T - E_T S),  S += V_T^T B_T,  B[i][c] = src[m + c][m + i]
__global__ __launch_bounds__(64 * kDropWaves) void gp_drop_apply_kernel(GPDrop a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = blockIdx.x * kDropWaves + wave;
    const int nt = a.npad1 / 16;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.ok) *a.ok = *a.flag;
    if (J >= nt) return;   // wave-uniform
    const int lc = lane & 15, kq = lane >> 4;
    const int m = a.m, n2 = a.n0 - a.m;
    const int c = 16 * J + lc;
    const bool cok = c < n2;
    double* drow = a.dst + (size_t)c * a.npad1;
    for (int T = 0; T < J; ++T)   // above the diagonal
#pragma unroll
        for (int r = 0; r < 4; ++r) drow[16 * T + kq + 4 * r] = 0.0;
    const double* srow = a.src + (size_t)(m + (cok ? c : 0)) * a.npad0 + m;
    const double* varow = a.vt + (size_t)lc * a.ldv;
    f64x4 S = {0.0, 0.0, 0.0, 0.0};
    double da = 0.0;
    for (int T = J; T < nt; ++T) {
        const int i0 = 16 * T + kq;   // this lane's rows i0 + 4s
        const double* et = a.et + (size_t)T * 256 + lc * 16 + kq;
        const double* dt = a.dt + (size_t)T * 256 + lc * 16 + kq;
        f64x4 bt, va, ea, dd;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = i0 + 4 * s;
            bt[s] = (cok && i < n2) ? srow[i] : 0.0;   // B_T[kq + 4s][c]
            va[s] = varow[i];                          // V^T[lc][i]
            ea[s] = et[4 * s];                         // E_T[lc][kq + 4s]
            dd[s] = dt[4 * s];                         // D_T[lc][kq + 4s]
            da = fma(bt[s], a.w[i], da);               // (M22^T (M21 g))_c
        }
        f64x4 y = bt;
#pragma unroll
        for (int s = 0; s < 4; ++s) y = __builtin_amdgcn_mfma_f64_16x16x4f64(-ea[s], S[s], y, 0, 0, 0);
        f64x4 o = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) o = __builtin_amdgcn_mfma_f64_16x16x4f64(dd[s], y[s], o, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) S = __builtin_amdgcn_mfma_f64_16x16x4f64(va[s], bt[s], S, 0, 0, 0);
        // o[r] = M'[i0 + 4r][c]; exact zeros above the diagonal and in the padding
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * r;
            drow[i] = (cok && i < n2 && i >= c) ? o[r] : 0.0;
        }
    }
    da += __shfl_xor(da, 16);
    da += __shfl_xor(da, 32);
    if (kq == 0) {   // row c of the kept rows: its weight, its inputs and its tile-pack entries, staged
        const int i = m + (cok ? c : 0);
        const double4 zero = {0.0, 0.0, 0.0, 0.0};
        const double4 rw = cok ? reinterpret_cast<const double4*>(a.rows)[i] : zero;
        const double4 tx = cok ? reinterpret_cast<const double4*>(a.tX)[i] : zero;   // tX[t][16][4]: row i
        const double al = cok ? rw.w - da : 0.0;
        reinterpret_cast<double4*>(a.srows)[c] = double4{rw.x, rw.y, rw.z, al};
        reinterpret_cast<double4*>(a.stX)[c] = tx;
        double xc[3];
        tile_centre(xc, rw.x, rw.y, rw.z, a.xbar, a.d);
        tile_write_w(a.stW, tile_slot(J, lc), al, xc, cok);
    }
}

hipError_t launch_gp_drop(const GPDrop& a, hipStream_t stream) {
    if (a.m < 1 || a.m > 16 || a.m >= a.n0 || a.npad0 % 16 != 0 || a.npad1 % 16 != 0 || a.n0 > a.npad0 ||
        a.n0 - a.m > a.npad1 || a.npad1 > a.npad0 || a.ldv < a.npad1)
        return hipErrorInvalidValue;
    const int nt = a.npad1 / 16;
    GP_LAUNCH(gp_drop_head_kernel, dim3(1), dim3(256), stream, a);
    GP_LAUNCH(gp_drop_tile_kernel, dim3(nt), dim3(64), stream, a);
    GP_LAUNCH(gp_drop_apply_kernel, dim3((nt + kDropWaves - 1) / kDropWaves), dim3(64 * kDropWaves), stream, a);
    return hipSuccess;
}

}  // namespace gpmpc
