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
#include "gp_pick.h"
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

// ---------------------------------------------------------------------------- arbitrary rows (gpmpc_gp_drop_rows)
// D: the block's m <= 16 rows, ascending; k: the kept rows in their old order.  M[D, k] is no longer zero (entry
// (d, j) is non-zero for j < d), so the trailing factor is first restored and then updated as above:
//
//   V = -M[k, D] M[D, D]^-1,  B = M[k, k] + V M[D, k]  (= L[k, k]^-1, lower triangular),  M' = C^-1 B
//   g = P[D, D]^-1 alpha[D],  u = M[:, D] g  (all n rows),  alpha'_c = alpha[k_c] - linvT[k_c] . u
//
// with G_T, E_T, D_T, S_T unchanged: gp_drop_tile_kernel serves both.  The head and the apply kernel read the old
// factor through the kept-row map, which needs no array (drop_kept_row); the apply kernel's B tiles carry the rank-m
// term V_T M[D, k], one more 16 x 16 x 16 product per tile.  For D = {0 .. m-1} every formula is the one above.
// A call's rows are sorted once (gp_drop_prep_kernel) and its blocks taken from the highest indices down, so no
// block shifts the indices of the blocks after it.

// The old index of kept row c when the ascending rows d[0 .. m-1] leave
__device__ __forceinline__ int drop_kept_row(const int (&d)[16], int m, int c) {
    int i = c;
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (b < m && d[b] <= i) ++i;
    return i;
}
// The block's rows, held to 0 .. n0-1 whatever the scratch holds (entries past m: 0)
__device__ __forceinline__ int drop_row_at(const GPDrop& a, int b) {
    return b < a.m ? min(max(a.didx[b], 0), a.n0 - 1) : 0;
}
__device__ __forceinline__ void drop_rows_load(const GPDrop& a, int (&d)[16]) {
#pragma unroll
    for (int b = 0; b < 16; ++b) d[b] = drop_row_at(a, b);
}

// The flags set in the threads before this one (workgroup of 256) and their total
__device__ __forceinline__ int prep_rank(bool f, int tid, int* wsum, int& total) {
    const unsigned long long bal = __ballot(f);
    const int lane = tid & 63, wave = tid >> 6;
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();   // the previous call's sums have been read
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    return base + before;
}

// One workgroup: the membership mask of the indices in range, the lowest free rows added while fewer than m are
// marked, and the marked rows written in ascending order.
__global__ __launch_bounds__(256) void gp_drop_prep_kernel(GPDropPrep a) {
    __shared__ int wsum[4];
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    for (int i = tid; i < a.n; i += 256) a.mask[i] = 0;
    __syncthreads();
    for (int k = tid; k < a.m; k += 256) {
        const int v = a.idx[k];
        if (v >= 0 && v < a.n) a.mask[v] = 1;   // (duplicates write the same value)
        else bad = 1;
    }
    __syncthreads();
    int count = 0;
    for (int i0 = 0; i0 < a.n; i0 += 256) {
        int total;
        const int i = i0 + tid;
        (void)prep_rank(i < a.n && a.mask[i] != 0, tid, wsum, total);
        count += total;
    }
    const int deficit = a.m - count;   // (the same in every thread)
    int seen = 0;
    for (int i0 = 0; i0 < a.n && seen < deficit; i0 += 256) {
        int total;
        const int i = i0 + tid;
        const bool f = i < a.n && a.mask[i] == 0;
        const int r = prep_rank(f, tid, wsum, total);
        if (f && seen + r < deficit) a.mask[i] = 1;
        seen += total;
    }
    __syncthreads();
    int at = 0;
    for (int i0 = 0; i0 < a.n; i0 += 256) {
        int total;
        const int i = i0 + tid;
        const bool f = i < a.n && a.mask[i] != 0;
        const int r = prep_rank(f, tid, wsum, total);
        if (f && at + r < a.m) {
            a.sorted[at + r] = i;
            if (a.dropped != nullptr) a.dropped[at + r] = i;
        }
        at += total;
    }
    if (tid == 0) *a.acc = (bad == 0 && deficit == 0) ? 1 : 0;
}

// gp_drop_head_kernel through the row set: M[D, D] and its inverse, P[D, D] and g; then u over all old rows and V^T
// over the kept ones.
__global__ __launch_bounds__(256) void gp_drop_rows_head_kernel(GPDrop a) {
    __shared__ double A[16][17], Li[16][17], P[16][17], gv[16], tmp[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int m = a.m, n2 = a.n0 - a.m;
    int d[16];
    drop_rows_load(a, d);
    {   // M[D, D] padded with the identity; an inert row's zero diagonal reads as 1
        const int p = tid >> 4, q = tid & 15;
        double v = (p == q) ? 1.0 : 0.0;
        if (p < m && q <= p) {
            v = a.src[(size_t)drop_row_at(a, q) * a.npad0 + drop_row_at(a, p)];
            if (p == q && v == 0.0) v = 1.0;
        }
        A[p][q] = v;
        Li[p][q] = 0.0;
    }
    if (wave == 0) {
        // P[D, D] = Gram matrix of the rows D of linvT
        const f64x4 g = gram16(a.src + (size_t)drop_row_at(a, lc) * a.npad0 + 4 * kq, a.npad0 / 16, lc < m);
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
    inv_lower16(A, Li, tid);   // M[D, D]^-1
    ok = chol16(P, tmp, tid) && ok;
    if (tid == 0) {   // g = P[D, D]^-1 alpha[D]
        for (int i = 0; i < 16; ++i) {
            double s = i < m ? a.rows[(size_t)drop_row_at(a, i) * 4 + 3] : 0.0;
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
    // u_i = (M[:, D] g)_i over the old rows, zero past n0
    for (int i = tid; i < a.npad0; i += 256) {
        double ws = 0.0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const double v = (b < m && i < a.n0) ? a.src[(size_t)d[b] * a.npad0 + i] : 0.0;
            ws = fma(v, gv[b], ws);
        }
        a.w[i] = ws;
    }
    // kept row c: V^T[.][c] = -(M[D, D]^-1)^T M[k_c, D]^T; zero past n2
    for (int c = tid; c < a.npad1; c += 256) {
        const int i = c < n2 ? drop_kept_row(d, m, c) : 0;
        double col[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) col[b] = (b < m && c < n2) ? a.src[(size_t)d[b] * a.npad0 + i] : 0.0;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            double s = 0.0;
#pragma unroll
            for (int b = p; b < 16; ++b) s = fma(Li[b][p], col[b], s);
            a.vt[(size_t)p * a.ldv + c] = p < m ? -s : 0.0;
        }
    }
}

// gp_drop_apply_kernel through the row set.  Column tile J holds the kept rows c = 16J .. 16J + 15 (old rows k_c):
//   B_T[i][c] = src[k_c][k_i] + sum_b V[i][b] src[k_c][d_b],  M'_T = D_T (B_T - E_T S),  S += V_T^T B_T
__global__ __launch_bounds__(64 * kDropWaves) void gp_drop_rows_apply_kernel(GPDrop a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = blockIdx.x * kDropWaves + wave;
    const int nt = a.npad1 / 16;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the call's status so far and this block's
        const int v = (*a.acc != 0 && *a.flag != 0) ? 1 : 0;
        *a.acc = v;
        if (a.ok) *a.ok = v;
    }
    if (J >= nt) return;   // wave-uniform
    const int lc = lane & 15, kq = lane >> 4;
    const int m = a.m, n2 = a.n0 - a.m;
    int d[16];
    drop_rows_load(a, d);
    const int c = 16 * J + lc;
    const bool cok = c < n2;
    const int kc = cok ? drop_kept_row(d, m, c) : 0;
    double* drow = a.dst + (size_t)c * a.npad1;
    for (int T = 0; T < J; ++T)   // above the diagonal
#pragma unroll
        for (int r = 0; r < 4; ++r) drow[16 * T + kq + 4 * r] = 0.0;
    const double* srow = a.src + (size_t)kc * a.npad0;
    const double* varow = a.vt + (size_t)lc * a.ldv;
    // M[D, k_c] in the B operand's layout (row b = kq + 4s), and its part of linvT[k_c] . u
    f64x4 md;
    double da = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int b = kq + 4 * s, db = drop_row_at(a, b);
        md[s] = (cok && b < m) ? srow[db] : 0.0;
        da = fma(md[s], a.w[db], da);
    }
    f64x4 S = {0.0, 0.0, 0.0, 0.0};
    for (int T = J; T < nt; ++T) {
        const int i0 = 16 * T + kq;   // this lane's kept rows i0 + 4s
        const double* et = a.et + (size_t)T * 256 + lc * 16 + kq;
        const double* dt = a.dt + (size_t)T * 256 + lc * 16 + kq;
        f64x4 bt, va, vb, ea, dd;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = i0 + 4 * s;
            const int ki = i < n2 ? drop_kept_row(d, m, i) : 0;
            bt[s] = (cok && i < n2) ? srow[ki] : 0.0;              // M[k_i][k_c]
            va[s] = varow[i];                                      // V^T[lc][i]
            vb[s] = a.vt[(size_t)(kq + 4 * s) * a.ldv + 16 * T + lc];   // V[16T + lc][kq + 4s]
            ea[s] = et[4 * s];                                     // E_T[lc][kq + 4s]
            dd[s] = dt[4 * s];                                     // D_T[lc][kq + 4s]
            da = fma(bt[s], a.w[ki], da);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) bt = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[s], md[s], bt, 0, 0, 0);
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
    if (kq == 0) {   // kept row c: its weight, its inputs and its tile-pack entries, staged
        const double4 zero = {0.0, 0.0, 0.0, 0.0};
        const double4 rw = cok ? reinterpret_cast<const double4*>(a.rows)[kc] : zero;
        const double4 tx = cok ? reinterpret_cast<const double4*>(a.tX)[kc] : zero;
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
    if (a.didx != nullptr) {
        if (a.acc == nullptr || a.ldv < a.npad0) return hipErrorInvalidValue;
        GP_LAUNCH(gp_drop_rows_head_kernel, dim3(1), dim3(256), stream, a);
        GP_LAUNCH(gp_drop_tile_kernel, dim3(nt), dim3(64), stream, a);
        GP_LAUNCH(gp_drop_rows_apply_kernel, dim3((nt + kDropWaves - 1) / kDropWaves), dim3(64 * kDropWaves), stream, a);
        return hipSuccess;
    }
    GP_LAUNCH(gp_drop_head_kernel, dim3(1), dim3(256), stream, a);
    GP_LAUNCH(gp_drop_tile_kernel, dim3(nt), dim3(64), stream, a);
    GP_LAUNCH(gp_drop_apply_kernel, dim3((nt + kDropWaves - 1) / kDropWaves), dim3(64 * kDropWaves), stream, a);
    return hipSuccess;
}

hipError_t launch_gp_drop_prep(const GPDropPrep& a, hipStream_t stream) {
    if (a.m < 1 || a.m >= a.n || !a.idx || !a.mask || !a.sorted || !a.acc) return hipErrorInvalidValue;
    GP_LAUNCH(gp_drop_prep_kernel, dim3(1), dim3(256), stream, a);
    return hipSuccess;
}

// ---------------------------------------------------------------------------- the rows missed least (gpmpc_gp_redundant)
// Deleting row j turns the precision P = M^T M into P[k, k] - P[k, j] P[j, k] / P_jj, and 1 / P_ii - sn2 is row i's
// latent leave-one-out variance: what the other rows still say about x_i.  Greedy backward selection is therefore a
// pivoted partial Cholesky of P, the mirror of gpmpc_gp_select: with P_ij = linvT[i] . linvT[j],
//   c_t[i] = (P_ij - sum_{s<t} c_s[i] c_s[j]) / sqrt(p_j),  p_i -= c_t[i]^2,
// the pick being the row whose score max_g (1 / p_g,i - sn2_g) / sf2_g is smallest.  A row inert in GP g (a zero on
// the diagonal of M) has a zero row of linvT: its term is 0 and g is not conditioned on it.
// This is the pick loop of gp_pick.h with the smallest score as the best; p is double-buffered by the parity of t as
// the bests are.  Part q of the inner product takes the column tiles [q nt / 16, (q + 1) nt / 16) of the two rows
// and the c columns s = q, q + 16, .. .  No atomics.

// Part kp of linvT[i] . linvT[j] (whole tiles: rows are 128-byte aligned)
__device__ __forceinline__ double red_dot_part(const GPRedundantGP& g, int i, int j, int kp) {
    const int nt = g.npad / 16;
    const int q0 = 4 * (kp * nt / kPickParts), q1 = 4 * ((kp + 1) * nt / kPickParts);
    const double4* ri = reinterpret_cast<const double4*>(g.linvT + (size_t)i * g.npad);
    const double4* rj = reinterpret_cast<const double4*>(g.linvT + (size_t)j * g.npad);
    double acc = 0.0;
    for (int q = q0; q < q1; ++q) {
        const double4 x = ri[q], y = rj[q];
        acc = fma(x.x, y.x, acc);
        acc = fma(x.y, y.y, acc);
        acc = fma(x.z, y.z, acc);
        acc = fma(x.w, y.w, acc);
    }
    return acc;
}
__device__ __forceinline__ bool red_live(const GPRedundantGP& g, int i) { return g.linvT[(size_t)i * g.npad + i] != 0.0; }
// GP g's term of row i's score, folded into the largest so far (a NaN stays: nothing compares above it)
__device__ __forceinline__ double red_score(const GPRedundantGP& g, int gi, bool live, double p, double s) {
    const double t = live ? (1.0 / p - g.sn2) / g.sf2 : 0.0;
    return (gi == 0 || t > s || t != t) ? t : s;
}

// The start state: p_g,i = |linvT_g[i]|^2, nothing picked, each block's best, ok = 1
__global__ __launch_bounds__(kPickThreads) void gp_redundant_init_kernel(const GPRedundant a) {
    __shared__ double part[kPickParts][kPickBlock];
    const int tid = threadIdx.x;
    const int ci = tid % kPickBlock, kp = tid / kPickBlock;
    const int i = blockIdx.x * kPickBlock + ci;
    const bool valid = i < a.n;
    const int ii = valid ? i : a.n - 1;
    double score = 0.0;
    for (int gi = 0; gi < a.n_gp; ++gi) {
        const GPRedundantGP& g = a.g[gi];
        part[kp][ci] = red_dot_part(g, ii, ii, kp);
        __syncthreads();
        if (kp == 0 && valid) {
            const double p = pick_tree(part, ci);
            a.p[(size_t)gi * a.ldn + i] = p;
            score = red_score(g, gi, red_live(g, i), p, score);
        }
        __syncthreads();
    }
    if (kp == 0) {
        PickBest nb = pick_none();
        if (valid) {
            a.state[i] = 0;
            nb = pick_candidate(score, i, true);
        }
        nb = pick_group_best<kPickSmallest>(nb);
        if (tid == 0) pick_store_best<true>(a.bval, a.bidx, blockIdx.x, nb);
    }
    if (blockIdx.x == 0 && tid == 0 && a.ok != nullptr) a.ok[0] = 1;
}

// Pick t
__global__ __launch_bounds__(kPickThreads) void gp_redundant_step_kernel(const GPRedundant a, const int t) {
    __shared__ double sval[kPickThreads];
    __shared__ int sidx[kPickThreads], snf[kPickThreads];
    __shared__ double part[kPickParts][kPickBlock];
    const int tid = threadIdx.x;
    const int cur = t & 1, nxt = cur ^ 1;
    const PickBest best = pick_reduce_blocks<kPickSmallest, true>(a.bval, a.bidx, a.nblk, cur, sval, sidx, snf);
    const bool fin = best.idx != kPickNone;   // a finite score is left; else the non-finite ones in index order
    const int j = fin ? best.idx : best.nf;
    const double sj = best.val;
    if (j < 0 || j >= a.n) return;   // (m < n leaves a row for every pick; uniform)
    if (blockIdx.x == 0 && tid == 0) {
        a.pick[t] = j;
        if (a.score != nullptr) a.score[t] = fin ? sj : __longlong_as_double(0x7ff8000000000000ll);
    }
    const int ci = tid % kPickBlock, kp = tid / kPickBlock;
    const int i = blockIdx.x * kPickBlock + ci;
    const bool valid = i < a.n;
    const int ii = valid ? i : a.n - 1;
    const size_t ldn = a.ldn;
    double score = 0.0;
    for (int gi = 0; gi < a.n_gp; ++gi) {
        const GPRedundantGP& g = a.g[gi];
        const double* pin = a.p + ((size_t)cur * a.n_gp + gi) * ldn;
        double* pout = a.p + ((size_t)nxt * a.n_gp + gi) * ldn;
        const double pj = pin[j];
        const bool livej = red_live(g, j);
        const bool good = livej && isfinite(pj) && pj > 0.0;   // (uniform over the workgroup)
        if (livej && !good && blockIdx.x == 0 && tid == 0 && a.ok != nullptr) a.ok[0] = 0;
        double cv = 0.0;
        if (good) {
            double acc = red_dot_part(g, ii, j, kp);
            for (int s = kp; s < t; s += kPickParts) acc = fma(-g.ccol[(size_t)s * ldn + ii], g.ccol[(size_t)s * ldn + j], acc);
            part[kp][ci] = acc;
            __syncthreads();
            if (kp == 0) cv = pick_tree(part, ci) / sqrt(pj);
            __syncthreads();
        }
        if (kp == 0 && valid) {
            g.ccol[(size_t)t * ldn + i] = cv;
            const double pn = pin[i] - cv * cv;
            pout[i] = pn;
            score = red_score(g, gi, red_live(g, i), pn, score);
        }
    }
    if (kp == 0) {   // (the first kPickBlock lanes of wave 0)
        PickBest nb = pick_none();
        if (valid) {
            int st = a.state[i];
            if (i == j) a.state[i] = st = 1;
            nb = pick_candidate(score, i, st == 0);
        }
        nb = pick_group_best<kPickSmallest>(nb);
        if (tid == 0) pick_store_best<true>(a.bval, a.bidx, (size_t)nxt * a.nblk + blockIdx.x, nb);
    }
}

hipError_t launch_gp_redundant(const GPRedundant& a, hipStream_t stream) {
    if (a.n < 2 || a.m < 1 || a.m >= a.n || a.m > kRedundantMaxPicks || a.n > a.ldn || a.n_gp < 1 || a.n_gp > kMaxGP ||
        a.nblk != (a.n + kPickBlock - 1) / kPickBlock)
        return hipErrorInvalidValue;
    for (int g = 0; g < a.n_gp; ++g)
        if (a.g[g].npad < 16 || a.g[g].npad % 16 != 0 || a.n > a.g[g].npad) return hipErrorInvalidValue;
    GP_LAUNCH(gp_redundant_init_kernel, dim3(a.nblk), dim3(kPickThreads), stream, a);
    for (int t = 0; t < a.m; ++t) GP_LAUNCH(gp_redundant_step_kernel, dim3(a.nblk), dim3(kPickThreads), stream, a, t);
    return hipSuccess;
}

}  // namespace gpmpc
