// Building the LOVE variance root of an exact GP on the device (gpmpc_gp_love_root): Lanczos with full
// reorthogonalisation on Khat = k(X, X) + sn2 I, generated from the handle's own rows and current
// hyperparameters, restating GaussianProcess.love_root (gpmpc/gp.py) up to the last step:
//
//   q_0 = q0 / |q0|;  iteration j:  v = Khat q_j,  alpha_j = q_j . v,  v -= alpha_j q_j + beta_{j-1} q_{j-1},
//   twice v -= Q (Q^T v) over the columns 0 .. j,  b = |v|;  stop when j + 1 = min(rank, n_live) or
//   b <= 1e-12 max |alpha|;  otherwise beta_j = b, q_{j+1} = v / b.
//
// The root needs no eigensolver: only R R^T = Q T^-1 Q^T reaches the variance, so with the Cholesky factor
// T = C C^T of the tridiagonal matrix (C lower bidiagonal: c_jj = sqrt(alpha_j - l_j^2), l_{j+1} = beta_j / c_jj)
// R = Q C^-T is the recurrence R[:, j] = (Q[:, j] - l_j R[:, j-1]) / c_jj, one thread per row.
//
// Layout.  Khat lies in full, symmetric, at stride npad in the GP's spare factor buffer (scratch between the
// updates); Q is kept transposed, Qt[k][i] at stride ld (the padded capacity), so that q_j, every column of the
// update v -= Q c and the MFMA operand of Q^T v are contiguous along the rows.  Qt's columns are zeroed first:
// the columns past j of the last 16-column tile contribute exact zeros.
//
// Launches (plain, on the caller's stream).  Begin: 1 memset of the state, 1 of Qt, mask, build, start.
// Iteration j, six launches over row blocks; every sum that crosses waves goes through memory and is added in
// a fixed order by every workgroup that needs it, so there are no floating-point atomics, no grid-wide barrier
// and no spin-wait, and two runs on the same inputs give the same bits:
//
//   gp_love_matvec_kernel    16 rows per workgroup, a wave per 4 rows over coalesced double4 of Khat and q_j;
//                            v and the workgroup's part of alpha_j
//   gp_love_orth_kernel x 3  64 rows per workgroup.  mode 0: alpha_j from the parts, v -= alpha q_j + beta
//                            q_{j-1}; mode 1, 2: c = the sum of the workgroups' parts of Q^T v, v -= Q c.
//                            Modes 0, 1 then form the workgroup's part of Q^T v for the next one, a wave per
//                            16-column tile of Q on v_mfma_f64_16x16x4_f64 (the loop of gram16 with v as the
//                            B operand); mode 2 its part of |v|^2.
//   gp_love_decide_kernel    one workgroup: b, the stop rule; at the stop the pivots c_jj, l_j and the status
//   gp_love_next_kernel      q_{j+1} = v / b
//
// Kernels queued after the stop read the state's done word and return.  End: gp_love_root_kernel writes R at
// stride pad16(m), zero padded, as gpmpc_set_gp_variance_root lays it out.
//
// Inert rows (rejected append blocks) and the padding rows past n have a zero on the factor's diagonal.  Their
// rows and columns of Khat are zero (the diagonal included) and their q0 entry is never read into a sum, so
// their rows of Q and of R are exact zeros.  Every access stays in bounds whatever the values.
#include "gp_tile.h"

namespace gpmpc {

constexpr int kLoveRows = 256;   // rows per workgroup of the elementwise kernels
constexpr int kLoveOrthRows = 64;  // rows per workgroup of the orthogonalisation steps
constexpr int kLoveMvRows = 16;  // rows per workgroup of the matrix-vector product (4 per wave)

// The sum of p[0 .. count) in an order that depends on nothing but count: the same value in every thread of
// every 256-thread workgroup that calls it (red: 256 doubles of LDS)
__device__ __forceinline__ double love_fixed_sum(const double* p, int count, double* red) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < count; i += 256) s += p[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// mask[i] = 1 for an inert or padding row; v = the start vector with those rows' entries replaced by zero;
// the workgroup's parts of |q0|^2 and of the live-row count
__global__ __launch_bounds__(kLoveRows) void gp_love_mask_kernel(GPLove a) {
    __shared__ double red[kLoveRows], cnt[kLoveRows];
    const int tid = threadIdx.x, i = blockIdx.x * kLoveRows + tid;
    double qi = 0.0, live = 0.0;
    if (i < a.npad) {
        const bool inert = i >= a.n || a.linvT[(size_t)i * a.npad + i] == 0.0;
        qi = inert ? 0.0 : a.q0[i];
        live = inert ? 0.0 : 1.0;
        a.mask[i] = inert ? 1 : 0;
        a.v[i] = qi;
    }
    red[tid] = qi * qi;
    cnt[tid] = live;
    __syncthreads();
    for (int w = kLoveRows / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w], cnt[tid] += cnt[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.npart[blockIdx.x] = red[0], a.ipart[blockIdx.x] = cnt[0];
}

// Khat in full into A; one workgroup per 16 x 16 tile.  The kernel's value depends on the squares of the row
// differences only, so the two triangles are equal bit for bit.
__global__ __launch_bounds__(256) void gp_love_build_kernel(GPLove a) {
    const int i = 16 * blockIdx.y + (threadIdx.x >> 4), j = 16 * blockIdx.x + (threadIdx.x & 15);
    const double4* rows = reinterpret_cast<const double4*>(a.rows);
    const double4 xi = rows[i], xj = rows[j];
    double v = rbf_raw(-0.5 * a.inv_ell2, a.sf2, xi.x - xj.x, xi.y - xj.y, xi.z - xj.z);
    if (i == j) v = a.sf2 + a.sn2;
    if (a.mask[i] || a.mask[j]) v = 0.0;
    a.A[(size_t)i * a.npad + j] = v;
}

// q_0 = q0 / |q0| over the live rows; the state: the iteration cap min(rank, n_live), done at once without a
// live row
__global__ __launch_bounds__(kLoveRows) void gp_love_start_kernel(GPLove a) {
    __shared__ double red[kLoveRows];
    const int nb = gridDim.x, i = blockIdx.x * kLoveRows + threadIdx.x;
    const double nrm = sqrt(love_fixed_sum(a.npart, nb, red));
    const double live = love_fixed_sum(a.ipart, nb, red);
    if (i < a.npad) a.qt[i] = nrm > 0.0 ? a.v[i] / nrm : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int n_live = (int)live;
        a.state[kLoveKmax] = a.rank < n_live ? a.rank : n_live;
        a.state[kLoveLive] = n_live;
        if (n_live < 1) a.state[kLoveDone] = 1;   // (m = 0, ok = 0 from the memset)
    }
}

// v = Khat q_j for the workgroup's 16 rows and its part of alpha_j = q_j . v
__global__ __launch_bounds__(256) void gp_love_matvec_kernel(GPLove a, int j) {
    __shared__ double part[kLoveMvRows];
    if (a.state[kLoveDone]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kLoveMvRows + 4 * wave;
    const double* q = a.qt + (size_t)j * a.ld;
    const double* row = a.A + (size_t)r0 * a.npad;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 4 * lane; c < a.npad; c += 256) {
        const double4 qv = *reinterpret_cast<const double4*>(q + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double4 av = *reinterpret_cast<const double4*>(row + (size_t)r * a.npad + c);
            s[r] = fma(av.x, qv.x, s[r]);
            s[r] = fma(av.y, qv.y, s[r]);
            s[r] = fma(av.z, qv.z, s[r]);
            s[r] = fma(av.w, qv.w, s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s[r] += __shfl_xor(s[r], 32);
        s[r] += __shfl_xor(s[r], 16);
        s[r] += __shfl_xor(s[r], 8);
        s[r] += __shfl_xor(s[r], 4);
        s[r] += __shfl_xor(s[r], 2);
        s[r] += __shfl_xor(s[r], 1);
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a.v[r0 + r] = s[r];
            part[4 * wave + r] = q[r0 + r] * s[r];
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = part[0];
#pragma unroll
    for (int r = 1; r < kLoveMvRows; ++r) t += part[r];
    a.apart[blockIdx.x] = t;
}

// One step of the orthogonalisation on the workgroup's 64 rows of v (see the head of the file).  Thread (r, q)
// belongs to row r and wave q: the waves share the columns of v -= Q c (k = q, q + 4, ..; the four sums are added
// in a fixed order through LDS) and the 16-column tiles of Q^T v.
__global__ __launch_bounds__(256) void gp_love_orth_kernel(GPLove a, int j, int mode) {
    __shared__ double red[256], cs[256], ps[4][kLoveOrthRows];
    __shared__ __attribute__((aligned(32))) double vs[kLoveOrthRows];
    if (a.state[kLoveDone]) return;
    const int tid = threadIdx.x, r = tid & 63, q = tid >> 6;
    const int i0 = blockIdx.x * kLoveOrthRows, i = i0 + r;
    const int ncol = 16 * (j / 16 + 1);   // the columns 0 .. j in whole tiles
    const size_t ld = a.ld;
    const bool in = i < a.npad;
    double vi = in ? a.v[i] : 0.0;
    if (mode == 0) {
        const double al = love_fixed_sum(a.apart, a.npad / kLoveMvRows, red);
        if (blockIdx.x == 0 && tid == 0) a.alpha[j] = al;
        if (in) {
            vi = vi - al * a.qt[(size_t)j * ld + i];
            if (j > 0) vi = vi - a.beta[j - 1] * a.qt[(size_t)(j - 1) * ld + i];
        }
    } else {
        // c = the sum of the workgroups' parts: the 256 threads form 256 / w groups over the w >= ncol columns
        // (w a power of two), group h adds the parts h, h + groups, .. in ascending order, then the groups' sums
        // are added in the order of h
        const double* cp = mode == 1 ? a.cpa : a.cpb;
        int w = 16;
        while (w < ncol) w *= 2;
        const int groups = 256 / w, k0 = tid & (w - 1), h = tid / w;
        double c = 0.0;
#pragma unroll 8
        for (int b = h; b < (int)gridDim.x; b += groups) c += cp[(size_t)b * 256 + k0];
        red[tid] = c;
        __syncthreads();
        c = 0.0;
        if (tid < w)
            for (int g = 0; g < groups; ++g) c += red[g * w + tid];
        cs[tid] = c;
        __syncthreads();
        double s = 0.0;
        if (in) {
#pragma unroll 4
            for (int k = q; k <= j; k += 4) s = fma(cs[k], a.qt[(size_t)k * ld + i], s);
        }
        ps[q][r] = s;
        __syncthreads();
        vi -= (ps[0][r] + ps[1][r]) + (ps[2][r] + ps[3][r]);
    }
    if (q == 0 && in) a.v[i] = vi;
    if (mode == 2) {   // the workgroup's part of |v|^2
        red[tid] = (q == 0 && in) ? vi * vi : 0.0;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.npart[blockIdx.x] = red[0];
        return;
    }
    if (q == 0) vs[r] = in ? vi : 0.0;
    __syncthreads();
    // The workgroup's part of Q^T v: wave = 16-column tile t of Q.  Lane (lc, kq) takes rows 16 s + 4 kq + jj of
    // column 16 t + lc as the A operand and the same rows of v, whatever lc, as the B operand, so every column
    // of the product holds c; entry r of the result is c[16 t + kq + 4 r].  Steps past npad are left out.
    const int lc = r & 15, kq = r >> 4;
    const int left = (a.npad - i0) / 16, steps = left < kLoveOrthRows / 16 ? left : kLoveOrthRows / 16;
    double* out = (mode == 0 ? a.cpa : a.cpb) + (size_t)blockIdx.x * 256;
    for (int t = q; t < ncol / 16; t += 4) {
        const double* col = a.qt + (size_t)(16 * t + lc) * ld + i0 + 4 * kq;
        f64x4 g[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) g[p] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < steps; ++s) {
            const double4 w = *reinterpret_cast<const double4*>(col + 16 * s);
            const double4 x = *reinterpret_cast<const double4*>(vs + 16 * s + 4 * kq);
            g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.x, x.x, g[0], 0, 0, 0);
            g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.y, x.y, g[1], 0, 0, 0);
            g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.z, x.z, g[2], 0, 0, 0);
            g[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.w, x.w, g[3], 0, 0, 0);
        }
        if (lc == 0) {
#pragma unroll
            for (int p = 0; p < 4; ++p) out[16 * t + kq + 4 * p] = (g[0][p] + g[1][p]) + (g[2][p] + g[3][p]);
        }
    }
}

// b = |v| and the stop rule; at the stop the rank m = j + 1, the bidiagonal factor's pivots and the status
__global__ __launch_bounds__(256) void gp_love_decide_kernel(GPLove a, int j, int nb) {
    __shared__ double red[256];
    if (a.state[kLoveDone]) return;
    const double b2 = love_fixed_sum(a.npart, nb, red);
    if (threadIdx.x != 0) return;
    const double b = sqrt(b2);
    double amax = 0.0;
    for (int k = 0; k <= j; ++k) amax = fmax(amax, fabs(a.alpha[k]));
    // (a b that is not a number stops too: the pivots then decide the status)
    if (j + 1 < a.state[kLoveKmax] && b > 1e-12 * amax) {
        a.beta[j] = b;
        return;
    }
    const int m = j + 1;
    int ok = 1;
    double l = 0.0;
    for (int k = 0; k < m; ++k) {
        const double piv = a.alpha[k] - l * l;
        if (!(isfinite(piv) && piv > 0.0)) {
            ok = 0;
            break;
        }
        const double c = sqrt(piv);
        a.cd[k] = c;
        a.lsub[k] = l;
        if (k + 1 < m) l = a.beta[k] / c;
    }
    a.state[kLoveM] = m;
    a.state[kLoveOk] = ok;
    a.state[kLoveDone] = 1;
}

// q_{j+1} = v / beta_j
__global__ __launch_bounds__(kLoveRows) void gp_love_next_kernel(GPLove a, int j) {
    if (a.state[kLoveDone] || j + 1 >= a.rank) return;
    const int i = blockIdx.x * kLoveRows + threadIdx.x;
    if (i < a.npad) a.qt[(size_t)(j + 1) * a.ld + i] = a.v[i] / a.beta[j];
}

// R = Q C^-T, row i of R [npad][rp] (zeroed before the launch: the padding columns stay zero)
__global__ __launch_bounds__(kLoveRows) void gp_love_root_kernel(GPLove a, int m, double* R, int rp) {
    const int i = blockIdx.x * kLoveRows + threadIdx.x;
    if (i >= a.npad || a.mask[i]) return;
    double prev = 0.0;
    for (int k = 0; k < m; ++k) {
        prev = (a.qt[(size_t)k * a.ld + i] - a.lsub[k] * prev) / a.cd[k];
        R[(size_t)i * rp + k] = prev;
    }
}

static bool love_shape_ok(const GPLove& a) {
    return a.n >= 1 && a.npad % 16 == 0 && a.n <= a.npad && a.npad <= a.ld && a.ld % 16 == 0 && a.rank >= 1 &&
           a.rank <= kLoveMaxRank;
}

hipError_t launch_gp_love_begin(const GPLove& a, hipStream_t stream) {
    if (!love_shape_ok(a)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.state, 0, kLoveInts * sizeof(int32_t), stream);
    // the columns the tiles of Q^T v can reach
    const size_t cols = (size_t)((a.rank + 15) / 16 * 16);
    if (e == hipSuccess) e = hipMemsetAsync(a.qt, 0, cols * a.ld * sizeof(double), stream);
    if (e != hipSuccess) return e;
    const int nb = (a.npad + kLoveRows - 1) / kLoveRows, nt = a.npad / 16;
    GP_LAUNCH(gp_love_mask_kernel, dim3(nb), dim3(kLoveRows), stream, a);
    GP_LAUNCH(gp_love_build_kernel, dim3(nt, nt), dim3(256), stream, a);
    GP_LAUNCH(gp_love_start_kernel, dim3(nb), dim3(kLoveRows), stream, a);
    return hipSuccess;
}

hipError_t launch_gp_love_iteration(const GPLove& a, int j, hipStream_t stream) {
    if (!love_shape_ok(a) || j < 0 || j >= a.rank) return hipErrorInvalidValue;
    const int nb = (a.npad + kLoveRows - 1) / kLoveRows, nbo = (a.npad + kLoveOrthRows - 1) / kLoveOrthRows;
    GP_LAUNCH(gp_love_matvec_kernel, dim3(a.npad / kLoveMvRows), dim3(256), stream, a, j);
    for (int mode = 0; mode < 3; ++mode) GP_LAUNCH(gp_love_orth_kernel, dim3(nbo), dim3(256), stream, a, j, mode);
    GP_LAUNCH(gp_love_decide_kernel, dim3(1), dim3(256), stream, a, j, nbo);
    GP_LAUNCH(gp_love_next_kernel, dim3(nb), dim3(kLoveRows), stream, a, j);
    return hipSuccess;
}

hipError_t launch_gp_love_root(const GPLove& a, int m, double* R, int rp, hipStream_t stream) {
    if (!love_shape_ok(a) || m < 1 || m > a.rank || rp < m || !R) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(R, 0, (size_t)a.npad * rp * sizeof(double), stream);
    if (e != hipSuccess) return e;
    GP_LAUNCH(gp_love_root_kernel, dim3((a.npad + kLoveRows - 1) / kLoveRows), dim3(kLoveRows), stream, a, m, R, rp);
    return hipSuccess;
}

}  // namespace gpmpc
