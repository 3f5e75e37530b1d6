// The pick loop that gpmpc_gp_select, gpmpc_gp_inducing (gp_observe.hip) and gpmpc_gp_redundant (gp_drop.hip) share:
// a pivoted partial Cholesky as one launch per pick, no grid-wide barrier ("the pick loop").
// Launch t:
//   1. every workgroup reduces the previous launch's per-block bests to the same pick j_t (pick_reduce_blocks);
//   2. a workgroup of kPickBlock rows times kPickParts parts forms one inner product per row: each part is one
//      sequential sum of the kernel's own operands, and the parts are added as a balanced tree (pick_tree), so a
//      row's value does not depend on where it sits;
//   3. the first kPickBlock lanes build a candidate each from the new score (pick_candidate), reduce it over the group
//      (pick_group_best), and lane 0 leaves the block's best for the next launch (pick_store_best).
// The bests are double-buffered by the parity of t: launch t reads half t & 1 and writes the other.  The kernels
// declare the LDS arrays and pass them in.
#pragma once
#include "gpmpc_common.h"

namespace gpmpc {

constexpr int kPickParts = 16;
constexpr int kPickThreads = kPickBlock * kPickParts;
constexpr int kPickNone = 0x7fffffff;
constexpr bool kPickLargest = true, kPickSmallest = false;   // which finite score is the best (kLargest below)

// A block's best rows: the best finite score (kLargest: the largest, else the smallest; ties to the lower index; idx
// kPickNone: none) and the lowest index among the open rows whose score is not finite (kPickNone: none).  The order is
// total, so a reduction gives the same result in whatever order it merges.
struct PickBest {
    double val;
    int idx, nf;
};
__device__ __forceinline__ PickBest pick_none() { return PickBest{0.0, kPickNone, kPickNone}; }
template <bool kLargest>
__device__ __forceinline__ PickBest pick_merge(const PickBest& x, const PickBest& y) {
    PickBest r = x;
    const bool beats = kLargest ? y.val > x.val : y.val < x.val;
    if (y.idx != kPickNone && (x.idx == kPickNone || beats || (y.val == x.val && y.idx < x.idx))) {
        r.val = y.val;
        r.idx = y.idx;
    }
    r.nf = min(x.nf, y.nf);
    return r;
}
__device__ __forceinline__ PickBest pick_candidate(double s, int i, bool open) {
    const bool fin = isfinite(s);
    return PickBest{(open && fin) ? s : 0.0, (open && fin) ? i : kPickNone, (open && !fin) ? i : kPickNone};
}
// over each group of kPickBlock consecutive lanes; the group's first lane holds the result
template <bool kLargest>
__device__ __forceinline__ PickBest pick_group_best(PickBest b) {
#pragma unroll
    for (int off = kPickBlock / 2; off >= 1; off >>= 1) {
        PickBest o;
        o.val = __shfl_down(b.val, off, kPickBlock);
        o.idx = __shfl_down(b.idx, off, kPickBlock);
        o.nf = __shfl_down(b.nf, off, kPickBlock);
        b = pick_merge<kLargest>(b, o);
    }
    return b;
}

// The blocks' bests are bval[2][nblk] and, with kNf, bidx[2][nblk][2] = {idx, nf}; without, bidx[2][nblk] = idx and
// nf is kPickNone throughout.  `at` = half * nblk + block.
template <bool kNf>
__device__ __forceinline__ PickBest pick_load_best(const double* bval, const int32_t* bidx, size_t at) {
    return PickBest{bval[at], bidx[kNf ? 2 * at : at], kNf ? bidx[2 * at + 1] : kPickNone};
}
template <bool kNf>
__device__ __forceinline__ void pick_store_best(double* bval, int32_t* bidx, size_t at, const PickBest& b) {
    bval[at] = b.val;
    bidx[kNf ? 2 * at : at] = b.idx;
    if (kNf) bidx[2 * at + 1] = b.nf;
}

// Step 1: half `cur` of the blocks' bests reduced to the workgroup's pick, the same in every workgroup.  All
// kPickThreads threads call it; sval, sidx and (with kNf, else null) snf are LDS arrays of kPickThreads entries.
template <bool kLargest, bool kNf>
__device__ __forceinline__ PickBest pick_reduce_blocks(const double* bval, const int32_t* bidx, int nblk, int cur,
                                                       double* sval, int* sidx, int* snf) {
    const int tid = threadIdx.x;
    PickBest b = pick_none();
    for (int k = tid; k < nblk; k += kPickThreads)
        b = pick_merge<kLargest>(b, pick_load_best<kNf>(bval, bidx, (size_t)cur * nblk + k));
    sval[tid] = b.val;
    sidx[tid] = b.idx;
    if (kNf) snf[tid] = b.nf;
    __syncthreads();
    for (int s = kPickThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            const PickBest r = pick_merge<kLargest>(PickBest{sval[tid], sidx[tid], kNf ? snf[tid] : kPickNone},
                                                    PickBest{sval[tid + s], sidx[tid + s], kNf ? snf[tid + s] : kPickNone});
            sval[tid] = r.val;
            sidx[tid] = r.idx;
            if (kNf) snf[tid] = r.nf;
        }
        __syncthreads();
    }
    return PickBest{sval[0], sidx[0], kNf ? snf[0] : kPickNone};
}

// Step 2's end: the parts of row ci, ((0 + 1) + (2 + 3)) + ..
__device__ __forceinline__ double pick_tree(const double (*part)[kPickBlock], int ci) {
    double r[kPickParts];
#pragma unroll
    for (int q = 0; q < kPickParts; ++q) r[q] = part[q][ci];
#pragma unroll
    for (int w = kPickParts / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int q = 0; q < w; ++q) r[q] = r[2 * q] + r[2 * q + 1];
    return r[0];
}

}  // namespace gpmpc
