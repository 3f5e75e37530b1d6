// C ABI (include/gpmpc_mi355x.h): handle management, GP upload, batched control step.
#include "../../include/gpmpc_mi355x.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "gp_tile.h"   // (the tile pack's slot mapping)
#include "gpmpc_common.h"

using namespace gpmpc;

static_assert(GPMPC_STATS_SLOTS == kStatsSlots, "public stats-slot count must match the kernel's");

// A new handle's GPMPC_TUNE_VAR_TRIM (a variant build with -DGPMPC_VAR_TRIM_DEFAULT=0 runs the
// benchmark, which has no switch for it, on the untrimmed variance kernel)
#ifndef GPMPC_VAR_TRIM_DEFAULT
#define GPMPC_VAR_TRIM_DEFAULT 1
#endif

namespace {
thread_local std::string g_err;

gpmpc_status fail(gpmpc_status s, const std::string& msg) {
    g_err = msg;
    return s;
}

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(GPMPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

struct ModelDims {
    int nx, nu, ngp, nparams;
    int gp_dim[kMaxGP];
    int var_src[kMaxGP][3];
};

bool model_dims(int id, ModelDims& m) {
    switch (id) {
        case kQuad2D:
            m = ModelDims{6, 2, 2, 6, {1, 3, 0, 0}, {{6, 0, 0}, {4, 5, 7}, {0, 0, 0}, {0, 0, 0}}};
            return true;
        case kQuad3D:
            m = ModelDims{12, 4, 3, 9, {1, 3, 3, 0}, {{0, 0, 0}, {1, 2, 3}, {4, 5, 6}, {0, 0, 0}}};
            return true;
        case kCartpole:
            m = ModelDims{4, 1, 2, 4, {3, 3, 0, 0}, {{2, 3, 4}, {2, 3, 4}, {0, 0, 0}, {0, 0, 0}}};
            return true;
    }
    return false;
}

// What the handle keeps of one GP next to ProblemDev::gp[g] (GPDev: what the kernels read)
struct GPSlot {
    bool set = false, exact = false;   // uploaded; exactly (Xv == X)
    int npad = 0, cap = 0;   // padded rows of the factor; training rows the buffers hold (the uploaded size until reserved)
    double *rows = nullptr, *vrows = nullptr, *linvT = nullptr, *tiles = nullptr;   // tiles: tX | tW (MFMA tile pack)
    double* linvT_alt = nullptr;   // second factor buffer: the factor moves to it when npad changes, the two swap roles
    double *app = nullptr, *drp = nullptr, *rfc = nullptr;   // scratch of gpmpc_gp_append / _drop_oldest / _refactor
    double* fit = nullptr;         // tile partials and state block of gpmpc_gp_mll / _fit
    double* love = nullptr;        // Lanczos vectors, partial sums and state of gpmpc_gp_love_root
    double* ind = nullptr;         // d, bests, row state and state words of gpmpc_gp_inducing (InducingLayout)
    double* vroot = nullptr;       // LOVE root (tightening only), its padded columns and its rank
    int vroot_cols = 0, vroot_rank = 0;
    // FITC mean built by gpmpc_gp_fitc, an overlay on the exact mean: its rows, tile pack and indices (FitcOut) and
    // its inducing rows (0: none installed, the buffer is spare); the work space and the sizes it was allocated for
    double *fitc = nullptr, *fitc_ws = nullptr;
    int fitc_M = 0, fitc_ws_m = 0, fitc_ws_c = 0;
    // The slot's device buffers: the kReserved ones gpmpc_gp_reserve replaces, then the others
    static constexpr int kReserved = 10, kBuffers = 14;
    static constexpr double* GPSlot::*kBuffer[kBuffers] = {&GPSlot::rows,  &GPSlot::tiles, &GPSlot::linvT,
                                                            &GPSlot::linvT_alt, &GPSlot::app, &GPSlot::drp,
                                                            &GPSlot::rfc, &GPSlot::fit, &GPSlot::love, &GPSlot::ind,
                                                            &GPSlot::vrows, &GPSlot::vroot, &GPSlot::fitc,
                                                            &GPSlot::fitc_ws};
    hipError_t release(int count) {   // frees and clears the first `count` of them; returns the first error
        hipError_t first = hipSuccess;
        for (int i = 0; i < count; ++i) {
            double*& p = this->*kBuffer[i];
            const hipError_t e = p ? hipFree(p) : hipSuccess;
            if (first == hipSuccess) first = e;
            p = nullptr;
        }
        return first;
    }
    void drop_root() {   // back to the exact variance: root, columns and rank together
        if (vroot) (void)hipFree(vroot);
        vroot = nullptr;
        vroot_cols = vroot_rank = 0;
    }
};
// Scratch of the three device-side updates for a capacity of c (padded) rows, in doubles: the offsets
// gpmpc_gp_append / _drop_oldest / _refactor carve their buffer at and the size (end) gpmpc_gp_reserve allocates
struct AppendLayout {   // W^T [16][c] | per-tile means [c/16][16] | L_b^-1 [256] | beta [16] | status word
    size_t c, wt = 0, pmean = 16 * c, lbinv = pmean + c, beta = lbinv + 256, flag = beta + 16, end = flag + 1;
};
// V^T [16][c] | M21 g [c] | E_T, D_T [c/16][256] each | staged rows [c][4], tX, tW [c/16][64] each | status word |
// gpmpc_gp_drop_rows: the sorted rows [c] and the membership mask [c] int32 (in c/2 doubles each) | the call's status
struct DropLayout {
    size_t c, vt = 0, w = 16 * c, et = w + c, dt = et + 16 * c, srows = dt + 16 * c, stX = srows + 4 * c,
              stW = stX + 4 * c, flag = stW + 4 * c, sorted = flag + 1, mask = sorted + c / 2, acc = mask + c / 2,
              end = acc + 1;
};
// L_kk^-1 [c/16][256] | w [c] | masked targets [c] | the inert mask [c] int32 (in c/2 doubles) | status word
struct RefactorLayout {
    size_t c, dinv = 0, w = 16 * c, ym = w + c, mask = ym + c, flag = mask + c / 2, end = flag + 1;
};
// the lower tiles' partial sums [c/16 (c/16 + 1) / 2][3] | the fit-state block (gpmpc_common.h kFit*)
struct FitLayout {
    size_t c, part = 0, state = 3 * ((c / 16) * (c / 16 + 1) / 2), end = state + kFitDoubles;
};
// Q^T [256][c] | v [c] | the inert mask [c] int32 (in c/2 doubles) | parts of alpha [c/16] | parts of Q^T v, two
// buffers [ceil(c/64)][256] each | parts of |v|^2 [ceil(c/64)] and of the live count [ceil(c/256)] | alpha, beta, the
// bidiagonal factor's diagonal and subdiagonal [256] each | the state words (gpmpc_common.h kLove*)
struct LoveLayout {
    size_t c, nb = (c + 255) / 256, nbo = (c + 63) / 64, qt = 0, v = kLoveMaxRank * c, mask = v + c, apart = mask + c / 2,
              cpa = apart + c / 16, cpb = cpa + 256 * nbo, npart = cpb + 256 * nbo, ipart = npart + nbo, alpha = ipart + nb,
              beta = alpha + kLoveMaxRank, cd = beta + kLoveMaxRank, lsub = cd + kLoveMaxRank, state = lsub + kLoveMaxRank,
              end = state + kLoveInts / 2;
};
// gpmpc_gp_fitc's work space for m (padded) inducing rows of a GP with a capacity of c (padded) rows: K_ss / B and
// the two inverse factors [m][m] each | L_kk^-1 [m/16][256] | Gamma^-1, Gamma^-1 y [c] each | u, p, q [m] each | the
// inert mask [c] and the padding mask [m] int32 | status word
struct FitcLayout {
    size_t m, c, A = 0, lt1 = m * m, lt2 = 2 * m * m, dinv = 3 * m * m, ginv = dinv + 16 * m, t = ginv + c, u = t + c,
              p = u + m, q = p + m, lmask = q + m, smask = lmask + c / 2, flag = smask + m / 2, end = flag + 1;
};
// Scratch of gpmpc_gp_inducing for a capacity of c (padded) rows, in doubles: d [2][c] | the blocks' best scores
// [2][c/16] | their indices [2][c/16] int32 | the rows' state [c] int32 | the state words (gpmpc_common.h kInd*).
// The l columns go into the second factor buffer.
struct InducingLayout {
    size_t c, nb = c / kPickBlock, d = 0, bval = 2 * c, bidx = bval + 2 * nb, state = bidx + nb,
              flag = state + c / 2, end = flag + kIndInts / 2;
};
static_assert(kPickBlock == 16, "InducingLayout takes its blocks to be the 16 rows a capacity is padded to");
// what it installs: rows [m][4] | tX, tW [m/16][64] each | the indices [m] int32
struct FitcOut {
    size_t m, rows = 0, tX = 4 * m, tW = 8 * m, idx = 12 * m, end = idx + m / 2;
};
// Scratch of gpmpc_gp_informative and gpmpc_gp_observe for b = max_batch points of a model with D = sum d_g GP inputs
// and g GPs, in doubles: gathered inputs [b][D] | variances [g][b] | scores [b] | staged X_g [b][d_g], GP after GP |
// staged y_g [g][b]
struct ObserveLayout {
    size_t b, D, g, zin = 0, var = b * D, score = var + g * b, sx = score + b, sy = sx + b * D, end = sy + g * b;
};
// Scratch of gpmpc_gp_select for max_batch = b candidates (stride ldp: b rounded up to the pick loop's block) and GPs
// of c_g padded rows, in doubles: V_g^T [c_g][ldp], GP after GP | the l columns [g][256][ldp] | d [2][g][ldp] | the
// blocks' best scores [2][nblk] | their indices [2][nblk][2] int32 | the candidates' state [ldp] int32
struct SelectLayout {
    size_t ldp, nblk, g, vt[kMaxGP], lcol, d, bval, bidx, state, end;
    SelectLayout(size_t b, size_t ngp, const size_t* rows) {
        ldp = (b + kPickBlock - 1) / kPickBlock * kPickBlock;
        nblk = ldp / kPickBlock;
        g = ngp;
        size_t at = 0;
        for (size_t q = 0; q < (size_t)kMaxGP; ++q) {
            vt[q] = at;
            if (q < ngp) at += rows[q] * ldp;
        }
        lcol = at;
        d = lcol + ngp * kSelectMaxPicks * ldp;
        bval = d + 2 * ngp * ldp;
        bidx = bval + 2 * nblk;
        state = bidx + 2 * nblk;
        end = state + ldp / 2;
    }
};
// Scratch of gpmpc_gp_redundant for g GPs of at most ldn (padded) rows and mcap picks, in doubles: the c columns
// [g][mcap][ldn] | p [2][g][ldn] | the blocks' best scores [2][nblk] | their indices [2][nblk][2] int32 | the rows'
// state [ldn] int32
struct RedundantLayout {
    size_t ldn, mcap, g, nblk = ldn / kPickBlock, ccol = 0, p = g * mcap * ldn, bval = p + 2 * g * ldn,
                         bidx = bval + 2 * nblk, state = bidx + 2 * nblk, end = state + ldn / 2;
};
constexpr bool layouts_hold(size_t c) {
    return AppendLayout{c}.end == 16 * c + c + 256 + 16 + 1 && AppendLayout{c}.flag == 17 * c + 272 &&
           DropLayout{c}.flag == 61 * c && DropLayout{c}.end == 62 * c + 2 && DropLayout{c}.srows == 49 * c && RefactorLayout{c}.mask == 18 * c &&
           RefactorLayout{c}.end == 18 * c + c / 2 + 1 && LoveLayout{c}.v == 256 * c &&
           LoveLayout{c}.end == 257 * c + c / 2 + c / 16 + 513 * ((c + 63) / 64) + (c + 255) / 256 + 4 * 256 + 4;
}
static_assert(layouts_hold(16) && layouts_hold(4096), "scratch layouts of the GP updates changed size or offsets");
}  // namespace

struct gpmpc_handle {
    int device = 0;
    int model = 0;
    int H = 0;
    int max_batch = 0;
    ModelDims md{};
    int nb = 0;
    bool model_set = false, ref_set = false;
    bool any_prev = false;
    ProblemDev P{};
    // device state
    double *x = nullptr, *u = nullptr, *pi = nullptr, *lam = nullptr, *var = nullptr, *tight = nullptr;
    int32_t* has_prev = nullptr;
    double* lin = nullptr;          // linearisation cache of the stored iterate (StateDev::lin)
    int32_t* lin_tag = nullptr;
    int32_t* t_prev = nullptr;      // reference index of each instance's last good solve (StateDev::t_prev)
    bool lin_cache = true;          // GPMPC_TUNE_LIN_CACHE
    int32_t* order = nullptr;       // cost-ordered dispatch (StateDev::order / cost)
    uint32_t* cost = nullptr;
    double* traj = nullptr;
    double* tgain = nullptr;        // [H][nb][n_unc] tightening gain table (ProblemDev::tgain)
    GPSlot gp[kMaxGP];
    // optional per-kernel HIP-event timing (bench.py's roofline leg)
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    // whether each profiling event was created fenced (GPMPC_TUNE_EVENT_FENCE at its creation): events
    // still in ev_var / ev_sqp when the option changes return to the pool later and are dropped there
    std::unordered_map<hipEvent_t, bool> ev_fenced;
    // (start, end) per launch; a variance launch's end event is also the following SQP launch's
    // start (one event between the two kernels), so the SQP list owns it
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_var, ev_sqp;
    // end events of ev_var pairs that no SQP pair took over (the SQP launch failed or got no
    // end event): the variance list returns these to the pool itself
    std::vector<hipEvent_t> ev_var_owned;
    unsigned long long* timing = nullptr;  // diagnostic phase cycles (GPMPC_TIMING builds)
    long long* stats = nullptr;            // optional per-instance solver statistics accumulators
    int32_t* scratch_i = nullptr;   // [2][max_batch]
    double* scratch_d = nullptr;    // [max_batch][4]
    double* obs = nullptr;          // scratch of gpmpc_gp_informative / gpmpc_gp_observe (ObserveLayout), on first use
    double* roll = nullptr;         // scratch of gpmpc_rollout: the gathered variance inputs [P T][sum d_g], kept for a
    size_t roll_doubles = 0;        // later call of the same or a smaller size
    double* sel = nullptr;          // scratch of gpmpc_gp_select (SelectLayout), on first use and when a capacity has grown
    size_t sel_rows[kMaxGP] = {0, 0, 0, 0};   // the padded rows its V regions were sized for
    double* red = nullptr;          // scratch of gpmpc_gp_redundant (RedundantLayout), on first use and when a capacity has grown
    size_t red_rows = 0, red_m = 0; // the padded rows and the picks it was sized for
    // the batch whose tightening variances the last solve's variance launch wrote into `var`
    // (0: the last solve ran none, var is stale or unset)
    int var_batch = 0;
    // stream of the last call that queued work on the handle's device state and an event recorded
    // on it when that call returned: a call on another stream first waits for the event
    // (order_after_last / StreamMark), so consecutive calls never overlap
    hipStream_t last_stream = nullptr;
    hipEvent_t ev_last = nullptr;
    bool ev_last_valid = false;
    bool tail_unmarked = false;     // last_stream holds work queued after ev_last was recorded (DeferredMark)
    // overlapped steps (gpmpc_solve): the second half's variance and SQP launches run on `side`,
    // forked from and joined back into the caller's stream by two events
    bool overlap = true;            // GPMPC_TUNE_OVERLAP
    int var_split = 0;              // GPMPC_TUNE_VAR_SPLIT
    bool var_trim = GPMPC_VAR_TRIM_DEFAULT != 0;   // GPMPC_TUNE_VAR_TRIM
    bool event_fence = false;       // GPMPC_TUNE_EVENT_FENCE
    double* stage_cost = nullptr;   // caller's [max_batch][H+1] stage-cost buffer (StepIO::stage_cost)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // tail boost (GPMPC_TUNE_TAIL): the costliest `tail` instances of a one-wave, one-round step run
    // as two-wave segment solves on the caller's stream, the others' one-wave launch on `side`
    // (-1: as many as the launch leaves SIMDs free, sqp_tail_spare)
    int tail = -1;
};

// The handle's device state (iterate, multipliers, variances, dispatch order) is read and written
// by every queued call, so calls on different streams must not overlap.  Each such call ends by
// recording the handle's event on its stream (StreamMark); a call on another stream first makes
// its stream wait for that event.  No host synchronisation, and a destroyed previous stream leaves
// nothing dangling (the event outlives it).
static hipError_t order_after_last(gpmpc_handle* h, hipStream_t s) {
    if (!h->ev_last) {
        const hipError_t e = hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming);
        if (e != hipSuccess) {
            h->ev_last = nullptr;
            return e;
        }
    }
    if (h->last_stream == s) return hipSuccess;
    if (h->tail_unmarked) {
        // gpmpc_plant_step's deferred record (DeferredMark), made up for now that a call on another stream needs
        // it.  If the stream has been destroyed meanwhile the older record stands: it still orders every call that
        // touched the handle's device state.
        if (hipEventRecord(h->ev_last, h->last_stream) == hipSuccess) {
            h->ev_last_valid = true;
        } else {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(h->last_stream);
            (void)hipGetLastError();
        }
        h->tail_unmarked = false;
    }
    if (h->ev_last_valid) return hipStreamWaitEvent(s, h->ev_last, 0);
    return hipSuccess;
}
// Records the handle's event on the call's stream when the call returns, whatever it queued.  If
// the record fails the stream is drained on the host instead, so the next call needs no wait.
struct StreamMark {
    gpmpc_handle* h;
    hipStream_t s;
    ~StreamMark() {
        if (h->ev_last && hipEventRecord(h->ev_last, s) == hipSuccess) {
            h->ev_last_valid = true;
        } else {
            (void)hipStreamSynchronize(s);
            h->ev_last_valid = false;
        }
        h->last_stream = s;
        h->tail_unmarked = false;
    }
};
// gpmpc_plant_step's mark.  The call touches nothing of the handle on the device and closes every step of a control
// loop, where a second event record per step is a dispatch gap of several microseconds for nothing (the next call comes
// on the same stream).  So it only notes that its stream holds work behind the last record; order_after_last records
// the event when a call arrives on another stream.  The stream must still exist then for the launch to be waited for.
struct DeferredMark {
    gpmpc_handle* h;
    hipStream_t s;
    ~DeferredMark() {
        h->last_stream = s;
        h->tail_unmarked = true;
    }
};

// The second stream of overlapped and tail-boosted steps and its fork / join events (lowest
// priority), created together on first use or not at all.
static hipError_t ensure_side(gpmpc_handle* h) {
    if (h->side) return hipSuccess;
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hipError_t ce = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, lo);   // lowest priority
    if (ce == hipSuccess) ce = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
    if (ce == hipSuccess) ce = hipEventCreateWithFlags(&join, hipEventDisableTiming);
    if (ce != hipSuccess) {
        if (join) (void)hipEventDestroy(join);
        if (fork) (void)hipEventDestroy(fork);
        if (side) (void)hipStreamDestroy(side);
        return ce;
    }
    h->side = side;
    h->ev_fork = fork;
    h->ev_join = join;
    return hipSuccess;
}

// Instances the tail boost runs on two waves for this step (0: none, the ordinary launch)
static int tail_count(const gpmpc_handle* h, const ProblemDev& P, int batch) {
    if (h->tail == 0 || !sqp_tail_ok(P, batch)) return 0;
    return h->tail < 0 ? sqp_tail_spare(P, batch) : std::min(h->tail, batch - 1);
}

static hipEvent_t take_event(gpmpc_handle* h) {
    while (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        const auto it = h->ev_fenced.find(e);
        if (it != h->ev_fenced.end() && it->second == h->event_fence) return e;
        // created under the other GPMPC_TUNE_EVENT_FENCE setting: an A/B run must not mix them
        if (it != h->ev_fenced.end()) h->ev_fenced.erase(it);
        (void)hipEventDestroy(e);
    }
    hipEvent_t e = nullptr;
    // timing-only events: no system-scope fence (cache writeback / invalidate) when recorded,
    // which otherwise adds ~5 us of dispatch gap around every kernel it brackets
    const unsigned flags = h->event_fence ? hipEventDefault : hipEventDisableSystemFence;
    if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
    h->ev_fenced[e] = h->event_fence;
    return e;
}

// Invalidate every instance's linearisation cache (StateDev::lin): the iterate, the GPs or the
// model changed.  Tags written by earlier launches no longer match the new generation.
static void bump_lin(gpmpc_handle* h) {
    if (++h->P.lin_gen <= 0) h->P.lin_gen = 1;
}

static void free_handle(gpmpc_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (auto& pr : h->ev_var) h->ev_pool.push_back(pr.first);
    for (hipEvent_t e : h->ev_var_owned) h->ev_pool.push_back(e);
    for (auto& pr : h->ev_sqp) { h->ev_pool.push_back(pr.first); h->ev_pool.push_back(pr.second); }
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->ev_last) (void)hipEventDestroy(h->ev_last);
    if (h->side) (void)hipStreamDestroy(h->side);
    for (double* p : {h->x, h->u, h->pi, h->lam, h->var, h->tight, h->traj, h->tgain, h->lin})
        if (p) (void)hipFree(p);
    if (h->has_prev) (void)hipFree(h->has_prev);
    if (h->lin_tag) (void)hipFree(h->lin_tag);
    if (h->t_prev) (void)hipFree(h->t_prev);
    if (h->order) (void)hipFree(h->order);
    if (h->cost) (void)hipFree(h->cost);
    if (h->scratch_i) (void)hipFree(h->scratch_i);
    if (h->scratch_d) (void)hipFree(h->scratch_d);
    if (h->obs) (void)hipFree(h->obs);
    if (h->roll) (void)hipFree(h->roll);
    if (h->sel) (void)hipFree(h->sel);
    if (h->red) (void)hipFree(h->red);
    for (GPSlot& gs : h->gp) (void)gs.release(GPSlot::kBuffers);
    delete h;
}

extern "C" {

const char* gpmpc_last_error(void) { return g_err.c_str(); }

int64_t gpmpc_lds_bytes(int32_t model_id, int32_t horizon) {
    return (int64_t)sqp_lds_bytes(model_id, horizon);
}

gpmpc_status gpmpc_create(int32_t model_id, int32_t horizon, int32_t max_batch, int32_t device, gpmpc_handle** out) {
    if (!out) return fail(GPMPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    ModelDims md;
    if (!model_dims(model_id, md)) return fail(GPMPC_ERR_ARG, "unknown model id " + std::to_string(model_id));
    if (horizon < 1 || horizon > kMaxH) return fail(GPMPC_ERR_ARG, "horizon must be in [1, 63]");
    if (max_batch < 1) return fail(GPMPC_ERR_ARG, "max_batch must be >= 1");
    auto* h = new gpmpc_handle();
    h->device = device;
    h->model = model_id;
    h->H = horizon;
    h->max_batch = max_batch;
    h->md = md;
    h->nb = md.nx + md.nu;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        delete h;
        return fail(GPMPC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    }
    const size_t B = max_batch, H = horizon;
    struct A { void** p; size_t bytes; } allocs[] = {
        {(void**)&h->x, B * (H + 1) * md.nx * sizeof(double)},
        {(void**)&h->u, B * H * md.nu * sizeof(double)},
        {(void**)&h->pi, B * H * md.nx * sizeof(double)},
        {(void**)&h->lam, B * (H + 1) * 2 * h->nb * sizeof(double)},
        {(void**)&h->var, B * H * md.ngp * sizeof(double)},
        {(void**)&h->tight, B * (H + 1) * h->nb * sizeof(double)},
        {(void**)&h->has_prev, B * sizeof(int32_t)},
        {(void**)&h->lin, B * H * md.nx * (h->nb + 1) * sizeof(double)},
        {(void**)&h->lin_tag, B * sizeof(int32_t)},
        {(void**)&h->order, B * sizeof(int32_t)},
        {(void**)&h->cost, B * sizeof(uint32_t)},
        {(void**)&h->scratch_i, 2 * B * sizeof(int32_t)},
        {(void**)&h->scratch_d, 4 * B * sizeof(double)},
    };
    for (auto& a : allocs) {
        e = hipMalloc(a.p, a.bytes);
        if (e == hipSuccess) e = hipMemset(*a.p, 0, a.bytes);
        if (e != hipSuccess) {
            free_handle(h);
            return fail(GPMPC_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
    }
    ProblemDev& P = h->P;
    P.model = model_id;
    P.nx = md.nx;
    P.nu = md.nu;
    P.H = horizon;
    P.n_gp = md.ngp;
    P.use_gp = 0;
    P.cost_scale = 1.0;
    P.uh = -1e-8;
    P.tighten = 0;
    P.max_iter = 25;          // gpmpc.py:262
    P.tol_stat = P.tol_eq = P.tol_ineq = P.tol_comp = 1e-6;  // acados defaults
    P.qp_max_iter = 50;   // acados qp_solver_iter_max default
    // QP tolerances = the NLP tolerances: gpmpc.py:257-263 leaves qp_solver_tol_* unset, and acados'
    // SQP passes each NLP tolerance it is given (tol_stat/eq/ineq/comp, 1e-6 by default) on to the QP
    // solver as that solver's tolerance (ocp_nlp_sqp_opts_set -> qp_solver opts_set "tol_stat", ...)
    P.qp_tol = 1e-6;
    P.qp_mu0 = 1.0;
    P.lin_gen = 1;   // tags start at 0: nothing cached
    P.waves = 0;            // automatic launch shape (gpmpc_set_launch)
    P.order_dispatch = 1;   // cost-ordered dispatch of multi-round launches (GPMPC_TUNE_ORDER)
    P.seg = 1;              // segment-parallel Newton solves (GPMPC_TUNE_SEG)
    P.seg_piv_rel = 1e-10;  // their boundary chain's pivot threshold (GPMPC_TUNE_SEG_PIVOT)
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
        P.n_cu = ncu;
    }
    // t_prev = -1: no instance has a solve to shift from (GPMPC_TUNE_SHIFT)
    e = hipMalloc((void**)&h->t_prev, B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->t_prev, 0xff, B * sizeof(int32_t));
    if (e != hipSuccess) {
        free_handle(h);
        return fail(GPMPC_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    P.shift = 0;            // one-stage shifted warm start (GPMPC_TUNE_SHIFT)
    const size_t lds = sqp_lds_bytes(model_id, horizon);
    if (lds > 160 * 1024) {
        free_handle(h);
        return fail(GPMPC_ERR_ARG, "horizon too long for the LDS budget (" + std::to_string(lds) + " bytes)");
    }
    *out = h;
    return GPMPC_OK;
}

void gpmpc_destroy(gpmpc_handle* h) { free_handle(h); }

gpmpc_status gpmpc_set_model(gpmpc_handle* h, const double* params, int32_t n_params, double dt, const double* x_lo,
                             const double* x_hi, const double* u_lo, const double* u_hi, const double* q_diag,
                             const double* r_diag, const double* u_eq, double uh, int32_t cost_scaling) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (!params || !x_lo || !x_hi || !u_lo || !u_hi || !q_diag || !r_diag || !u_eq)
        return fail(GPMPC_ERR_ARG, "null array");
    if (n_params != h->md.nparams)
        return fail(GPMPC_ERR_ARG, "model expects " + std::to_string(h->md.nparams) + " parameters");
    if (!(dt > 0.0)) return fail(GPMPC_ERR_ARG, "dt must be > 0");
    ProblemDev& P = h->P;
    std::memset(P.params, 0, sizeof(P.params));
    for (int i = 0; i < n_params; ++i) P.params[i] = params[i];
    P.dt = dt;
    for (int i = 0; i < h->md.nx; ++i) {
        P.x_lo[i] = x_lo[i];
        P.x_hi[i] = x_hi[i];
        P.q[i] = q_diag[i];
        if (!(q_diag[i] >= 0.0)) return fail(GPMPC_ERR_ARG, "q_diag must be >= 0");
    }
    for (int a = 0; a < h->md.nu; ++a) {
        P.u_lo[a] = u_lo[a];
        P.u_hi[a] = u_hi[a];
        P.r[a] = r_diag[a];
        P.u_eq[a] = u_eq[a];
        if (!(r_diag[a] > 0.0)) return fail(GPMPC_ERR_ARG, "r_diag must be > 0 (GN Hessian)");
    }
    P.uh = uh;
    P.cost_scale = cost_scaling ? dt : 1.0;
    bump_lin(h);
    h->model_set = true;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_reference(gpmpc_handle* h, const double* traj, int32_t L) {
    if (!h || !traj || L < 1) return fail(GPMPC_ERR_ARG, "bad reference");
    (void)hipSetDevice(h->device);
    const int nx = h->md.nx;
    std::vector<double> tm((size_t)L * nx);
    for (int t = 0; t < L; ++t)
        for (int i = 0; i < nx; ++i) tm[(size_t)t * nx + i] = traj[(size_t)i * L + t];
    if (h->traj) HIPCHK(hipFree(h->traj));
    h->traj = nullptr;
    HIPCHK(hipMalloc(&h->traj, tm.size() * sizeof(double)));
    HIPCHK(hipMemcpy(h->traj, tm.data(), tm.size() * sizeof(double), hipMemcpyHostToDevice));
    h->P.traj = h->traj;
    h->P.traj_len = L;
    h->ref_set = true;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_options(gpmpc_handle* h, int32_t max_iter, double tol_stat, double tol_eq, double tol_ineq,
                               double tol_comp, int32_t qp_max_iter, double qp_tol, double qp_mu0) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (max_iter < 0 || qp_max_iter < 1 || !(qp_mu0 > 0.0)) return fail(GPMPC_ERR_ARG, "bad options");
    ProblemDev& P = h->P;
    P.max_iter = max_iter;
    P.tol_stat = tol_stat;
    P.tol_eq = tol_eq;
    P.tol_ineq = tol_ineq;
    P.tol_comp = tol_comp;
    P.qp_max_iter = qp_max_iter;
    P.qp_tol = qp_tol;
    P.qp_mu0 = qp_mu0;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_gp(gpmpc_handle* h, int32_t gp_id, int32_t n, int32_t d, const double* X, const double* alpha,
                          int32_t nv, const double* Xv, const double* Linv, double lengthscale, double outputscale,
                          double noise) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    if (d != h->md.gp_dim[gp_id])
        return fail(GPMPC_ERR_ARG, "GP " + std::to_string(gp_id) + " expects input dimension " +
                                       std::to_string(h->md.gp_dim[gp_id]));
    if (n < 1 || !X || !alpha) return fail(GPMPC_ERR_ARG, "empty GP");
    if (!(lengthscale > 0.0) || !(outputscale > 0.0) || !(noise >= 0.0)) return fail(GPMPC_ERR_ARG, "bad hyperparameters");
    if (!Xv) { Xv = X; nv = n; }
    if (nv < 1) return fail(GPMPC_ERR_ARG, "empty variance GP");
    (void)hipSetDevice(h->device);
    auto pack = [&](const double* Xs, const double* w, int m, std::vector<double>& out) {
        const int mp = (m + 15) / 16 * 16;
        out.assign((size_t)mp * 4, 0.0);
        for (int i = 0; i < m; ++i) {
            for (int k = 0; k < d; ++k) out[(size_t)i * 4 + k] = Xs[(size_t)i * d + k];
            out[(size_t)i * 4 + 3] = w ? w[i] : 0.0;
        }
    };
    std::vector<double> rows, vrows;
    pack(X, alpha, n, rows);
    const bool exact = (Xv == X);
    if (!exact) pack(Xv, nullptr, nv, vrows);
    const int npad = (nv + 15) / 16 * 16;
    // MFMA tile pack of the mean rows, centred on their mean (sqp_kernel.hip gp_tiles)
    const double c = -0.5 / (lengthscale * lengthscale);
    double xbar[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < d; ++k) xbar[k] += X[(size_t)i * d + k] / n;
    const int ntile = (n + 15) / 16;
    std::vector<double> tiles((size_t)ntile * (64 + 64), 0.0);
    double* tX = tiles.data();
    double* tW = tiles.data() + (size_t)ntile * 64;
    const double m2c = 1.0 / (lengthscale * lengthscale);
    for (int i = 0; i < n; ++i) {
        const TileSlot sl = tile_slot(i);   // (gp_tile.h: the layout the device-side updates write too)
        double xc[3] = {0.0, 0.0, 0.0}, sq = 0.0;
        for (int k = 0; k < d; ++k) {
            xc[k] = X[(size_t)i * d + k] - xbar[k];
            sq += xc[k] * xc[k];
            tX[tile_x_at(sl) + k] = m2c * xc[k];
        }
        tX[tile_x_at(sl) + 3] = c * sq;
        const double wv[4] = {alpha[i], alpha[i] * xc[0], alpha[i] * xc[1], alpha[i] * xc[2]};
        for (int j = 0; j < 4; ++j) tW[tile_w_at(sl, j)] = wv[j];
    }
    GPSlot& gs = h->gp[gp_id];
    HIPCHK(gs.release(GPSlot::kBuffers));   // (a LOVE root and a FITC mean belong to the previous training set)
    gs.vroot_cols = gs.vroot_rank = 0;
    gs.fitc_M = gs.fitc_ws_m = gs.fitc_ws_c = 0;
    HIPCHK(hipMalloc(&gs.rows, rows.size() * sizeof(double)));
    HIPCHK(hipMemcpy(gs.rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&gs.tiles, tiles.size() * sizeof(double)));
    HIPCHK(hipMemcpy(gs.tiles, tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!exact) {
        HIPCHK(hipMalloc(&gs.vrows, vrows.size() * sizeof(double)));
        HIPCHK(hipMemcpy(gs.vrows, vrows.data(), vrows.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (Linv) {
        std::vector<double> lt((size_t)npad * npad, 0.0);
        for (int i = 0; i < nv; ++i)
            for (int j = 0; j <= i; ++j) lt[(size_t)j * npad + i] = Linv[(size_t)i * nv + j];  // (L^-1)^T
        HIPCHK(hipMalloc(&gs.linvT, lt.size() * sizeof(double)));
        HIPCHK(hipMemcpy(gs.linvT, lt.data(), lt.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    GPDev& g = h->P.gp[gp_id];
    g.rows = gs.rows;
    g.vrows = exact ? gs.rows : gs.vrows;
    g.linvT = gs.linvT;
    g.tX = gs.tiles;
    g.tW = gs.tiles + (size_t)ntile * 64;
    g.ntile = ntile;
    for (int k = 0; k < 3; ++k) g.xbar[k] = xbar[k];
    g.n = n;
    g.nv = nv;
    g.d = d;
    g.inv_ell2 = 1.0 / (lengthscale * lengthscale);
    g.sf2 = outputscale;
    g.sn2 = noise;
    gs.npad = npad;
    gs.cap = n;   // (appending needs gpmpc_gp_reserve)
    gs.exact = exact;
    gs.set = true;
    bump_lin(h);
    return GPMPC_OK;
}

// A device-side update as the refusals word it ("append" needs ..; only an exact GP "takes appended rows"; a LOVE root
// belongs to "the old training set") and its scratch, which comes with the second factor buffer (null: not asked for)
struct GPUpdate {
    const char *verb, *takes, *root_of;
    double* GPSlot::*scratch;
    bool keeps_fitc = false;   // a FITC mean built by gpmpc_gp_fitc is no obstacle (the others change what it was built from)
};
static const GPUpdate kAppend{"append", "takes appended rows", "the old training set", nullptr};
static const GPUpdate kDrop{"drop", "drops rows", "the old training set", &GPSlot::drp};
static const GPUpdate kRefactor{"refactor", "is refactorised", "the old factor", &GPSlot::rfc};
static const GPUpdate kMll{"the likelihood", "has its likelihood evaluated", "the old factor", &GPSlot::fit};
static const GPUpdate kFit{"fit", "is fitted", "the old factor", &GPSlot::fit};
// (root_of null: an installed root is no obstacle, the call replaces it)
static const GPUpdate kLove{"the LOVE root", "has its LOVE root built", nullptr, &GPSlot::love, true};
static const GPUpdate kFitc{"the FITC mean", "has its FITC mean built", nullptr, &GPSlot::rfc, true};
static const GPUpdate kInducing{"the inducing rows' selection", "has its inducing rows picked", nullptr, &GPSlot::ind, true};

// What the three updates ask first, in this order (bad_args: what is wrong with the call's own arguments, or
// null).  gpmpc_gp_reserve asks the same up to the exact upload (factor = false).
static gpmpc_status gp_update_ready(gpmpc_handle* h, int gp_id, const GPUpdate& op, const char* bad_args,
                                    bool factor = true) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    if (bad_args) return fail(GPMPC_ERR_ARG, bad_args);
    const GPSlot& gs = h->gp[gp_id];
    if (!gs.set) return fail(GPMPC_ERR_STATE, "GP not set (gpmpc_set_gp first)");
    if (!gs.exact) return fail(GPMPC_ERR_STATE, std::string("FITC upload (Xv != X): only an exact GP ") + op.takes);
    if (gs.fitc_M && !op.keeps_fitc)
        return fail(GPMPC_ERR_STATE, "a FITC mean is installed: it belongs to the old training set (drop it first, "
                                     "gpmpc_gp_fitc with M = 0, or rebuild it afterwards)");
    if (!factor) return GPMPC_OK;
    if (!gs.linvT) return fail(GPMPC_ERR_STATE, std::string(op.verb) + " needs Linv (the GP was set without it)");
    if (gs.vroot && op.root_of)
        return fail(GPMPC_ERR_STATE, std::string("a LOVE root is installed: it belongs to ") + op.root_of +
                                         " (drop it first, gpmpc_set_gp_variance_root with R = NULL)");
    if (op.scratch && (!(gs.*op.scratch) || !gs.linvT_alt))
        return fail(GPMPC_ERR_STATE, std::string(op.verb) + " needs the second factor buffer (gpmpc_gp_reserve first)");
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_reserve(gpmpc_handle* h, int32_t gp_id, int32_t capacity) {
    const gpmpc_status ready = gp_update_ready(h, gp_id, kAppend, nullptr, false);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    GPDev& g = h->P.gp[gp_id];
    if (capacity < g.n) return fail(GPMPC_ERR_ARG, "capacity below the GP's " + std::to_string(g.n) + " training rows");
    if (capacity > (1 << 15)) return fail(GPMPC_ERR_ARG, "capacity above 32768 rows");
    (void)hipSetDevice(h->device);
    HIPCHK(hipDeviceSynchronize());   // a setup call: nothing queued still reads the buffers replaced below
    const size_t cpad = ((size_t)capacity + 15) / 16 * 16, ct = cpad / 16;
    const size_t npad = gs.npad, nt = g.ntile;
    const bool lin = gs.linvT != nullptr;
    // everything is allocated and filled before the handle changes: `fresh` holds the new buffers
    GPSlot fresh;
    const struct { double** p; size_t doubles; bool zero; } want[] = {
        {&fresh.rows, cpad * 4, true},
        {&fresh.tiles, 2 * ct * 64, true},
        {&fresh.linvT, lin ? cpad * cpad : 0, false},
        {&fresh.linvT_alt, lin ? cpad * cpad : 0, false},
        {&fresh.app, lin ? AppendLayout{cpad}.end : 0, true},
        {&fresh.drp, lin ? DropLayout{cpad}.end : 0, true},
        {&fresh.rfc, lin ? RefactorLayout{cpad}.end : 0, true},
        {&fresh.fit, lin ? FitLayout{cpad}.end : 0, true},
        {&fresh.love, lin ? LoveLayout{cpad}.end : 0, true},
        {&fresh.ind, lin ? InducingLayout{cpad}.end : 0, true},
    };
    hipError_t e = hipSuccess;
    auto undo = [&](gpmpc_status st, const char* what) {
        (void)fresh.release(GPSlot::kReserved);
        return fail(st, std::string(what) + hipGetErrorString(e));
    };
    for (const auto& w : want)
        if (e == hipSuccess && w.doubles) e = hipMalloc(w.p, w.doubles * sizeof(double));
    if (e != hipSuccess) return undo(GPMPC_ERR_NOMEM, "hipMalloc: ");
    for (const auto& w : want)
        if (e == hipSuccess && w.doubles && w.zero) e = hipMemset(*w.p, 0, w.doubles * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(fresh.rows, gs.rows, npad * 4 * sizeof(double), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(fresh.tiles, g.tX, nt * 64 * sizeof(double), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(fresh.tiles + ct * 64, g.tW, nt * 64 * sizeof(double), hipMemcpyDeviceToDevice);
    // the factor keeps its stride npad (the variance kernels' layout) at the head of the first buffer
    if (e == hipSuccess && lin) e = hipMemcpy(fresh.linvT, gs.linvT, npad * npad * sizeof(double), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return undo(GPMPC_ERR_HIP, "gpmpc_gp_reserve: ");
    (void)gs.release(GPSlot::kReserved);
    for (int i = 0; i < GPSlot::kReserved; ++i) gs.*GPSlot::kBuffer[i] = fresh.*GPSlot::kBuffer[i];
    g.rows = g.vrows = gs.rows;
    g.linvT = gs.linvT;
    g.tX = gs.tiles;
    g.tW = gs.tiles + ct * 64;
    gs.cap = capacity;
    bump_lin(h);
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_size(gpmpc_handle* h, int32_t gp_id, int32_t* n, int32_t* capacity) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    if (!h->gp[gp_id].set) return fail(GPMPC_ERR_STATE, "GP not set (gpmpc_set_gp first)");
    // (an exact GP's training rows are its variance rows, whether or not a FITC mean overlays the exact one)
    if (n) *n = h->gp[gp_id].exact ? h->P.gp[gp_id].nv : h->P.gp[gp_id].n;
    if (capacity) *capacity = h->gp[gp_id].cap;
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_append(gpmpc_handle* h, int32_t gp_id, int32_t m, const double* Xnew_dev, const double* ynew_dev,
                             int32_t* accepted_dev, void* stream) {
    const gpmpc_status ready =
        gp_update_ready(h, gp_id, kAppend, (m < 1 || !Xnew_dev || !ynew_dev) ? "no rows to append" : nullptr);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    GPDev& g = h->P.gp[gp_id];
    if ((int64_t)g.n + m > gs.cap)
        return fail(GPMPC_ERR_ARG, "capacity exceeded: " + std::to_string(g.n) + " + " + std::to_string(m) +
                                       " rows, capacity " + std::to_string(gs.cap) + " (gpmpc_gp_reserve)");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const int cpad = (gs.cap + 15) / 16 * 16, d = h->md.gp_dim[gp_id];
    const AppendLayout lay{(size_t)cpad};
    for (int done = 0, blk = 0; done < m; done += 16, ++blk) {
        const int mb = std::min(16, m - done);
        const int n0 = g.n, npad0 = gs.npad, npad1 = (n0 + mb + 15) / 16 * 16;
        // the model changes with the first launch queued: the cache must not serve its old rows
        bump_lin(h);
        if (npad1 > npad0) {
            // the factor moves to the other buffer at the new stride, the new border zeroed
            double* dst = gs.linvT_alt;
            const size_t p0 = (size_t)npad0 * sizeof(double), p1 = (size_t)npad1 * sizeof(double);
            HIPCHK(hipMemcpy2DAsync(dst, p1, gs.linvT, p0, p0, npad0, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemset2DAsync(dst + npad0, p1, 0, p1 - p0, npad0, s));
            HIPCHK(hipMemsetAsync(dst + (size_t)npad0 * npad1, 0, (size_t)(npad1 - npad0) * p1, s));
            std::swap(gs.linvT, gs.linvT_alt);
            g.linvT = gs.linvT;
            gs.npad = npad1;
        }
        GPAppend a{};
        a.rows = gs.rows;
        a.tX = gs.tiles;
        a.tW = gs.tiles + (size_t)(cpad / 16) * 64;
        a.linvT = gs.linvT;
        a.npad = npad1;
        a.n0 = n0;
        a.m = mb;
        a.d = d;
        for (int k = 0; k < 3; ++k) a.xbar[k] = g.xbar[k];
        a.inv_ell2 = g.inv_ell2;
        a.sf2 = g.sf2;
        a.sn2 = g.sn2;
        a.Xnew = Xnew_dev + (size_t)done * d;
        a.ynew = ynew_dev + done;
        a.wt = gs.app + lay.wt;
        a.ldw = cpad;
        a.pmean = gs.app + lay.pmean;
        a.lbinv = gs.app + lay.lbinv;
        a.beta = gs.app + lay.beta;
        a.flag = reinterpret_cast<int32_t*>(gs.app + lay.flag);
        a.accepted = accepted_dev ? accepted_dev + blk : nullptr;
        HIPCHK(launch_gp_append(a, s));
        // the row count advances whether the block is accepted or written as inert rows
        g.n = g.nv = n0 + mb;
        g.ntile = (g.n + 15) / 16;
    }
    return GPMPC_OK;
}

// One block of mb <= 16 rows of GP gp_id queued on s: the oldest (didx null, ok the block's status word) or the
// ascending rows didx names in the GP's drop scratch (ok the call's status word)
static gpmpc_status queue_drop_block(gpmpc_handle* h, int gp_id, int mb, const int32_t* didx, int32_t* ok, hipStream_t s) {
    GPSlot& gs = h->gp[gp_id];
    GPDev& g = h->P.gp[gp_id];
    const int cpad = (gs.cap + 15) / 16 * 16, ct = cpad / 16, d = h->md.gp_dim[gp_id];
    const DropLayout lay{(size_t)cpad};
    double* rows = gs.rows;
    double* tX = gs.tiles;
    double* tW = gs.tiles + (size_t)ct * 64;
    {
        const int n0 = g.n, npad0 = gs.npad, n1 = n0 - mb, npad1 = (n1 + 15) / 16 * 16;
        // the model changes with the first launch queued: the cache must not serve its old rows
        bump_lin(h);
        GPDrop a{};
        a.src = gs.linvT;
        a.dst = gs.linvT_alt;
        a.rows = rows;
        a.tX = tX;
        a.npad0 = npad0;
        a.npad1 = npad1;
        a.n0 = n0;
        a.m = mb;
        a.d = d;
        for (int k = 0; k < 3; ++k) a.xbar[k] = g.xbar[k];
        a.vt = gs.drp + lay.vt;
        a.ldv = cpad;
        a.w = gs.drp + lay.w;
        a.et = gs.drp + lay.et;
        a.dt = gs.drp + lay.dt;
        a.srows = gs.drp + lay.srows;
        a.stX = gs.drp + lay.stX;
        a.stW = gs.drp + lay.stW;
        a.flag = reinterpret_cast<int32_t*>(gs.drp + lay.flag);
        a.ok = ok;
        a.didx = didx;
        a.acc = didx ? reinterpret_cast<int32_t*>(gs.drp + lay.acc) : nullptr;
        HIPCHK(launch_gp_drop(a, s));
        // the staged rows and tile pack replace the live ones (disjoint buffers); what lies between the
        // new and the old padded size becomes what rows past n always are: zero
        const size_t rb = (size_t)npad1 * 4 * sizeof(double), rb0 = (size_t)npad0 * 4 * sizeof(double);
        HIPCHK(hipMemcpyAsync(rows, a.srows, rb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(tX, a.stX, rb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(tW, a.stW, rb, hipMemcpyDeviceToDevice, s));
        if (npad1 < npad0) {
            HIPCHK(hipMemsetAsync(rows + (size_t)npad1 * 4, 0, rb0 - rb, s));
            HIPCHK(hipMemsetAsync(tX + (size_t)npad1 * 4, 0, rb0 - rb, s));
            HIPCHK(hipMemsetAsync(tW + (size_t)npad1 * 4, 0, rb0 - rb, s));
        }
        // the two factor buffers swap roles
        std::swap(gs.linvT, gs.linvT_alt);
        g.linvT = gs.linvT;
        gs.npad = npad1;
        g.n = g.nv = n1;
        g.ntile = (n1 + 15) / 16;
    }
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_drop_oldest(gpmpc_handle* h, int32_t gp_id, int32_t m, int32_t* ok_dev, void* stream) {
    const gpmpc_status ready = gp_update_ready(h, gp_id, kDrop, nullptr);
    if (ready != GPMPC_OK) return ready;
    GPDev& g = h->P.gp[gp_id];
    if (m < 1) return fail(GPMPC_ERR_ARG, "no rows to drop");
    if (m >= g.n)
        return fail(GPMPC_ERR_ARG, "at least one row stays: " + std::to_string(m) + " of " + std::to_string(g.n) +
                                       " rows asked for");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    for (int done = 0, blk = 0; done < m; done += 16, ++blk) {
        const gpmpc_status st = queue_drop_block(h, gp_id, std::min(16, m - done), nullptr, ok_dev ? ok_dev + blk : nullptr, s);
        if (st != GPMPC_OK) return st;
    }
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_drop_rows(gpmpc_handle* h, int32_t gp_id, int32_t m, const int32_t* idx_dev, int32_t* dropped_dev,
                                int32_t* ok_dev, void* stream) {
    const gpmpc_status ready = gp_update_ready(h, gp_id, kDrop, nullptr);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    GPDev& g = h->P.gp[gp_id];
    if (m < 1 || !idx_dev) return fail(GPMPC_ERR_ARG, "no rows to drop");
    if (m >= g.n)
        return fail(GPMPC_ERR_ARG, "at least one row stays: " + std::to_string(m) + " of " + std::to_string(g.n) +
                                       " rows asked for");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const DropLayout lay{(size_t)((gs.cap + 15) / 16 * 16)};
    int32_t* sorted = reinterpret_cast<int32_t*>(gs.drp + lay.sorted);
    GPDropPrep p{};
    p.idx = idx_dev;
    p.n = g.n;
    p.m = m;
    p.mask = reinterpret_cast<int32_t*>(gs.drp + lay.mask);
    p.sorted = sorted;
    p.dropped = dropped_dev;
    p.acc = reinterpret_cast<int32_t*>(gs.drp + lay.acc);
    HIPCHK(launch_gp_drop_prep(p, s));
    // from the highest rows down, so no block shifts the rows of the blocks after it
    for (int left = m; left > 0;) {
        const int mb = std::min(16, left);
        left -= mb;
        const gpmpc_status st = queue_drop_block(h, gp_id, mb, sorted + left, ok_dev, s);
        if (st != GPMPC_OK) return st;
    }
    return GPMPC_OK;
}

// The refactorisation of GP gp_id as launch_gp_refactor and the fit's iterations take it
static GPRefactor refactor_args(gpmpc_handle* h, int gp_id, const double* y_dev, double inv_ell2, double sf2, double sn2,
                                int32_t* ok_dev) {
    const GPSlot& gs = h->gp[gp_id];
    const GPDev& g = h->P.gp[gp_id];
    const int cpad = (gs.cap + 15) / 16 * 16;
    const RefactorLayout lay{(size_t)cpad};
    GPRefactor a{};
    a.rows = gs.rows;
    a.tX = gs.tiles;
    a.tW = gs.tiles + (size_t)(cpad / 16) * 64;
    a.linvT = gs.linvT;
    a.A = gs.linvT_alt;
    a.y = y_dev;
    a.npad = gs.npad;
    a.n = g.n;
    a.d = h->md.gp_dim[gp_id];
    for (int k = 0; k < 3; ++k) a.xbar[k] = g.xbar[k];
    a.inv_ell2 = inv_ell2;
    a.sf2 = sf2;
    a.sn2 = sn2;
    a.dinv = gs.rfc + lay.dinv;
    a.w = gs.rfc + lay.w;
    a.ym = gs.rfc + lay.ym;
    a.mask = reinterpret_cast<int32_t*>(gs.rfc + lay.mask);
    a.flag = reinterpret_cast<int32_t*>(gs.rfc + lay.flag);
    a.ok = ok_dev;
    return a;
}

// What gpmpc_gp_mll and the fit's iterations read of GP gp_id, and the fit scratch
static GPFit fit_args(gpmpc_handle* h, int gp_id, const double* y_dev) {
    const GPSlot& gs = h->gp[gp_id];
    const FitLayout lay{(size_t)((gs.cap + 15) / 16 * 16)};
    GPFit f{};
    f.rows = gs.rows;
    f.linvT = gs.linvT;
    f.y = y_dev;
    f.npad = gs.npad;
    f.n = h->P.gp[gp_id].n;
    f.part = gs.fit + lay.part;
    f.state = gs.fit + lay.state;
    return f;
}

gpmpc_status gpmpc_gp_refactor(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double lengthscale,
                               double outputscale, double noise, int32_t* ok_dev, void* stream) {
    const bool hyp_ok = std::isfinite(lengthscale) && lengthscale > 0.0 && std::isfinite(outputscale) &&
                        outputscale > 0.0 && std::isfinite(noise) && noise > 0.0;
    const gpmpc_status ready =
        gp_update_ready(h, gp_id, kRefactor,
                        !y_dev ? "no targets" : !hyp_ok ? "hyperparameters must be finite and positive" : nullptr);
    if (ready != GPMPC_OK) return ready;
    GPDev& g = h->P.gp[gp_id];
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    // the model changes with the first launch queued: the cache must not serve its old rows
    bump_lin(h);
    const GPRefactor a = refactor_args(h, gp_id, y_dev, 1.0 / (lengthscale * lengthscale), outputscale, noise, ok_dev);
    HIPCHK(launch_gp_refactor(a, s));
    // every kernel reads the hyperparameters from the handle: they change with the factor
    g.inv_ell2 = a.inv_ell2;
    g.sf2 = a.sf2;
    g.sn2 = a.sn2;
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_mll(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double* out_dev, void* stream) {
    const gpmpc_status ready = gp_update_ready(h, gp_id, kMll, (!y_dev || !out_dev) ? "no targets or no output" : nullptr);
    if (ready != GPMPC_OK) return ready;
    const GPDev& g = h->P.gp[gp_id];
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const GPFit f = fit_args(h, gp_id, y_dev);
    HIPCHK(launch_gp_fit_set_hyp(f.state, g.inv_ell2, g.sf2, g.sn2, s));
    HIPCHK(launch_gp_fit_eval(f, out_dev, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_fit(gpmpc_handle* h, int32_t gp_id, const double* y_dev, double lr, int32_t max_iter, double* raw,
                          int32_t* iters_out, int32_t* ok_out, double* hist_dev, void* stream) {
    const char* bad = nullptr;
    if (!y_dev) bad = "no targets";
    else if (!raw) bad = "no raw parameters";
    else if (!std::isfinite(raw[0]) || !std::isfinite(raw[1]) || !std::isfinite(raw[2])) bad = "raw parameters must be finite";
    else if (!std::isfinite(lr) || !(lr > 0.0)) bad = "the learning rate must be finite and positive";
    else if (max_iter < 1) bad = "at least one iteration";
    const gpmpc_status ready = gp_update_ready(h, gp_id, kFit, bad);
    if (ready != GPMPC_OK) return ready;
    GPDev& g = h->P.gp[gp_id];
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    // the model changes with the first launch queued: the cache must not serve its old rows
    bump_lin(h);
    // the iterations' factorisations: the hyperparameters come from the state block, the tile pack they write is
    // rewritten at the end, no status word but the scratch's own
    const GPRefactor a = refactor_args(h, gp_id, y_dev, g.inv_ell2, g.sf2, g.sn2, nullptr);
    const GPFit f = fit_args(h, gp_id, y_dev);
    HIPCHK(launch_gp_refactor_begin(a, s));
    HIPCHK(launch_gp_fit_init(f.state, raw, s));
    // the stop and fail flags are read back once per kFitQueue iterations; what is queued past a stop changes nothing
    constexpr int kFitQueue = 8;
    double st[kFitDoubles];
    for (int done = 0; done < max_iter;) {
        const int q = std::min(kFitQueue, max_iter - done);
        for (int i = 0; i < q; ++i) HIPCHK(launch_gp_fit_iteration(a, f, lr, hist_dev, s));
        done += q;
        HIPCHK(hipMemcpyAsync(st, f.state, sizeof(st), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (st[kFitStop] != 0.0 || st[kFitFail] != 0.0) break;
    }
    const bool fitted = st[kFitFail] == 0.0;
    // softplus as the device computes it (torch's, threshold 20)
    auto sp = [](double x) { return x > 20.0 ? x : std::log1p(std::exp(x)); };
    double inv_ell2 = g.inv_ell2, sf2 = g.sf2, sn2 = g.sn2;
    if (fitted) {
        const double ell = sp(st[kFitRaw]);
        inv_ell2 = 1.0 / (ell * ell);
        sf2 = sp(st[kFitRaw + 1]);
        sn2 = 1e-6 + sp(st[kFitRaw + 2]);
    }
    // the ordinary refactorisation at the fitted hyperparameters (after a failure: at the ones the GP had)
    GPRefactor last = a;
    last.inv_ell2 = inv_ell2, last.sf2 = sf2, last.sn2 = sn2;
    HIPCHK(launch_gp_refactor(last, s));
    g.inv_ell2 = inv_ell2;
    g.sf2 = sf2;
    g.sn2 = sn2;
    int32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, last.flag, sizeof(flag), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (fitted)
        for (int k = 0; k < 3; ++k) raw[k] = st[kFitRaw + k];
    if (iters_out) *iters_out = (int32_t)st[kFitStep];
    if (ok_out) *ok_out = (fitted && flag == 1) ? 1 : 0;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_var_inputs(gpmpc_handle* h, int32_t gp_id, const int32_t* src, int32_t d) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    if (!src || d != h->md.gp_dim[gp_id]) return fail(GPMPC_ERR_ARG, "variance input map must have the GP's dimension");
    for (int k = 0; k < d; ++k)
        if (src[k] < 0 || src[k] >= h->md.nx + h->md.nu) return fail(GPMPC_ERR_ARG, "variance input index out of range");
    for (int k = 0; k < 3; ++k) h->md.var_src[gp_id][k] = k < d ? src[k] : 0;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_gp_variance_root(gpmpc_handle* h, int32_t gp_id, int32_t n, int32_t r, const double* R) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    (void)hipSetDevice(h->device);
    GPSlot& gs = h->gp[gp_id];
    if (!R) {
        gs.drop_root();
        return GPMPC_OK;
    }
    if (h->gp[gp_id].npad == 0) return fail(GPMPC_ERR_STATE, "gpmpc_set_gp first");
    if (n != h->P.gp[gp_id].nv) return fail(GPMPC_ERR_ARG, "root rows must equal the variance GP's training rows");
    if (r < 1 || r > 16 * 16) return fail(GPMPC_ERR_ARG, "root rank must be 1..256");
    const int npad = h->gp[gp_id].npad, rpad = (r + 15) / 16 * 16;
    std::vector<double> rp((size_t)npad * rpad, 0.0);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < r; ++c) rp[(size_t)i * rpad + c] = R[(size_t)i * r + c];
    // staged in a local buffer: the handle's root, columns and rank change together, on success only
    double* buf = nullptr;
    hipError_t e = hipMalloc(&buf, rp.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(buf, rp.data(), rp.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (buf) (void)hipFree(buf);
        return fail(GPMPC_ERR_HIP, std::string("LOVE root upload: ") + hipGetErrorString(e));
    }
    gs.drop_root();
    gs.vroot = buf;
    gs.vroot_cols = rpad;
    gs.vroot_rank = r;
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_love_root(gpmpc_handle* h, int32_t gp_id, int32_t rank, const double* q0_dev, int32_t* rank_out,
                                int32_t* ok_out, void* stream) {
    const gpmpc_status ready =
        gp_update_ready(h, gp_id, kLove,
                        !q0_dev ? "no start vector" : (rank < 1 || rank > kLoveMaxRank) ? "root rank must be 1..256" : nullptr);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    const GPDev& g = h->P.gp[gp_id];
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const int cpad = (gs.cap + 15) / 16 * 16;
    const LoveLayout lay{(size_t)cpad};
    GPLove a{};
    a.rows = gs.rows;
    a.linvT = gs.linvT;
    a.A = gs.linvT_alt;
    a.q0 = q0_dev;
    a.npad = gs.npad;
    a.n = g.nv;   // (the training rows: g.n counts the inducing rows under a FITC mean)
    a.ld = cpad;
    a.rank = rank;
    a.inv_ell2 = g.inv_ell2;
    a.sf2 = g.sf2;
    a.sn2 = g.sn2;
    a.qt = gs.love + lay.qt;
    a.v = gs.love + lay.v;
    a.mask = reinterpret_cast<int32_t*>(gs.love + lay.mask);
    a.apart = gs.love + lay.apart;
    a.cpa = gs.love + lay.cpa;
    a.cpb = gs.love + lay.cpb;
    a.npart = gs.love + lay.npart;
    a.ipart = gs.love + lay.ipart;
    a.alpha = gs.love + lay.alpha;
    a.beta = gs.love + lay.beta;
    a.cd = gs.love + lay.cd;
    a.lsub = gs.love + lay.lsub;
    a.state = reinterpret_cast<int32_t*>(gs.love + lay.state);
    HIPCHK(launch_gp_love_begin(a, s));
    // the done word is read back once per kLoveQueue iterations; what is queued past the stop changes nothing
    constexpr int kLoveQueue = 8;
    const int iters = std::min(rank, a.n);
    int32_t st[kLoveInts] = {0};
    for (int done = 0; done < iters && !st[kLoveDone];) {
        const int q = std::min(kLoveQueue, iters - done);
        for (int i = 0; i < q; ++i) HIPCHK(launch_gp_love_iteration(a, done + i, s));
        done += q;
        HIPCHK(hipMemcpyAsync(st, a.state, sizeof(st), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const int m = st[kLoveM];
    const bool ok = st[kLoveDone] == 1 && st[kLoveOk] == 1 && m >= 1 && m <= rank;
    if (rank_out) *rank_out = ok ? m : 0;
    if (ok_out) *ok_out = ok ? 1 : 0;
    if (!ok) return GPMPC_OK;   // (the handle's root, if any, stays)
    // staged in a local buffer: the handle's root, columns and rank change together, on success only
    const int rp = (m + 15) / 16 * 16;
    double* buf = nullptr;
    hipError_t e = hipMalloc(&buf, (size_t)gs.npad * rp * sizeof(double));
    if (e == hipSuccess) e = launch_gp_love_root(a, m, buf, rp, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        if (buf) (void)hipFree(buf);
        if (rank_out) *rank_out = 0;
        if (ok_out) *ok_out = 0;
        return fail(GPMPC_ERR_HIP, std::string("LOVE root: ") + hipGetErrorString(e));
    }
    gs.drop_root();
    gs.vroot = buf;
    gs.vroot_cols = rp;
    gs.vroot_rank = m;
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_gp_variance_root(gpmpc_handle* h, int32_t gp_id, int32_t* n, int32_t* r, double* R_dev,
                                        void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    const GPSlot& gs = h->gp[gp_id];
    if (!gs.set || !gs.vroot) return fail(GPMPC_ERR_STATE, "no LOVE root installed");
    const int rows = h->P.gp[gp_id].nv;
    if (n) *n = rows;
    if (r) *r = gs.vroot_rank;
    if (!R_dev) return GPMPC_OK;
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const size_t wb = (size_t)gs.vroot_rank * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(R_dev, wb, gs.vroot, (size_t)gs.vroot_cols * sizeof(double), wb, rows,
                            hipMemcpyDeviceToDevice, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_fitc(gpmpc_handle* h, int32_t gp_id, int32_t M, const int32_t* idx_dev, const double* y_dev,
                           double jitter, int32_t* ok_out, void* stream) {
    const char* bad = nullptr;
    if (M < 0) bad = "M must be 0 (remove the FITC mean) or 1 .. n";
    else if (M == 0 && idx_dev) bad = "M = 0 removes the FITC mean and takes no indices (idx_dev must be NULL)";
    else if (M >= 1 && (!idx_dev || !y_dev)) bad = "no indices or no targets";
    else if (M >= 1 && !(std::isfinite(jitter) && jitter >= 0.0)) bad = "jitter must be finite and not negative";
    const gpmpc_status ready = gp_update_ready(h, gp_id, kFitc, bad);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    GPDev& g = h->P.gp[gp_id];
    const int n = g.nv;
    if (M > n) return fail(GPMPC_ERR_ARG, "M must be 1 .. n: " + std::to_string(M) + " inducing rows of " +
                                              std::to_string(n) + " training rows asked for");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const int cpad = (gs.cap + 15) / 16 * 16;
    if (M == 0) {   // back to the exact mean (the overlay's buffer stays as a spare: nothing is freed under queued work)
        if (!gs.fitc_M) return GPMPC_OK;
        g.rows = gs.rows;
        g.tX = gs.tiles;
        g.tW = gs.tiles + (size_t)(cpad / 16) * 64;
        g.n = n;
        g.ntile = (n + 15) / 16;
        gs.fitc_M = 0;
        bump_lin(h);
        return GPMPC_OK;
    }
    if (ok_out) *ok_out = 0;
    const int mpad = (M + 15) / 16 * 16;
    if (!gs.fitc_ws || gs.fitc_ws_m < mpad || gs.fitc_ws_c < cpad) {
        double* ws = nullptr;
        if (hipMalloc(&ws, FitcLayout{(size_t)mpad, (size_t)cpad}.end * sizeof(double)) != hipSuccess)
            return fail(GPMPC_ERR_NOMEM, "gpmpc_gp_fitc: no memory for the work space of " + std::to_string(M) + " inducing rows");
        if (gs.fitc_ws) (void)hipFree(gs.fitc_ws);   // (every earlier build has synchronised: nothing reads it)
        gs.fitc_ws = ws;
        gs.fitc_ws_m = mpad;
        gs.fitc_ws_c = cpad;
    }
    // staged in a local buffer: the handle's mean changes on success only
    const FitcOut out{(size_t)mpad};
    double* buf = nullptr;
    if (hipMalloc(&buf, out.end * sizeof(double)) != hipSuccess)
        return fail(GPMPC_ERR_NOMEM, "gpmpc_gp_fitc: no memory for " + std::to_string(M) + " inducing rows");
    const FitcLayout lay{(size_t)mpad, (size_t)cpad};
    GPFitc a{};
    a.rows = gs.rows;
    a.linvT = gs.linvT;
    a.y = y_dev;
    a.idx = idx_dev;
    a.V = gs.linvT_alt;
    a.npad = gs.npad;
    a.n = n;
    a.mpad = mpad;
    a.M = M;
    a.d = h->md.gp_dim[gp_id];
    for (int k = 0; k < 3; ++k) a.xbar[k] = g.xbar[k];
    a.inv_ell2 = g.inv_ell2;
    a.sf2 = g.sf2;
    a.sn2 = g.sn2;
    a.jitter = jitter;
    double* ws = gs.fitc_ws;
    a.A = ws + lay.A;
    a.lt1 = ws + lay.lt1;
    a.lt2 = ws + lay.lt2;
    a.dinv = ws + lay.dinv;
    a.ginv = ws + lay.ginv;
    a.t = ws + lay.t;
    a.u = ws + lay.u;
    a.p = ws + lay.p;
    a.q = ws + lay.q;
    a.lmask = reinterpret_cast<int32_t*>(ws + lay.lmask);
    a.smask = reinterpret_cast<int32_t*>(ws + lay.smask);
    a.flag = reinterpret_cast<int32_t*>(ws + lay.flag);
    a.srows = buf + out.rows;
    a.stX = buf + out.tX;
    a.stW = buf + out.tW;
    a.sidx = reinterpret_cast<int32_t*>(buf + out.idx);
    int32_t flag = 0;
    hipError_t e = launch_gp_fitc(a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, a.flag, sizeof(flag), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return fail(GPMPC_ERR_HIP, std::string("FITC mean: ") + hipGetErrorString(e));
    }
    if (flag != 1) {   // (the handle's mean, exact or FITC, stays)
        (void)hipFree(buf);
        return GPMPC_OK;
    }
    if (gs.fitc) (void)hipFree(gs.fitc);   // (the stream is drained, and every other stream's work was ordered before it)
    gs.fitc = buf;
    gs.fitc_M = M;
    g.rows = a.srows;
    g.tX = a.stX;
    g.tW = a.stW;
    g.n = M;
    g.ntile = mpad / 16;
    bump_lin(h);
    if (ok_out) *ok_out = 1;
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_inducing(gpmpc_handle* h, int32_t gp_id, int32_t M, double tol, int32_t* idx_dev,
                               double* gain_dev, double* resid_dev, int32_t* count_out) {
    const char* bad = nullptr;
    if (M < 1) bad = "M must be 1 .. n";
    else if (!(std::isfinite(tol) && tol >= 0.0)) bad = "tol must be finite and not negative";
    else if (!idx_dev) bad = "no room for the picks (idx_dev is NULL)";
    // (a LOVE root and a FITC mean are no obstacle: both were built in the second factor buffer by calls that had
    // finished with it when they returned, and neither keeps anything there)
    const gpmpc_status ready = gp_update_ready(h, gp_id, kInducing, bad);
    if (ready != GPMPC_OK) return ready;
    GPSlot& gs = h->gp[gp_id];
    const GPDev& g = h->P.gp[gp_id];
    const int n = g.nv;   // (the training rows: g.n counts the inducing rows under a FITC mean)
    if (M > n) return fail(GPMPC_ERR_ARG, "M must be 1 .. n: " + std::to_string(M) + " inducing rows of " +
                                              std::to_string(n) + " training rows asked for");
    (void)hipSetDevice(h->device);
    // on a stream of the handle's own, behind the handle's last call, and drained before the call returns
    HIPCHK(ensure_side(h));
    hipStream_t s = h->side;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const int cpad = (gs.cap + 15) / 16 * 16;
    const InducingLayout lay{(size_t)cpad};
    GPInducing a{};
    a.rows = gs.rows;
    a.linvT = gs.linvT;
    a.lcol = gs.linvT_alt;
    a.npad = gs.npad;
    a.n = n;
    a.M = M;
    a.d = h->md.gp_dim[gp_id];
    a.ld = cpad;
    a.nblk = (n + kPickBlock - 1) / kPickBlock;
    a.c = -0.5 * g.inv_ell2;
    a.sf2 = g.sf2;
    a.tol = tol;
    a.dd = gs.ind + lay.d;
    a.bval = gs.ind + lay.bval;
    a.bidx = reinterpret_cast<int32_t*>(gs.ind + lay.bidx);
    a.state = reinterpret_cast<int32_t*>(gs.ind + lay.state);
    a.flag = reinterpret_cast<int32_t*>(gs.ind + lay.flag);
    a.idx = idx_dev;
    a.gain = gain_dev;
    a.resid = resid_dev;
    HIPCHK(launch_gp_inducing_begin(a, s));
    // the count is read back once per kInducingQueue picks; what is queued past the stop changes nothing
    constexpr int kInducingQueue = 64;
    int32_t count = -1;
    for (int done = 0; done < M && count < 0;) {
        const int q = std::min(kInducingQueue, M - done);
        for (int i = 0; i < q; ++i) HIPCHK(launch_gp_inducing_step(a, done + i, s));
        done += q;
        HIPCHK(hipMemcpyAsync(&count, a.flag + kIndCount, sizeof(count), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (count < 0 || count > M) return fail(GPMPC_ERR_HIP, "gpmpc_gp_inducing: the selection left no count");
    if (count_out) *count_out = count;
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_gp_fitc(gpmpc_handle* h, int32_t gp_id, int32_t* M, int32_t* idx_dev, double* w_dev, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp) return fail(GPMPC_ERR_ARG, "gp_id out of range");
    const GPSlot& gs = h->gp[gp_id];
    const int m = gs.set ? gs.fitc_M : 0;
    if (M) *M = m;
    if (m == 0 || (!idx_dev && !w_dev)) return GPMPC_OK;
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const FitcOut out{(size_t)((m + 15) / 16 * 16)};
    if (idx_dev) HIPCHK(hipMemcpyAsync(idx_dev, gs.fitc + out.idx, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (w_dev)
        HIPCHK(hipMemcpy2DAsync(w_dev, sizeof(double), gs.fitc + out.rows + 3, 4 * sizeof(double), sizeof(double), m,
                                hipMemcpyDeviceToDevice, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_use_gp(gpmpc_handle* h, int32_t enabled) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (enabled)
        for (int g = 0; g < h->md.ngp; ++g)
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP " + std::to_string(g) + " not set");
    if (h->P.use_gp != (enabled ? 1 : 0)) bump_lin(h);
    h->P.use_gp = enabled ? 1 : 0;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_tightening(gpmpc_handle* h, int32_t enabled, double inverse_cdf, const double* Ad,
                                  const double* Bd, const double* K) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    ProblemDev& P = h->P;
    P.tighten = enabled ? 1 : 0;
    if (!enabled) return GPMPC_OK;
    if (!Ad || !Bd || !K) return fail(GPMPC_ERR_ARG, "null tightening matrices");
    const int nx = h->md.nx, nu = h->md.nu;
    P.icdf = inverse_cdf;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            double acc = Ad[i * nx + j];
            for (int a = 0; a < nu; ++a) acc += Bd[i * nu + a] * K[a * nx + j];
            P.Acl[i * nx + j] = acc;
        }
    for (int a = 0; a < nu * nx; ++a) P.K[a] = K[a];
    // Gain table of the covariance convolution: column q of Acl^m Bd is column unc[q] of Acl^m
    // (Bd selects the uncertain state dims, gpmpc.py:68-69), squared entrywise, and likewise
    // for K Acl^m.  m = 0..H-1.
    int32_t unc[kMaxNX];
    const int nunc = model_unc_dims(h->model, unc);
    const int H = h->H, nb = nx + nu;
    std::vector<double> tab((size_t)H * nb * nunc), Am((size_t)nx * nx, 0.0), tmp((size_t)nx * nx);
    for (int i = 0; i < nx; ++i) Am[i * nx + i] = 1.0;
    for (int m = 0; m < H; ++m) {
        double* t = tab.data() + (size_t)m * nb * nunc;
        for (int q = 0; q < nunc; ++q) {
            for (int i = 0; i < nx; ++i) {
                const double a = Am[i * nx + unc[q]];
                t[i * nunc + q] = a * a;
            }
            for (int a = 0; a < nu; ++a) {
                double acc = 0.0;
                for (int j = 0; j < nx; ++j) acc += K[a * nx + j] * Am[j * nx + unc[q]];
                t[(nx + a) * nunc + q] = acc * acc;
            }
        }
        for (int i = 0; i < nx; ++i)   // Am <- Acl Am
            for (int j = 0; j < nx; ++j) {
                double acc = 0.0;
                for (int l = 0; l < nx; ++l) acc += P.Acl[i * nx + l] * Am[l * nx + j];
                tmp[i * nx + j] = acc;
            }
        Am.swap(tmp);
    }
    (void)hipSetDevice(h->device);
    if (!h->tgain) {
        const hipError_t e = hipMalloc(&h->tgain, tab.size() * sizeof(double));
        if (e != hipSuccess) {
            h->tgain = nullptr;
            P.tighten = 0;
            return fail(GPMPC_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
    }
    HIPCHK(hipMemcpy(h->tgain, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    P.tgain = h->tgain;
    return GPMPC_OK;
}

gpmpc_status gpmpc_reset(gpmpc_handle* h, int32_t batch, int32_t reset_iterate, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = batch, H = h->H;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    HIPCHK(hipMemsetAsync(h->has_prev, 0, B * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(h->t_prev, 0xff, B * sizeof(int32_t), s));   // -1: nothing to shift from
    bump_lin(h);
    if (reset_iterate) {
        HIPCHK(hipMemsetAsync(h->x, 0, B * (H + 1) * h->md.nx * sizeof(double), s));
        HIPCHK(hipMemsetAsync(h->u, 0, B * H * h->md.nu * sizeof(double), s));
        HIPCHK(hipMemsetAsync(h->pi, 0, B * H * h->md.nx * sizeof(double), s));
        HIPCHK(hipMemsetAsync(h->lam, 0, B * (H + 1) * 2 * h->nb * sizeof(double), s));
    }
    if (batch == h->max_batch) h->any_prev = false;
    h->var_batch = 0;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_iterate(gpmpc_handle* h, int32_t batch, const double* x_dev, const double* u_dev, void* stream) {
    if (!h || !x_dev || !u_dev) return fail(GPMPC_ERR_ARG, "null argument");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = batch, H = h->H;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    HIPCHK(hipMemcpyAsync(h->x, x_dev, B * (H + 1) * h->md.nx * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(h->u, u_dev, B * H * h->md.nu * sizeof(double), hipMemcpyDeviceToDevice, s));
    bump_lin(h);
    HIPCHK(hipMemsetAsync(h->t_prev, 0xff, B * sizeof(int32_t), s));   // -1: an explicit guess is not shifted
    HIPCHK(hipMemsetAsync(h->pi, 0, B * H * h->md.nx * sizeof(double), s));
    HIPCHK(hipMemsetAsync(h->lam, 0, B * (H + 1) * 2 * h->nb * sizeof(double), s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_solve(gpmpc_handle* h, int32_t batch, const double* x0, const int32_t* tstep, double* u0,
                         int32_t* status, int32_t* sqp_iter, int32_t* qp_iter, double* res, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "gpmpc_set_model not called");
    if (!h->ref_set) return fail(GPMPC_ERR_STATE, "gpmpc_set_reference not called");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    if (!x0 || !tstep || !u0 || !status) return fail(GPMPC_ERR_ARG, "null output/input");
    if (h->P.tighten && h->P.use_gp)
        for (int g = 0; g < h->md.ngp; ++g)
            if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "tightening needs Linv for every GP");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    ProblemDev P = h->P;
    P.tighten = (h->P.tighten && h->P.use_gp) ? 1 : 0;
    // Profiling events are best effort: a failed record drops that launch's timing (the events go
    // back to the pool), never the solve.  Every early return below recycles what it took.
    auto give_back = [&](hipEvent_t& e) {
        if (e) h->ev_pool.push_back(e);
        e = nullptr;
    };
    // GP variances at the previous solution (the MFMA contraction) of the instances of ranks
    // first .. first + count - 1 in `order` (null: instances first .. first + count - 1)
    auto launch_var = [&](int first, int count, const int32_t* order, hipStream_t st) -> hipError_t {
        PostBatch pb{};
        pb.n = h->md.ngp;
        pb.step_points = batch * h->H;
        pb.var_split = h->var_split;
        pb.var_full = h->var_trim ? 0 : 1;
        for (int g = 0; g < h->md.ngp; ++g) {
            PostArgs& a = pb.a[g];
            a.sx = h->x;
            a.su = h->u;
            a.H = h->H;
            a.nx = h->md.nx;
            a.nu = h->md.nu;
            a.ngp = h->md.ngp;
            a.gp_index = g;
            for (int k = 0; k < 3; ++k) a.src[k] = h->md.var_src[g][k];
            a.P = count * h->H;
            a.d = h->md.gp_dim[g];
            a.with_noise = 1;   // gp.likelihood(gp(z)) (gpmpc.py:444)
            a.mean = nullptr;
            a.var = h->var;
            a.var_stride = h->md.ngp;
            a.var_off = g;
            a.order = order;
            a.first = first;
            pb.g[g] = P.gp[g];
            pb.g[g].vroot = h->gp[g].vroot;   // LOVE (fast_pred_var) when a root is set
            pb.g[g].vroot_cols = h->gp[g].vroot_cols;
            pb.g[g].vroot_rank = h->gp[g].vroot_rank;
            pb.npad[g] = h->gp[g].npad;
        }
        return launch_gp_post_batch(pb, true, st);
    };
    StateDev S{h->x, h->u, h->pi, h->lam, h->has_prev, h->var, h->tight, h->lin_cache ? h->lin : nullptr, h->lin_tag,
               h->order, h->cost, 0, h->t_prev};
    StepIO io{x0, tstep, u0, status, sqp_iter, qp_iter, res, h->timing, h->stats};
    // optional outputs go to handle-owned scratch when NULL
    if (!io.sqp_iter) io.sqp_iter = h->scratch_i;
    if (!io.qp_iter) io.qp_iter = h->scratch_i + h->max_batch;
    if (!io.res) io.res = h->scratch_d;
    hipEvent_t e0 = nullptr, e1 = nullptr, mid = nullptr;
    const bool var_launch = P.tighten && h->any_prev;

    // Overlapped step: when the variance launch precedes an SQP launch that fills the device with one
    // wave per instance (or needs more than one round of workgroups), the instances are ranked by
    // the cost of their last solve and split in two halves.  The costlier half's variances run
    // first and its SQP launch starts right after them; the cheaper half's variances and SQP launch
    // run on a second stream beside it, so the step waits only for the first half's variances before
    // the solves that set its length begin.  Each instance's arithmetic is unchanged (same kernels,
    // same per-instance data), so the results are bit-identical to the sequential order.
    if (var_launch && h->overlap && batch >= 2 && batch <= 16384 && sqp_overlap_ok(P, batch)) {
        if (const hipError_t ce = ensure_side(h); ce != hipSuccess)
            return fail(GPMPC_ERR_HIP, std::string("side stream: ") + hipGetErrorString(ce));
        const int b1 = (batch + 1) / 2, b2 = batch - b1;
        HIPCHK(launch_sqp_order(S, batch, s));
        if (h->profiling) {
            e0 = take_event(h);
            e1 = take_event(h);
            if (e0 && hipEventRecord(e0, s) != hipSuccess) give_back(e0);
        }
        hipError_t ve = launch_var(0, b1, h->order, s);
        if (ve == hipSuccess && e0 && e1 && hipEventRecord(e1, s) == hipSuccess) {
            h->ev_var.push_back({e0, e1});
            mid = e1;
        } else {
            give_back(e0);
            give_back(e1);
        }
        if (ve == hipSuccess) ve = hipEventRecord(h->ev_fork, s);
        if (ve == hipSuccess) ve = hipStreamWaitEvent(h->side, h->ev_fork, 0);
        if (ve != hipSuccess) {
            h->var_batch = 0;
            if (mid) h->ev_var_owned.push_back(mid);
            return fail(GPMPC_ERR_HIP, std::string("variance launch: ") + hipGetErrorString(ve));
        }
        // var rows are valid only for what is queued: the costlier half now (ranked instances, so
        // no prefix of the batch is complete: none), the whole batch once the second half's
        // variance launch is queued too
        h->var_batch = 0;
        hipEvent_t e2 = h->profiling && mid ? take_event(h) : nullptr;
        hipError_t le = launch_sqp(P, S, io, batch, s, 0, b1);
        // once an SQP launch is queued it will update the iterate: the host state follows it
        if (le == hipSuccess) h->any_prev = true;
        if (le == hipSuccess) le = launch_var(b1, b2, h->order, h->side);
        if (le == hipSuccess) h->var_batch = batch;
        if (le == hipSuccess) le = launch_sqp(P, S, io, batch, h->side, b1, b2);
        // the join is recorded whatever happened above, so the caller's stream never runs ahead of
        // work already queued on the side stream
        const hipError_t je = hipEventRecord(h->ev_join, h->side);
        const hipError_t we = je == hipSuccess ? hipStreamWaitEvent(s, h->ev_join, 0) : je;
        if (le == hipSuccess) le = we;
        if (le != hipSuccess) {
            if (mid) h->ev_var_owned.push_back(mid);
            give_back(e2);
            return fail(GPMPC_ERR_HIP, std::string("launch_sqp: ") + hipGetErrorString(le));
        }
        if (mid && e2 && hipEventRecord(e2, s) == hipSuccess) {
            h->ev_sqp.push_back({mid, e2});
        } else {
            if (mid) h->ev_var_owned.push_back(mid);
            give_back(e2);
        }
        if (h->stage_cost) HIPCHK(launch_stage_cost(P, h->x, h->u, tstep, status, h->stage_cost, batch, s));
        return GPMPC_OK;
    }

    // 1. GP variances at the previous solution, only when needed
    if (var_launch) {
        if (h->profiling) {
            e0 = take_event(h);
            e1 = take_event(h);
            if (e0 && hipEventRecord(e0, s) != hipSuccess) give_back(e0);
        }
        const hipError_t ve = launch_var(0, batch, nullptr, s);
        if (ve != hipSuccess) {
            give_back(e0);
            give_back(e1);
            h->var_batch = 0;
            return fail(GPMPC_ERR_HIP, std::string("launch_gp_post_batch: ") + hipGetErrorString(ve));
        }
        if (e0 && e1 && hipEventRecord(e1, s) == hipSuccess) {
            h->ev_var.push_back({e0, e1});
            mid = e1;   // also the SQP launch's start
        } else {
            give_back(e0);
            give_back(e1);
        }
    }
    h->var_batch = var_launch ? batch : 0;
    // 2. the SQP step
    e0 = e1 = nullptr;
    if (h->profiling) {
        e0 = mid;
        if (!e0) {
            e0 = take_event(h);
            if (e0 && hipEventRecord(e0, s) != hipSuccess) give_back(e0);
        }
        e1 = take_event(h);
        if (!e0) give_back(e1);
    }
    // events not handed to ev_sqp: the shared `mid` stays in use as ev_var's end event (the
    // variance list takes ownership of it), the others go back to the pool, on every exit path
    auto recycle = [&]() {
        if (e0 && e0 == mid) h->ev_var_owned.push_back(e0);
        else if (e0) h->ev_pool.push_back(e0);
        if (e1) h->ev_pool.push_back(e1);
    };
    // Tail boost (GPMPC_TUNE_TAIL = K > 0): a launch that gives every instance one wave in one round
    // of workgroups (the metric's 1024 quad2d instances on one MI355X) lasts as long as its slowest
    // instance, and the costliest instances stay costly from step to step (StateDev::cost).  The
    // instances are ranked by the cost of their previous solve; the K costliest run as two-wave
    // segment solves (their recursions split over two waves) on the caller's stream, right behind the
    // ranking kernel, and the others as one-wave instances on the side stream, released by the same
    // ranking kernel (the side stream's wait resolves after the caller's next packet is dispatched, so
    // the two-wave instances take their SIMDs first).  With one SIMD per wave the K extra waves make
    // the K cheapest instances (dispatched last) wait for the SIMDs of the first instances to finish.
    // Each instance's arithmetic is its launch shape's, identical up to rounding to the one-wave
    // solve (the parity tests cover both shapes).
    bool tail_queued = false;
    auto launch_step = [&]() -> hipError_t {
        const int K = tail_count(h, P, batch);
        if (K <= 0) return launch_sqp(P, S, io, batch, s);
        hipError_t e = ensure_side(h);
        if (e == hipSuccess) e = launch_sqp_order(S, batch, s);
        if (e == hipSuccess) e = hipEventRecord(h->ev_fork, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->side, h->ev_fork, 0);
        if (e != hipSuccess) return e;
        ProblemDev P2 = P, P1 = P;
        P2.waves = 2;   // (sqp_tail_ok: segment solves on two waves)
        P1.waves = 1;
        e = launch_sqp(P2, S, io, batch, s, 0, K);
        if (e == hipSuccess) tail_queued = true;
        if (e == hipSuccess) e = launch_sqp(P1, S, io, batch, h->side, K, batch - K);
        // the join is recorded whatever happened above, so the caller's stream never runs ahead of
        // work already queued on the side stream
        const hipError_t je = hipEventRecord(h->ev_join, h->side);
        const hipError_t we = je == hipSuccess ? hipStreamWaitEvent(s, h->ev_join, 0) : je;
        return e == hipSuccess ? we : e;
    };
    const hipError_t le = launch_step();
    if (le != hipSuccess) {
        if (tail_queued) h->any_prev = true;   // part of the batch's iterate is being updated
        recycle();
        return fail(GPMPC_ERR_HIP, std::string("launch_sqp: ") + hipGetErrorString(le));
    }
    // the SQP kernel is queued and will update the iterate: from here on the host state follows it
    h->any_prev = true;
    if (e0 && e1 && hipEventRecord(e1, s) == hipSuccess) h->ev_sqp.push_back({e0, e1});
    else recycle();   // lost profiling data only
    // stage costs of the stored solution, behind the SQP launch (and outside its timing events)
    if (h->stage_cost) HIPCHK(launch_stage_cost(P, h->x, h->u, tstep, status, h->stage_cost, batch, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_variance(gpmpc_handle* h, int32_t batch, double* var_dev, void* stream) {
    if (!h || !var_dev) return fail(GPMPC_ERR_ARG, "null argument");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    if (h->var_batch == 0)
        return fail(GPMPC_ERR_STATE, "the last solve ran no variance launch (first step, tightening or GPs off)");
    if (batch > h->var_batch)
        return fail(GPMPC_ERR_ARG, "the last variance launch covered " + std::to_string(h->var_batch) + " instances");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const size_t B = batch, H = h->H;
    HIPCHK(hipMemcpyAsync(var_dev, h->var, B * H * h->md.ngp * sizeof(double), hipMemcpyDeviceToDevice, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_launch(gpmpc_handle* h, int32_t waves) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4) return fail(GPMPC_ERR_ARG, "waves must be 0 (auto), 1, 2 or 4");
    if (h->model == kQuad3D && waves != 0 && waves != 4)
        return fail(GPMPC_ERR_ARG, "quad3d runs four waves per instance (waves must be 0 or 4)");
    h->P.waves = waves;
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_launch_info(gpmpc_handle* h, int32_t batch, int32_t* waves, int32_t* overlapped) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    if (waves) *waves = sqp_launch_waves(h->P, batch);
    // the overlap needs a variance launch (tightening with GPs) besides the shape
    if (overlapped) {
        *overlapped = (h->overlap && h->P.tighten && h->P.use_gp && batch >= 2 && batch <= 16384 &&
                       sqp_overlap_ok(h->P, batch)) ? 1 : 0;
        if (*overlapped == 0 && tail_count(h, h->P, batch) > 0) *overlapped = 2;   // tail boost
    }
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_launch_segments(gpmpc_handle* h, int32_t batch, int32_t* segments) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    if (!segments) return fail(GPMPC_ERR_ARG, "null output");
    *segments = sqp_launch_segments(h->P, batch);
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_tuning(gpmpc_handle* h, int32_t option, int32_t value) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    switch (option) {
        case GPMPC_TUNE_LIN_CACHE:
            if (value != 0 && value != 1) break;
            if (h->lin_cache != (value == 1)) bump_lin(h);   // tags written under the other setting are stale
            h->lin_cache = value == 1;
            return GPMPC_OK;
        case GPMPC_TUNE_ORDER:
            if (value < 0 || value > 2) break;
            h->P.order_dispatch = value;
            return GPMPC_OK;
        case GPMPC_TUNE_OVERLAP:
            if (value != 0 && value != 1) break;
            h->overlap = value == 1;
            return GPMPC_OK;
        case GPMPC_TUNE_VAR_SPLIT:
            if (value != 0 && value != 1 && value != 4) break;
            h->var_split = value;
            return GPMPC_OK;
        case GPMPC_TUNE_VAR_TRIM:
            if (value != 0 && value != 1) break;
            h->var_trim = value == 1;
            return GPMPC_OK;
        case GPMPC_TUNE_SEG:
            if (value != 0 && value != 1) break;
            h->P.seg = value;
            return GPMPC_OK;
        case GPMPC_TUNE_SEG_PIVOT:
            // threshold 10^-value; -1: every pivot refused (every solve takes the fallback, a test of it)
            if (value < -1 || value > 300) break;
            h->P.seg_piv_rel = value < 0 ? HUGE_VAL : std::pow(10.0, -value);
            return GPMPC_OK;
        case GPMPC_TUNE_TAIL:
            if (value < -1 || value > 16384) break;
            h->tail = value;
            return GPMPC_OK;
        case GPMPC_TUNE_SHIFT:
            if (value != 0 && value != 1) break;
            h->P.shift = value;
            return GPMPC_OK;
        case GPMPC_TUNE_EVENT_FENCE:
            if (value != 0 && value != 1) break;
            if (h->event_fence != (value == 1)) {   // pooled events carry the old flags (the ones still in
                for (hipEvent_t e : h->ev_pool) {     // use are dropped when they come back: take_event)
                    h->ev_fenced.erase(e);
                    (void)hipEventDestroy(e);
                }
                h->ev_pool.clear();
            }
            h->event_fence = value == 1;
            return GPMPC_OK;
        default:
            return fail(GPMPC_ERR_ARG, "unknown tuning option " + std::to_string(option));
    }
    return fail(GPMPC_ERR_ARG, "bad value " + std::to_string(value) + " for tuning option " + std::to_string(option));
}

gpmpc_status gpmpc_set_cost_buffer(gpmpc_handle* h, void* cost_dev) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    h->stage_cost = (double*)cost_dev;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_profiling(gpmpc_handle* h, int32_t enabled) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    h->profiling = enabled != 0;
    return GPMPC_OK;
}

// true (and forgotten) if `e` is an ev_var end event that the variance list owns
static bool release_owned(gpmpc_handle* h, hipEvent_t e) {
    for (size_t i = 0; i < h->ev_var_owned.size(); ++i)
        if (h->ev_var_owned[i] == e) {
            h->ev_var_owned.erase(h->ev_var_owned.begin() + i);
            return true;
        }
    return false;
}

gpmpc_status gpmpc_kernel_times(gpmpc_handle* h, double* var_ms, int32_t* n_var, double* sqp_ms, int32_t* n_sqp) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    (void)hipSetDevice(h->device);
    // (the variance list's end events belong to the SQP list, which returns them to the pool)
    auto sum = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* ms, int32_t* n) -> gpmpc_status {
        const bool sqp_list = &v == &h->ev_sqp;
        double acc = 0.0;
        for (auto& pr : v) {
            HIPCHK(hipEventSynchronize(pr.second));
            float t = 0.0f;
            HIPCHK(hipEventElapsedTime(&t, pr.first, pr.second));
            acc += t;
            h->ev_pool.push_back(pr.first);
            if (sqp_list || release_owned(h, pr.second)) h->ev_pool.push_back(pr.second);
        }
        if (ms) *ms = acc;
        if (n) *n = (int32_t)v.size();
        v.clear();
        return GPMPC_OK;
    };
    gpmpc_status st = sum(h->ev_var, var_ms, n_var);
    if (st != GPMPC_OK) return st;
    return sum(h->ev_sqp, sqp_ms, n_sqp);
}

gpmpc_status gpmpc_kernel_time_list(gpmpc_handle* h, int32_t cap, double* var_ms, int32_t* n_var, double* sqp_ms,
                                    int32_t* n_sqp) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (cap < 0) return fail(GPMPC_ERR_ARG, "negative capacity");
    (void)hipSetDevice(h->device);
    // (the variance list's end events belong to the SQP list, which returns them to the pool)
    auto take = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* ms, int32_t* n) -> gpmpc_status {
        const bool sqp_list = &v == &h->ev_sqp;
        int32_t i = 0;
        for (auto& pr : v) {
            HIPCHK(hipEventSynchronize(pr.second));
            float t = 0.0f;
            HIPCHK(hipEventElapsedTime(&t, pr.first, pr.second));
            if (ms && i < cap) ms[i] = t;
            ++i;
            h->ev_pool.push_back(pr.first);
            if (sqp_list || release_owned(h, pr.second)) h->ev_pool.push_back(pr.second);
        }
        if (n) *n = i;
        v.clear();
        return GPMPC_OK;
    };
    gpmpc_status st = take(h->ev_var, var_ms, n_var);
    if (st != GPMPC_OK) return st;
    return take(h->ev_sqp, sqp_ms, n_sqp);
}

gpmpc_status gpmpc_set_timing_buffer(gpmpc_handle* h, void* timing_dev) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    h->timing = (unsigned long long*)timing_dev;
    return GPMPC_OK;
}

gpmpc_status gpmpc_set_stats_buffer(gpmpc_handle* h, void* stats_dev, int32_t slots) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (stats_dev && slots < kStatsSlots)
        return fail(GPMPC_ERR_ARG, "stats buffer needs GPMPC_STATS_SLOTS = " + std::to_string(kStatsSlots) +
                                       " int64 slots per instance, got " + std::to_string(slots));
    if (stats_dev && slots != kStatsSlots)
        return fail(GPMPC_ERR_ARG, "stats buffer row stride must be GPMPC_STATS_SLOTS = " + std::to_string(kStatsSlots));
    h->stats = (long long*)stats_dev;
    return GPMPC_OK;
}

gpmpc_status gpmpc_get_solution(gpmpc_handle* h, int32_t batch, double* x_dev, double* u_dev, double* tight_dev,
                                void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (batch < 1 || batch > h->max_batch) return fail(GPMPC_ERR_ARG, "batch out of range");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = batch, H = h->H;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    if (x_dev) HIPCHK(hipMemcpyAsync(x_dev, h->x, B * (H + 1) * h->md.nx * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (u_dev) HIPCHK(hipMemcpyAsync(u_dev, h->u, B * H * h->md.nu * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (tight_dev)
        HIPCHK(hipMemcpyAsync(tight_dev, h->tight, B * (H + 1) * h->nb * sizeof(double), hipMemcpyDeviceToDevice, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_predict(gpmpc_handle* h, int32_t gp_id, const double* Z, int32_t P, double* mean, double* var,
                              int32_t with_noise, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp || !h->gp[gp_id].set) return fail(GPMPC_ERR_STATE, "GP not set");
    if (P < 0 || (P > 0 && !Z)) return fail(GPMPC_ERR_ARG, "bad points");
    if (var && !h->gp[gp_id].linvT) return fail(GPMPC_ERR_STATE, "variance needs Linv");
    if (P == 0) return GPMPC_OK;
    (void)hipSetDevice(h->device);
    // a reader of the rows, weights, factor and tile pack: it waits for an update queued on another stream, and an
    // update queued later on another stream waits for it (they rewrite all of these in place)
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const GPDev& g = h->P.gp[gp_id];
    PostArgs a{};
    a.Z = Z;
    a.ldz = h->md.gp_dim[gp_id];
    a.P = P;
    a.d = h->md.gp_dim[gp_id];
    a.with_noise = with_noise;
    a.var_stride = 1;
    a.var_off = 0;
    if (mean) {  // mean over the mean set (exact: training set; FITC: inducing set)
        GPDev gm = g;
        gm.vrows = g.rows;
        gm.nv = g.n;
        gm.linvT = nullptr;
        a.mean = mean;
        a.var = nullptr;
        HIPCHK(launch_gp_post(gm, (g.n + 15) / 16 * 16, a, false, s));
    }
    if (var) {
        a.mean = nullptr;
        a.var = var;
        HIPCHK(launch_gp_post(g, h->gp[gp_id].npad, a, false, s, h->var_trim ? 0 : 1));
    }
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_mean_grad(gpmpc_handle* h, int32_t gp_id, const double* Z, int32_t P, double* mean,
                                double* grad, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (gp_id < 0 || gp_id >= h->md.ngp || !h->gp[gp_id].set) return fail(GPMPC_ERR_STATE, "GP not set");
    if (P < 0 || (P > 0 && !Z)) return fail(GPMPC_ERR_ARG, "bad points");
    if (P == 0) return GPMPC_OK;
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;   // ordered as gpmpc_gp_predict is: it reads the rows and the tile pack
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    HIPCHK(launch_gp_mean_grad(h->P.gp[gp_id], Z, P, mean, grad, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_posterior(int32_t n, int32_t d, int32_t npad, const double* rows, const double* linvT,
                                double lengthscale, double outputscale, double noise, const double* Z, int32_t P,
                                double* mean, double* var, int32_t with_noise, void* stream) {
    if (n < 1 || d < 1 || d > kMaxGPDim || npad < n || npad % 16 != 0 || !rows)
        return fail(GPMPC_ERR_ARG, "bad GP layout (need 1 <= d <= 3, npad = 16-multiple >= n)");
    if (P < 0 || (P > 0 && !Z)) return fail(GPMPC_ERR_ARG, "bad points");
    if (var && !linvT) return fail(GPMPC_ERR_ARG, "variance needs linvT");
    if (!(lengthscale > 0.0) || !(outputscale > 0.0) || !(noise >= 0.0)) return fail(GPMPC_ERR_ARG, "bad hyperparameters");
    if (P == 0) return GPMPC_OK;
    GPDev g{};
    g.rows = rows;
    g.vrows = rows;
    g.linvT = linvT;
    g.n = g.nv = n;
    g.d = d;
    g.inv_ell2 = 1.0 / (lengthscale * lengthscale);
    g.sf2 = outputscale;
    g.sn2 = noise;
    PostArgs a{};
    a.Z = Z;
    a.ldz = d;
    a.P = P;
    a.d = d;
    a.with_noise = with_noise;
    a.mean = mean;
    a.var = var;
    a.var_stride = 1;
    a.var_off = 0;
    HIPCHK(launch_gp_post(g, npad, a, false, (hipStream_t)stream));
    return GPMPC_OK;
}

gpmpc_status gpmpc_plant_step(gpmpc_handle* h, int32_t batch, const double* params, const double* x, const double* u,
                              double* x_next, int32_t* tstep, void* stream) {
    if (!h || !params || !x || !u || !x_next) return fail(GPMPC_ERR_ARG, "null argument");
    if (batch < 1) return fail(GPMPC_ERR_ARG, "batch out of range");
    (void)hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    // x and u are as a rule gpmpc_solve's outputs and tstep its next input: the call is ordered like the others
    HIPCHK(order_after_last(h, s));
    DeferredMark mark{h, s};
    PlantParams p{};   // by value: the launch keeps the parameters of its own call (no table of the handle)
    for (int i = 0; i < h->md.nparams; ++i) p.v[i] = params[i];
    HIPCHK(launch_plant(h->model, p, h->P.dt, x, u, x_next, tstep, batch, s));
    return GPMPC_OK;
}

// What is wrong with the transitions and picks of gpmpc_preprocess / gpmpc_gp_observe, or null
static const char* transitions_bad(int32_t P, const double* x, const double* u, const double* xnext, int32_t m,
                                   const int32_t* pick, double dt_diff, double gravity) {
    if (P < 1 || m < 1) return "no transitions or no rows (P, m >= 1)";
    if (!x || !u || !xnext) return "null transition array";
    if (!pick && m > P) return "without picks the rows are transitions 0 .. m-1: m <= P";
    if (!std::isfinite(dt_diff) || !(dt_diff > 0.0)) return "dt_diff must be finite and positive";
    if (!std::isfinite(gravity)) return "gravity must be finite";
    return nullptr;
}

static GPObserve observe_args(const gpmpc_handle* h, int32_t P, const double* x, const double* u, const double* xnext,
                              int32_t m, const int32_t* pick, double dt_diff, double gravity) {
    GPObserve a{};
    a.model = h->model;
    for (int i = 0; i < kMaxParams; ++i) a.params[i] = h->P.params[i];
    a.P = P;
    a.m = m;
    a.x = x;
    a.u = u;
    a.xnext = xnext;
    a.pick = pick;
    a.dt_diff = dt_diff;
    a.gravity = gravity;
    return a;
}

static ObserveLayout observe_layout(const gpmpc_handle* h) {
    size_t D = 0;
    for (int g = 0; g < h->md.ngp; ++g) D += h->md.gp_dim[g];
    return ObserveLayout{(size_t)h->max_batch, D, (size_t)h->md.ngp};
}

// Replaces a scratch buffer of the handle by a fresh one of `doubles` (a synchronous setup step); a failed allocation
// leaves the handle as it was
static gpmpc_status replace_scratch(double** buf, size_t doubles) {
    double* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, doubles * sizeof(double));
    if (e != hipSuccess) return fail(GPMPC_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    if (*buf) (void)hipFree(*buf);   // (waits for the work queued on it)
    *buf = fresh;
    return GPMPC_OK;
}

// The scratch of gpmpc_gp_informative / gpmpc_gp_observe, allocated by the first call that needs it (a setup step)
static gpmpc_status ensure_observe_scratch(gpmpc_handle* h) {
    return h->obs ? GPMPC_OK : replace_scratch(&h->obs, observe_layout(h).end);
}

// The GP inputs of P points, gathered as gpmpc_preprocess gathers them (no targets: x_next is not read), and their
// variances per GP, gpmpc_gp_predict's variance launch (with_noise = 0) on GP g's columns of the gathered rows: both
// in the observe scratch, queued on s
struct PointVariances {
    const double* Z;      // [P][ldz]
    int32_t ldz;
    const double* var;    // [n_gp][ldv]
    int32_t ldv;
};
static gpmpc_status queue_point_variances(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev,
                                          hipStream_t s, PointVariances* out) {
    const ObserveLayout lay = observe_layout(h);
    GPObserve a = observe_args(h, P, x_dev, u_dev, nullptr, P, nullptr, 1.0, 0.0);
    a.inputs = h->obs + lay.zin;
    HIPCHK(launch_gp_observe(a, s));
    for (int g = 0, col = 0; g < h->md.ngp; col += h->md.gp_dim[g], ++g) {
        PostArgs pa{};
        pa.Z = h->obs + lay.zin + col;
        pa.ldz = (int)lay.D;
        pa.P = P;
        pa.d = h->md.gp_dim[g];
        pa.with_noise = 0;
        pa.var = h->obs + lay.var + (size_t)g * h->max_batch;
        pa.var_stride = 1;
        pa.var_off = 0;
        HIPCHK(launch_gp_post(h->P.gp[g], h->gp[g].npad, pa, false, s, h->var_trim ? 0 : 1));
    }
    *out = PointVariances{h->obs + lay.zin, (int32_t)lay.D, h->obs + lay.var, h->max_batch};
    return GPMPC_OK;
}

gpmpc_status gpmpc_preprocess(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev,
                              const double* xnext_dev, int32_t m, const int32_t* pick_dev, double dt_diff,
                              double gravity, double* inputs_dev, double* targets_dev, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    const char* bad = transitions_bad(P, x_dev, u_dev, xnext_dev, m, pick_dev, dt_diff, gravity);
    if (!bad && !inputs_dev && !targets_dev) bad = "no output (inputs_dev and targets_dev both NULL)";
    if (bad) return fail(GPMPC_ERR_ARG, bad);
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "the prior parameters are not set (gpmpc_set_model first)");
    (void)hipSetDevice(h->device);
    GPObserve a = observe_args(h, P, x_dev, u_dev, xnext_dev, m, pick_dev, dt_diff, gravity);
    a.inputs = inputs_dev;
    a.targets = targets_dev;
    HIPCHK(launch_gp_observe(a, (hipStream_t)stream));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_informative(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev, int32_t m,
                                  int32_t* pick_dev, double* score_dev, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (P < 1 || P > h->max_batch) return fail(GPMPC_ERR_ARG, "P must be in 1 .. max_batch");
    if (m < 1 || m > P) return fail(GPMPC_ERR_ARG, "m must be in 1 .. P");
    if (!x_dev || !u_dev || !pick_dev) return fail(GPMPC_ERR_ARG, "null points or picks");
    for (int g = 0; g < h->md.ngp; ++g) {
        if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP not set (gpmpc_set_gp first)");
        if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "the variance needs Linv (the GP was set without it)");
    }
    (void)hipSetDevice(h->device);
    const gpmpc_status got = ensure_observe_scratch(h);
    if (got != GPMPC_OK) return got;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    PointVariances pv{};
    const gpmpc_status queued = queue_point_variances(h, P, x_dev, u_dev, s, &pv);
    if (queued != GPMPC_OK) return queued;
    GPRank r{};
    r.Z = pv.Z;
    r.ldz = pv.ldz;
    r.var = pv.var;
    r.ldv = pv.ldv;
    r.n_gp = h->md.ngp;
    for (int g = 0; g < h->md.ngp; ++g) r.sf2[g] = h->P.gp[g].sf2;
    r.P = P;
    r.m = m;
    r.score = h->obs + observe_layout(h).score;
    r.score_out = score_dev;
    r.pick = pick_dev;
    HIPCHK(launch_gp_score_rank(r, s));
    return GPMPC_OK;
}

// The scratch of gpmpc_gp_select: made by the first call and made again when a GP's capacity has grown past what its
// V region holds (replace_scratch).
static gpmpc_status ensure_select_scratch(gpmpc_handle* h) {
    size_t rows[kMaxGP] = {0, 0, 0, 0};
    bool fits = h->sel != nullptr;
    for (int g = 0; g < h->md.ngp; ++g) {
        rows[g] = (size_t)std::max((h->gp[g].cap + 15) / 16 * 16, h->gp[g].npad);
        fits = fits && rows[g] <= h->sel_rows[g];
    }
    if (fits) return GPMPC_OK;
    const gpmpc_status got = replace_scratch(&h->sel, SelectLayout((size_t)h->max_batch, (size_t)h->md.ngp, rows).end);
    if (got != GPMPC_OK) return got;
    for (int g = 0; g < kMaxGP; ++g) h->sel_rows[g] = rows[g];
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_select(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev, int32_t m,
                             int32_t* pick_dev, double* gain_dev, double* resid_dev, int32_t* ok_dev, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (P < 1 || P > h->max_batch) return fail(GPMPC_ERR_ARG, "P must be in 1 .. max_batch");
    if (m < 1 || m > P) return fail(GPMPC_ERR_ARG, "m must be in 1 .. P");
    if (m > kSelectMaxPicks) return fail(GPMPC_ERR_ARG, "m must be at most " + std::to_string(kSelectMaxPicks));
    if (!x_dev || !u_dev || !pick_dev) return fail(GPMPC_ERR_ARG, "null points or picks");
    for (int g = 0; g < h->md.ngp; ++g) {
        if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP not set (gpmpc_set_gp first)");
        if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "the variance needs Linv (the GP was set without it)");
    }
    (void)hipSetDevice(h->device);
    gpmpc_status got = ensure_observe_scratch(h);
    if (got != GPMPC_OK) return got;
    got = ensure_select_scratch(h);
    if (got != GPMPC_OK) return got;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const SelectLayout sl((size_t)h->max_batch, (size_t)h->md.ngp, h->sel_rows);
    // the GP inputs of the P candidates and their start variances: gpmpc_gp_informative's launches
    PointVariances pv{};
    got = queue_point_variances(h, P, x_dev, u_dev, s, &pv);
    if (got != GPMPC_OK) return got;
    GPSelect q{};
    q.P = P;
    q.m = m;
    q.n_gp = h->md.ngp;
    q.ldp = (int)sl.ldp;
    q.nblk = (P + kPickBlock - 1) / kPickBlock;
    q.Z = pv.Z;
    q.ldz = pv.ldz;
    q.var0 = pv.var;
    q.ldv = pv.ldv;
    for (int g = 0, col = 0; g < h->md.ngp; col += h->md.gp_dim[g], ++g) {
        const GPDev& gd = h->P.gp[g];
        GPSelectGP& sg = q.g[g];
        sg.rows = gd.vrows;
        sg.linvT = gd.linvT;
        sg.Vt = h->sel + sl.vt[g];
        sg.lcol = h->sel + sl.lcol + (size_t)g * kSelectMaxPicks * sl.ldp;
        sg.npad = h->gp[g].npad;
        sg.nv = gd.nv;
        sg.d = h->md.gp_dim[g];
        sg.zcol = col;
        sg.c = -0.5 * gd.inv_ell2;
        sg.sf2 = gd.sf2;
        sg.sn2 = gd.sn2;
    }
    q.d = h->sel + sl.d;
    q.bval = h->sel + sl.bval;
    q.bidx = reinterpret_cast<int32_t*>(h->sel + sl.bidx);
    q.state = reinterpret_cast<int32_t*>(h->sel + sl.state);
    q.pick = pick_dev;
    q.gain = gain_dev;
    q.resid = resid_dev;
    q.ok = ok_dev;
    HIPCHK(launch_gp_select(q, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_redundant(gpmpc_handle* h, int32_t m, int32_t* pick_dev, double* score_dev, int32_t* ok_dev,
                                void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    if (!pick_dev) return fail(GPMPC_ERR_ARG, "null picks");
    const int ngp = h->md.ngp;
    size_t rows = 0;
    for (int g = 0; g < ngp; ++g) {
        const GPSlot& gs = h->gp[g];
        if (!gs.set) return fail(GPMPC_ERR_STATE, "GP not set (gpmpc_set_gp first)");
        if (!gs.exact) return fail(GPMPC_ERR_STATE, "FITC upload (Xv != X): only an exact GP has its rows ranked");
        if (!gs.linvT) return fail(GPMPC_ERR_STATE, "the precision needs Linv (the GP was set without it)");
        rows = std::max(rows, (size_t)std::max((gs.cap + 15) / 16 * 16, gs.npad));
    }
    const int n = h->P.gp[0].nv;
    for (int g = 1; g < ngp; ++g)
        if (h->P.gp[g].nv != n)
            return fail(GPMPC_ERR_STATE, "the GPs differ in their training rows: the call ranks the same rows in all");
    if (m < 1 || m >= n)
        return fail(GPMPC_ERR_ARG, "m must be in 1 .. n - 1 (at least one row stays): " + std::to_string(m) + " of " +
                                       std::to_string(n) + " rows asked for");
    if (m > kRedundantMaxPicks) return fail(GPMPC_ERR_ARG, "m must be at most " + std::to_string(kRedundantMaxPicks));
    (void)hipSetDevice(h->device);
    // the scratch: made by the first call and made again when a capacity or the picks have grown past it
    if (!h->red || rows > h->red_rows || (size_t)m > h->red_m) {
        const size_t want_rows = std::max(rows, h->red_rows), want_m = std::max(((size_t)m + 15) / 16 * 16, h->red_m);
        const gpmpc_status got = replace_scratch(&h->red, RedundantLayout{want_rows, want_m, (size_t)ngp}.end);
        if (got != GPMPC_OK) return got;
        h->red_rows = want_rows;
        h->red_m = want_m;
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const RedundantLayout lay{h->red_rows, h->red_m, (size_t)ngp};
    GPRedundant q{};
    q.n = n;
    q.m = m;
    q.n_gp = ngp;
    q.ldn = (int)lay.ldn;
    q.nblk = (n + kPickBlock - 1) / kPickBlock;
    for (int g = 0; g < ngp; ++g) {
        GPRedundantGP& rg = q.g[g];
        rg.linvT = h->P.gp[g].linvT;
        rg.ccol = h->red + lay.ccol + (size_t)g * lay.mcap * lay.ldn;
        rg.npad = h->gp[g].npad;
        rg.sf2 = h->P.gp[g].sf2;
        rg.sn2 = h->P.gp[g].sn2;
    }
    q.p = h->red + lay.p;
    q.bval = h->red + lay.bval;
    q.bidx = reinterpret_cast<int32_t*>(h->red + lay.bidx);
    q.state = reinterpret_cast<int32_t*>(h->red + lay.state);
    q.pick = pick_dev;
    q.score = score_dev;
    q.ok = ok_dev;
    HIPCHK(launch_gp_redundant(q, s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_gp_observe(gpmpc_handle* h, int32_t P, const double* x_dev, const double* u_dev,
                              const double* xnext_dev, int32_t m, const int32_t* pick_dev, double dt_diff,
                              double gravity, int32_t evict_oldest, double* inputs_dev, double* targets_dev,
                              int32_t* accepted_dev, int32_t* dropped_ok_dev, void* stream) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    const char* bad = transitions_bad(P, x_dev, u_dev, xnext_dev, m, pick_dev, dt_diff, gravity);
    if (!bad && m > h->max_batch) bad = "more rows than max_batch (the staging scratch holds max_batch rows)";
    if (bad) return fail(GPMPC_ERR_ARG, bad);
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "the prior parameters are not set (gpmpc_set_model first)");
    // every refusal comes before any GP changes
    const int ngp = h->md.ngp;
    for (int g = 0; g < ngp; ++g) {
        const gpmpc_status ready = gp_update_ready(h, g, kAppend, nullptr);
        if (ready != GPMPC_OK) return ready;
    }
    const int n = h->P.gp[0].n, cap = h->gp[0].cap;
    for (int g = 1; g < ngp; ++g)
        if (h->P.gp[g].n != n || h->gp[g].cap != cap)
            return fail(GPMPC_ERR_STATE, "the GPs differ in their training rows or capacity: the call appends the same rows to all");
    const int64_t excess = (int64_t)n + m - cap;
    if (excess > 0) {
        if (!evict_oldest)
            return fail(GPMPC_ERR_ARG, "capacity exceeded: " + std::to_string(n) + " + " + std::to_string(m) +
                                           " rows, capacity " + std::to_string(cap) + " (gpmpc_gp_reserve, or evict_oldest)");
        if (excess >= n)
            return fail(GPMPC_ERR_ARG, "at least one row stays: " + std::to_string(excess) + " of " + std::to_string(n) +
                                           " rows would be dropped");
        for (int g = 0; g < ngp; ++g) {
            const gpmpc_status ready = gp_update_ready(h, g, kDrop, nullptr);
            if (ready != GPMPC_OK) return ready;
        }
    }
    (void)hipSetDevice(h->device);
    const gpmpc_status got = ensure_observe_scratch(h);
    if (got != GPMPC_OK) return got;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    const ObserveLayout lay = observe_layout(h);
    GPObserve a = observe_args(h, P, x_dev, u_dev, xnext_dev, m, pick_dev, dt_diff, gravity);
    a.inputs = inputs_dev;
    a.targets = targets_dev;
    for (int g = 0, col = 0; g < ngp; col += h->md.gp_dim[g], ++g) {
        a.Xg[g] = h->obs + lay.sx + (size_t)h->max_batch * col;
        a.yg[g] = h->obs + lay.sy + (size_t)h->max_batch * g;
    }
    HIPCHK(launch_gp_observe(a, s));
    // the drops and appends are the calls a caller would make on the staged rows, GP after GP
    const int ablk = (m + 15) / 16, dblk = excess > 0 ? (int)((excess + 15) / 16) : 1;
    for (int g = 0; g < ngp; ++g) {
        int32_t* dok = dropped_ok_dev ? dropped_ok_dev + (size_t)g * dblk : nullptr;
        if (excess > 0) {
            const gpmpc_status st = gpmpc_gp_drop_oldest(h, g, (int32_t)excess, dok, stream);
            if (st != GPMPC_OK) return st;
        } else if (dok) {
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dok, 1, 1, s));
        }
        const gpmpc_status st = gpmpc_gp_append(h, g, m, a.Xg[g], a.yg[g],
                                                accepted_dev ? accepted_dev + (size_t)g * ablk : nullptr, stream);
        if (st != GPMPC_OK) return st;
    }
    return GPMPC_OK;
}


gpmpc_status gpmpc_rollout(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                           int32_t with_gp, double* x_dev, double* var_dev) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    const char* bad = nullptr;
    if (P < 1 || T < 1) bad = "no trajectories or no steps (P, T >= 1)";
    else if (!x0_dev || !u_dev || !x_dev) bad = "null array (x0_dev, u_dev and x_dev are required)";
    else if (with_gp != 0 && with_gp != 1) bad = "with_gp must be 0 or 1";
    else if ((int64_t)P * ((int64_t)T + 1) * h->md.nx > INT32_MAX) bad = "P (T + 1) nx does not fit an int32";
    if (bad) return fail(GPMPC_ERR_ARG, bad);
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "the prior parameters are not set (gpmpc_set_model first)");
    const int ngp = h->md.ngp;
    if (with_gp) {
        if (!h->P.use_gp) return fail(GPMPC_ERR_STATE, "with_gp = 1 while the handle's GPs are off (gpmpc_use_gp)");
        for (int g = 0; g < ngp; ++g)
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP " + std::to_string(g) + " not set");
    }
    if (var_dev)
        for (int g = 0; g < ngp; ++g) {
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "the variance needs GP " + std::to_string(g) + ", which is not set");
            if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "the variance needs Linv (GP " + std::to_string(g) + " has none)");
        }
    (void)hipSetDevice(h->device);
    size_t D = 0;
    for (int g = 0; g < ngp; ++g) D += h->md.gp_dim[g];
    const size_t need = var_dev ? (size_t)P * T * D : 0;
    if (need > h->roll_doubles) {   // (before anything is queued: a failed allocation leaves the handle as it was)
        const gpmpc_status got = replace_scratch(&h->roll, need);
        if (got != GPMPC_OK) return got;
        h->roll_doubles = need;
    }
    // on a stream of the handle's own, behind the handle's last call, and drained before the call returns
    HIPCHK(ensure_side(h));
    hipStream_t s = h->side;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    RolloutArgs a{};
    for (int i = 0; i < kMaxParams; ++i) a.params[i] = h->P.params[i];
    a.dt = h->P.dt;
    a.P = P;
    a.T = T;
    a.x0 = x0_dev;
    a.u = u_dev;
    a.x = x_dev;
    if (with_gp)   // the means as the solver reads them: the tile pack of ProblemDev::gp (a FITC overlay included)
        for (int g = 0; g < ngp; ++g) a.gp[g] = h->P.gp[g];
    HIPCHK(launch_rollout(h->model, a, with_gp != 0, s));
    if (var_dev) {
        // gpmpc_gp_predict's variance launch (with_noise = 0) on GP g's columns of the gathered inputs, written
        // straight into the caller's [P][T][n_gp]
        HIPCHK(launch_rollout_inputs(h->model, x_dev, u_dev, P, T, h->roll, s));
        for (int g = 0, col = 0; g < ngp; col += h->md.gp_dim[g], ++g) {
            PostArgs pa{};
            pa.Z = h->roll + col;
            pa.ldz = (int)D;
            pa.P = P * T;
            pa.d = h->md.gp_dim[g];
            pa.with_noise = 0;
            pa.var = var_dev;
            pa.var_stride = ngp;
            pa.var_off = g;
            HIPCHK(launch_gp_post(h->P.gp[g], h->gp[g].npad, pa, false, s, h->var_trim ? 0 : 1));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_rollout_lin(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                               int32_t with_gp, double* x_dev, double* A_dev, double* B_dev, double* var_dev,
                               const double* K, const double* cov0_dev, int32_t with_noise, double* cov_dev) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    const int nx = h->md.nx, nu = h->md.nu;
    const char* bad = nullptr;
    if (P < 1 || T < 1) bad = "no trajectories or no steps (P, T >= 1)";
    else if (!x0_dev || !u_dev || !x_dev) bad = "null array (x0_dev, u_dev and x_dev are required)";
    else if (!A_dev || !B_dev) bad = "null array (A_dev and B_dev are required)";
    else if (with_gp != 0 && with_gp != 1) bad = "with_gp must be 0 or 1";
    else if (with_noise != 0 && with_noise != 1) bad = "with_noise must be 0 or 1";
    else if ((int64_t)P * ((int64_t)T + 1) * nx > INT32_MAX) bad = "P (T + 1) nx does not fit an int32";
    else if ((int64_t)P * (int64_t)T * nx * nx > INT32_MAX) bad = "P T nx nx does not fit an int32";
    if (!bad && K)
        for (int i = 0; i < nu * nx; ++i)
            if (!std::isfinite(K[i])) bad = "K has a non-finite entry";
    if (bad) return fail(GPMPC_ERR_ARG, bad);
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "the prior parameters are not set (gpmpc_set_model first)");
    const int ngp = h->md.ngp;
    if (with_gp) {
        if (!h->P.use_gp) return fail(GPMPC_ERR_STATE, "with_gp = 1 while the handle's GPs are off (gpmpc_use_gp)");
        for (int g = 0; g < ngp; ++g)
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP " + std::to_string(g) + " not set");
    }
    const bool want_var = var_dev || cov_dev;
    if (want_var)
        for (int g = 0; g < ngp; ++g) {
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "the variance needs GP " + std::to_string(g) + ", which is not set");
            if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "the variance needs Linv (GP " + std::to_string(g) + " has none)");
        }
    (void)hipSetDevice(h->device);
    size_t D = 0;
    for (int g = 0; g < ngp; ++g) D += h->md.gp_dim[g];
    // the gathered variance inputs, and behind them the variances themselves when the caller takes none
    const size_t gathered = want_var ? (size_t)P * T * D : 0;
    const size_t need = gathered + (cov_dev && !var_dev ? (size_t)P * T * ngp : 0);
    if (need > h->roll_doubles) {   // (before anything is queued: a failed allocation leaves the handle as it was)
        const gpmpc_status got = replace_scratch(&h->roll, need);
        if (got != GPMPC_OK) return got;
        h->roll_doubles = need;
    }
    HIPCHK(ensure_side(h));
    hipStream_t s = h->side;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    RolloutLinArgs a{};
    for (int i = 0; i < kMaxParams; ++i) a.r.params[i] = h->P.params[i];
    a.r.dt = h->P.dt;
    a.r.P = P;
    a.r.T = T;
    a.r.x0 = x0_dev;
    a.r.u = u_dev;
    a.r.x = x_dev;
    a.A = A_dev;
    a.B = B_dev;
    if (with_gp)
        for (int g = 0; g < ngp; ++g) a.r.gp[g] = h->P.gp[g];
    HIPCHK(launch_rollout_lin(h->model, a, with_gp != 0, s));
    if (want_var) {
        // gpmpc_rollout's gather and variance launches, statement by statement
        double* var = var_dev ? var_dev : h->roll + gathered;
        HIPCHK(launch_rollout_inputs(h->model, x_dev, u_dev, P, T, h->roll, s));
        for (int g = 0, col = 0; g < ngp; col += h->md.gp_dim[g], ++g) {
            PostArgs pa{};
            pa.Z = h->roll + col;
            pa.ldz = (int)D;
            pa.P = P * T;
            pa.d = h->md.gp_dim[g];
            pa.with_noise = 0;
            pa.var = var;
            pa.var_stride = ngp;
            pa.var_off = g;
            HIPCHK(launch_gp_post(h->P.gp[g], h->gp[g].npad, pa, false, s, h->var_trim ? 0 : 1));
        }
        if (cov_dev) {
            RolloutCovArgs c{};
            c.dt = h->P.dt;
            c.P = P;
            c.T = T;
            c.closed = K ? 1 : 0;
            if (K)
                for (int i = 0; i < nu * nx; ++i) c.K[i] = K[i];
            for (int g = 0; g < ngp; ++g) c.noise[g] = with_noise ? h->P.gp[g].sn2 : 0.0;
            c.x = x_dev;
            c.u = u_dev;
            c.A = A_dev;
            c.B = B_dev;
            c.var = var;
            c.cov0 = cov0_dev;
            c.cov = cov_dev;
            HIPCHK(launch_rollout_cov(h->model, c, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    return GPMPC_OK;
}

gpmpc_status gpmpc_rollout_sample(gpmpc_handle* h, int32_t P, int32_t T, const double* x0_dev, const double* u_dev,
                                  const double* xref_dev, const double* K, int32_t clip, const double* xi_dev,
                                  int32_t with_gp, int32_t with_noise, double* x_dev, double* uapp_dev,
                                  double* var_dev) {
    if (!h) return fail(GPMPC_ERR_ARG, "null handle");
    const int nx = h->md.nx, nu = h->md.nu;
    const char* bad = nullptr;
    if (P < 1 || T < 1) bad = "no trajectories or no steps (P, T >= 1)";
    else if (!x0_dev || !u_dev || !x_dev) bad = "null array (x0_dev, u_dev and x_dev are required)";
    else if (with_gp != 0 && with_gp != 1) bad = "with_gp must be 0 or 1";
    else if (with_noise != 0 && with_noise != 1) bad = "with_noise must be 0 or 1";
    else if (clip != 0 && clip != 1) bad = "clip must be 0 or 1";
    else if ((K != nullptr) != (xref_dev != nullptr)) bad = "K and xref_dev go together (both given, or both NULL)";
    else if ((int64_t)P * ((int64_t)T + 1) * nx > INT32_MAX) bad = "P (T + 1) nx does not fit an int32";
    if (!bad && K)
        for (int i = 0; i < nu * nx; ++i)
            if (!std::isfinite(K[i])) bad = "K has a non-finite entry";
    if (bad) return fail(GPMPC_ERR_ARG, bad);
    if (!h->model_set) return fail(GPMPC_ERR_STATE, "the prior parameters are not set (gpmpc_set_model first)");
    const int ngp = h->md.ngp;
    if (with_gp) {
        if (!h->P.use_gp) return fail(GPMPC_ERR_STATE, "with_gp = 1 while the handle's GPs are off (gpmpc_use_gp)");
        for (int g = 0; g < ngp; ++g)
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "GP " + std::to_string(g) + " not set");
    }
    const bool want_var = xi_dev || var_dev;
    if (want_var)
        for (int g = 0; g < ngp; ++g) {
            if (!h->gp[g].set) return fail(GPMPC_ERR_STATE, "the variance needs GP " + std::to_string(g) + ", which is not set");
            if (!h->gp[g].linvT) return fail(GPMPC_ERR_STATE, "the variance needs Linv (GP " + std::to_string(g) + " has none)");
        }
    (void)hipSetDevice(h->device);
    // on the handle's side stream, behind the handle's last call, and drained before the call returns (gpmpc_rollout)
    HIPCHK(ensure_side(h));
    hipStream_t s = h->side;
    HIPCHK(order_after_last(h, s));
    StreamMark mark{h, s};
    RolloutSampleArgs a{};
    for (int i = 0; i < kMaxParams; ++i) a.r.params[i] = h->P.params[i];
    a.r.dt = h->P.dt;
    a.r.P = P;
    a.r.T = T;
    a.r.x0 = x0_dev;
    a.r.u = u_dev;
    a.r.x = x_dev;
    if (with_gp)
        for (int g = 0; g < ngp; ++g) a.r.gp[g] = h->P.gp[g];
    a.xref = xref_dev;
    a.xi = xi_dev;
    a.uapp = uapp_dev;
    a.var = var_dev;
    a.closed = K ? 1 : 0;
    a.clip = clip;
    if (K)
        for (int i = 0; i < nu * nx; ++i) a.K[i] = K[i];
    for (int c = 0; c < nu; ++c) {
        a.u_lo[c] = h->P.u_lo[c];
        a.u_hi[c] = h->P.u_hi[c];
    }
    if (want_var)   // the exact rows and their factor, as gpmpc_gp_predict reads them (no LOVE root, no FITC overlay)
        for (int g = 0; g < ngp; ++g) {
            const GPDev& d = h->P.gp[g];
            a.noise[g] = with_noise ? d.sn2 : 0.0;
            a.vg[g] = RolloutSampleGP{d.vrows, d.linvT, d.nv, h->gp[g].npad, d.inv_ell2, d.sf2};
        }
    HIPCHK(launch_rollout_sample(h->model, a, with_gp != 0, s));
    HIPCHK(hipStreamSynchronize(s));
    return GPMPC_OK;
}

}  // extern "C"
