// The local/global iterations of the reference's projective-dynamics solver (projective_dynamics/Simulators.py:494-526) for a
// batch of frames of the resident animation: q_0 given, q_{k+1} = A^-1 (sum_i S_i^T p_i(q_k) + M/h^2 s), s fixed.  Every
// selected frame is its own solve.  Self-collisions are not modelled; positional constraints (pins) are a constant added to ms,
// external forces and the floor (resolve_collision) act on s before the iterations: both further down.  The end of the reference's step
// (:531-532: velocities = (q - positions) / dt, positions = q) is asb_pdsolve_advance below: a roll-out is iterate, advance, iterate ...
//
// State of a solve over the n_sel frames range(f0, f1, fj), owned by the context and reused by the next solve:
//   ms  (n_sel, N, 3) frame-major   the inertia term diag[n] s_f[n, d], formed once by k_gs_inertia<false> (asb_gstep.hip): the
//                                   very values asb_gstep_inertia adds
//   Q   (3 N, ld) vertex-major      the iterate, row 3 v + d, frames contiguous, ld = n_sel rounded up to 64.  The layout of
//                                   CpWorld: with T = Q, no mean, no masses and inv_psf = 1, cp_pos returns the stored value
//                                   and the per-element routines of asb_cproj.hip run on it unchanged.  The padding columns
//                                   [n_sel, ld) are zeroed once and never read as frames nor written.
//   b   (n_sel, N, 3) frame-major   the right-hand side of the iteration in flight
//   P   (3 N, ld) vertex-major      only after asb_pdsolve_carry: the positions at the START of the current time step (the
//                                   reference's model.positions), laid out and padded like Q; with it the solve's own device
//                                   copy of diag, which ctx->gs_diag is not (asb_gstep_inertia rewrites that one)
//   slots                           per kind the element set-up of an asb_cproj_setup (a CpSetup, moved out of the context by
//                                   asb_cp_move) and the CSR of its S^T, registered once: no host-to-device copy happens inside
//                                   the iteration loop.  A reduced slot owns no operator: it names a bank, and every use reads
//                                   ctx->rf_bank[slot.bank], where the bank's buffers stay whichever bank is current
//
// One iteration, in stream order:
//   per slot, in order, per chunk of frames   k_cproj_em on the iterate's world, then k_st_apply (the first slot overwrites b,
//                                   the later ones accumulate); a reduced slot: k_cproj_em of the sampled elements,
//                                   k_rforce_coef, k_rforce_gemm with the operator and solver of the slot's BANK
//                                   (asb_rforce_bank: the one current when the slot was registered; one reduced slot per bank)
//   k_pd_add                        b += ms, elementwise -- the order of asb_gstep_inertia
//   k_pdsolve_gemm                  the tile of k_gstep_gemm (asb_gstep_tile.h: same loop, same accumulators) with a
//                                   VERTEX-major epilogue: the 64 frames x 96 rows of a block go through LDS rows of PD_LDQ =
//                                   65 doubles, row 3 m + d holding its 64 frames.  Writes: lane (i, g) stores frame g + 4 q
//                                   of vertex i, ds_write_b64 serves 16 lanes (one g) at a time and their addresses differ by
//                                   3 * 65 * i doubles -- odd, so the 16 land in 16 different bank pairs.  Reads: 64 lanes read 64
//                                   consecutive doubles of a row and store them as one 512-byte run of Q.  On request the same
//                                   accumulators are staged a second time, frame-major (gs_store_fm), into the caller's tensor.
//                                   With the history on, the block first reads the entries of Q it is about to overwrite:
//                                   wave w sums rows w, w + 4, .. of its 64 frames, the four partials are added in wave order,
//                                   and k_pd_hist adds the vertex tiles' records of a frame in ascending order.
// Nothing is split and nothing is atomic: repeats, frame sub-ranges and any chunk width give identical bits.
// With the slab factor of asb_gslab.hip held instead of the inverse, the product of an iteration, c of a hyper-reduced solve and
// the operator A^-1 S^T V go through that unit's sweep (asb_gslab_solve_fm / _rows); the history is then refused.
// With the position subspace of asb_gsub.hip held, the same three go through asb_gsub_solve_fm (the affine map o' + P rhs: the
// product of an iteration, c) and asb_gsub_solve_rows (its linear part P S^T V: the operator); the history is refused too.
#include "asb_gstep_tile.h"

#include <algorithm>
#include <cmath>
#include <vector>

#define PD_LDQ 65           // LDS row of the vertex-major epilogue: 64 frames + 1
#define PD_MAX_SLOTS 8

struct PdSlot {
    CpSetup cp;                                                 // the element set-up of asb_cproj_setup, taken over from the context
    int reduced = 0;
    long long n_cols = 0;                                       // rows of its stacked projections
    int *st_ptr = nullptr, *st_idx = nullptr;                   // the CSR of S^T (not for the reduced kind)
    double* st_val = nullptr;
    double smin = 1.0, smax = 1.0;
    int bank = 0;                                               // reduced: ctx->rf_bank[bank] holds its operator and solver
};

struct asb_pds {
    bool begun = false;
    long long n = 0, n_sel = 0, ld = 0;
    double *ms = nullptr, *Q = nullptr, *b = nullptr;
    double *part = nullptr, *hist = nullptr;      // (vertex tiles, n_sel, 2) records of one iteration; (iterations, n_sel, 2)
    // asb_hyper_iterate: c = A^-1 ms (3 N, ld) vertex-major like Q; the touched rows of Q and c (3 N_t, ld).  (The touched
    // columns of G^T belong to the banks: RfBank::Gc.)
    double *c = nullptr, *Qc = nullptr, *cc = nullptr;
    // the time step: what asb_pdsolve_begin was given (for asb_pdsolve_carry) and what asb_pdsolve_carry made
    bool carry = false;
    CpWorld w = {};
    int f0 = 0, fj = 1;
    double acc[3] = {0.0, 0.0, 0.0};
    std::vector<double> diag_host;
    double *P = nullptr, *diag = nullptr;
    // the context's pins bound to this solve (asb_pdsolve_pins): their term is in ms; row of shift = pin_row0 + frame + pin_step
    bool pins = false;
    long long pin_row0 = 0, pin_step = 0;
    // the context's forces and floor bound to this solve (asb_pdsolve_external): row of fa = ext_row0 + frame + ext_step
    bool ext = false;
    long long ext_row0 = 0, ext_step = 0;
    int mode = 0;                                 // of asb_pdsolve_begin
    bool q_is_s = false;                          // the iterate holds the explicit state: begun with start 0, or advanced
    int n_slots = 0;
    PdSlot slot[PD_MAX_SLOTS];
};

void asb_pdsolve_free(asb_ctx* ctx) {             // (the buffers went with the context's registered allocations)
    delete ctx->pds;
    ctx->pds = nullptr;
}

// ---------------------------------------------------------------- the start state
// grid (rows / 4, frame tiles): wave = one row 3 v + d x 64 frames.  start 0: the explicit state s_f (mode as k_gs_inertia),
// 1: the frame x_f
__global__ __launch_bounds__(256) void k_pd_init(CpWorld w, int f0, int fj, int n_sel, long long n_verts, int start, int mode, double acc0,
                                                 double acc1, double acc2, double* __restrict__ Q, long long ld) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int c = (int)blockIdx.y * 64 + lane;
    if (r >= 3 * n_verts || c >= n_sel) return;
    const int v = (int)(r / 3), d = (int)(r % 3);
    const long long f = (long long)f0 + (long long)c * fj;
    const double acc[3] = {acc0, acc1, acc2};
    double x[3], xp[3];
    cp_pos(w, f, v, x);
    if (start == 0) {
        if (mode == 1) {
            cp_pos(w, f > 0 ? f - 1 : 0, v, xp);
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = 2.0 * x[k] - xp[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = x[k] + acc[k];
    }
    Q[r * ld + c] = d == 0 ? x[0] : (d == 1 ? x[1] : x[2]);
}

// grid (row tiles of 64, frame tiles of 64): in (n_sel, rows) frame-major -> Q (rows, ld), a copy
__global__ __launch_bounds__(256) void k_pd_transpose(const double* __restrict__ in, int n_sel, long long rows, double* __restrict__ Q,
                                                      long long ld) {
    __shared__ double tile[64 * 65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64;
    const int t0 = (int)blockIdx.y * 64;
    for (int fl = wv; fl < 64; fl += 4)
        if (t0 + fl < n_sel && r0 + lane < rows) tile[fl * 65 + lane] = in[(long long)(t0 + fl) * rows + r0 + lane];
    __syncthreads();
    for (int rl = wv; rl < 64; rl += 4)
        if (r0 + rl < rows && t0 + lane < n_sel) Q[(r0 + rl) * ld + t0 + lane] = tile[lane * 65 + rl];
}

// b[i] += ms[i]
__global__ __launch_bounds__(256) void k_pd_add(double* __restrict__ b, const double* __restrict__ ms, long long len) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long long)gridDim.x * 256) b[i] += ms[i];
}

// ---------------------------------------------------------------- the product, written into the iterate
// grid (Np / GS_TN, frame tiles); b (F, n, 3) frame-major; Q (3 n, ld); out (F, n, 3) with FM; part (gridDim.x, F, 2) with HIST
template <bool FM, bool HIST>
__global__ __launch_bounds__(256) void k_pdsolve_gemm(const double* __restrict__ b, const double* __restrict__ Ainv, int n, int np,
                                                      long long F, double* __restrict__ Q, long long ld, double* __restrict__ out,
                                                      double* __restrict__ part) {
    constexpr int ROWS = GS_TN * 3;
    static_assert(ROWS * PD_LDQ + 4 * 64 * 2 <= GS_SM, "the vertex-major stage and the history partials reuse the operand buffers");
    __shared__ double sm[GS_SM];
    const int m0 = (int)blockIdx.x * GS_TN;
    const long long t0 = (long long)blockIdx.y * GS_TF;
    d4 acc[3][2];
    gs_contract(b, Ainv, n, np, F, m0, t0, sm, acc);
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) sm[((16 * y + i) * 3 + d) * PD_LDQ + wave * 16 + g + 4 * q] = acc[d][y][q];
    __syncthreads();
    const int nv = n - m0 < GS_TN ? n - m0 : GS_TN;
    const int nf = F - t0 < GS_TF ? (int)(F - t0) : GS_TF;
    const int run = nv * 3;
    double* qt = Q + 3LL * m0 * ld + t0;          // the tile's corner: row r, frame fl at qt[r * ld + fl]
    if (HIST) {
        double d2 = 0.0, n2 = 0.0;
        if (lane < nf)
            for (int r = wave; r < run; r += 4) {
                const double nw = sm[r * PD_LDQ + lane], e = nw - qt[(long long)r * ld + lane];
                d2 = fma(e, e, d2);
                n2 = fma(nw, nw, n2);
            }
        double* hp = sm + ROWS * PD_LDQ;
        hp[(wave * 64 + lane) * 2] = d2;
        hp[(wave * 64 + lane) * 2 + 1] = n2;
        __syncthreads();                          // every read of the old entries is done before the first write below
        if (wave == 0 && lane < nf) {
            double* o = part + ((long long)blockIdx.x * F + t0 + lane) * 2;
            o[0] = ((hp[lane * 2] + hp[(64 + lane) * 2]) + hp[(128 + lane) * 2]) + hp[(192 + lane) * 2];
            o[1] = ((hp[lane * 2 + 1] + hp[(64 + lane) * 2 + 1]) + hp[(128 + lane) * 2 + 1]) + hp[(192 + lane) * 2 + 1];
        }
    }
    for (int e = tid; e < ROWS * 64; e += 256) {
        const int r = e >> 6, fl = e & 63;
        if (r < run && fl < nf) qt[(long long)r * ld + fl] = sm[r * PD_LDQ + fl];
    }
    if (FM) {
        __syncthreads();                          // the stage is read out: it is staged again, frame-major
        gs_store_fm(acc, sm, n, F, m0, t0, out);
    }
}

// one thread per frame: rec[f] = the vertex tiles' records of frame f added in ascending tile order
__global__ __launch_bounds__(256) void k_pd_hist(const double* __restrict__ part, int tiles, long long F, double* __restrict__ rec) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double d2 = 0.0, n2 = 0.0;
    for (int t = 0; t < tiles; ++t) {
        d2 += part[((long long)t * F + f) * 2];
        n2 += part[((long long)t * F + f) * 2 + 1];
    }
    rec[f * 2] = d2;
    rec[f * 2 + 1] = n2;
}

// the vertices of the solver the context holds: the explicit inverse, the slab factor (asb_gslab.hip) or the position subspace
// (asb_gsub.hip); 0: none
static long long pd_solver_n(const asb_ctx* ctx) {
    const long long m = asb_gslab_n(ctx), u = asb_gsub_n(ctx);
    return u > 0 ? u : (m > 0 ? m : (ctx->gs_Ainv ? ctx->gs_n : 0));
}

// ---------------------------------------------------------------- entry points
extern "C" int asb_pdsolve_begin(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean,
                                 double psf, const double* diag, int mode, const double* acc3, int start, const double* start_dev) {
    if (!ctx || !diag || !acc3) return ASB_ERR_ARG;
    if (ctx->pds) ctx->pds->begun = false, ctx->pds->n_slots = 0, ctx->pds->carry = false, ctx->pds->pins = false, ctx->pds->ext = false;
    if (fj >= 1 && f1 > f0 && ((f1 - f0 + fj - 1) / fj + 63) / 64 > 65535)        // on the count alone, before any tensor is looked at
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_pdsolve_begin: %lld frames in one solve (at most %d)", (long long)((f1 - f0 + fj - 1) / fj), 65535 * 64);
    if (mode != 0 && mode != 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_begin: mode %d (0: s = x, 1: s = 2 x - x_prev)", mode);
    if (start < 0 || start > 2 || (start == 2 && !start_dev))
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_begin: start %d (0: the explicit state, 1: the frame, 2: a device tensor)", start);
    CpWorld w;
    int64_t n_sel;
    int rc;
    if ((rc = asb_world_frames(ctx, "asb_pdsolve_begin", which, f0, f1, fj, add_mean, psf, &w, &n_sel))) return rc;
    const int64_t n = ctx->n_loc;
    if (pd_solver_n(ctx) != n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_begin: no inverse for the %lld vertices of the tensor on the device (asb_gstep_setup)", (long long)n);
    for (int64_t v = 0; v < n; ++v)
        if (!std::isfinite(diag[v])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_begin: diag[%lld] is not finite", (long long)v);
    if (!std::isfinite(acc3[0]) || !std::isfinite(acc3[1]) || !std::isfinite(acc3[2])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_begin: acc is not finite");
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    if (!ctx->pds) ctx->pds = new asb_pds();
    asb_pds* s = ctx->pds;
    const long long ld = (n_sel + 63) / 64 * 64;
    const size_t len = (size_t)n_sel * n * 3;
    if ((rc = asb_alloc(ctx, &ctx->gs_diag, (size_t)n))) return rc;
    if ((rc = asb_alloc(ctx, &s->ms, len))) return rc;
    if ((rc = asb_alloc(ctx, &s->b, len))) return rc;
    if ((rc = asb_alloc(ctx, &s->Q, (size_t)3 * n * ld))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(ctx->gs_diag, diag, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(s->Q, 0, (size_t)3 * n * ld * sizeof(double), ctx->stream));
    asb_gs_inertia_launch(ctx, w, (int)f0, (int)fj, (int)n_sel, (long long)n, ctx->gs_diag, mode, acc3, false, s->ms);
    const unsigned gt = (unsigned)((n_sel + 63) / 64);
    if (start == 2)
        hipLaunchKernelGGL(k_pd_transpose, dim3((unsigned)((3 * n + 63) / 64), gt), dim3(256), 0, ctx->stream, start_dev, (int)n_sel,
                           (long long)(3 * n), s->Q, ld);
    else
        hipLaunchKernelGGL(k_pd_init, dim3((unsigned)((3 * n + 3) / 4), gt), dim3(256), 0, ctx->stream, w, (int)f0, (int)fj, (int)n_sel,
                           (long long)n, start, mode, acc3[0], acc3[1], acc3[2], s->Q, ld);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the host arrays and the caller's start tensor may go
    s->n = n, s->n_sel = n_sel, s->ld = ld, s->begun = true;
    s->w = w, s->f0 = (int)f0, s->fj = (int)fj;
    s->acc[0] = acc3[0], s->acc[1] = acc3[1], s->acc[2] = acc3[2];
    s->diag_host.assign(diag, diag + n);
    s->mode = mode, s->q_is_s = start == 0;
    return ASB_OK;
}

extern "C" int asb_pdsolve_slot(asb_ctx* ctx, double sigma_min, double sigma_max, int reduced, int64_t n_rows, const int64_t* indptr,
                                const int64_t* indices, const double* data) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: no solve begun (asb_pdsolve_begin)");
    if (s->n_slots >= PD_MAX_SLOTS) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_pdsolve_slot: more than %d kinds", PD_MAX_SLOTS);
    if (ctx->cp.kind < 0 || ctx->cp.verts != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: no element set-up for the resident tensor (asb_cproj_setup)");
    if (!(sigma_min <= sigma_max)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: sigma_min %g > sigma_max %g", sigma_min, sigma_max);
    const long long n_cols = asb_cproj_rows(ctx->cp.kind, ctx->cp.n);
    PdSlot& p = s->slot[s->n_slots];
    int rc;
    if (reduced) {
        const asb_ctx::RfBank& b = asb_rf_cur(ctx);
        for (int k = 0; k < s->n_slots; ++k)
            if (s->slot[k].reduced && s->slot[k].bank == ctx->rf_cur)       // (another bank: asb_rforce_bank before the operator)
                ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: a second reduced kind (the context holds one operator and one solver)");
        if (b.mp < 1 || b.r < 1 || b.n != s->n)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: no operator or solver for the tensor on the device (asb_rforce_operator, asb_rforce_solver)");
        if (b.pt_max >= n_cols)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: an interpolation point names row %lld, the sampled elements have %lld", (long long)b.pt_max, n_cols);
    } else {
        if (!indptr) return ASB_ERR_ARG;
        if (n_rows != s->n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_slot: S^T has %lld rows, the tensor %lld vertices", (long long)n_rows, s->n);
        std::vector<int> p32, c32;
        if ((rc = asb_csr_check32(ctx, "asb_pdsolve_slot", n_rows, indptr, indices, data, n_cols, p32, c32))) return rc;
        ASB_HIP(ctx, hipSetDevice(ctx->dev));
        if ((rc = asb_alloc(ctx, &p.st_ptr, p32.size()))) return rc;
        if ((rc = asb_alloc(ctx, &p.st_idx, c32.size() + 1))) return rc;
        if ((rc = asb_alloc(ctx, &p.st_val, c32.size() + 1))) return rc;
        if ((rc = asb_csr_stage(ctx, p32, c32, data, p.st_ptr, p.st_idx, p.st_val))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the staging vectors die here)
    }
    // the set-up of asb_cproj_setup passes to the slot (the slot's previous buffers to the context, which has no set-up now)
    asb_cp_move(ctx, ctx->cp, p.cp);
    p.n_cols = n_cols, p.reduced = reduced ? 1 : 0;
    p.smin = sigma_min, p.smax = sigma_max, p.bank = ctx->rf_cur;
    ++s->n_slots;
    return ASB_OK;
}

extern "C" int asb_pdsolve_iterate(asb_ctx* ctx, int64_t n_iter, int64_t chunk_frames, double* out_dev, double* hist_out) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun || s->n_slots < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: no solve begun or no kind registered (asb_pdsolve_begin, asb_pdsolve_slot)");
    if (n_iter < 1 || n_iter > (1 << 20)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: %lld iterations", (long long)n_iter);
    if (chunk_frames < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: chunk_frames %lld", (long long)chunk_frames);
    if (pd_solver_n(ctx) != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: the inverse or the tensor changed since asb_pdsolve_begin");
    const bool slab = asb_gslab_n(ctx) > 0, sub = asb_gsub_n(ctx) > 0;
    if (slab && hist_out)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: the history of step norms is not built for the slab factor (asb_gslab_setup)");
    if (sub && hist_out)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: the history of step norms is not built for the position subspace (asb_gsub_setup)");
    const long long n_sel = s->n_sel, n = s->n;
    long long cw[PD_MAX_SLOTS];
    size_t scratch = 0;
    for (int k = 0; k < s->n_slots; ++k) {
        const PdSlot& p = s->slot[k];
        if (p.reduced) {
            const asb_ctx::RfBank& b = ctx->rf_bank[p.bank];
            if (b.mp < 1 || b.r < 1 || b.n != n || b.pt_max >= p.n_cols)
                ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_iterate: the operator or solver changed since asb_pdsolve_slot");
            cw[k] = asb_rforce_chunk_width(b.r, p.n_cols, n_sel);
        } else {
            cw[k] = asb_cforce_chunk_width(p.n_cols, chunk_frames, n_sel);
        }
        scratch = std::max<size_t>(scratch, (size_t)3 * p.n_cols * cw[k]);
    }
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const int tiles = slab || sub ? 0 : (int)(ctx->gs_Np / GS_TN);
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_scratch, scratch))) return rc;
    for (int k = 0; k < s->n_slots; ++k) {          // the coefficients of one chunk, per reduced slot in its bank
        if (!s->slot[k].reduced) continue;
        asb_ctx::RfBank& b = ctx->rf_bank[s->slot[k].bank];
        if ((rc = asb_alloc(ctx, &b.coef, (size_t)3 * (((size_t)b.r + 3) / 4 * 4) * cw[k]))) return rc;
    }
    if (hist_out) {
        if ((rc = asb_alloc(ctx, &s->part, (size_t)tiles * n_sel * 2))) return rc;
        if ((rc = asb_alloc(ctx, &s->hist, (size_t)n_iter * n_sel * 2))) return rc;
    }
    const CpWorld wq = {s->Q, s->ld, nullptr, nullptr, 1.0};
    const long long len = n_sel * n * 3;
    const unsigned g_add = (unsigned)std::min<long long>((len + 255) / 256, 1 << 20);
    const dim3 grid((unsigned)tiles, (unsigned)((n_sel + GS_TF - 1) / GS_TF));
    for (int64_t it = 0; it < n_iter; ++it) {
        for (int k = 0; k < s->n_slots; ++k) {
            const PdSlot& p = s->slot[k];
            for (long long c0 = 0; c0 < n_sel; c0 += cw[k]) {
                const int cn = (int)(c0 + cw[k] < n_sel ? cw[k] : n_sel - c0);
                asb_cproj_em_launch(ctx, p.cp, wq, 0, 1, (int)c0, cn, (int)cw[k], p.smin, p.smax, ctx->cf_scratch);
                if (p.reduced) asb_rforce_chunk_launch(ctx, ctx->rf_bank[p.bank], ctx->cf_scratch, (int)cw[k], (int)c0, cn, k > 0, s->b);
                else asb_st_apply_launch(ctx, p.st_ptr, p.st_idx, p.st_val, ctx->cf_scratch, (int)cw[k], (int)c0, cn, n, k > 0, s->b);
            }
        }
        hipLaunchKernelGGL(k_pd_add, dim3(g_add), dim3(256), 0, ctx->stream, s->b, s->ms, len);
        const bool fm = out_dev && it == n_iter - 1;
        if (sub) {                                  // in -> reduce -> expand into the iterate (frame-major too)
            if ((rc = asb_gsub_solve_fm(ctx, s->b, n_sel, s->Q, fm ? out_dev : nullptr))) return rc;
            continue;
        }
        if (slab) {                                 // in -> sweep -> rows into the iterate (-> k_pd_untranspose)
            if ((rc = asb_gslab_solve_fm(ctx, s->b, n_sel, s->Q, fm ? out_dev : nullptr))) return rc;
            continue;
        }
        auto kern = fm ? (hist_out ? k_pdsolve_gemm<true, true> : k_pdsolve_gemm<true, false>)
                       : (hist_out ? k_pdsolve_gemm<false, true> : k_pdsolve_gemm<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, ctx->stream, s->b, ctx->gs_Ainv, (int)n, (int)ctx->gs_Np, n_sel, s->Q, s->ld, out_dev, s->part);
        if (hist_out)
            hipLaunchKernelGGL(k_pd_hist, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0, ctx->stream, s->part, tiles, n_sel,
                               s->hist + (size_t)it * n_sel * 2);
    }
    ASB_CHECK_LAUNCH(ctx);
    if (hist_out)
        ASB_HIP(ctx, hipMemcpyAsync(hist_out, s->hist, (size_t)n_iter * n_sel * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// ================================================================ the end of a time step
// Simulators.py:531-532 and the next :495 in one pass over the state: per entry (row r = 3 v + d, frame f)
//   s = fl(fl(2 Q - P) + acc[d]),   P <- Q,   Q <- s,   ms[f][v][d] <- fl(diag[v] s)
// the operation order of k_gs_inertia<false> and k_pd_init(start 0, mode 1): an advance from (Q, P) = (x_f, x_{f-1}) leaves the
// bits asb_pdsolve_begin(mode 1, start 0) leaves.  Q and P are vertex-major, ms is frame-major: a block owns 64 rows x 64
// frames, wave w takes rows w, w + 4, ..  Its 64 lanes run along the frames: Q and P are read and written as 512-byte runs.
// diag s goes through an LDS tile of 64 x PD_LDQ doubles, entry (frame fl, row rl) at fl * 65 + rl: the 64 lanes of a write sit
// 65 doubles apart (odd: every bank pair once per 16 lanes), the 64 lanes of a read are consecutive, and ms is written as
// runs of up to 64 doubles along r.  Tail predicates: rows >= 3 N, frames >= n_sel; the padding columns of Q and P are never
// written and stay zero.  Two tensors read, three written, no atomics.
// grid (row tiles of 64, frame tiles of 64)
__global__ __launch_bounds__(256) void k_pd_advance(double* __restrict__ Q, double* __restrict__ P, const double* __restrict__ diag, int n_sel,
                                                    long long rows, long long ld, double acc0, double acc1, double acc2,
                                                    double* __restrict__ ms) {
    __shared__ double tile[64 * PD_LDQ];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64;
    const int t0 = (int)blockIdx.y * 64;
    for (int rl = wv; rl < 64; rl += 4) {
        const long long r = r0 + rl;
        if (r < rows && t0 + lane < n_sel) {
            const long long at = r * ld + t0 + lane;
            const int d = (int)(r % 3);
            const double q = Q[at];
            const double x = 2.0 * q - P[at];
            const double s = x + (d == 0 ? acc0 : (d == 1 ? acc1 : acc2));
            P[at] = q;
            Q[at] = s;
            tile[lane * PD_LDQ + rl] = diag[r / 3] * s;
        }
    }
    __syncthreads();
    for (int fl = wv; fl < 64; fl += 4)
        if (t0 + fl < n_sel && r0 + lane < rows) ms[(long long)(t0 + fl) * rows + r0 + lane] = tile[fl * PD_LDQ + lane];
}

// grid (row tiles of 64, frame tiles of 64): P (rows, ld) vertex-major -> out (n_sel, rows) frame-major, k_pd_transpose reversed
__global__ __launch_bounds__(256) void k_pd_untranspose(const double* __restrict__ P, int n_sel, long long rows, long long ld,
                                                        double* __restrict__ out) {
    __shared__ double tile[64 * PD_LDQ];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64;
    const int t0 = (int)blockIdx.y * 64;
    for (int rl = wv; rl < 64; rl += 4)
        if (r0 + rl < rows && t0 + lane < n_sel) tile[lane * PD_LDQ + rl] = P[(r0 + rl) * ld + t0 + lane];
    __syncthreads();
    for (int fl = wv; fl < 64; fl += 4)
        if (t0 + fl < n_sel && r0 + lane < rows) out[(long long)(t0 + fl) * rows + r0 + lane] = tile[fl * PD_LDQ + lane];
}

void asb_pd_transpose_launch(asb_ctx* ctx, const double* in, int n_sel, long long rows, double* Q, long long ld) {
    hipLaunchKernelGGL(k_pd_transpose, dim3((unsigned)((rows + 63) / 64), (unsigned)((n_sel + 63) / 64)), dim3(256), 0, ctx->stream, in, n_sel, rows,
                       Q, ld);
}

void asb_pd_untranspose_launch(asb_ctx* ctx, const double* P, int n_sel, long long rows, long long ld, double* out) {
    hipLaunchKernelGGL(k_pd_untranspose, dim3((unsigned)((rows + 63) / 64), (unsigned)((n_sel + 63) / 64)), dim3(256), 0, ctx->stream, P, n_sel, rows,
                       ld, out);
}

// ================================================================ positional constraints (pins)
// PositionalConstraint of the reference (Constraint_projections.py:77-113; the first summand of b, Simulators.py:401-413,
// :513-520): pin i holds vertex v_i at p0_i + shift[row] with weight wi_i.  It adds wi_i to A's diagonal (the host's matrix)
// and the constant wi_i (p0_i + shift[row]) to the right-hand side, which does not depend on q: the term lives in ms, and the
// iterations -- plain, hyper-reduced, under either solver -- read ms and are not changed.
// Arithmetic, per pin i, coordinate d and row r (pin_term, the one place):
//   t = fl(p0 + shift[r]) (p0 without a shift),  term = fl(wi t) rounded on its own (no contraction with the add behind it),
//   out = term (STORE)  or  out = fl(out + term) (ADD).
// k_pins_fm: grid (pins / 4, frame tiles of 64), wave w of a block = pin 4 b + w, lane = frame: one thread owns one
// (frame, pin) and its three coordinates of the frame-major tensor (n_sel, n, 3).  No two pins share a vertex (asb_pins_set),
// so no entry has two writers: no atomics.  Tails: pins >= P, frames >= n_sel.  Entries of vertices that are not pinned are not
// touched (a STORE pass is preceded by a memset of the whole tensor: +0.0 there).  Traffic: P n_sel 24 bytes written (and read
// with ADD) plus the tables -- next to the 24 N n_sel bytes of every other pass over ms; the layout is not a performance question.
struct PinsDev {
    const int* v;
    const double *wi, *p0, *shift;      // shift NULL: fixed pins
    int P, per_pin;
    long long n;
};

__device__ __forceinline__ double pin_term(const PinsDev& p, int i, int d, long long row) {
#pragma clang fp contract(off)
    double t = p.p0[3 * i + d];
    if (p.shift) t = t + p.shift[(p.per_pin ? row * p.P + i : row) * 3 + d];
    return p.wi[i] * t;
}

template <bool ADD>
__global__ __launch_bounds__(256) void k_pins_fm(PinsDev p, long long row_base, int fj, int n_sel, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int c = (int)blockIdx.y * 64 + (int)(threadIdx.x & 63);
    if (i >= p.P || c >= n_sel) return;
    const long long row = row_base + (long long)c * fj;
    double* o = out + ((long long)c * p.n + p.v[i]) * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double term = pin_term(p, i, d, row);
        o[d] = ADD ? o[d] + term : term;
    }
}

// the pin term of the frames c = 0 .. n_sel - 1, rows row_base + c fj, into (ADD: onto) a frame-major tensor (n_sel, n, 3)
template <bool ADD>
static void asb_pins_launch(asb_ctx* ctx, long long row_base, int fj, int n_sel, double* out) {
    const asb_ctx::Pins& h = ctx->pins;
    const PinsDev p = {h.v, h.wi, h.p0, h.T > 0 ? h.shift : nullptr, (int)h.P, h.per_pin, (long long)h.n};
    hipLaunchKernelGGL(k_pins_fm<ADD>, dim3((unsigned)((h.P + 3) / 4), (unsigned)((n_sel + 63) / 64)), dim3(256), 0, ctx->stream, p, row_base, fj,
                       n_sel, out);
}

// the pins fit the tensor and the rows row_base + c fj, c < n_sel, lie inside shift
static int asb_pins_rows_ok(asb_ctx* ctx, const char* who, long long n, long long row_base, long long fj, long long n_sel) {
    const asb_ctx::Pins& h = ctx->pins;
    if (h.P < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no pins on the device (asb_pins_set)", who);
    if (h.n != n) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the pins were checked against %lld vertices, the tensor has %lld", who, (long long)h.n, n);
    if (h.T > 0 && (row_base < 0 || row_base + (n_sel - 1) * fj >= h.T))
        ASB_FAIL(ctx, ASB_ERR_ARG, "%s: row %lld of the shift is needed, it has %lld", who, row_base + (n_sel - 1) * fj, (long long)h.T);
    return ASB_OK;
}

static int asb_pd_pins_check(asb_ctx* ctx, const asb_pds* s, const char* who, long long step) {
    return asb_pins_rows_ok(ctx, who, s->n, s->pin_row0 + s->f0 + step, s->fj, s->n_sel);
}

extern "C" int asb_pins_clear(asb_ctx* ctx) {
    if (!ctx) return ASB_ERR_ARG;
    ctx->pins.P = ctx->pins.n = ctx->pins.T = 0;
    if (ctx->pds) ctx->pds->pins = false;
    return ASB_OK;
}

extern "C" int asb_pins_set(asb_ctx* ctx, int64_t P, const int64_t* verts, const double* wi, const double* p0, int64_t T_s, const double* shift,
                            int per_pin) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pins_clear(ctx);
    const int64_t n = ctx->n_loc;
    if (n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: no tensor on the device");
    if (P < 1 || P > n || T_s < 0 || (T_s > 0 && !shift) || !verts || !wi || !p0)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: %lld pins on %lld vertices, %lld rows of shift", (long long)P, (long long)n, (long long)T_s);
    std::vector<char> seen((size_t)n, 0);
    std::vector<int> v32((size_t)P);
    for (int64_t i = 0; i < P; ++i) {
        if (verts[i] < 0 || verts[i] >= n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: pin %lld names vertex %lld of %lld", (long long)i, (long long)verts[i], (long long)n);
        if (seen[verts[i]]) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: vertex %lld is pinned twice", (long long)verts[i]);
        seen[verts[i]] = 1, v32[i] = (int)verts[i];
        if (!std::isfinite(wi[i]) || wi[i] < 0.0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: wi[%lld] is not finite and >= 0", (long long)i);
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(p0[3 * i + d])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: the position of pin %lld is not finite", (long long)i);
    }
    const size_t n_shift = (size_t)T_s * (per_pin ? (size_t)P : 1) * 3;
    for (size_t k = 0; k < n_shift; ++k)
        if (!std::isfinite(shift[k])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_set: shift[%lld] is not finite", (long long)k);
    asb_ctx::Pins& h = ctx->pins;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    int rc;
    if ((rc = asb_alloc(ctx, &h.v, (size_t)P))) return rc;
    if ((rc = asb_alloc(ctx, &h.wi, (size_t)P))) return rc;
    if ((rc = asb_alloc(ctx, &h.p0, (size_t)3 * P))) return rc;
    if ((rc = asb_alloc(ctx, &h.shift, n_shift))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(h.v, v32.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(h.wi, wi, (size_t)P * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(h.p0, p0, (size_t)3 * P * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n_shift) ASB_HIP(ctx, hipMemcpyAsync(h.shift, shift, n_shift * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the host arrays may go
    h.P = P, h.n = n, h.T = T_s, h.per_pin = per_pin ? 1 : 0;
    return ASB_OK;
}

extern "C" int asb_pins_term(asb_ctx* ctx, int64_t f0, int64_t f1, int64_t fj, int64_t row0, int accumulate, double* out_dev) {
    if (!ctx || !out_dev) return ASB_ERR_ARG;
    if (fj < 1 || f0 < 0 || f1 <= f0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pins_term: empty frame range (%lld, %lld, %lld)", (long long)f0, (long long)f1, (long long)fj);
    const long long n_sel = (f1 - f0 + fj - 1) / fj;
    if ((n_sel + 63) / 64 > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_pins_term: %lld frames in one call (at most %d)", n_sel, 65535 * 64);
    int rc;
    if ((rc = asb_pins_rows_ok(ctx, "asb_pins_term", ctx->n_loc, row0 + f0, fj, n_sel))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if (accumulate) {
        asb_pins_launch<true>(ctx, row0 + f0, (int)fj, (int)n_sel, out_dev);
    } else {
        ASB_HIP(ctx, hipMemsetAsync(out_dev, 0, (size_t)n_sel * ctx->n_loc * 3 * sizeof(double), ctx->stream));
        asb_pins_launch<false>(ctx, row0 + f0, (int)fj, (int)n_sel, out_dev);
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// a[i] = fl(a[i] + b[i]) on two caller-owned device tensors of len doubles: k_pd_add, the add of an iteration
extern "C" int asb_fm_add(asb_ctx* ctx, double* a_dev, const double* b_dev, int64_t len) {
    if (!ctx || !a_dev || !b_dev || len < 1) return ASB_ERR_ARG;
    if (a_dev < b_dev + len && b_dev < a_dev + len) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_fm_add: the two tensors overlap");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    hipLaunchKernelGGL(k_pd_add, dim3((unsigned)std::min<long long>((len + 255) / 256, 1 << 20)), dim3(256), 0, ctx->stream, a_dev, b_dev, (long long)len);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

extern "C" int asb_pdsolve_pins(asb_ctx* ctx, int64_t row0) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_pins: no solve begun (asb_pdsolve_begin)");
    if (s->pins) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_pins: the solve has its pins already (their term is in the inertia term)");
    if (row0 < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_pins: row0 %lld", (long long)row0);
    if (ctx->n_loc != s->n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_pins: the tensor changed since asb_pdsolve_begin");
    s->pin_row0 = row0, s->pin_step = 0;
    int rc;
    if ((rc = asb_pd_pins_check(ctx, s, "asb_pdsolve_pins", 0))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_pins_launch<true>(ctx, row0 + s->f0, s->fj, (int)s->n_sel, s->ms);
    ASB_CHECK_LAUNCH(ctx);
    s->pins = true;
    return ASB_OK;
}

// ================================================================ external forces and the floor
// The start of the reference's step (Simulators.py:494-498): explicit = positions + dt velocities + dt^2 fext / mass, then
// resolve_collision on every vertex (Constraint_projections.py:1287-1298: a coordinate below the floor is set onto it); sn and
// the first iterate are both taken from the result.  The host forms fa = dt^2 force / mass without gravity (gravity stays in
// acc); the device holds fa as (T, 3 n) rows, or one row for a constant force.  Per entry (row r = 3 v + d, frame column c,
// table row rho(c) = row0 + f0 + c fj + step), after today's s = fl(fl(2 Q - P) + acc[d]):
//   x = fl(s + fa[rho(c)][r])                        (a table is held)
//   if (d == axis && x < height) x = height          (the floor is on; a comparison: NaN stays NaN, in its own frame)
//   Q <- x,  ms <- fl(diag[v] x)
// pd_ext_apply is the one place of the two lines; contraction is off, so the add is rounded on its own.  The iterations read ms
// and Q and are not changed; pins go onto ms afterwards.
// pd_ext_body: the tiling of k_pd_advance (a block owns 64 rows x 64 frames; wave w takes rows w, w + 4, .., lanes along the
// frames).  rho(c) differs per lane, so a direct read of fa would be a gather with a stride of fj 3 n doubles.  Instead the LDS
// tile is filled first, wave = frame, lanes along r: 512-byte runs of fa, entry (frame fl, row rl) at fl * 65 + rl -- the ms
// store in reverse.  After a barrier each thread reads its entry tile[lane * 65 + rl] and later overwrites THE SAME address
// with diag x: same thread, same slot, no further barrier before the one k_pd_advance has, and no LDS beyond its 33 280 bytes.
// A constant force (FORCE 1) is a broadcast load of fa[r] per wave and needs no fill.  Tail predicates as k_pd_advance: rows >=
// 3 n and frames >= n_sel neither read nor write; the padding columns of Q and P are never written.  No atomics.
// ADV: the fused advance (reads Q and P; writes P, Q, ms).  Otherwise the correction: reads S, which holds s (Q itself, or a
// scratch tensor when the iterate is not the explicit state), writes Qw (NULL: the iterate is left alone) and ms.
template <int FORCE, bool FLOOR>
__device__ __forceinline__ double pd_ext_apply(double x, double f, int d, int axis, double height) {
#pragma clang fp contract(off)
    if (FORCE) x = x + f;
    if (FLOOR && d == axis && x < height) x = height;
    return x;
}

struct PdExt {
    const double* fa;           // FORCE 1: (rows); 2: the table's row 0
    long long row_base;         // FORCE 2: frame column c reads row row_base + c fj
    int fj, axis;
    double height;
};

template <int FORCE, bool FLOOR, bool ADV>
__device__ __forceinline__ void pd_ext_body(double* tile, const double* S, double* Qw, double* P, const double* __restrict__ diag, int n_sel,
                                            long long rows, long long ld, double acc0, double acc1, double acc2, const PdExt& e,
                                            double* __restrict__ ms) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64;
    const int t0 = (int)blockIdx.y * 64;
    if (FORCE == 2) {
        for (int fl = wv; fl < 64; fl += 4)
            if (t0 + fl < n_sel && r0 + lane < rows)
                tile[fl * PD_LDQ + lane] = e.fa[(e.row_base + (long long)(t0 + fl) * e.fj) * rows + r0 + lane];
        __syncthreads();
    }
    for (int rl = wv; rl < 64; rl += 4) {
        const long long r = r0 + rl;
        if (r < rows && t0 + lane < n_sel) {
            const long long at = r * ld + t0 + lane;
            const int d = (int)(r % 3);
            double x;
            if (ADV) {
                const double q = S[at];
                x = 2.0 * q - P[at];
                x = x + (d == 0 ? acc0 : (d == 1 ? acc1 : acc2));
                P[at] = q;
            } else {
                x = S[at];
            }
            const double f = FORCE == 2 ? tile[lane * PD_LDQ + rl] : (FORCE == 1 ? e.fa[r] : 0.0);
            x = pd_ext_apply<FORCE, FLOOR>(x, f, d, e.axis, e.height);
            if (Qw) Qw[at] = x;
            tile[lane * PD_LDQ + rl] = diag[r / 3] * x;
        }
    }
    __syncthreads();
    for (int fl = wv; fl < 64; fl += 4)
        if (t0 + fl < n_sel && r0 + lane < rows) ms[(long long)(t0 + fl) * rows + r0 + lane] = tile[fl * PD_LDQ + lane];
}

// grid (row tiles of 64, frame tiles of 64): k_pd_advance with the force and the floor in the same pass
template <int FORCE, bool FLOOR>
__global__ __launch_bounds__(256) void k_pd_advance_ext(double* Q, double* P, const double* __restrict__ diag, int n_sel, long long rows,
                                                        long long ld, double acc0, double acc1, double acc2, PdExt e,
                                                        double* __restrict__ ms) {
    __shared__ double tile[64 * PD_LDQ];
    pd_ext_body<FORCE, FLOOR, true>(tile, Q, Q, P, diag, n_sel, rows, ld, acc0, acc1, acc2, e, ms);
}

// grid as above: the correction of a state that holds s already (S; S == Qw, or Qw NULL)
template <int FORCE, bool FLOOR>
__global__ __launch_bounds__(256) void k_pd_external(const double* S, double* Qw, const double* __restrict__ diag, int n_sel, long long rows,
                                                     long long ld, PdExt e, double* __restrict__ ms) {
    __shared__ double tile[64 * PD_LDQ];
    pd_ext_body<FORCE, FLOOR, false>(tile, S, Qw, nullptr, diag, n_sel, rows, ld, 0.0, 0.0, 0.0, e, ms);
}

static PdExt pd_ext_dev(const asb_ctx* ctx, const asb_pds* s, long long step) {
    const asb_ctx::Ext& h = ctx->ext;
    return PdExt{h.fa, s->ext_row0 + s->f0 + step, s->fj, h.axis, h.height};
}

// the forces and the floor fit the solve, and step `step` finds its rows in the table
static int asb_pd_ext_check(asb_ctx* ctx, const asb_pds* s, const char* who, long long row0, long long step) {
    const asb_ctx::Ext& h = ctx->ext;
    if (h.n < 1 || (!h.force && !h.floor)) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no forces and no floor on the device (asb_ext_set)", who);
    if (h.n != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the forces were checked against %lld vertices, the solve has %lld", who, (long long)h.n, s->n);
    const long long last = row0 + s->f0 + step + (s->n_sel - 1) * s->fj;
    if (h.force && h.T > 0 && last >= h.T) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: row %lld of the force table is needed, it has %lld", who, last, (long long)h.T);
    return ASB_OK;
}

extern "C" int asb_ext_clear(asb_ctx* ctx) {
    if (!ctx) return ASB_ERR_ARG;
    ctx->ext.n = ctx->ext.T = 0;
    ctx->ext.force = ctx->ext.floor = 0;
    if (ctx->pds) ctx->pds->ext = false;
    return ASB_OK;
}

extern "C" int asb_ext_set(asb_ctx* ctx, int64_t T_s, const double* table_host, int floor_on, int axis, double height) {
    if (!ctx) return ASB_ERR_ARG;
    asb_ext_clear(ctx);
    const int64_t n = ctx->n_loc;
    if (n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_ext_set: no tensor on the device");
    if (T_s < 0 || (T_s > 0 && !table_host)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_ext_set: %lld rows of a table that is %s", (long long)T_s, table_host ? "given" : "missing");
    if (!table_host && !floor_on) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_ext_set: neither a force table nor a floor");
    if (floor_on && (axis < 0 || axis > 2 || !std::isfinite(height)))
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_ext_set: floor along axis %d at height %g (an axis 0..2, a finite height)", axis, height);
    const size_t len = table_host ? (size_t)(T_s > 0 ? T_s : 1) * 3 * (size_t)n : 0;
    if (len > ((size_t)1 << 31) / sizeof(double))
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_ext_set: a force table of %lld x %lld doubles, %.3g GiB (at most 2 GiB)", (long long)(T_s > 0 ? T_s : 1), (long long)(3 * n),
                 (double)len * sizeof(double) / 1073741824.0);
    for (size_t k = 0; k < len; ++k)
        if (!std::isfinite(table_host[k])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_ext_set: entry %lld of the force table is not finite", (long long)k);
    asb_ctx::Ext& h = ctx->ext;
    if (len) {
        ASB_HIP(ctx, hipSetDevice(ctx->dev));
        int rc;
        if ((rc = asb_alloc(ctx, &h.fa, len))) return rc;
        ASB_HIP(ctx, hipMemcpyAsync(h.fa, table_host, len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the host array may go
    }
    h.n = n, h.T = table_host ? T_s : 0, h.force = table_host ? 1 : 0;
    h.floor = floor_on ? 1 : 0, h.axis = floor_on ? axis : 1, h.height = floor_on ? height : 0.0;
    return ASB_OK;
}

template <int FORCE, bool FLOOR>
static void pd_external_launch(asb_ctx* ctx, asb_pds* s, const double* S, double* Qw, const PdExt& e) {
    const dim3 grid((unsigned)((3 * s->n + 63) / 64), (unsigned)((s->n_sel + 63) / 64));
    hipLaunchKernelGGL((k_pd_external<FORCE, FLOOR>), grid, dim3(256), 0, ctx->stream, S, Qw, s->diag, (int)s->n_sel, 3 * s->n, s->ld, e, s->ms);
}

template <int FORCE, bool FLOOR>
static void pd_advance_ext_launch(asb_ctx* ctx, asb_pds* s, const PdExt& e) {
    const dim3 grid((unsigned)((3 * s->n + 63) / 64), (unsigned)((s->n_sel + 63) / 64));
    hipLaunchKernelGGL((k_pd_advance_ext<FORCE, FLOOR>), grid, dim3(256), 0, ctx->stream, s->Q, s->P, s->diag, (int)s->n_sel, 3 * s->n, s->ld,
                       s->acc[0], s->acc[1], s->acc[2], e, s->ms);
}

extern "C" int asb_pdsolve_external(asb_ctx* ctx, int64_t row0) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_external: no solve begun (asb_pdsolve_begin)");
    if (s->pins)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_external: the solve has its pins already: this call rewrites the inertia term and their term would be lost "
                                   "(asb_pdsolve_external before asb_pdsolve_pins)");
    if (s->ext) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_external: the solve has its forces and floor already");
    if (row0 < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_external: row0 %lld", (long long)row0);
    int rc;
    if ((rc = asb_pd_ext_check(ctx, s, "asb_pdsolve_external", row0, 0))) return rc;      // before any launch, the solve untouched
    s->ext_row0 = row0, s->ext_step = 0;
    if (!s->q_is_s && s->w.T != ctx->X && s->w.T != ctx->ho_Y)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_external: the tensor changed since asb_pdsolve_begin");
    const long long n = s->n, n_sel = s->n_sel, ld = s->ld;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if (!s->carry) {                                // the solve's own copy of diag, as asb_pdsolve_carry makes it
        if ((rc = asb_alloc(ctx, &s->diag, (size_t)n))) return rc;
        ASB_HIP(ctx, hipMemcpyAsync(s->diag, s->diag_host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    const double* S = s->Q;
    double* Qw = s->Q;
    if (!s->q_is_s) {
        // the iterate is x_f or the caller's tensor, not s: s is formed as k_pd_init(start 0) forms it, into the buffer of c
        // (asb_hyper_iterate rewrites c from ms in every call), and the iterate is left alone
        if ((rc = asb_alloc(ctx, &s->c, (size_t)3 * n * ld))) return rc;
        hipLaunchKernelGGL(k_pd_init, dim3((unsigned)((3 * n + 3) / 4), (unsigned)((n_sel + 63) / 64)), dim3(256), 0, ctx->stream, s->w, s->f0, s->fj,
                           (int)n_sel, n, 0, s->mode, s->acc[0], s->acc[1], s->acc[2], s->c, ld);
        S = s->c, Qw = nullptr;
    }
    const PdExt e = pd_ext_dev(ctx, s, 0);
    const asb_ctx::Ext& h = ctx->ext;
    const int force = h.force ? (h.T > 0 ? 2 : 1) : 0;
    if (h.floor) {
        if (force == 2) pd_external_launch<2, true>(ctx, s, S, Qw, e);
        else if (force == 1) pd_external_launch<1, true>(ctx, s, S, Qw, e);
        else pd_external_launch<0, true>(ctx, s, S, Qw, e);
    } else {
        if (force == 2) pd_external_launch<2, false>(ctx, s, S, Qw, e);
        else pd_external_launch<1, false>(ctx, s, S, Qw, e);
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (diag_host was read)
    s->ext = true;
    return ASB_OK;
}

extern "C" int asb_pdsolve_carry(asb_ctx* ctx, const double* pos_dev) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_carry: no solve begun (asb_pdsolve_begin)");
    s->carry = false;
    if (ctx->n_loc != s->n || (!pos_dev && s->w.T != ctx->X && s->w.T != ctx->ho_Y))
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_carry: the tensor changed since asb_pdsolve_begin");
    const long long n = s->n, n_sel = s->n_sel, ld = s->ld;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    int rc;
    if ((rc = asb_alloc(ctx, &s->P, (size_t)3 * n * ld))) return rc;
    if ((rc = asb_alloc(ctx, &s->diag, (size_t)n))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(s->diag, s->diag_host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(s->P, 0, (size_t)3 * n * ld * sizeof(double), ctx->stream));      // the padding columns, once per carry
    const unsigned gt = (unsigned)((n_sel + 63) / 64);
    if (pos_dev)
        hipLaunchKernelGGL(k_pd_transpose, dim3((unsigned)((3 * n + 63) / 64), gt), dim3(256), 0, ctx->stream, pos_dev, (int)n_sel,
                           (long long)(3 * n), s->P, ld);
    else
        hipLaunchKernelGGL(k_pd_init, dim3((unsigned)((3 * n + 3) / 4), gt), dim3(256), 0, ctx->stream, s->w, s->f0, s->fj, (int)n_sel,
                           (long long)n, 1, 0, 0.0, 0.0, 0.0, s->P, ld);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller's tensor may go
    s->carry = true;
    return ASB_OK;
}

extern "C" int asb_pdsolve_advance(asb_ctx* ctx) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_advance: no solve begun (asb_pdsolve_begin)");
    if (!s->carry || !s->P || !s->diag)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_advance: the solve carries no previous positions (asb_pdsolve_carry after asb_pdsolve_begin)");
    int rc;
    if (s->pins && (rc = asb_pd_pins_check(ctx, s, "asb_pdsolve_advance", s->pin_step + 1))) return rc;       // before any launch
    if (s->ext && (rc = asb_pd_ext_check(ctx, s, "asb_pdsolve_advance", s->ext_row0, s->ext_step + 1))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const dim3 grid((unsigned)((3 * s->n + 63) / 64), (unsigned)((s->n_sel + 63) / 64));
    if (s->ext) {                                   // the same pass with the force and the floor of the next step in it
        const PdExt e = pd_ext_dev(ctx, s, ++s->ext_step);
        const asb_ctx::Ext& h = ctx->ext;
        const int force = h.force ? (h.T > 0 ? 2 : 1) : 0;
        if (h.floor) {
            if (force == 2) pd_advance_ext_launch<2, true>(ctx, s, e);
            else if (force == 1) pd_advance_ext_launch<1, true>(ctx, s, e);
            else pd_advance_ext_launch<0, true>(ctx, s, e);
        } else {
            if (force == 2) pd_advance_ext_launch<2, false>(ctx, s, e);
            else pd_advance_ext_launch<1, false>(ctx, s, e);
        }
    } else {
        hipLaunchKernelGGL(k_pd_advance, grid, dim3(256), 0, ctx->stream, s->Q, s->P, s->diag, (int)s->n_sel, 3 * s->n, s->ld, s->acc[0], s->acc[1],
                           s->acc[2], s->ms);
    }
    s->q_is_s = true;
    if (s->pins) {                                  // ms of the next step is rewritten: its pin term, one row of shift later
        ++s->pin_step;
        asb_pins_launch<true>(ctx, s->pin_row0 + s->f0 + s->pin_step, s->fj, (int)s->n_sel, s->ms);
    }
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

extern "C" int asb_pdsolve_positions(asb_ctx* ctx, double* out_dev) {
    if (!ctx || !out_dev) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_positions: no solve begun (asb_pdsolve_begin)");
    if (!s->carry || !s->P)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_pdsolve_positions: the solve carries no previous positions (asb_pdsolve_carry after asb_pdsolve_begin)");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const dim3 grid((unsigned)((3 * s->n + 63) / 64), (unsigned)((s->n_sel + 63) / 64));
    hipLaunchKernelGGL(k_pd_untranspose, grid, dim3(256), 0, ctx->stream, s->P, (int)s->n_sel, 3 * s->n, s->ld, out_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// test hook: the iterate Q (which 0) or the carried positions P (1) as they lie on the device, (3 n, ld) with the padding
extern "C" int asb_test_pdsolve_state(asb_ctx* ctx, int which, double* out_host, int64_t rows, int64_t ld) {
    if (!ctx || !out_host) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun || (which != 0 && which != 1) || (which == 1 && (!s->carry || !s->P)))
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_pdsolve_state: no such state (0: the iterate of a begun solve, 1: the positions of a carry)");
    if (rows != 3 * s->n || ld != s->ld)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_pdsolve_state: the state is (%lld, %lld), not (%lld, %lld)", 3 * s->n, s->ld, (long long)rows, (long long)ld);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    ASB_HIP(ctx, hipMemcpyAsync(out_host, which ? s->P : s->Q, (size_t)rows * ld * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

// ================================================================ hyper-reduced iterations
// When every kind of the solve is reduced (each on its own bank of asb_rforce_bank), an iteration is affine in the coefficients:
// per coordinate d
//   q_{k+1} = c + sum_s G_{s,d} coef_{s,d}(q_k),   c = A^-1 ms (once per solve),   G_{s,d} = A^-1 M_{s,d} (N x mp_s, once per matrix and basis),
// and coef(q_k) reads q_k at the vertices of the sampled elements only -- the TOUCHED vertices, the union over the kinds.  Iterations 1 .. K-1 therefore
// run on the touched rows of c, G and q (compact buffers of N_t vertices, the element tables renumbered by the host); only
// the last iteration expands to all N rows.  No N^2 product is left in the loop.
//
//   asb_hyper_operator    k_hy_operator: Gt_d[j][m] = sum_n A^-1[n][m] M_d[n][j], one thread per (m, 8 values of j), n ascending,
//                         one FMA accumulator per entry, never split.  Stored in the current bank (RfBank::G) like its M, (3, mpp, Np),
//                         zero padding.  Marked valid (RfBank::ok); asb_gstep_setup / asb_gslab_setup clear the mark of every bank, asb_rforce_operator that of
//                         its own, and a stale G is refused.
//   asb_hyper_iterate     c by ONE launch of k_pdsolve_gemm<false, false> on ms (gs_contract, vertex-major epilogue) into a buffer
//                         shaped like Q.  touched given: k_hy_gather_rows copies the touched rows of Q and c, k_hy_gather_cols
//                         the touched columns of every bank's Gt.  Then per iteration and chunk of frames 2 S + 1 launches for S
//                         kinds: per kind k_cproj_em on the (compact) iterate and k_rforce_coef into its bank's coefficients --
//                         ALL of them from the old iterate -- and then ONE k_hyper_apply, which alone writes the iterate (a
//                         Jacobi update over the kinds, as the reference's; kind-by-kind applies would be Gauss-Seidel).  No
//                         host-to-device copy, no synchronisation in the loop.
//   k_hyper_apply         Q'[3 v + d][f] = fl(c[3 v + d][f] + acc), acc from 0 over the segments (kinds) in slot order and inside
//                         a segment over j = 0 .. rpp in order, acc += G_d[v][j] coef_d[j][f]; the segments come as a by-value
//                         table {Gt, coef, mpp, rpp} x 8 with a count (200 bytes of kernel arguments, read by scalar loads): v_mfma_f64_16x16x4_f64 with A = G (vertices x j) and B = coef (j x frames), the roles of
//                         k_rforce_gemm swapped, so that an accumulator row is a vertex and its 16 lanes run along 16 contiguous
//                         frames.  A block of 4 waves owns 32 vertices x 64 frames x 3 coordinates (wave w: frames 16 w ..).
//                         The vertex-major store is DIRECT, no LDS: a store instruction of a wave writes four 128-byte runs (16
//                         frames of rows g, g + 4, ..), each a whole aligned cache line of Q -- staging could only widen the
//                         runs to 512 bytes at the price of a barrier and 24 KB of LDS.  c is read with the same addresses.
//                         FM (the last iteration): the same values fl(c + acc) are also staged frame-major in LDS, rows of 97
//                         doubles (the 16 lanes of a ds_write_b64 pass sit 97 doubles apart: odd, 16 different bank pairs),
//                         and written per frame as its contiguous run of 96 doubles, as gs_store_fm does.
//                         Tail predicates: vertices >= nv, frames >= cn of the chunk; the padding columns of Q are never
//                         written.  An entry's value does not depend on the tile, chunk or row set it falls in: "touched" and
//                         "all" give the same bits.  No atomics.
#define HY_TF 64
#define HY_TN 32
#define HY_JB 8

// grid (blocks of 256 over n, mp / HY_JB, 3)
__global__ __launch_bounds__(256) void k_hy_operator(const double* __restrict__ Ainv, int n, int np, const double* __restrict__ Mt,
                                                     long long Np, int mp, int mpp, double* __restrict__ Gt) {
    const int m = (int)blockIdx.x * 256 + threadIdx.x;
    const int j0 = (int)blockIdx.y * HY_JB, d = blockIdx.z;
    if (m >= n) return;
    const double* row = Mt + ((long long)d * mpp + j0) * Np;
    double a[HY_JB];
#pragma unroll
    for (int q = 0; q < HY_JB; ++q) a[q] = 0.0;
    for (int k = 0; k < n; ++k) {                 // ascending n, one accumulator per entry
        const double x = Ainv[(long long)k * np + m];
#pragma unroll
        for (int q = 0; q < HY_JB; ++q)
            if (j0 + q < mp) a[q] = fma(x, row[q * Np + k], a[q]);
    }
#pragma unroll
    for (int q = 0; q < HY_JB; ++q)
        if (j0 + q < mp) Gt[((long long)d * mpp + j0 + q) * Np + m] = a[q];
}

// grid (3 nt, ld / 64), one wave: row 3 tv[t] + d of src (ld doubles, the padding included) -> row 3 t + d of dst
__global__ __launch_bounds__(64) void k_hy_gather_rows(const double* __restrict__ src, const int* __restrict__ tv, long long ld,
                                                       double* __restrict__ dst) {
    const long long r = blockIdx.x, col = (long long)blockIdx.y * 64 + threadIdx.x;
    dst[r * ld + col] = src[(3LL * tv[r / 3] + r % 3) * ld + col];
}

// grid (rows, blocks of 64 over ntp), one wave: column tv[t] of src (rows x Np) -> column t of dst (rows x ntp), 0 for t >= nt
__global__ __launch_bounds__(64) void k_hy_gather_cols(const double* __restrict__ src, long long Np, const int* __restrict__ tv, int nt, int ntp,
                                                       double* __restrict__ dst) {
    const long long r = blockIdx.x;
    const int t = (int)blockIdx.y * 64 + threadIdx.x;
    if (t < ntp) dst[r * ntp + t] = t < nt ? src[r * Np + tv[t]] : 0.0;
}

// One term of the affine form: Gt (3, mpp, ldg) of a bank, zero past nv; coef (3, rpp, cw) of that bank, zero past row r and frame cn
#define HY_MAX_SEG PD_MAX_SLOTS
struct HySeg {
    const double *Gt, *coef;
    int mpp, rpp;
};
struct HySegs {
    HySeg s[HY_MAX_SEG];
    int n;
};

// grid (ldg / HY_TN covering nv, frame tiles of the chunk).  ldg (shared by the segments) a multiple of HY_TN; cw (shared) a
// multiple of HY_TF; c, Q (3 nv, ld); out (n_sel, nv, 3) with FM.  The segments run in slot order, j ascending inside each, as ONE
// chain of MFMAs per accumulator from 0; then Q' = fl(c + acc).  One segment: the instruction order of the single-kind kernel.
template <bool FM>
__global__ __launch_bounds__(256) void k_hyper_apply(const HySegs segs, long long ldg, int cw, const double* __restrict__ c,
                                                     double* __restrict__ Q, long long ld, int c0, int cn, int nv, double* __restrict__ out) {
    constexpr int RUN = HY_TN * 3, ROW = RUN + 1;
    __shared__ double stage[FM ? HY_TF * ROW : 1];
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int v0 = (int)blockIdx.x * HY_TN;
    const int t0 = (int)blockIdx.y * HY_TF;
    d4 acc[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[d][y] = d4{0.0, 0.0, 0.0, 0.0};
    for (int sg = 0; sg < segs.n; ++sg) {
        const int mpp = segs.s[sg].mpp, rpp = segs.s[sg].rpp;
        const double* pa = segs.s[sg].Gt + v0 + i;                    // A: vertex i of 16, k = g
        const double* pb = segs.s[sg].coef + t0 + wave * 16 + i;      // B: k = g, frame i of the wave's 16
        for (int k0 = 0; k0 < rpp; k0 += 4) {
            const int k = k0 + g;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double* a = pa + ((long long)d * mpp + k) * ldg;
                const double b = pb[((long long)d * rpp + k) * cw];
                acc[d][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b, acc[d][0], 0, 0, 0);
                acc[d][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[16], b, acc[d][1], 0, 0, 0);
            }
        }
    }
    // accumulator q of lane (i, g): vertex g + 4 q of the 16, frame i of the wave's 16
    const int fl = wave * 16 + i;
    const bool fok = t0 + fl < cn;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int vl = 16 * y + g + 4 * q;
                double val = 0.0;
                if (fok && v0 + vl < nv) {
                    const long long at = (3LL * (v0 + vl) + d) * ld + c0 + t0 + fl;
                    val = c[at] + acc[d][y][q];
                    Q[at] = val;
                }
                if (FM) stage[fl * ROW + vl * 3 + d] = val;
            }
    if (FM) {
        __syncthreads();
        const int nvt = nv - v0 < HY_TN ? nv - v0 : HY_TN;
        const int nf = cn - t0 < HY_TF ? cn - t0 : HY_TF;
        const int run = nvt * 3;
        for (int e = threadIdx.x; e < HY_TF * RUN; e += 256) {
            const int f = e / RUN, k = e % RUN;
            if (f < nf && k < run) out[((long long)(c0 + t0 + f) * nv + v0) * 3 + k] = stage[f * ROW + k];
        }
    }
}

extern "C" int asb_hyper_operator(asb_ctx* ctx) {
    if (!ctx) return ASB_ERR_ARG;
    asb_ctx::RfBank& b = asb_rf_cur(ctx);
    b.ok = 0;
    const long long ns = pd_solver_n(ctx);
    if (ns < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_operator: no inverse on the device (asb_gstep_setup)");
    if (b.mp < 1 || !b.M) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_operator: no operator S^T V on the device (asb_rforce_operator)");
    if (b.n != ns || ns != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_operator: the inverse has %lld rows, S^T V %lld, the tensor %lld vertices", ns,
                 (long long)b.n, (long long)ctx->n_loc);
    const long long jb = (b.mp + HY_JB - 1) / HY_JB;
    if (jb > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_hyper_operator: %lld basis vectors (at most %d)", (long long)b.mp, 65535 * HY_JB);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const size_t len = (size_t)3 * b.mpp * b.Np;
    int rc;
    if ((rc = asb_alloc(ctx, &b.G, len))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(b.G, 0, len * sizeof(double), ctx->stream));
    if (asb_gsub_n(ctx) > 0) {                      // the position subspace: G = P S^T V, the linear part of its map
        if ((rc = asb_gsub_solve_rows(ctx, b.M, 3 * b.mpp, b.Np, b.G))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        b.ok = 1;
        return ASB_OK;
    }
    if (asb_gslab_n(ctx) > 0) {                     // the slab factor: the 3 mpp rows of M are the columns of one sweep
        if ((rc = asb_gslab_solve_rows(ctx, b.M, 3 * b.mpp, b.Np, b.G))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        b.ok = 1;
        return ASB_OK;
    }
    hipLaunchKernelGGL(k_hy_operator, dim3((unsigned)((ctx->gs_n + 255) / 256), (unsigned)jb, 3), dim3(256), 0, ctx->stream, ctx->gs_Ainv,
                       (int)ctx->gs_n, (int)ctx->gs_Np, b.M, (long long)b.Np, (int)b.mp, (int)b.mpp, b.G);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    b.ok = 1;
    return ASB_OK;
}

extern "C" int asb_hyper_iterate(asb_ctx* ctx, int64_t n_iter, int64_t n_touched, const int64_t* touched, int64_t chunk_frames,
                                 double* out_dev) {
    if (!ctx) return ASB_ERR_ARG;
    asb_pds* s = ctx->pds;
    if (!s || !s->begun || s->n_slots < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: no solve begun or no kind registered (asb_pdsolve_begin, asb_pdsolve_slot)");
    for (int k = 0; k < s->n_slots; ++k)
        if (!s->slot[k].reduced)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: %d kinds, kind %d not reduced: every kind must be reduced, each on a bank of its own "
                                       "(asb_rforce_bank)", s->n_slots, k);
    if (n_iter < 1 || n_iter > (1 << 20)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: %lld iterations", (long long)n_iter);
    if (chunk_frames < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: chunk_frames %lld", (long long)chunk_frames);
    if (pd_solver_n(ctx) != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: the inverse or the tensor changed since asb_pdsolve_begin");
    const int ns = s->n_slots;
    asb_ctx::RfBank* bank[PD_MAX_SLOTS] = {};       // the slots' banks, where they live
    for (int k = 0; k < ns; ++k) {
        bank[k] = &ctx->rf_bank[s->slot[k].bank];
        if (bank[k]->mp < 1 || bank[k]->r < 1 || bank[k]->n != s->n || bank[k]->pt_max >= s->slot[k].n_cols)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: the operator or solver changed since asb_pdsolve_slot");
        if (!bank[k]->ok || !bank[k]->G)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: no operator A^-1 S^T V for the inverse and the basis on the device (asb_hyper_operator "
                                       "after asb_gstep_setup and asb_rforce_operator): a stale one is refused");
    }
    const long long n = s->n, n_sel = s->n_sel, ld = s->ld;
    const bool compact = touched != nullptr;
    const long long nt = compact ? n_touched : n;
    if (compact) {
        if (nt < 1 || nt > n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: %lld touched vertices of %lld", (long long)nt, n);
        for (long long t = 0; t < nt; ++t)
            if (touched[t] < 0 || touched[t] >= n || (t > 0 && touched[t] <= touched[t - 1]))
                ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: touched[%lld] = %lld: ascending vertices of 0..%lld", t, (long long)touched[t], n - 1);
    }
    for (int k = 0; k < ns; ++k)
        if (s->slot[k].cp.vmax >= nt)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_hyper_iterate: the element set-up names vertex %lld, the iterate has %lld rows",
                     (long long)s->slot[k].cp.vmax, nt);
    // one chunk width for all slots: the smallest of the banks'
    long long cw = 0, cols_max = 0;
    for (int k = 0; k < ns; ++k) {
        const long long w = asb_rforce_chunk_width(bank[k]->r, s->slot[k].n_cols, n_sel);
        cw = k == 0 ? w : std::min(cw, w);
        cols_max = std::max(cols_max, s->slot[k].n_cols);
    }
    if (chunk_frames > 0) cw = std::min<long long>(cw, (chunk_frames + HY_TF - 1) / HY_TF * HY_TF);
    const long long ntp = (nt + HY_TN - 1) / HY_TN * HY_TN;
    const long long Np = bank[0]->Np;                // (every bank's operator has the n vertices of the solve: one padding)
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_scratch, (size_t)3 * cols_max * cw))) return rc;
    for (int k = 0; k < ns; ++k) {                  // per bank: the coefficients of one chunk, the touched columns of G^T
        if ((rc = asb_alloc(ctx, &bank[k]->coef, (size_t)3 * (((size_t)bank[k]->r + 3) / 4 * 4) * cw))) return rc;
        if (compact && (rc = asb_alloc(ctx, &bank[k]->Gc, (size_t)3 * bank[k]->mpp * ntp))) return rc;
    }
    if ((rc = asb_alloc(ctx, &s->c, (size_t)3 * n * ld))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(s->c, 0, (size_t)3 * n * ld * sizeof(double), ctx->stream));
    if (asb_gsub_n(ctx) > 0) {                      // c = o' + P ms through the position subspace
        if ((rc = asb_gsub_solve_fm(ctx, s->ms, n_sel, s->c, nullptr))) return rc;
    } else if (asb_gslab_n(ctx) > 0) {              // c through the slab factor: in -> sweep -> rows
        if ((rc = asb_gslab_solve_fm(ctx, s->ms, n_sel, s->c, nullptr))) return rc;
    } else {
        hipLaunchKernelGGL((k_pdsolve_gemm<false, false>), dim3((unsigned)(ctx->gs_Np / GS_TN), (unsigned)((n_sel + GS_TF - 1) / GS_TF)), dim3(256), 0,
                           ctx->stream, s->ms, ctx->gs_Ainv, (int)n, (int)ctx->gs_Np, n_sel, s->c, ld, nullptr, nullptr);
    }
    asb_tmp<int> tv;
    double *Qi = s->Q, *ci = s->c;                  // what iterations 1 .. K-1 run on
    HySegs full = {}, part = {};                    // the segments of the last iteration (all rows) and of the others
    full.n = part.n = ns;
    for (int k = 0; k < ns; ++k) {
        const int rpp = ((int)bank[k]->r + 3) / 4 * 4;
        full.s[k] = HySeg{bank[k]->G, bank[k]->coef, (int)bank[k]->mpp, rpp};
        part.s[k] = full.s[k];
    }
    long long ldg = Np;
    if (compact) {
        std::vector<int> t32((size_t)nt);
        for (long long t = 0; t < nt; ++t) t32[t] = (int)touched[t];
        if ((rc = tv.alloc(ctx, (size_t)nt))) return rc;
        if ((rc = asb_alloc(ctx, &s->Qc, (size_t)3 * nt * ld))) return rc;
        if ((rc = asb_alloc(ctx, &s->cc, (size_t)3 * nt * ld))) return rc;
        ASB_HIP(ctx, hipMemcpyAsync(tv.get(), t32.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        const dim3 gr((unsigned)(3 * nt), (unsigned)(ld / 64));
        hipLaunchKernelGGL(k_hy_gather_rows, gr, dim3(64), 0, ctx->stream, s->Q, tv.get(), ld, s->Qc);
        hipLaunchKernelGGL(k_hy_gather_rows, gr, dim3(64), 0, ctx->stream, s->c, tv.get(), ld, s->cc);
        for (int k = 0; k < ns; ++k) {              // the columns of G^T per bank
            hipLaunchKernelGGL(k_hy_gather_cols, dim3((unsigned)(3 * bank[k]->mpp), (unsigned)((ntp + 63) / 64)), dim3(64), 0, ctx->stream, bank[k]->G, Np,
                               tv.get(), (int)nt, (int)ntp, bank[k]->Gc);
            part.s[k].Gt = bank[k]->Gc;
        }
        ASB_CHECK_LAUNCH(ctx);
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the staging vector dies here, before the loop)
        Qi = s->Qc, ci = s->cc, ldg = ntp;
    }
    const CpWorld wq = {Qi, ld, nullptr, nullptr, 1.0};
    for (int64_t it = 0; it < n_iter; ++it) {
        const bool last = it == n_iter - 1;
        for (long long c0 = 0; c0 < n_sel; c0 += cw) {
            const int cn = (int)(c0 + cw < n_sel ? cw : n_sel - c0);
            // ALL coefficients from the old iterate first (the element-major scratch is reused in stream order), then one
            // launch writes the new iterate: applying kind by kind would make the Jacobi update a Gauss-Seidel one
            for (int k = 0; k < ns; ++k) {
                const PdSlot& p = s->slot[k];
                asb_cproj_em_launch(ctx, p.cp, wq, 0, 1, (int)c0, cn, (int)cw, p.smin, p.smax, ctx->cf_scratch);
                asb_rforce_coef_launch(ctx, *bank[k], ctx->cf_scratch, (int)cw, cn);
            }
            const unsigned gy = (unsigned)((cn + HY_TF - 1) / HY_TF);
            if (!last)
                hipLaunchKernelGGL((k_hyper_apply<false>), dim3((unsigned)(ntp / HY_TN), gy), dim3(256), 0, ctx->stream, part, ldg, (int)cw, ci, Qi, ld,
                                   (int)c0, cn, (int)nt, nullptr);
            else if (out_dev)
                hipLaunchKernelGGL((k_hyper_apply<true>), dim3((unsigned)(Np / HY_TN), gy), dim3(256), 0, ctx->stream, full, Np, (int)cw, s->c, s->Q, ld,
                                   (int)c0, cn, (int)n, out_dev);
            else
                hipLaunchKernelGGL((k_hyper_apply<false>), dim3((unsigned)(Np / HY_TN), gy), dim3(256), 0, ctx->stream, full, Np, (int)cw, s->c, s->Q, ld,
                                   (int)c0, cn, (int)n, nullptr);
        }
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}
