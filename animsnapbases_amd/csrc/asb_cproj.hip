// Constraint-projection snapshots from the resident position tensor: per element and frame the projection `get_pi` of the
// reference's five element constraints (projective_dynamics/Constraint_projections.py: edge spring :291-312, triangle strain
// :407-426, tetrahedron strain :534-554, tetrahedron deformation gradient :669-687, vertex bending :197-215), written as the
// (F', n_elem p, 3) tensor that Simulators.py:655-724 stacks, without the simulator's Python loop over elements and frames.
//
// World space as in asb_onmesh.hip: x = (T * (1 / psf) + mean) * (1 / massL_v), same arguments, same reciprocals.
//
// Reads: the tensor is vertex-major (row 3 v + d, frames contiguous), so lanes run along the selected frames.  A wave owns one
// element x 64 frames: the element's indices and table are the same in every lane (scalar loads), each of its 2 - 4 vertices'
// rows is a coalesced 512-byte load (frame_jump 1).  Writes: the output is frame-major, so a block of CP_EB elements x 64
// frames stages its p x 3 results in LDS, one row of CP_EB * 3p + 1 doubles per frame (the odd row length spreads the 64 lanes
// of a column store over all banks), and then writes per frame the block's contiguous run of elements x 3p doubles.
//
// SVD and "project F": asb_cproj_elem.h (host and device).  A kernel forms F from the world positions and calls
// cp_project_tri / cp_project_tet on it; every result is a function of F.  A (frame, element) is computed by one thread from
// its own loads only and nothing is accumulated across threads: no atomics, repeated calls and sub-ranges of frames are
// bit-identical.
#include "asb_common.h"
#include "asb_cproj_elem.h"

#include <vector>

#define CP_EB 16            // elements per block
#define CP_WAVES 4

template <int KIND> struct CpShape;
template <> struct CpShape<CP_EDGE> { static constexpr int NV = 2, P = 1, TW = 1; };
template <> struct CpShape<CP_TRI> { static constexpr int NV = 3, P = 2, TW = 10; };
template <> struct CpShape<CP_TET_STRAIN> { static constexpr int NV = 4, P = 3, TW = 9; };
template <> struct CpShape<CP_TET_DEFGRAD> { static constexpr int NV = 4, P = 3, TW = 9; };
template <> struct CpShape<CP_BEND> { static constexpr int NV = 1, P = 1, TW = 5; };

// LAUNCH<KIND>(arguments) for the kind of an element set-up (asb_cproj_setup admits the five only)
#define CP_FOR_KIND(kind, LAUNCH, ...)                                   \
    switch (kind) {                                                      \
        case CP_EDGE: LAUNCH<CP_EDGE>(__VA_ARGS__); break;               \
        case CP_TRI: LAUNCH<CP_TRI>(__VA_ARGS__); break;                 \
        case CP_TET_STRAIN: LAUNCH<CP_TET_STRAIN>(__VA_ARGS__); break;   \
        case CP_TET_DEFGRAD: LAUNCH<CP_TET_DEFGRAD>(__VA_ARGS__); break; \
        default: LAUNCH<CP_BEND>(__VA_ARGS__); break;                    \
    }

// ---------------------------------------------------------------- the five projections: r[3 p] of one (element, frame)
__device__ __forceinline__ void cp_edge(const CpWorld& w, long long f, const int* __restrict__ ix, const double* __restrict__ tb,
                                        double (&r)[3]) {
    double a[3], b[3];
    cp_pos(w, f, ix[0], a);
    cp_pos(w, f, ix[1], b);
    const double s0 = b[0] - a[0], s1 = b[1] - a[1], s2 = b[2] - a[2];
    const double len = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    // 0.5 (pi2 - pi1) of :306-311 is 0.5 d s / |s|; |s| = 0 (:303-304: no projection) gives 0 / 0 = NaN, what storing the
    // reference's None in a float row gives
    const double g = 0.5 * tb[0] / len;
    r[0] = len == 0.0 ? NAN : g * s0;
    r[1] = len == 0.0 ? NAN : g * s1;
    r[2] = len == 0.0 ? NAN : g * s2;
}

__device__ __forceinline__ void cp_tri(const CpWorld& w, long long f, const int* __restrict__ ix, const double* __restrict__ tb,
                                       double smin, double smax, double (&r)[6]) {
    double q1[3], q2[3], q3[3];
    cp_pos(w, f, ix[0], q1);
    cp_pos(w, f, ix[1], q2);
    cp_pos(w, f, ix[2], q3);
    // tb: P (3 x 2) row-major, DmInv (2 x 2) row-major.  Ds2 = P^T [q2 - q1, q3 - q1], F = Ds2 DmInv
    double ds[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ds[j][0] = tb[j] * (q2[0] - q1[0]) + tb[2 + j] * (q2[1] - q1[1]) + tb[4 + j] * (q2[2] - q1[2]);
        ds[j][1] = tb[j] * (q3[0] - q1[0]) + tb[2 + j] * (q3[1] - q1[1]) + tb[4 + j] * (q3[2] - q1[2]);
    }
    double Fm[2][2], Fh[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) Fm[i][j] = ds[i][0] * tb[6 + j] + ds[i][1] * tb[8 + j];
    cp_project_tri(Fm, smin, smax, Fh);
    // pi = (P Fhat)^T: row a, column c = sum_b P[c][b] Fhat[b][a]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) r[3 * a + c] = tb[2 * c] * Fh[0][a] + tb[2 * c + 1] * Fh[1][a];
}

template <int KIND>
__device__ __forceinline__ void cp_tet(const CpWorld& w, long long f, const int* __restrict__ ix, const double* __restrict__ tb,
                                       double smin, double smax, double (&r)[9]) {
    double q[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) cp_pos(w, f, ix[i], q[i]);
    double Fm[3][3];
    // F = [q1 - q4, q2 - q4, q3 - q4] DmInv
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Fm[i][j] = (q[0][i] - q[3][i]) * tb[j] + (q[1][i] - q[3][i]) * tb[3 + j] + (q[2][i] - q[3][i]) * tb[6 + j];
    cp_project_tet<KIND>(Fm, smin, smax, r);
}

__device__ __forceinline__ void cp_bend(const CpWorld& w, long long f, int v, const double* __restrict__ tb, const int* __restrict__ nb,
                                        const double* __restrict__ wt, int e0, int e1, double (&r)[3]) {
    double x[3], y[3], ss[3] = {0.0, 0.0, 0.0};
    cp_pos(w, f, v, x);
    for (int e = e0; e < e1; ++e) {                 // (:201-202) in the star's edge order
        cp_pos(w, f, nb[e], y);
        const double we = wt[e];
#pragma unroll
        for (int d = 0; d < 3; ++d) ss[d] += (x[d] - y[d]) * we;
    }
    const double nrm = sqrt(ss[0] * ss[0] + ss[1] * ss[1] + ss[2] * ss[2]);
    const double rmc = tb[0];
    const double g = rmc / nrm;
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] = nrm < 1e-10 ? tb[1 + d] * rmc : ss[d] * g;                // (:205-208)
    const double dot = tb[1] * r[0] + tb[2] * r[1] + tb[3] * r[2];
    if (nrm > 1e-5 && dot * tb[4] < 0.0) r[0] = -r[0], r[1] = -r[1], r[2] = -r[2];              // (:210-213)
}

// grid (element blocks, frame tiles); out (n_sel, n_elem * P, 3)
template <int KIND>
__global__ __launch_bounds__(64 * CP_WAVES) void k_cproj(CpWorld w, const int* __restrict__ idx, const double* __restrict__ table,
                                                         const int* __restrict__ sptr, const int* __restrict__ sidx,
                                                         const double* __restrict__ swt, long long n_elem, int f0, int fj, int n_sel,
                                                         double smin, double smax, double* __restrict__ out) {
    constexpr int NV = CpShape<KIND>::NV, P3 = 3 * CpShape<KIND>::P, TW = CpShape<KIND>::TW;
    constexpr int RUN = CP_EB * P3, ROW = RUN + 1;
    __shared__ double stage[64 * ROW];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s0 = (int)blockIdx.y * 64;
    // a lane past the last selected frame recomputes frame f0 (an address inside the tensor); its row is never written out
    const long long f = (long long)f0 + (long long)(s0 + lane < n_sel ? s0 + lane : 0) * fj;
    const long long e_base = (long long)blockIdx.x * CP_EB;
    for (int j = wid; j < CP_EB; j += CP_WAVES) {
        const long long e = e_base + j;
        if (e >= n_elem) break;                     // the same in every lane
        double r[P3];
        const int* ix = idx + e * NV;
        const double* tb = table + e * TW;
        if constexpr (KIND == CP_EDGE) cp_edge(w, f, ix, tb, r);
        else if constexpr (KIND == CP_TRI) cp_tri(w, f, ix, tb, smin, smax, r);
        else if constexpr (KIND == CP_BEND) cp_bend(w, f, ix[0], tb, sidx, swt, sptr[e], sptr[e + 1], r);
        else cp_tet<KIND>(w, f, ix, tb, smin, smax, r);
#pragma unroll
        for (int k = 0; k < P3; ++k) stage[lane * ROW + j * P3 + k] = r[k];
    }
    __syncthreads();
    const int ne = n_elem - e_base < CP_EB ? (int)(n_elem - e_base) : CP_EB;
    const int nf = n_sel - s0 < 64 ? n_sel - s0 : 64;
    const int run = ne * P3;
    const long long row_len = n_elem * P3;
    for (int i = threadIdx.x; i < 64 * RUN; i += 64 * CP_WAVES) {
        const int fl = i / RUN, k = i % RUN;
        if (fl < nf && k < run) out[(long long)(s0 + fl) * row_len + e_base * P3 + k] = stage[fl * ROW + k];
    }
}

// The element kind of the next asb_cproj_run calls: indices (n_elem x NV), tables (n_elem x TW; verts_bending: followed by the
// star edges' weights) and, for verts_bending, the star CSR.  Every index the kernel follows is checked against the vertices
// of the resident tensor here.  Replaces the previous set-up of this context.
extern "C" int asb_cproj_setup(asb_ctx* ctx, int kind, int64_t n_elem, const int64_t* idx, const double* table, const int64_t* star_ptr,
                               const int64_t* star_idx) {
    if (!ctx || !idx || !table || n_elem < 1) return ASB_ERR_ARG;
    if (kind < CP_EDGE || kind > CP_BEND) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: unknown kind %d", kind);
    if (!ctx->X || ctx->n_loc < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: no snapshots on the device");
    if (ctx->v0 != 0 || ctx->n_loc != ctx->N_glob)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: vertices [%lld, +%lld) of %lld: elements straddle vertex shards, one rank only",
                 (long long)ctx->v0, (long long)ctx->n_loc, (long long)ctx->N_glob);
    static const int NV[5] = {2, 3, 4, 4, 1}, TW[5] = {1, 10, 9, 9, 5};
    const int nv = NV[kind], tw = TW[kind];
    const long long n_loc = ctx->n_loc;
    if (n_loc > 0x7fffffffLL || n_elem > 0x7fffffffLL / 16) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_cproj_setup: too large for 32-bit indices");
    CpSetup& cp = ctx->cp;
    cp.kind = -1;
    int64_t vmax = -1;
    std::vector<int> i32((size_t)n_elem * nv), p32, s32;
    for (int64_t i = 0; i < n_elem * nv; ++i) {
        if (idx[i] < 0 || idx[i] >= n_loc)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: element %lld names vertex %lld of %lld", (long long)(i / nv), (long long)idx[i], n_loc);
        i32[i] = (int)idx[i];
        if (idx[i] > vmax) vmax = idx[i];
    }
    int64_t nnz = 0;
    if (kind == CP_BEND) {
        if (!star_ptr || !star_idx) return ASB_ERR_ARG;
        if (star_ptr[0] != 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: the star offsets do not start at 0");
        for (int64_t v = 0; v < n_elem; ++v)
            if (star_ptr[v + 1] < star_ptr[v]) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: star offsets decrease at element %lld", (long long)v);
        nnz = star_ptr[n_elem];
        if (nnz > 0x7fffffffLL) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_cproj_setup: too many star edges for 32-bit indices");
        p32.resize((size_t)n_elem + 1);
        s32.resize((size_t)nnz);
        for (int64_t v = 0; v <= n_elem; ++v) p32[v] = (int)star_ptr[v];
        for (int64_t i = 0; i < nnz; ++i) {
            if (star_idx[i] < 0 || star_idx[i] >= n_loc)
                ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cproj_setup: star edge %lld names vertex %lld of %lld", (long long)i, (long long)star_idx[i], n_loc);
            s32[i] = (int)star_idx[i];
            if (star_idx[i] > vmax) vmax = star_idx[i];
        }
    }
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const size_t n_table = (size_t)n_elem * tw + (size_t)nnz;
    int rc;
    if ((rc = asb_alloc(ctx, &cp.idx, i32.size()))) return rc;
    if ((rc = asb_alloc(ctx, &cp.table, n_table))) return rc;
    if ((rc = asb_alloc(ctx, &cp.sptr, p32.size() + 1))) return rc;
    if ((rc = asb_alloc(ctx, &cp.sidx, s32.size() + 1))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(cp.idx, i32.data(), i32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(cp.table, table, n_table * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!p32.empty()) ASB_HIP(ctx, hipMemcpyAsync(cp.sptr, p32.data(), p32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (!s32.empty()) ASB_HIP(ctx, hipMemcpyAsync(cp.sidx, s32.data(), s32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the staging vectors die here)
    cp.kind = kind, cp.n = n_elem, cp.verts = n_loc, cp.vmax = vmax;
    return ASB_OK;
}

template <int KIND>
static void cp_launch(asb_ctx* ctx, const CpWorld& w, int f0, int fj, int n_sel, double smin, double smax, double* out) {
    const CpSetup& cp = ctx->cp;
    const dim3 grid((unsigned)((cp.n + CP_EB - 1) / CP_EB), (unsigned)((n_sel + 63) / 64));
    hipLaunchKernelGGL(k_cproj<KIND>, grid, dim3(64 * CP_WAVES), 0, ctx->stream, w, cp.idx, cp.table, cp.sptr, cp.sidx,
                       cp.table + (size_t)cp.n * CpShape<KIND>::TW, (long long)cp.n, f0, fj, n_sel, smin, smax, out);
}

int asb_world_frames(asb_ctx* ctx, const char* who, int which, int64_t f0, int64_t f1, int64_t fj, int add_mean, double psf, CpWorld* w,
                     int64_t* n_sel_out) {
    if (!ctx->X || ctx->v0 != 0 || ctx->n_loc != ctx->N_glob) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no whole tensor on the device (one rank only)", who);
    int64_t F;
    if (which == 0) {
        w->T = ctx->X, w->ldt = ctx->Fp, F = ctx->F;
    } else if (which == 1) {
        if (!ctx->ho_Y) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no held-out animation on the device (asb_heldout_upload)", who);
        w->T = ctx->ho_Y, w->ldt = ctx->ho_Fp, F = ctx->ho_F;
    } else {
        return ASB_ERR_ARG;
    }
    if (f0 < 0 || f1 > F || f0 >= f1 || fj < 1)
        ASB_FAIL(ctx, ASB_ERR_ARG, "%s: range(%lld, %lld, %lld) is not a selection of the %lld frames", who, (long long)f0, (long long)f1,
                 (long long)fj, (long long)F);
    if (add_mean && !ctx->have_mean) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no mean on the device", who);
    if (!(psf > 0.0)) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: scale %g", who, psf);
    w->mean = add_mean ? ctx->mean : nullptr;
    w->invm = nullptr;
    w->inv_psf = 1.0 / psf;
    *n_sel_out = (f1 - f0 + fj - 1) / fj;
    return ASB_OK;
}

int asb_cproj_world(asb_ctx* ctx, const char* who, int which, int64_t f0, int64_t f1, int64_t fj, int add_mean, double psf,
                    double sigma_min, double sigma_max, CpWorld* w, int64_t* n_sel_out) {
    if (ctx->cp.kind < 0 || !ctx->X || ctx->cp.verts != ctx->n_loc || ctx->v0 != 0 || ctx->n_loc != ctx->N_glob)
        ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no element set-up for the resident tensor (asb_cproj_setup)", who);
    int rc;
    if ((rc = asb_world_frames(ctx, who, which, f0, f1, fj, add_mean, psf, w, n_sel_out))) return rc;
    if (!(sigma_min <= sigma_max)) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: sigma_min %g > sigma_max %g", who, sigma_min, sigma_max);
    if ((*n_sel_out + 63) / 64 > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "%s: %lld frames in one call (at most %d)", who, (long long)*n_sel_out, 65535 * 64);
    return ASB_OK;
}

int asb_cproj_invm(asb_ctx* ctx, const double* inv_massL, CpWorld* w) {
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if (inv_massL) {
        int rc;
        if ((rc = asb_alloc(ctx, &ctx->cp_invm, (size_t)ctx->n_loc))) return rc;
        ASB_HIP(ctx, hipMemcpyAsync(ctx->cp_invm, inv_massL, (size_t)ctx->n_loc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        w->invm = ctx->cp_invm;
    }
    return ASB_OK;
}

extern "C" int asb_cproj_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                             double sigma_min, double sigma_max, double* out_dev) {
    if (!ctx || !out_dev) return ASB_ERR_ARG;
    CpWorld w;
    int64_t n_sel;
    int rc;
    if ((rc = asb_cproj_world(ctx, "asb_cproj_run", which, f0, f1, fj, add_mean, psf, sigma_min, sigma_max, &w, &n_sel))) return rc;
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    CP_FOR_KIND(ctx->cp.kind, cp_launch, ctx, w, (int)f0, (int)fj, (int)n_sel, sigma_min, sigma_max, out_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// ---------------------------------------------------------------- constraint forces b = S^T p of the resident animation
// b[f] = S^T p(q_f), (n_sel, N, 3) frame-major (Simulators.py:643-724, one kind's term), in chunks of cw selected frames so
// that p is never formed at full size.  Per chunk, in stream order:
//   k_cproj_em   the projections of the chunk, ELEMENT-major: scratch row (e P + i) 3 + d holds cw doubles, one per frame of
//                the chunk.  Same per-thread routines, same world positions, same wave = one element x 64 frames as k_cproj;
//                every store is a coalesced 512-byte run, so no LDS transposition.
//   k_st_apply   a wave owns one vertex x 64 frames: it walks the vertex's row of S^T in ascending column order (indices and
//                values are the same in every lane), accumulates the three coordinates by f64 FMA in that order from
//                coalesced reads of the scratch rows, and a block of CF_VB vertices x 64 frames stages its results in LDS
//                (odd row length) to write per frame its contiguous run of CF_VB * 3 doubles -- a plain read-modify-write
//                of the block's own entries when accumulating.
// An (frame, vertex) entry is summed by one thread in a fixed order and no thread touches another's entry: no atomics;
// repeated calls, sub-ranges and any chunk width give the same bits.  A NaN of a collapsed edge reaches the vertices whose
// row stores that column (S^T stores no zeros: the edge's two vertices) and nothing else.
#define CF_VB 16                                // vertices per block of k_st_apply
#define CF_SCRATCH_BYTES (256ull << 20)         // bound on the element-major scratch of one chunk

template <int KIND>
__global__ __launch_bounds__(64 * CP_WAVES) void k_cproj_em(CpWorld w, const int* __restrict__ idx, const double* __restrict__ table,
                                                            const int* __restrict__ sptr, const int* __restrict__ sidx,
                                                            const double* __restrict__ swt, long long n_elem, int f0, int fj, int c0,
                                                            int cn, int cw, double smin, double smax, double* __restrict__ S) {
    constexpr int NV = CpShape<KIND>::NV, P3 = 3 * CpShape<KIND>::P, TW = CpShape<KIND>::TW;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = (int)blockIdx.y * 64 + lane;            // frame of the chunk: selected frame c0 + col
    const bool ok = col < cn;
    // a lane past the chunk's last frame recomputes frame f0 (an address inside the tensor) and stores nothing
    const long long f = (long long)f0 + (long long)(ok ? c0 + col : 0) * fj;
    const long long e_base = (long long)blockIdx.x * CP_EB;
    for (int j = wid; j < CP_EB; j += CP_WAVES) {
        const long long e = e_base + j;
        if (e >= n_elem) break;                     // the same in every lane
        double r[P3];
        const int* ix = idx + e * NV;
        const double* tb = table + e * TW;
        if constexpr (KIND == CP_EDGE) cp_edge(w, f, ix, tb, r);
        else if constexpr (KIND == CP_TRI) cp_tri(w, f, ix, tb, smin, smax, r);
        else if constexpr (KIND == CP_BEND) cp_bend(w, f, ix[0], tb, sidx, swt, sptr[e], sptr[e + 1], r);
        else cp_tet<KIND>(w, f, ix, tb, smin, smax, r);
        if (ok) {
#pragma unroll
            for (int k = 0; k < P3; ++k) S[(e * P3 + k) * cw + col] = r[k];
        }
    }
}

// grid (vertex blocks, frame tiles of the chunk); out (n_sel, N, 3), rows c0 .. c0 + cn of it
__global__ __launch_bounds__(64 * CP_WAVES) void k_st_apply(const int* __restrict__ ptr, const int* __restrict__ ci,
                                                            const double* __restrict__ val, const double* __restrict__ S, int cw,
                                                            int c0, int cn, long long n_verts, int accumulate,
                                                            double* __restrict__ out) {
    constexpr int RUN = CF_VB * 3, ROW = RUN + 1;
    __shared__ double stage[64 * ROW];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = (int)blockIdx.y * 64;
    const int col = t0 + lane;
    const bool ok = col < cn;
    const long long v_base = (long long)blockIdx.x * CF_VB;
    for (int j = wid; j < CF_VB; j += CP_WAVES) {
        const long long v = v_base + j;
        if (v >= n_verts) break;                    // the same in every lane
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const int t1 = ptr[v + 1];
        for (int t = ptr[v]; t < t1; ++t) {         // ascending columns
            const double s = val[t];
            if (ok) {
                const double* row = S + 3LL * ci[t] * cw + col;
                a0 = fma(s, row[0], a0);
                a1 = fma(s, row[cw], a1);
                a2 = fma(s, row[2LL * cw], a2);
            }
        }
        stage[lane * ROW + j * 3 + 0] = a0;
        stage[lane * ROW + j * 3 + 1] = a1;
        stage[lane * ROW + j * 3 + 2] = a2;
    }
    __syncthreads();
    const int nv = n_verts - v_base < CF_VB ? (int)(n_verts - v_base) : CF_VB;
    const int nf = cn - t0 < 64 ? cn - t0 : 64;
    const int run = nv * 3;
    for (int i = threadIdx.x; i < 64 * RUN; i += 64 * CP_WAVES) {
        const int fl = i / RUN, k = i % RUN;
        if (fl < nf && k < run) {
            double* o = out + ((long long)(c0 + t0 + fl) * n_verts + v_base) * 3 + k;
            *o = accumulate ? *o + stage[fl * ROW + k] : stage[fl * ROW + k];
        }
    }
}

template <int KIND>
static void cf_launch(asb_ctx* ctx, const CpSetup& t, const CpWorld& w, int f0, int fj, int c0, int cn, int cw, double smin, double smax,
                      double* S) {
    const dim3 grid((unsigned)((t.n + CP_EB - 1) / CP_EB), (unsigned)((cn + 63) / 64));
    hipLaunchKernelGGL(k_cproj_em<KIND>, grid, dim3(64 * CP_WAVES), 0, ctx->stream, w, t.idx, t.table, t.sptr, t.sidx,
                       t.table + (size_t)t.n * CpShape<KIND>::TW, (long long)t.n, f0, fj, c0, cn, cw, smin, smax, S);
}

void asb_cproj_em_launch(asb_ctx* ctx, const CpSetup& t, const CpWorld& w, int f0, int fj, int c0, int cn, int cw, double smin, double smax,
                         double* S) {
    CP_FOR_KIND(t.kind, cf_launch, ctx, t, w, f0, fj, c0, cn, cw, smin, smax, S);
}

long long asb_cproj_rows(int kind, long long n_elem) {
    static const int PK[5] = {1, 2, 3, 3, 1};
    return n_elem * PK[kind];
}

// whole 128-byte lines per scratch row, the scratch within CF_SCRATCH_BYTES, whole waves if it can
long long asb_cforce_chunk_width(long long n_cols, long long chunk_frames, long long n_sel) {
    long long cw = (long long)(CF_SCRATCH_BYTES / (24ull * (unsigned long long)n_cols));
    cw = cw >= 64 ? cw / 64 * 64 : (cw >= 16 ? cw / 16 * 16 : 16);
    if (chunk_frames > 0 && (chunk_frames + 15) / 16 * 16 < cw) cw = (chunk_frames + 15) / 16 * 16;
    const long long span = (n_sel + 15) / 16 * 16;
    return cw > span ? span : cw;
}

void asb_st_apply_launch(asb_ctx* ctx, const int* ptr, const int* ci, const double* val, const double* S, int cw, int c0, int cn,
                         long long n_rows, int accumulate, double* out) {
    hipLaunchKernelGGL(k_st_apply, dim3((unsigned)((n_rows + CF_VB - 1) / CF_VB), (unsigned)((cn + 63) / 64)), dim3(64 * CP_WAVES), 0, ctx->stream,
                       ptr, ci, val, S, cw, c0, cn, n_rows, accumulate ? 1 : 0, out);
}

int asb_csr_check32(asb_ctx* ctx, const char* who, int64_t n_rows, const int64_t* indptr, const int64_t* indices, const double* data,
                    long long n_cols, std::vector<int>& p32, std::vector<int>& c32, const char* what) {
    if (indptr[0] != 0) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the row offsets of %s do not start at 0", who, what);
    for (int64_t v = 0; v < n_rows; ++v)
        if (indptr[v + 1] < indptr[v]) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: row offsets of %s decrease at row %lld", who, what, (long long)v);
    const int64_t nnz = indptr[n_rows];
    if (nnz > 0x7fffffffLL) ASB_FAIL(ctx, ASB_ERR_LIMIT, "%s: too many entries of %s for 32-bit indices", who, what);
    if (nnz > 0 && (!indices || !data)) return ASB_ERR_ARG;
    p32.resize((size_t)n_rows + 1);
    c32.resize((size_t)nnz);
    for (int64_t v = 0; v <= n_rows; ++v) p32[v] = (int)indptr[v];
    for (int64_t v = 0; v < n_rows; ++v)
        for (int64_t t = indptr[v]; t < indptr[v + 1]; ++t) {
            if (indices[t] < 0 || indices[t] >= n_cols)
                ASB_FAIL(ctx, ASB_ERR_ARG, "%s: row %lld of %s names column %lld of %lld", who, (long long)v, what, (long long)indices[t], n_cols);
            if (t > indptr[v] && indices[t] <= indices[t - 1])
                ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the columns of row %lld of %s are not ascending", who, (long long)v, what);
            c32[t] = (int)indices[t];
        }
    return ASB_OK;
}

extern "C" int asb_cforce_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean,
                              double psf, double sigma_min, double sigma_max, int64_t n_rows, const int64_t* indptr,
                              const int64_t* indices, const double* data, int accumulate, int64_t chunk_frames, double* out_dev) {
    if (!ctx || !out_dev || !indptr || n_rows < 1) return ASB_ERR_ARG;
    CpWorld w;
    int64_t n_sel;
    int rc;
    if ((rc = asb_cproj_world(ctx, "asb_cforce_run", which, f0, f1, fj, add_mean, psf, sigma_min, sigma_max, &w, &n_sel))) return rc;
    if (chunk_frames < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cforce_run: chunk_frames %lld", (long long)chunk_frames);
    // ---- the CSR of S^T: one row per vertex of the tensor, columns = rows of the stacked projections, ascending in a row
    const long long n_cols = asb_cproj_rows(ctx->cp.kind, ctx->cp.n);
    if (n_rows != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_cforce_run: S^T has %lld rows, the tensor %lld vertices", (long long)n_rows, (long long)ctx->n_loc);
    std::vector<int> p32, c32;
    if ((rc = asb_csr_check32(ctx, "asb_cforce_run", n_rows, indptr, indices, data, n_cols, p32, c32))) return rc;
    const long long cw = asb_cforce_chunk_width(n_cols, chunk_frames, n_sel);
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_ptr, p32.size()))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_idx, c32.size() + 1))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_val, c32.size() + 1))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_scratch, (size_t)3 * n_cols * cw))) return rc;
    if ((rc = asb_csr_stage(ctx, p32, c32, data, ctx->cf_ptr, ctx->cf_idx, ctx->cf_val))) return rc;
    for (long long c0 = 0; c0 < n_sel; c0 += cw) {
        const int cn = (int)(c0 + cw < n_sel ? cw : n_sel - c0);
        asb_cproj_em_launch(ctx, ctx->cp, w, (int)f0, (int)fj, (int)c0, cn, (int)cw, sigma_min, sigma_max, ctx->cf_scratch);
        asb_st_apply_launch(ctx, ctx->cf_ptr, ctx->cf_idx, ctx->cf_val, ctx->cf_scratch, (int)cw, (int)c0, cn, (long long)n_rows, accumulate,
                            out_dev);
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the staging vectors die here; the caller owns out_dev
    return ASB_OK;
}

// ---------------------------------------------------------------- test hooks: "project F" alone (tests/cproj_cases.py)
// m: one stored F row-major (tris_strain 2 x 2, the tet kinds 3 x 3) -> o: Fhat (2 x 2), U diag(c) V^T or R^T (3 x 3), row-major
__host__ __device__ static inline void cp_project_one(int kind, const double* m, double smin, double smax, double* o) {
    if (kind == CP_TRI) {
        const double F[2][2] = {{m[0], m[1]}, {m[2], m[3]}};
        double Fh[2][2];
        cp_project_tri(F, smin, smax, Fh);
        o[0] = Fh[0][0], o[1] = Fh[0][1], o[2] = Fh[1][0], o[3] = Fh[1][1];
        return;
    }
    const double F[3][3] = {{m[0], m[1], m[2]}, {m[3], m[4], m[5]}, {m[6], m[7], m[8]}};
    double r[9];
    if (kind == CP_TET_STRAIN) cp_project_tet<CP_TET_STRAIN>(F, smin, smax, r);
    else cp_project_tet<CP_TET_DEFGRAD>(F, smin, smax, r);
    for (int k = 0; k < 9; ++k) o[k] = r[k];
}

static int cp_probe_width(int kind) { return kind == CP_TRI ? 4 : (kind == CP_TET_STRAIN || kind == CP_TET_DEFGRAD ? 9 : 0); }

extern "C" int asb_test_cproj_project(int kind, const double* mats, int64_t n, double sigma_min, double sigma_max, double* out) {
    const int w = cp_probe_width(kind);
    if (!w || !mats || !out || n < 1 || !(sigma_min <= sigma_max)) return ASB_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) cp_project_one(kind, mats + i * w, sigma_min, sigma_max, out + i * w);
    return ASB_OK;
}

// one thread per matrix, no context state
static __global__ __launch_bounds__(64) void k_test_cproj_project(int kind, int w, const double* __restrict__ mats, long long n, double smin,
                                                                  double smax, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cp_project_one(kind, mats + i * w, smin, smax, out + i * w);
}

extern "C" int asb_test_cproj_project_dev(asb_ctx* ctx, int kind, const double* mats, int64_t n, double sigma_min, double sigma_max,
                                          double* out, int64_t out_len) {
    if (!ctx || !mats || !out) return ASB_ERR_ARG;
    const int w = cp_probe_width(kind);
    if (!w || n < 1 || n > (1 << 24) || out_len < w * n || !(sigma_min <= sigma_max))
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_cproj_project_dev: kind %d, n = %lld, out_len = %lld, clamp [%g, %g]", kind, (long long)n,
                 (long long)out_len, sigma_min, sigma_max);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<double> dm, dout;
    int rc = asb_test_stage(ctx, mats, (size_t)n * w, 64, dm);
    if (!rc) rc = asb_test_stage(ctx, out, (size_t)out_len, 0, dout);
    if (!rc) {
        hipLaunchKernelGGL(k_test_cproj_project, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, kind, w, dm.get(), (long long)n,
                           sigma_min, sigma_max, dout.get());
        if (hipGetLastError() != hipSuccess) rc = ASB_ERR_HIP;
    }
    return asb_test_finish(ctx, rc, dout.get(), out, (size_t)out_len);
}
