// On-mesh accuracy maps of a k-component reconstruction (generate_figures/onMesh_accuracyMeasures.py:61-151, compute_accuracy):
// per-vertex, per-frame relative position errors, per-frame whole-mesh errors and the angle between the per-vertex normals of
// the full and the reduced mesh, in world space, without downloading the tensor or forming an (F, N, 3) reconstruction.
//
// World space: x = (T / psf + mean) / massL_v (the inverse of what the upload applied; formed with the reciprocals 1 / psf and
// 1 / massL_v), x_r the same of R_r = A[:, :r] B[:r].
//
// Error pass (k_onmesh_err, ONE read of T, the shape of k_recon_sweep): a wave owns OM_VT vertices (all three rows) and 64 OM_NF
// frames, keeps T and the running reconstruction in registers and adds the r rank-1 terms by f64 FMA.  Every lane then holds
// all three coordinates of its (vertex, frame) elements.  blockIdx.y is the frame tile, so a lane's frames are fixed for the
// whole block: per-frame numerators / denominators stay in registers over the block's vertices, the block sums its waves in
// order through LDS and k_onmesh_frames sums the blocks in block order.  Per-vertex sums are reduced over the wave (DPP) into
// the tile's own row of a (tiles x n_loc) buffer; k_onmesh_verts sums the tiles in tile order.
//
// Normal pass, in chunks of frames: k_onmesh_fill writes the chunk's reconstruction to a scratch buffer in the tensor's
// vertex-major layout (rows of cw doubles, cw a multiple of 16: whole 128-byte lines; at most OM_SCRATCH_BYTES), k_onmesh_normals
// (lanes along the chunk's frames, a wave per vertex) walks the vertex's star through the CSR in increasing triangle number,
// recomputes the un-normalised cross product of each incident triangle for the full (from T, on the fly) and the reduced mesh,
// and forms the angle.  The triangle normals are recomputed per incident vertex rather than written once and gathered: a
// gather pass moves about as many bytes (18 loads + 6 stores per triangle, then 36 loads per vertex, against 108 loads per vertex
// that mostly hit in cache: a star's rows were just read by the neighbouring waves) and needs a second scratch twice the size of
// the first.  The per-vertex accumulator is updated once per chunk by the one wave that owns the vertex, chunks run in stream
// order: no atomics, repeated calls are bit-identical.
//
// min / max are kept NaN-propagating, as numpy.min / numpy.max are: a separate flag is max-reduced beside them.
#include "asb_common.h"

#include <cmath>
#include <vector>

#define OM_VT 2                         // vertices per wave work unit (error pass)
#define OM_NF 4                         // frames per lane, strided by 64
#define OM_WAVES 4
#define OM_TILE (64 * OM_NF)            // frames per tile
#define OM_FV 4                         // vertices per wave work unit (fill)
#define OM_SCRATCH_BYTES (256ull << 20) // bound on the reconstruction scratch of the normal pass

__device__ __forceinline__ bool om_selected(int f, int fs, int fe, int fj) { return f >= fs && f < fe && (f - fs) % fj == 0; }

// [-min, max, NaN seen] of a lane -> wave -> LDS row
__device__ __forceinline__ void om_track(double v, double (&st)[3]) {
    if (v != v) st[2] = 1.0;
    else {
        st[0] = fmax(st[0], -v);
        st[1] = fmax(st[1], v);
    }
}

__global__ __launch_bounds__(256) void k_onmesh_err(const double* __restrict__ T, long long ldt, int F, long long n_loc,
                                                    const double* __restrict__ A, long long lda, const double* __restrict__ B,
                                                    long long ldb, int r, const double* __restrict__ mean,
                                                    const double* __restrict__ invm, double inv_psf, double denom, int fs, int fe,
                                                    int fj, int tile0, double* __restrict__ vpart, double* __restrict__ fpart,
                                                    double* __restrict__ spart, double* __restrict__ frame_err) {
    __shared__ double fl[OM_WAVES][2][OM_TILE];
    __shared__ double sl[OM_WAVES][3];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f0 = (tile0 + (int)blockIdx.y) * OM_TILE + lane;
    bool fok[OM_NF], sel[OM_NF];
#pragma unroll
    for (int q = 0; q < OM_NF; ++q) {
        fok[q] = f0 + 64 * q < F;
        sel[q] = fok[q] && om_selected(f0 + 64 * q, fs, fe, fj);
    }
    double num[OM_NF], den[OM_NF], st[3] = {-INFINITY, -INFINITY, 0.0};
#pragma unroll
    for (int q = 0; q < OM_NF; ++q) num[q] = den[q] = 0.0;
    const long long n_vg = (n_loc + OM_VT - 1) / OM_VT;

    for (long long vg = (long long)blockIdx.x * OM_WAVES + wid; vg < n_vg; vg += (long long)gridDim.x * OM_WAVES) {
        const long long vbase = vg * OM_VT;
        bool rok[OM_VT * 3];
#pragma unroll
        for (int i = 0; i < OM_VT * 3; ++i) rok[i] = vbase + i / 3 < n_loc;
        double t[OM_VT * 3][OM_NF], a[OM_VT * 3][OM_NF];
#pragma unroll
        for (int i = 0; i < OM_VT * 3; ++i)
#pragma unroll
            for (int q = 0; q < OM_NF; ++q) {
                t[i][q] = (rok[i] && fok[q]) ? T[(3 * vbase + i) * ldt + f0 + 64 * q] : 0.0;
                a[i][q] = 0.0;
            }
#pragma unroll 2
        for (int k = 0; k < r; ++k) {               // + A[k] (x) B[k] on this tile (masked entries stay exactly 0)
            double w[OM_NF], c[OM_VT * 3];
#pragma unroll
            for (int q = 0; q < OM_NF; ++q) w[q] = fok[q] ? A[(long long)k * lda + f0 + 64 * q] : 0.0;
#pragma unroll
            for (int i = 0; i < OM_VT * 3; ++i) c[i] = rok[i] ? B[(long long)k * ldb + 3 * vbase + i] : 0.0;
#pragma unroll
            for (int i = 0; i < OM_VT * 3; ++i)
#pragma unroll
                for (int q = 0; q < OM_NF; ++q) a[i][q] = fma(w[q], c[i], a[i][q]);
        }
        double vs[OM_VT];
#pragma unroll
        for (int j = 0; j < OM_VT; ++j) {
            vs[j] = 0.0;
            const bool vok = rok[3 * j];
            const double im = (invm && vok) ? invm[vbase + j] : 1.0;
            const double s = inv_psf * im;
            double m3[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) m3[d] = (mean && vok) ? mean[3 * (vbase + j) + d] : 0.0;
#pragma unroll
            for (int q = 0; q < OM_NF; ++q) {
                double d2 = 0.0, x2 = 0.0;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double e = (t[3 * j + d][q] - a[3 * j + d][q]) * s;       // x - x_r: the mean cancels
                    const double x = (t[3 * j + d][q] * inv_psf + m3[d]) * im;
                    d2 = fma(e, e, d2);
                    x2 = fma(x, x, x2);
                }
                if (vok && sel[q]) {
                    const double fe_ = d2 / x2 / denom;       // (:116)
                    num[q] += d2;
                    den[q] += x2;
                    vs[j] += fe_;
                    om_track(fe_, st);
                    if (frame_err) frame_err[(long long)((f0 + 64 * q - fs) / fj) * n_loc + vbase + j] = fe_;
                }
            }
        }
        wave_sum_dpp<OM_VT>(vs);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < OM_VT; ++j)
                if (rok[3 * j]) vpart[(long long)blockIdx.y * n_loc + vbase + j] = vs[j];
        }
    }
#pragma unroll
    for (int q = 0; q < OM_NF; ++q) {
        fl[wid][0][lane + 64 * q] = num[q];
        fl[wid][1][lane + 64 * q] = den[q];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) st[i] = wave_max_dpp(st[i]);
    if (lane == 0)
        for (int i = 0; i < 3; ++i) sl[wid][i] = st[i];
    __syncthreads();
    const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    for (int i = threadIdx.x; i < 2 * OM_TILE; i += blockDim.x) {
        double v = fl[0][i / OM_TILE][i % OM_TILE];
        for (int w = 1; w < OM_WAVES; ++w) v += fl[w][i / OM_TILE][i % OM_TILE];
        fpart[blk * (2 * OM_TILE) + i] = v;
    }
    if (threadIdx.x < 3) {
        double v = sl[0][threadIdx.x];
        for (int w = 1; w < OM_WAVES; ++w) v = fmax(v, sl[w][threadIdx.x]);
        spart[blk * 3 + threadIdx.x] = v;
    }
}

// per selected frame: numerator and denominator summed over the blocks of its tile in block order
__global__ __launch_bounds__(256) void k_onmesh_frames(const double* __restrict__ fpart, int gx, int tile0, int fs, int fj, int n_sel,
                                                       double* __restrict__ num, double* __restrict__ den) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_sel) return;
    const int f = fs + s * fj;
    const long long by = f / OM_TILE - tile0;
    const int j = f % OM_TILE;
    double a = 0.0, b = 0.0;
    for (int bx = 0; bx < gx; ++bx) {
        const double* p = fpart + (by * gx + bx) * (2 * OM_TILE);
        a += p[j];
        b += p[OM_TILE + j];
    }
    num[s] = a;
    den[s] = b;
}

// per vertex: the tiles' sums in tile order
__global__ __launch_bounds__(256) void k_onmesh_verts(const double* __restrict__ vpart, int n_tiles, long long n_loc,
                                                      double* __restrict__ out) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_loc) return;
    double s = vpart[v];
    for (int c = 1; c < n_tiles; ++c) s += vpart[(long long)c * n_loc + v];
    out[v] = s;
}

// one block: out[0..2] = min, sum, max of vec (n); out[3..4] = min, max of the block records spart (nblk x [-min, max, NaN]);
// all NaN-propagating, sums in a fixed order
__global__ __launch_bounds__(256) void k_onmesh_stats(const double* __restrict__ vec, long long n, const double* __restrict__ spart,
                                                      long long nblk, double* __restrict__ out) {
    __shared__ double sh[256][7];
    double st[3] = {-INFINITY, -INFINITY, 0.0}, sum = 0.0, mp[3] = {-INFINITY, -INFINITY, 0.0};
    for (long long i = threadIdx.x; i < n; i += 256) {
        sum += vec[i];
        om_track(vec[i], st);
    }
    for (long long b = threadIdx.x; b < nblk; b += 256)
        for (int i = 0; i < 3; ++i) mp[i] = fmax(mp[i], spart[b * 3 + i]);
    for (int i = 0; i < 3; ++i) {
        sh[threadIdx.x][i] = st[i];
        sh[threadIdx.x][4 + i] = mp[i];
    }
    sh[threadIdx.x][3] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t) {
            for (int i = 0; i < 3; ++i) {
                st[i] = fmax(st[i], sh[t][i]);
                mp[i] = fmax(mp[i], sh[t][4 + i]);
            }
            sum += sh[t][3];
        }
        out[0] = st[2] > 0.0 ? NAN : -st[0];
        out[1] = sum;
        out[2] = st[2] > 0.0 ? NAN : st[1];
        out[3] = mp[2] > 0.0 ? NAN : -mp[0];
        out[4] = mp[2] > 0.0 ? NAN : mp[1];
    }
}

// the chunk's reconstruction R[:, cf0 : cf1] = B[:r]^T A[:r] -> S (rows of cw doubles), padding columns 0
__global__ __launch_bounds__(256) void k_onmesh_fill(const double* __restrict__ A, long long lda, const double* __restrict__ B,
                                                     long long ldb, int r, long long n_loc, int cf0, int cf1, int cw,
                                                     double* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_ft = (cw + 63) / 64;
    const long long n_units = (n_loc + OM_FV - 1) / OM_FV * n_ft;
    for (long long u = (long long)blockIdx.x * OM_WAVES + wid; u < n_units; u += (long long)gridDim.x * OM_WAVES) {
        const long long vbase = (u / n_ft) * OM_FV;
        const int col = (int)(u % n_ft) * 64 + lane;
        const bool fok = cf0 + col < cf1;
        double acc[OM_FV * 3];
#pragma unroll
        for (int i = 0; i < OM_FV * 3; ++i) acc[i] = 0.0;
        for (int k = 0; k < r; ++k) {
            const double w = fok ? A[(long long)k * lda + cf0 + col] : 0.0;
#pragma unroll
            for (int i = 0; i < OM_FV * 3; ++i) {
                const double c = vbase + i / 3 < n_loc ? B[(long long)k * ldb + 3 * vbase + i] : 0.0;
                acc[i] = fma(w, c, acc[i]);
            }
        }
        if (col < cw) {
#pragma unroll
            for (int i = 0; i < OM_FV * 3; ++i)
                if (vbase + i / 3 < n_loc) S[(3 * vbase + i) * cw + col] = acc[i];
        }
    }
}

__device__ __forceinline__ void om_pos(const double* __restrict__ P, long long ld, long long col, int v, const double* __restrict__ mean,
                                       const double* __restrict__ invm, double inv_psf, bool ok, double (&x)[3]) {
    const double im = invm ? invm[v] : 1.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double t = ok ? P[(3LL * v + d) * ld + col] : 0.0;
        x[d] = (t * inv_psf + (mean ? mean[3LL * v + d] : 0.0)) * im;
    }
}

__device__ __forceinline__ void om_cross_add(const double (&a)[3], const double (&b)[3], const double (&c)[3], double (&n)[3]) {
    const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
    const double w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
    n[0] += u1 * w2 - u2 * w1;
    n[1] += u2 * w0 - u0 * w2;
    n[2] += u0 * w1 - u1 * w0;
}

// frames [cf0, cf1) of the chunk: angle between the area-weighted vertex normals of the full (T) and the reduced (S) mesh
__global__ __launch_bounds__(256) void k_onmesh_normals(const double* __restrict__ T, long long ldt, const double* __restrict__ S,
                                                        int cw, int cf0, int cf1, long long n_loc, const int* __restrict__ tris,
                                                        const int* __restrict__ sptr, const int* __restrict__ star,
                                                        const double* __restrict__ mean, const double* __restrict__ invm,
                                                        double inv_psf, int fs, int fe, int fj, int first, double* __restrict__ acc,
                                                        double* __restrict__ spart, double* __restrict__ angle_out) {
    __shared__ double sl[OM_WAVES][3];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_ft = (cf1 - cf0 + 63) / 64;
    double st[3] = {-INFINITY, -INFINITY, 0.0};
    for (long long v = (long long)blockIdx.x * OM_WAVES + wid; v < n_loc; v += (long long)gridDim.x * OM_WAVES) {
        const int e0 = sptr[v], e1 = sptr[v + 1];
        double vs[1] = {0.0};
        for (int ft = 0; ft < n_ft; ++ft) {
            const int col = ft * 64 + lane, f = cf0 + col;
            const bool ok = f < cf1;
            double n[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0};
            for (int e = e0; e < e1; ++e) {
                const int t = star[e];
                const int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
                double a[3], b[3], c[3];
                om_pos(T, ldt, f, ia, mean, invm, inv_psf, ok, a);
                om_pos(T, ldt, f, ib, mean, invm, inv_psf, ok, b);
                om_pos(T, ldt, f, ic, mean, invm, inv_psf, ok, c);
                om_cross_add(a, b, c, n);
                om_pos(S, cw, col, ia, mean, invm, inv_psf, ok, a);
                om_pos(S, cw, col, ib, mean, invm, inv_psf, ok, b);
                om_pos(S, cw, col, ic, mean, invm, inv_psf, ok, c);
                om_cross_add(a, b, c, nr);
            }
            if (ok && om_selected(f, fs, fe, fj)) {
                const double dot = n[0] * nr[0] + n[1] * nr[1] + n[2] * nr[2];
                const double l1 = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                const double l2 = sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
                double cs = dot / (l1 * l2);                                 // 0 / 0 = NaN: no triangle, or a zero normal
                if (cs == cs) cs = fmin(fmax(cs, -1.0), 1.0);                // (:85; a NaN stays, as numpy.clip leaves it)
                const double ang = acos(cs) * (180.0 / 3.14159265358979323846);
                vs[0] += ang;
                om_track(ang, st);
                if (angle_out) angle_out[(long long)((f - fs) / fj) * n_loc + v] = ang;
            }
        }
        wave_sum_dpp<1>(vs);
        if (lane == 0) acc[v] = first ? vs[0] : acc[v] + vs[0];      // one wave owns v in this launch, chunks run in stream order
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) st[i] = wave_max_dpp(st[i]);
    if (lane == 0)
        for (int i = 0; i < 3; ++i) sl[wid][i] = st[i];
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = sl[0][threadIdx.x];
        for (int w = 1; w < OM_WAVES; ++w) v = fmax(v, sl[w][threadIdx.x]);
        double* p = spart + (long long)blockIdx.x * 3 + threadIdx.x;
        *p = first ? v : fmax(*p, v);
    }
}

extern "C" int asb_onmesh_mesh(asb_ctx* ctx, const int64_t* tris, int64_t n_tris, const int64_t* star_ptr, const int64_t* star_tri,
                               int64_t v0, int64_t n_loc) {
    if (!ctx || !tris || !star_ptr || !star_tri || n_tris < 0) return ASB_ERR_ARG;
    if (v0 != 0 || n_loc != ctx->n_loc || n_loc != ctx->N_glob || n_loc < 1)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_mesh: vertices [%lld, +%lld) but the normals need the whole mesh of %lld on one shard",
                 (long long)v0, (long long)n_loc, (long long)ctx->N_glob);
    if (3 * n_tris > 0x7fffffffLL || n_loc > 0x7fffffffLL) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_onmesh_mesh: mesh too large for 32-bit indices");
    // every index the kernels will follow is checked here
    if (star_ptr[0] != 0 || star_ptr[n_loc] != 3 * n_tris) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_mesh: the vertex-star CSR does not hold 3 entries per triangle");
    for (int64_t v = 0; v < n_loc; ++v)
        if (star_ptr[v + 1] < star_ptr[v]) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_mesh: vertex-star offsets decrease at vertex %lld", (long long)v);
    std::vector<int> t32((size_t)3 * n_tris), p32((size_t)n_loc + 1), s32((size_t)3 * n_tris);
    for (int64_t i = 0; i < 3 * n_tris; ++i) {
        if (tris[i] < 0 || tris[i] >= n_loc) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_mesh: triangle %lld names vertex %lld of %lld", (long long)(i / 3), (long long)tris[i], (long long)n_loc);
        if (star_tri[i] < 0 || star_tri[i] >= n_tris) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_mesh: vertex-star entry %lld names triangle %lld of %lld", (long long)i, (long long)star_tri[i], (long long)n_tris);
        t32[i] = (int)tris[i];
        s32[i] = (int)star_tri[i];
    }
    for (int64_t v = 0; v <= n_loc; ++v) p32[v] = (int)star_ptr[v];
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    ctx->om_verts = 0;
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->om_tris, (size_t)3 * n_tris + 1))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->om_star, (size_t)3 * n_tris + 1))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->om_ptr, (size_t)n_loc + 1))) return rc;
    if (n_tris) {
        ASB_HIP(ctx, hipMemcpyAsync(ctx->om_tris, t32.data(), t32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ASB_HIP(ctx, hipMemcpyAsync(ctx->om_star, s32.data(), s32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    ASB_HIP(ctx, hipMemcpyAsync(ctx->om_ptr, p32.data(), p32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the staging vectors die here)
    ctx->om_verts = n_loc;
    return ASB_OK;
}

extern "C" int asb_onmesh_run(asb_ctx* ctx, int which, int64_t r, int64_t f0, int64_t f1, int64_t fj, int want_normals,
                              const double* inv_massL, int add_mean, double psf, double denom, double* accum_norm_out,
                              double* mesh_num_out, double* mesh_den_out, double* accum_angle_out, double* stats_out,
                              double* frame_err_out, double* angle_out) {
    if (!ctx || !ctx->X || !ctx->comps || r < 0) return ASB_ERR_ARG;
    RcOperands o;
    int rc;
    if ((rc = asb_recon_operands(ctx, "asb_onmesh_run", "r", which, r, &o))) return rc;
    if (f0 < 0 || f1 > o.F || f0 >= f1 || fj < 1)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_run: range(%lld, %lld, %lld) is not a selection of the %d frames", (long long)f0,
                 (long long)f1, (long long)fj, o.F);
    if (add_mean && !ctx->have_mean) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_run: no mean on the device");
    if (!(psf > 0.0) || !(denom > 0.0)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_run: scale %g, denominator %g", psf, denom);
    if (want_normals && ctx->om_verts != ctx->n_loc) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_onmesh_run: no mesh for this shard (asb_onmesh_mesh)");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long n_loc = ctx->n_loc, ldb = 3 * n_loc;
    const int n_sel = (int)((f1 - f0 + fj - 1) / fj);
    const int tile0 = (int)(f0 / OM_TILE), n_tiles = (int)((f1 - 1) / OM_TILE) - tile0 + 1;
    const long long n_vg = (n_loc + OM_VT - 1) / OM_VT;
    long long gx = (n_vg + OM_WAVES - 1) / OM_WAVES;
    const long long gx_cap = 8LL * ctx->n_cu / n_tiles > 1 ? 8LL * ctx->n_cu / n_tiles : 1;
    if (gx > gx_cap) gx = gx_cap;
    const long long nblk = gx * n_tiles;
    long long gn = (n_loc + OM_WAVES - 1) / OM_WAVES;                 // blocks of the normal pass
    if (gn > 8LL * ctx->n_cu) gn = 8LL * ctx->n_cu;
    const double inv_psf = 1.0 / psf;
    const double* mean = add_mean ? ctx->mean : nullptr;
    if ((rc = asb_alloc(ctx, &ctx->om_vpart, (size_t)n_tiles * n_loc))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->om_fpart, (size_t)nblk * 2 * OM_TILE))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->om_spart, (size_t)(nblk + gn) * 3))) return rc;
    // results: accum_norm (n_loc) | accum_angle (n_loc) | numerators (n_sel) | denominators (n_sel) | statistics (10)
    const size_t n_out = (size_t)2 * n_loc + 2 * n_sel + 10;
    if ((rc = asb_alloc(ctx, &ctx->om_out, n_out))) return rc;
    double* d_an = ctx->om_out;
    double* d_aa = d_an + n_loc;
    double* d_num = d_aa + n_loc;
    double* d_den = d_num + n_sel;
    double* d_st = d_den + n_sel;
    if (inv_massL) {
        if ((rc = asb_alloc(ctx, &ctx->om_invm, (size_t)n_loc))) return rc;
        ASB_HIP(ctx, hipMemcpyAsync(ctx->om_invm, inv_massL + ctx->v0, (size_t)n_loc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    const double* invm = inv_massL ? ctx->om_invm : nullptr;
    double *d_fe = nullptr, *d_ang = nullptr;
    if (frame_err_out) {
        if ((rc = asb_alloc(ctx, &ctx->om_fe, (size_t)n_sel * n_loc))) return rc;
        d_fe = ctx->om_fe;
    }
    if (angle_out && want_normals) {
        if ((rc = asb_alloc(ctx, &ctx->om_ang, (size_t)n_sel * n_loc))) return rc;
        d_ang = ctx->om_ang;
    }

    hipLaunchKernelGGL(k_onmesh_err, dim3((unsigned)gx, (unsigned)n_tiles), dim3(64 * OM_WAVES), 0, ctx->stream, o.T, o.ldt, o.F, n_loc, o.A,
                       o.lda, o.B, ldb, (int)r, mean, invm, inv_psf, denom, (int)f0, (int)f1, (int)fj, tile0, ctx->om_vpart, ctx->om_fpart,
                       ctx->om_spart, d_fe);
    hipLaunchKernelGGL(k_onmesh_frames, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0, ctx->stream, ctx->om_fpart, (int)gx, tile0,
                       (int)f0, (int)fj, n_sel, d_num, d_den);
    hipLaunchKernelGGL(k_onmesh_verts, dim3((unsigned)((n_loc + 255) / 256)), dim3(256), 0, ctx->stream, ctx->om_vpart, n_tiles, n_loc,
                       d_an);
    hipLaunchKernelGGL(k_onmesh_stats, dim3(1), dim3(256), 0, ctx->stream, d_an, n_loc, ctx->om_spart, nblk, d_st);
    ASB_CHECK_LAUNCH(ctx);

    if (want_normals) {
        // chunk width: whole 128-byte lines per row, the scratch within OM_SCRATCH_BYTES (16 frames at least), whole waves if it can
        long long cw = (long long)(OM_SCRATCH_BYTES / (24ull * (unsigned long long)n_loc));
        cw = cw >= 64 ? cw / 64 * 64 : (cw >= 16 ? cw / 16 * 16 : 16);
        const long long span = (f1 - f0 + 15) / 16 * 16;
        if (cw > span) cw = span;
        if ((rc = asb_alloc(ctx, &ctx->om_scratch, (size_t)3 * n_loc * cw))) return rc;
        double* sp = ctx->om_spart + nblk * 3;
        const long long n_units = (n_loc + OM_FV - 1) / OM_FV * ((cw + 63) / 64);
        long long gf = (n_units + OM_WAVES - 1) / OM_WAVES;
        if (gf > 8LL * ctx->n_cu) gf = 8LL * ctx->n_cu;
        int first = 1;
        for (long long c0 = f0; c0 < f1; c0 += cw) {
            const long long c1 = c0 + cw < f1 ? c0 + cw : f1;
            hipLaunchKernelGGL(k_onmesh_fill, dim3((unsigned)gf), dim3(64 * OM_WAVES), 0, ctx->stream, o.A, o.lda, o.B, ldb, (int)r, n_loc,
                               (int)c0, (int)c1, (int)cw, ctx->om_scratch);
            hipLaunchKernelGGL(k_onmesh_normals, dim3((unsigned)gn), dim3(64 * OM_WAVES), 0, ctx->stream, o.T, o.ldt, ctx->om_scratch, (int)cw,
                               (int)c0, (int)c1, n_loc, ctx->om_tris, ctx->om_ptr, ctx->om_star, mean, invm, inv_psf, (int)f0, (int)f1,
                               (int)fj, first, d_aa, sp, d_ang);
            first = 0;
        }
        hipLaunchKernelGGL(k_onmesh_stats, dim3(1), dim3(256), 0, ctx->stream, d_aa, n_loc, sp, gn, d_st + 5);
        ASB_CHECK_LAUNCH(ctx);
    }

    std::vector<double> h(n_out);
    ASB_HIP(ctx, hipMemcpyAsync(h.data(), ctx->om_out, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (frame_err_out)
        ASB_HIP(ctx, hipMemcpyAsync(frame_err_out, d_fe, (size_t)n_sel * n_loc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (d_ang)
        ASB_HIP(ctx, hipMemcpyAsync(angle_out, d_ang, (size_t)n_sel * n_loc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (long long v = 0; v < n_loc; ++v) {
        if (accum_norm_out) accum_norm_out[v] = h[v];
        if (accum_angle_out && want_normals) accum_angle_out[v] = h[n_loc + v];
    }
    for (int s = 0; s < n_sel; ++s) {
        if (mesh_num_out) mesh_num_out[s] = h[2 * n_loc + s];
        if (mesh_den_out) mesh_den_out[s] = h[2 * n_loc + n_sel + s];
    }
    if (stats_out)
        for (int i = 0; i < 10; ++i) stats_out[i] = (i < 5 || want_normals) ? h[2 * n_loc + 2 * n_sel + i] : NAN;
    return ASB_OK;
}
