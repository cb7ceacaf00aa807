// Snapshot ingest: rigid Procrustes alignment of every frame to frame 0 -- utils/process.py:210-250
// (find_rbm_procrustes + transform inside align) of the reference.  gfx950 only.
//
// Frames arrive in the reference layout (F, N, 3).  One block per frame: centroid of the frame and of
// frame 0, the 3x3 cross-covariance M = (to - t1)^T (from - t0), its rotation R = U V^T (procrustes_rot of
// asb_kernels.h: one-sided Jacobi on M itself, R *= -1 when M has full rank and det < 0, as the reference does; the
// proper rotation where a flat frame leaves M with rank < 3), then v' = R v + (t1 - R t0).  Arithmetic in f64 (the
// reference works in f32 on the h5 data and stores f32).
#include "asb_kernels.h"

// T (F, 4, 4) row-major homogeneous matrices; frames (F, N, 3)
__global__ __launch_bounds__(256) void k_procrustes(const double* __restrict__ frames, long long N, int rigid,
                                                    double* __restrict__ T) {
    __shared__ double sh[15 * 4];
    const double* fr = frames + (long long)blockIdx.x * N * 3;
    const double* f0 = frames;
    // pass 1: centroids
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (long long v = threadIdx.x; v < N; v += blockDim.x) {
        s[0] += fr[3 * v]; s[1] += fr[3 * v + 1]; s[2] += fr[3 * v + 2];
        s[3] += f0[3 * v]; s[4] += f0[3 * v + 1]; s[5] += f0[3 * v + 2];
    }
    block_sum<6>(s, sh);
    double t0[3] = {s[0] / N, s[1] / N, s[2] / N}, t1[3] = {s[3] / N, s[4] / N, s[5] / N};
    // pass 2: M[a][b] = sum (to_a - t1_a)(from_b - t0_b)
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long v = threadIdx.x; v < N; v += blockDim.x) {
        const double p0 = fr[3 * v] - t0[0], p1 = fr[3 * v + 1] - t0[1], p2 = fr[3 * v + 2] - t0[2];
        const double q0 = f0[3 * v] - t1[0], q1 = f0[3 * v + 1] - t1[1], q2 = f0[3 * v + 2] - t1[2];
        m[0] += q0 * p0; m[1] += q0 * p1; m[2] += q0 * p2;
        m[3] += q1 * p0; m[4] += q1 * p1; m[5] += q1 * p2;
        m[6] += q2 * p0; m[7] += q2 * p1; m[8] += q2 * p2;
    }
    __syncthreads();
    block_sum<9>(m, sh);
    if (threadIdx.x != 0) return;
    double R[3][3];
    procrustes_rot(m, R);
    double* Tm = T + (long long)blockIdx.x * 16;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) Tm[4 * a + b] = rigid ? R[a][b] : (a == b ? 1.0 : 0.0);
        Tm[4 * a + 3] = t1[a] - (R[a][0] * t0[0] + R[a][1] * t0[1] + R[a][2] * t0[2]);     // (:232) uses R either way
    }
    Tm[12] = 0; Tm[13] = 0; Tm[14] = 0; Tm[15] = 1;
}

__global__ __launch_bounds__(256) void k_apply_rbm(double* __restrict__ frames, long long N, const double* __restrict__ T) {
    const double* Tm = T + (long long)blockIdx.y * 16;
    double* fr = frames + (long long)blockIdx.y * N * 3;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += (long long)gridDim.x * blockDim.x) {
        const double x = fr[3 * v], y = fr[3 * v + 1], z = fr[3 * v + 2];
        fr[3 * v] = Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3];
        fr[3 * v + 1] = Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7];
        fr[3 * v + 2] = Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11];
    }
}

// frames: host (F, N, 3) float64, aligned in place; T_out (optional, host F x 16): the rigid-body matrices
extern "C" int asb_align_frames(asb_ctx* ctx, double* frames, int64_t F, int64_t N, int rigid, double* T_out) {
    if (!ctx || !frames || F < 1 || N < 1) return ASB_ERR_ARG;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<double> d, T;
    const size_t bytes = (size_t)F * N * 3 * sizeof(double);
    int rc;
    if ((rc = d.alloc(ctx, (size_t)F * N * 3))) return rc;
    if ((rc = T.alloc(ctx, (size_t)F * 16))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(d.get(), frames, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_procrustes, dim3((unsigned)F), dim3(256), 0, ctx->stream, d.get(), (long long)N, rigid, T.get());
    long long bx = (N + 255) / 256;
    hipLaunchKernelGGL(k_apply_rbm, dim3((unsigned)(bx < 1024 ? bx : 1024), (unsigned)F), dim3(256), 0, ctx->stream, d.get(),
                       (long long)N, T.get());
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipMemcpyAsync(frames, d.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (T_out) ASB_HIP(ctx, hipMemcpyAsync(T_out, T.get(), (size_t)F * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

// procrustes_rot on the host: m9 = M row-major -> out9 = R row-major
extern "C" void asb_test_procrustes_rot(const double* m9, double* out9) {
    double R[3][3];
    procrustes_rot(m9, R);
    for (int i = 0; i < 9; ++i) out9[i] = R[i / 3][i % 3];
}
