// The product tile of the global step, shared by k_gstep_gemm (asb_gstep.hip) and k_pdsolve_gemm (asb_pdsolve.hip): the
// contraction of one block of 4 waves -- 64 frames x 32 vertices x 3 coordinates, every entry ONE accumulator summed over
// ascending n -- and the frame-major epilogue.  Both kernels run exactly this loop, so their entries have the same bits.
#pragma once
#include "asb_common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define GS_TF 64            // frames per block of k_gstep_gemm (16 per wave)
#define GS_TN 32            // vertices per block
#define GS_KC 16            // values of n per LDS stage
#define GS_LDR 49           // LDS row of the rhs stage: 48 doubles + 1 (the 16 frames of an MFMA operand fall into different banks)
#define GS_LDB 48           // LDS row of the A^-1 stage: 32 doubles + 16 (the four k-rows of an operand fall into different bank halves)
#define GS_R_STAGE (GS_TF * GS_LDR)
#define GS_B_STAGE (GS_KC * GS_LDB)
#define GS_SM (2 * GS_R_STAGE + 2 * GS_B_STAGE)       // doubles of LDS a block needs

// acc[d][y][q] of lane (i, g) = lane & 15, lane >> 4 of wave w: frame t0 + 16 w + g + 4 q, vertex m0 + 16 y + i, coordinate d.
// rhs (F, n, 3) frame-major; Ainv (np x np), only its n x n block is read; loads past n or past F are zero-filled.  Ends
// behind a barrier: every wave is past its last read of sm.
__device__ __forceinline__ void gs_contract(const double* __restrict__ rhs, const double* __restrict__ Ainv, int n, int np, long long F,
                                            int m0, long long t0, double* sm, d4 (&acc)[3][2]) {
    constexpr int R_STAGE = GS_R_STAGE, B_STAGE = GS_B_STAGE;
    double* Rs = sm;
    double* Bs = sm + 2 * R_STAGE;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long row_len = 3LL * n;
    // this thread's share of a stage: 12 doubles of rhs (frame fr[q], column cr[q] of the 48), 2 of A^-1 (row kb[q], column mb)
    double rr[12], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const int e = tid + 256 * q, fl = e / 48, c = e % 48;
            const long long f = t0 + fl, col = 3LL * k0 + c;
            rr[q] = (f < F && col < row_len) ? rhs[f * row_len + col] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q, k = k0 + e / GS_TN, m = m0 + e % GS_TN;
            rb[q] = (k < n && m < n) ? Ainv[(long long)k * np + m] : 0.0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const int e = tid + 256 * q;
            Rs[buf * R_STAGE + (e / 48) * GS_LDR + e % 48] = rr[q];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q;
            Bs[buf * B_STAGE + (e / GS_TN) * GS_LDB + e % GS_TN] = rb[q];
        }
    };
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[d][y] = d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    stash(0);
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < n; k0 += GS_KC) {
        const bool more = k0 + GS_KC < n;
        if (more) fetch(k0 + GS_KC);
        const double* ra = Rs + cur * R_STAGE + (wave * 16 + i) * GS_LDR;
        const double* bb = Bs + cur * B_STAGE + i;
#pragma unroll
        for (int ks = 0; ks < GS_KC / 4; ++ks) {
            const int k = ks * 4 + g;
            const double b0 = bb[k * GS_LDB], b1 = bb[k * GS_LDB + 16];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double a = ra[k * 3 + d];
                acc[d][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[d][0], 0, 0, 0);
                acc[d][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[d][1], 0, 0, 0);
            }
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
}

// The tile written frame-major: out (F, n, 3).  The operand buffers are dead (the barrier gs_contract ends with, or the
// caller's) and become the output stage: LDS rows of 97 doubles, 96 contiguous doubles per frame.
__device__ __forceinline__ void gs_store_fm(const d4 (&acc)[3][2], double* sm, int n, long long F, int m0, long long t0,
                                            double* __restrict__ out) {
    constexpr int RUN = GS_TN * 3, ROW = RUN + 1;
    static_assert(2 * GS_R_STAGE >= GS_TF * ROW, "the epilogue reuses the rhs buffers");
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long row_len = 3LL * n;
    // accumulator q of lane (i, g): frame g + 4 q of the wave's 16, vertex i of the 16
    double* stage = sm;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) stage[(wave * 16 + g + 4 * q) * ROW + (16 * y + i) * 3 + d] = acc[d][y][q];
    __syncthreads();
    const int nv = n - m0 < GS_TN ? n - m0 : GS_TN;
    const int nf = F - t0 < GS_TF ? (int)(F - t0) : GS_TF;
    const int run = nv * 3;
    for (int e = tid; e < GS_TF * RUN; e += 256) {
        const int fl = e / RUN, k = e % RUN;
        if (fl < nf && k < run) out[(t0 + fl) * row_len + 3LL * m0 + k] = stage[fl * ROW + k];
    }
}

