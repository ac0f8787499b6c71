// Nearest registered facial ID (reference face_identification.py:1117-1127, FaceIdentifier.test): for every query ID the
// registry row at the smallest Euclidean distance, np.argmin's choice among equal distances (the lowest index).
//
// Exact by construction: each (query, row) distance is sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64
// differences (no FMA contraction: -ffp-contract=off), and the reduction is the minimum of (distance, index) under the
// lexicographic order -- a total order, so its minimum does not depend on how rows are split over lanes, waves and workgroups, or
// on which other queries share a launch.  No atomics.
//
// Work: n * m * 64 * 3 fp64 vector ops (5.0 G at n = 3 000, m = 8 631: ~0.15 ms at the fp64 vector rate), the registry
// (m * 256 B, 2.2 MB at 8 631 rows) re-read from L2 by every workgroup.  Not the bottleneck of identification (one crop's
// extraction costs more than the whole match of a frame batch), so the kernel stays on the vector units; an MFMA form
// (|q|^2 + |r|^2 - 2 q.r) would give up the exact tie behaviour.
#include "block_ops.h"
#include <climits>

namespace {

constexpr int FM_DIM = 64;
constexpr int FM_THREADS = 256;

// QB queries per workgroup (staged in LDS, read as broadcasts); thread t scans registry rows t, t + 256, ... (16 float4 loads
// per row), keeping the best (distance, index) per query under lex_less (np.argmin's order); then a wave butterfly and the four
// waves in LDS.
template <int QB>
__global__ __launch_bounds__(FM_THREADS) void fid_match_kernel(const float* __restrict__ Q, int n, const float* __restrict__ R, int m,
                                                               int* __restrict__ best_index, double* __restrict__ best_dist) {
    __shared__ __attribute__((aligned(16))) float qs[QB][FM_DIM];
    __shared__ double wd[FM_THREADS / 64][QB];
    __shared__ int wi[FM_THREADS / 64][QB];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * QB;
    for (int i = tid; i < QB * FM_DIM; i += FM_THREADS) {
        const int q = i / FM_DIM, k = i % FM_DIM;
        qs[q][k] = q0 + q < n ? Q[(size_t)(q0 + q) * FM_DIM + k] : 0.f;
    }
    __syncthreads();
    double bd[QB];
    int bi[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) { bd[q] = __builtin_inf(); bi[q] = INT_MAX; }
    for (int r = tid; r < m; r += FM_THREADS) {
        const float4* rp = reinterpret_cast<const float4*>(R + (size_t)r * FM_DIM);
        double s[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q) s[q] = 0.0;
        // k is the outer loop and only partly unrolled: the query values are re-read from LDS per row instead of being hoisted
        // into (QB x 64 fp64) registers
#pragma unroll 2
        for (int k4 = 0; k4 < FM_DIM / 4; ++k4) {
            const float4 v = rp[k4];
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const float4 x = *reinterpret_cast<const float4*>(&qs[q][4 * k4]);
                double d;
                d = (double)x.x - (double)v.x; s[q] += d * d;
                d = (double)x.y - (double)v.y; s[q] += d * d;
                d = (double)x.z - (double)v.z; s[q] += d * d;
                d = (double)x.w - (double)v.w; s[q] += d * d;
            }
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const double dist = sqrt(s[q]);
            if (lex_less()(dist, r, bd[q], bi[q])) { bd[q] = dist; bi[q] = r; }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < QB; ++q) {
        double d = bd[q];
        int i = bi[q];
        fv_wave_best<lex_less>(d, i);
        if (lane == 0) { wd[wave][q] = d; wi[wave][q] = i; }
    }
    __syncthreads();
    if (tid < QB && q0 + tid < n) {
        double d;
        int i;
        fv_block_best<lex_less, FM_THREADS / 64>(&wd[0][tid], &wi[0][tid], QB, d, i);
        best_index[q0 + tid] = i;
        best_dist[q0 + tid] = d;
    }
}

template <int QB>
int launch_match(fv_ctx* ctx, const float* Q, int n, const float* R, int m, int* best_index, double* best_dist) {
    FvProfScope ps(ctx, "fid_match_kernel", 3.0 * n * (double)m * FM_DIM, (double)(n + m) * FM_DIM * 4 + 12.0 * n);
    hipLaunchKernelGGL(fid_match_kernel<QB>, dim3((n + QB - 1) / QB), dim3(FM_THREADS), 0, ctx->stream, Q, n, R, m, best_index,
                       best_dist);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

}  // namespace

extern "C" int fv_fid_match(fv_ctx* ctx, const float* queries, int n, const float* registry, int m, int32_t* best_index,
                            double* best_dist) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, queries && registry && best_index && best_dist && n >= 1, "fid_match: bad arguments");
    FV_REQUIRE(ctx, m >= 1, "fid_match: the registry is empty");
    FV_REQUIRE(ctx, ((uintptr_t)registry & 15) == 0, "fid_match: registry must be 16-byte aligned");
    // queries per workgroup: one while that still fills the CUs, more to share each registry pass when n is large
    if (n >= 2048) return launch_match<8>(ctx, queries, n, registry, m, best_index, best_dist);
    if (n >= 512) return launch_match<4>(ctx, queries, n, registry, m, best_index, best_dist);
    return launch_match<1>(ctx, queries, n, registry, m, best_index, best_dist);
}
