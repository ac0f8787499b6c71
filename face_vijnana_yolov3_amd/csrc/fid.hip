// FaceIdentifier head kernels (reference face_identification.py:318-345, 72-76): Dense(64) over the flattened Darknet-53 feature
// map, ReLU, l2_normalize, the triplet loss and the dense layer's gradients.
//
// Every launch is memory-bound: the kernel [F][64] is 44.3 MB at F = 173 056 (416 x 416 images) and the rows are few (<= 3 x 96).
// They run as fp32 FMA on the vector units, not as v_mfma_f32_16x16x4_f32: with M <= 16 rows per tower an MFMA tile would be mostly
// padding, the byte traffic is the same either way, and the VALU form gives each output one plain sequential fp32 sum whose order
// is fixed by F alone.  No atomics anywhere: the forward sums its per-chunk partials in chunk order, the weight-gradient workgroups
// own whole kernel rows -- the same image gives the same facial ID bits in any batch.
#include "fid.h"

#include <cmath>

namespace {

constexpr int FWD_MT = 32;     // rows per forward workgroup
constexpr int DG_MT = 64;      // rows of dE per data-gradient LDS tile
constexpr int WG_MT = 32;      // rows per weight-gradient LDS tile
constexpr int WG_F = 64;       // kernel rows per weight-gradient workgroup

__device__ __forceinline__ const float* row_ptr(const FidRows& r, int m, long long F) {
    return r.p[m / r.per] + (long long)(m % r.per) * F;
}

// Y partial of chunk blockIdx.y, rows [blockIdx.x * 32, + 32): thread (n = tid & 63, k-lane kl = tid >> 6) sums its 64 k of the
// chunk for 32 rows; the four k-lanes are added in lane order.  X rows are staged in LDS (row-major, a wave reads one address:
// broadcast); W rows stream from global memory, 256 contiguous bytes per wave and k.
__global__ __launch_bounds__(256) void fid_dense_fwd_kernel(FidRows X, int M, long long F, const float* __restrict__ W,
                                                            float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float xs[FWD_MT][FID_KC];
    const int tid = threadIdx.x, n = tid & 63, kl = tid >> 6;
    const int m0 = blockIdx.x * FWD_MT;
    const long long k0 = (long long)blockIdx.y * FID_KC;
    for (int i = tid; i < FWD_MT * FID_KC / 4; i += 256) {
        const int r = i / (FID_KC / 4), k4 = i % (FID_KC / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m0 + r < M) v = *reinterpret_cast<const float4*>(row_ptr(X, m0 + r, F) + k0 + 4 * k4);
        *reinterpret_cast<float4*>(&xs[r][4 * k4]) = v;
    }
    __syncthreads();
    float acc[FWD_MT];
#pragma unroll
    for (int r = 0; r < FWD_MT; ++r) acc[r] = 0.f;
    const int kb = kl * (FID_KC / 4);
    const float* w = W + (k0 + kb) * FID_DIM + n;
    for (int k = 0; k < FID_KC / 4; k += 4) {
        const float w0 = w[(k + 0) * FID_DIM], w1 = w[(k + 1) * FID_DIM], w2 = w[(k + 2) * FID_DIM], w3 = w[(k + 3) * FID_DIM];
#pragma unroll
        for (int r = 0; r < FWD_MT; ++r) {
            const float4 x = *reinterpret_cast<const float4*>(&xs[r][kb + k]);
            acc[r] += x.x * w0; acc[r] += x.y * w1; acc[r] += x.z * w2; acc[r] += x.w * w3;
        }
    }
    __syncthreads();
    float* red = &xs[0][0];   // [4][FWD_MT][64] = 8192 floats = the whole tile
#pragma unroll
    for (int r = 0; r < FWD_MT; ++r) red[(kl * FWD_MT + r) * FID_DIM + n] = acc[r];
    __syncthreads();
    for (int i = tid; i < FWD_MT * FID_DIM; i += 256) {
        const int r = i / FID_DIM;
        if (m0 + r >= M) break;
        const float s = ((red[i] + red[FWD_MT * FID_DIM + i]) + red[2 * FWD_MT * FID_DIM + i]) + red[3 * FWD_MT * FID_DIM + i];
        part[((long long)blockIdx.y * M + m0) * FID_DIM + i] = s;
    }
}

// one workgroup per row: wave g sums the partials of chunks [g * n / 16, (g + 1) * n / 16) in order (fp64), wave 0 adds the 16 sums
// in wave order, + bias, ReLU, x * rsqrt(max(sum x^2, 1e-12)) (TF 1.13 l2_normalize).  The order depends on the chunk count alone.
constexpr int FIN_WAVES = 16;
__global__ __launch_bounds__(64 * FIN_WAVES) void fid_dense_finish_kernel(const float* __restrict__ part, long long chunks, int M,
                                                                         const float* __restrict__ bias, float* __restrict__ pre,
                                                                         float* __restrict__ u) {
    __shared__ double s_part[FIN_WAVES][FID_DIM];
    const int m = blockIdx.x, n = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long c0 = g * chunks / FIN_WAVES, c1 = (g + 1) * chunks / FIN_WAVES;
    double s = 0.0;
#pragma unroll 8
    for (long long c = c0; c < c1; ++c) s += (double)part[(c * M + m) * FID_DIM + n];
    s_part[g][n] = s;
    __syncthreads();
    if (g) return;
    s = 0.0;
#pragma unroll
    for (int k = 0; k < FIN_WAVES; ++k) s += s_part[k][n];
    const float y = (float)s + bias[n];
    const float r = y > 0.f ? y : 0.f;
    const double ss = fv_wave_sum_all((double)r * (double)r);
    const double inv = 1.0 / sqrt(ss > 1e-12 ? ss : 1e-12);
    if (pre) pre[(long long)m * FID_DIM + n] = y;
    u[(long long)m * FID_DIM + n] = (float)((double)r * inv);
}

// Triplet loss mean_b max(|a - p| - |a - n| + 0.2, 0) (fi.py:72-76) and its gradient.  Wave w takes the triplets b = w, w + 4, ...
// (lane = column); max passes the gradient where its argument is >= 0 (TF's MaximumGrad); the gradient of a distance that is
// exactly 0 is defined as 0 (TF's sqrt gradient is NaN there).  Sums: per wave in b order, then the four waves in order.
// loss_weight (a data-parallel slice's share of the merged batch) scales dE where it is stored; dbias sums the stored rows in
// fp64, so it carries the same factor.  The loss is this call's own mean, unweighted.
__global__ __launch_bounds__(256) void fid_triplet_kernel(const float* __restrict__ pre, const float* __restrict__ u, int B,
                                                          float* __restrict__ loss, float* __restrict__ dE, float* __restrict__ dbias,
                                                          double loss_weight) {
    __shared__ double s_loss[4], s_db[4][FID_DIM];
    const int n = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double lsum = 0.0, db = 0.0;
    for (int b = wv; b < B; b += 4) {
        const long long ra = (long long)b * FID_DIM + n, rp = ra + (long long)B * FID_DIM, rn = rp + (long long)B * FID_DIM;
        // differences in fp64 (exact): an fp32 difference is off by 2^-24 of itself, and where a row's gradient nearly cancels in
        // the projection of l2_relu_bwd that rounding came out many times larger than 2^-24 of the result
        const double dap = (double)u[ra] - (double)u[rp], dan = (double)u[ra] - (double)u[rn];
        const double dp = sqrt(fv_wave_sum_all(dap * dap)), dn = sqrt(fv_wave_sum_all(dan * dan));
        const double h = dp - dn + 0.2;
        lsum += h > 0.0 ? h : 0.0;
        double ga = 0.0, gp = 0.0, gn = 0.0;
        if (h >= 0.0) {
            const double cp = dp > 0.0 ? 1.0 / ((double)B * dp) : 0.0, cn = dn > 0.0 ? 1.0 / ((double)B * dn) : 0.0;
            ga = cp * dap - cn * dan; gp = -cp * dap; gn = cn * dan;
        }
        const float ea = l2_relu_bwd(pre[ra], ga, loss_weight), ep = l2_relu_bwd(pre[rp], gp, loss_weight),
                    en = l2_relu_bwd(pre[rn], gn, loss_weight);
        dE[ra] = ea; dE[rp] = ep; dE[rn] = en;
        db += ((double)ea + (double)ep) + (double)en;
    }
    s_db[wv][n] = db;
    if (n == 0) s_loss[wv] = lsum;
    __syncthreads();
    if (threadIdx.x < FID_DIM) dbias[n] = (float)(((s_db[0][n] + s_db[1][n]) + s_db[2][n]) + s_db[3][n]);
    if (threadIdx.x == 0) *loss = (float)((((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3]) / (double)B);
}

// dX[m][f] = sum_n dE[m][n] W[f][n] (+ bias[f], added last): a thread owns one f (its kernel row in 64 registers) and walks the
// rows of dE, staged in LDS.
template <bool BIAS>
__device__ __forceinline__ void dense_dgrad_body(const float* __restrict__ dE, int M, long long F, const float* __restrict__ W,
                                                 const float* __restrict__ bias, const FidRows& dX) {
    __shared__ __attribute__((aligned(16))) float es[DG_MT][FID_DIM];
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    const float bf = BIAS ? bias[f] : 0.f;
    float w[FID_DIM];
#pragma unroll
    for (int q = 0; q < FID_DIM / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(W + f * FID_DIM + 4 * q);
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    for (int m0 = 0; m0 < M; m0 += DG_MT) {
        const int mt = M - m0 < DG_MT ? M - m0 : DG_MT;
        __syncthreads();
        for (int i = threadIdx.x; i < mt * FID_DIM; i += 256) es[i / FID_DIM][i % FID_DIM] = dE[(long long)m0 * FID_DIM + i];
        __syncthreads();
        for (int r = 0; r < mt; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < FID_DIM / 4; ++q) {
                const float4 e = *reinterpret_cast<const float4*>(&es[r][4 * q]);
                acc += e.x * w[4 * q]; acc += e.y * w[4 * q + 1]; acc += e.z * w[4 * q + 2]; acc += e.w * w[4 * q + 3];
            }
            const int m = m0 + r;
            dX.p[m / dX.per][(long long)(m % dX.per) * F + f] = BIAS ? acc + bf : acc;
        }
    }
}

__global__ __launch_bounds__(256) void fid_dense_dgrad_kernel(const float* __restrict__ dE, int M, long long F, const float* __restrict__ W,
                                                              FidRows dX) {
    dense_dgrad_body<false>(dE, M, F, W, nullptr, dX);
}

// The reconstruction model's dense layer (reference face_identification.py:1171-1180): x[m][f] = sum_n u[m][n] K[f][n] + b[f] -- the
// data-gradient's product with u in the place of dE, the same sequential sum over n, the bias added last.
__global__ __launch_bounds__(256) void fid_dense_bias_kernel(const float* __restrict__ u, int M, long long F, const float* __restrict__ W,
                                                             const float* __restrict__ bias, FidRows X) {
    dense_dgrad_body<true>(u, M, F, W, bias, X);
}

// u = relu(l2_normalize(ids)) over the 64 values of a row (x * rsqrt(max(sum x^2, 1e-12)), TF 1.13): one wave per row, the sum of
// squares by an xor butterfly -- one fixed order, the same in every lane.
__global__ __launch_bounds__(256) void fid_ids_l2_relu_kernel(const float* __restrict__ ids, int M, float* __restrict__ u) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), n = threadIdx.x & 63;
    const float v = m < M ? ids[(long long)m * FID_DIM + n] : 0.f;
    const float s = fv_wave_sum(v * v);
    const float r = v * (1.0f / sqrtf(fmaxf(s, 1e-12f)));
    if (m < M) u[(long long)m * FID_DIM + n] = r > 0.f ? r : 0.f;
}

// dW[f][n] = sum_m X[m][f] dE[m][n] in row order: workgroup = 64 kernel rows, thread (n = tid & 63, g = tid >> 6) owns the 16 rows
// f0 + 16 g .. + 15 of column n.  Every element is written once.
__global__ __launch_bounds__(256) void fid_dense_wgrad_kernel(FidRows X, const float* __restrict__ dE, int M, long long F,
                                                              float* __restrict__ dW) {
    __shared__ __attribute__((aligned(16))) float xs[WG_MT][WG_F];
    __shared__ float es[WG_MT][FID_DIM];
    const int tid = threadIdx.x, n = tid & 63, g = tid >> 6;
    const long long f0 = (long long)blockIdx.x * WG_F;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int m0 = 0; m0 < M; m0 += WG_MT) {
        const int mt = M - m0 < WG_MT ? M - m0 : WG_MT;
        __syncthreads();
        for (int i = tid; i < mt * WG_F; i += 256) {
            const int r = i / WG_F, c = i % WG_F;
            xs[r][c] = row_ptr(X, m0 + r, F)[f0 + c];
            es[r][c] = dE[(long long)(m0 + r) * FID_DIM + c];
        }
        __syncthreads();
        for (int r = 0; r < mt; ++r) {
            const float e = es[r][n];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 x = *reinterpret_cast<const float4*>(&xs[r][16 * g + 4 * q]);
                acc[4 * q] += x.x * e; acc[4 * q + 1] += x.y * e; acc[4 * q + 2] += x.z * e; acc[4 * q + 3] += x.w * e;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dW[(f0 + 16 * g + i) * FID_DIM + n] = acc[i];
}

bool rows_ok(const FidRows& r, int M) {
    if (r.per < 1 || M < 1 || M > 3 * r.per) return false;
    for (int t = 0; t * r.per < M; ++t) if (!r.p[t]) return false;
    return true;
}

}  // namespace

int fv_fid_dense_fwd(fv_ctx* ctx, FidRows X, int M, long long F, const float* W, float* part) {
    FV_REQUIRE(ctx, F > 0 && F % FID_KC == 0 && rows_ok(X, M) && W && part, "fid_dense_fwd: F must be a positive multiple of %d", FID_KC);
    const long long chunks = fv_fid_chunks(F);
    FV_REQUIRE(ctx, chunks <= 65535, "fid_dense_fwd: F too large");
    FvProfScope ps(ctx, "fid_dense_fwd_kernel", 2.0 * M * F * FID_DIM,
                   4.0 * ((double)F * FID_DIM * ((M + FWD_MT - 1) / FWD_MT) + (double)M * F + (double)chunks * M * FID_DIM));
    hipLaunchKernelGGL(fid_dense_fwd_kernel, dim3((M + FWD_MT - 1) / FWD_MT, (unsigned)chunks), dim3(256), 0, ctx->stream, X, M, F, W, part);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

int fv_fid_dense_finish(fv_ctx* ctx, const float* part, long long chunks, int M, const float* bias, float* pre, float* u) {
    FV_REQUIRE(ctx, part && bias && u && M >= 1 && chunks >= 1, "fid_dense_finish: bad arguments");
    FvProfScope ps(ctx, "fid_dense_finish_kernel", 0.0, 4.0 * ((double)chunks * M * FID_DIM + 2.0 * M * FID_DIM));
    hipLaunchKernelGGL(fid_dense_finish_kernel, dim3(M), dim3(64 * FIN_WAVES), 0, ctx->stream, part, chunks, M, bias, pre, u);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

int fv_fid_triplet(fv_ctx* ctx, const float* pre, const float* u, int B, float* loss, float* dE, float* dbias, double loss_weight) {
    FV_REQUIRE(ctx, pre && u && loss && dE && dbias && B >= 1, "fid_triplet: bad arguments");
    FV_REQUIRE(ctx, std::isfinite(loss_weight) && loss_weight > 0.0, "fid_triplet: loss_weight must be finite and > 0");
    FvProfScope ps(ctx, "fid_triplet_kernel", 0.0, 4.0 * 9.0 * B * FID_DIM);
    hipLaunchKernelGGL(fid_triplet_kernel, dim3(1), dim3(256), 0, ctx->stream, pre, u, B, loss, dE, dbias, loss_weight);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

int fv_fid_dense_dgrad(fv_ctx* ctx, const float* dE, int M, long long F, const float* W, FidRows dX) {
    FV_REQUIRE(ctx, F > 0 && F % FID_KC == 0 && rows_ok(dX, M) && dE && W, "fid_dense_dgrad: F must be a positive multiple of %d", FID_KC);
    FvProfScope ps(ctx, "fid_dense_dgrad_kernel", 2.0 * M * F * FID_DIM, 4.0 * ((double)F * FID_DIM + (double)M * F));
    hipLaunchKernelGGL(fid_dense_dgrad_kernel, dim3((unsigned)(F / 256)), dim3(256), 0, ctx->stream, dE, M, F, W, dX);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

int fv_fid_recon_head(fv_ctx* ctx, const float* ids, int M, long long F, const float* W, const float* bias, float* u, float* x) {
    FV_REQUIRE(ctx, ids && W && bias && u && x, "fid_recon_head: NULL buffer");
    FV_REQUIRE(ctx, M >= 1 && F > 0 && F % FID_KC == 0, "fid_recon_head: needs rows >= 1 and F a positive multiple of %d (rows=%d, F=%lld)",
               FID_KC, M, F);
    {
        FvProfScope ps(ctx, "fid_ids_l2_relu_kernel", 0.0, 8.0 * M * FID_DIM);
        hipLaunchKernelGGL(fid_ids_l2_relu_kernel, dim3((M + 3) / 4), dim3(256), 0, ctx->stream, ids, M, u);
        FV_LAUNCH_CHECK(ctx);
    }
    FvProfScope ps(ctx, "fid_dense_bias_kernel", 2.0 * M * F * FID_DIM, 4.0 * ((double)F * (FID_DIM + 1) + (double)M * F));
    hipLaunchKernelGGL(fid_dense_bias_kernel, dim3((unsigned)(F / 256)), dim3(256), 0, ctx->stream, (const float*)u, M, F, W, bias,
                       FidRows{{x, nullptr, nullptr}, M});
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

int fv_fid_dense_wgrad(fv_ctx* ctx, FidRows X, const float* dE, int M, long long F, float* dW) {
    FV_REQUIRE(ctx, F > 0 && F % FID_KC == 0 && rows_ok(X, M) && dE && dW, "fid_dense_wgrad: F must be a positive multiple of %d", FID_KC);
    FvProfScope ps(ctx, "fid_dense_wgrad_kernel", 2.0 * M * F * FID_DIM, 4.0 * ((double)F * FID_DIM + (double)M * F));
    hipLaunchKernelGGL(fid_dense_wgrad_kernel, dim3((unsigned)(F / WG_F)), dim3(256), 0, ctx->stream, X, dE, M, F, dW);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
