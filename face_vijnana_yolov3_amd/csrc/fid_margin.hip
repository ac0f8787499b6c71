// Additive-margin softmax over the subjects (CosFace: Wang et al. 2018; ArcFace: Deng et al. 2019) on M <= 1024 labelled rows of
// facial IDs and a class kernel W [C][64], C <= 32768.  include/fv_hotpath.h (fv_fid_margin_softmax_loss_grad) has the contract.
// Everything is fp64 FMA on the vector units; every sum has a fixed order and one writer (no atomics): the same inputs give the
// same bits.
//
// Six launches over a caller-provided workspace: Z [M][ldz] doubles (ldz = C rounded up to 2: rows stay 16-byte aligned), the
// dU partial slabs [chunks][M][64] doubles, the row losses [M] doubles.
//   cos     a workgroup per (64 classes, 16 rows): the W tile is read as float4, normalised in LDS (stage_w_tile), the 16 rows of u
//           likewise; thread (class, row group) keeps four rows' cosines and stores Z(i, c) = cos_ic.
//   row     one wave per row, four rows per workgroup, lanes over C two classes at a time (double2): argmax of the cosines, the
//           margin on the target, the row maximum, the sum of exponentials (butterflies), then Z(i, c) is overwritten by the
//           coefficient g_ic; cos_t, pred and the row's loss are stored.  A row without a class gets g = 0.
//   du      a workgroup per (256 classes, 16 rows): dU partial (i, k) = sum over the chunk's classes of g_ic w^_ck, stored into
//           its slab.
//   dw      a workgroup per 64 classes walks all M rows, 16 at a time: dW^_ck = sum_i g_ic u_ik in row order, then back through
//           the normalisation of the class row.
//   rows    one wave per row: the slabs summed in chunk order, back through l2_normalize and ReLU (l2_relu_bwd) -> dE.
//   finish  one workgroup: dbias = the column sums of the stored dE (four waves, a quarter of the rows each, combined in wave
//           order); the loss from the row losses.
#include "fid.h"

#include <cmath>

namespace {

constexpr int MS_CT = 64;                 // classes per tile
constexpr int MS_RT = 16;                 // rows per tile
constexpr int MS_LD = MS_CT + 1;          // leading dimension of the W tile in LDS: class-major reads hit 64 different banks
constexpr int MS_DU_TILES = 4;            // class tiles per dU slab
constexpr int MS_THREADS = 256;
constexpr int MS_ROW_WAVES = 4;

struct WTile {
    double w[MS_CT][MS_LD];               // w^ of the tile's classes (zero beyond C)
    double inv[MS_CT];                    // 1 / sqrt(sum w^2), or the constant 1e6
    int live[MS_CT];                      // sum w^2 > 1e-12
};

// The tile's class rows, read as float4 (a row is 256 contiguous bytes), normalised by the l2_normalize rule; ends with a barrier.
__device__ __forceinline__ void stage_w_tile(WTile& T, const float* __restrict__ W, int c0, int C) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MS_CT * FID_DIM / 4 / MS_THREADS; ++j) {
        const int idx = t + MS_THREADS * j, row = idx >> 4, k4 = (idx & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + row < C) v = *reinterpret_cast<const float4*>(W + (size_t)(c0 + row) * FID_DIM + k4);
        T.w[row][k4] = v.x; T.w[row][k4 + 1] = v.y; T.w[row][k4 + 2] = v.z; T.w[row][k4 + 3] = v.w;
    }
    __syncthreads();
    if (t < MS_CT) {
        double ss = 0.0;
#pragma unroll 8
        for (int k = 0; k < FID_DIM; ++k) ss = __builtin_fma(T.w[t][k], T.w[t][k], ss);
        T.live[t] = ss > 1e-12;
        T.inv[t] = ss > 1e-12 ? 1.0 / sqrt(ss) : 1e6;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MS_CT * FID_DIM / 4 / MS_THREADS; ++j) {
        const int idx = t + MS_THREADS * j, row = idx >> 4, k4 = (idx & 15) * 4;
        const double s = T.inv[row];
#pragma unroll
        for (int q = 0; q < 4; ++q) T.w[row][k4 + q] *= s;
    }
    __syncthreads();
}

// rows r0 .. r0 + 15 of u as doubles (zero beyond M); the caller places the barrier
__device__ __forceinline__ void stage_u_tile(double (*ul)[FID_DIM], const float* __restrict__ u, int r0, int M) {
    const int row = threadIdx.x >> 4, k4 = (threadIdx.x & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < M) v = *reinterpret_cast<const float4*>(u + (size_t)(r0 + row) * FID_DIM + k4);
    ul[row][k4] = v.x; ul[row][k4 + 1] = v.y; ul[row][k4 + 2] = v.z; ul[row][k4 + 3] = v.w;
}

// rows r0 .. r0 + 15, classes c0 .. c0 + 63 of the coefficients (zero beyond M / C; the pad column of an odd C holds 0)
__device__ __forceinline__ void stage_g_tile(double (*gl)[MS_CT], const double* __restrict__ G, int ldz, int r0, int M, int c0, int C) {
#pragma unroll
    for (int j = 0; j < MS_RT * MS_CT / 2 / MS_THREADS; ++j) {
        const int idx = threadIdx.x + MS_THREADS * j, row = idx >> 5, c2 = (idx & 31) * 2;
        double2 v = make_double2(0.0, 0.0);
        if (r0 + row < M && c0 + c2 < C) v = *reinterpret_cast<const double2*>(G + (size_t)(r0 + row) * ldz + c0 + c2);
        gl[row][c2] = v.x; gl[row][c2 + 1] = v.y;
    }
}

__global__ __launch_bounds__(MS_THREADS) void fid_margin_cos_kernel(const float* __restrict__ u, const float* __restrict__ W, int M, int C,
                                                                    int ldz, double* __restrict__ Z) {
    __shared__ __attribute__((aligned(16))) WTile T;
    __shared__ __attribute__((aligned(16))) double ul[MS_RT][FID_DIM];
    const int c0 = blockIdx.x * MS_CT, r0 = blockIdx.y * MS_RT;
    stage_u_tile(ul, u, r0, M);
    stage_w_tile(T, W, c0, C);            // its barriers also cover ul
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < FID_DIM; ++k) {
        const double w = T.w[c][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_fma(ul[rg * 4 + j][k], w, acc[j]);
    }
    if (c0 + c < C) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + rg * 4 + j;
            if (r < M) Z[(size_t)r * ldz + c0 + c] = acc[j];
        }
    }
}

struct MarginArgs {
    int kind;                              // 0 CosFace, 1 ArcFace
    double s, m, cos_m, sin_m, cos_pm, sin_pm;   // pm: pi - m
};

__global__ __launch_bounds__(64 * MS_ROW_WAVES) void fid_margin_row_kernel(const int* __restrict__ labels, int M, int C, int ldz,
                                                                           MarginArgs a, double* __restrict__ Z,
                                                                           double* __restrict__ row_loss, int* __restrict__ pred,
                                                                           double* __restrict__ cos_t) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * MS_ROW_WAVES + wave;
    if (i >= M) return;                    // wave-uniform, and no barrier below
    int nv = 0;
    for (int r = lane; r < M; r += 64) { const int l = labels[r]; nv += l >= 0 && l < C; }
    nv = fv_wave_sum(nv);
    const int y = labels[i];
    const bool valid = y >= 0 && y < C;
    double* z = Z + (size_t)i * ldz;

    // the target's logit s psi and d psi / d cos (the clamp's derivative included); the same in every lane
    double zy = 0.0, dpsi = 0.0, cy = __builtin_nan("");
    if (valid) {
        cy = z[y];
        const double t = fmin(fmax(cy, -1.0), 1.0);
        const double dclamp = (cy >= -1.0 && cy <= 1.0) ? 1.0 : 0.0;
        double psi = t - a.m, dp = 1.0;
        if (a.kind == 1) {
            const double q = 1.0 - t * t, sn = sqrt(fmax(q, 1e-12));
            if (t > a.cos_pm) {
                psi = t * a.cos_m - sn * a.sin_m;
                dp = a.cos_m + (q > 1e-12 ? t * a.sin_m / sn : 0.0);
            } else {
                psi = t - a.m * a.sin_pm;
            }
        }
        zy = a.s * psi;
        dpsi = dp * dclamp;
    }

    // argmax of the cosines (the lowest c among equals) and the row maximum of the logits
    double best = -__builtin_inf(), mx = valid ? zy : 0.0;
    int bi = 0x7fffffff;
    for (int c = 2 * lane; c < C; c += 128) {
        const double2 v = *reinterpret_cast<const double2*>(z + c);
        if (v.x > best) { best = v.x; bi = c; }
        if (c + 1 < C && v.y > best) { best = v.y; bi = c + 1; }
        if (c != y) mx = fmax(mx, a.s * v.x);
        if (c + 1 < C && c + 1 != y) mx = fmax(mx, a.s * v.y);
    }
    fv_wave_best<max_more>(best, bi);
    if (lane == 0) {
        pred[i] = (y >= C) ? -2 : bi;
        cos_t[i] = cy;                     // one quiet NaN where the row has no class
    }
    if (!valid) {                          // the row adds nothing anywhere
        for (int c = 2 * lane; c < ldz; c += 128) *reinterpret_cast<double2*>(z + c) = make_double2(0.0, 0.0);
        if (lane == 0) row_loss[i] = 0.0;
        return;
    }
    mx = fv_wave_max(mx);
    double sum = 0.0;
    for (int c = 2 * lane; c < C; c += 128) {
        const double2 v = *reinterpret_cast<const double2*>(z + c);
        sum += exp((c == y ? zy : a.s * v.x) - mx);
        if (c + 1 < C) sum += exp((c + 1 == y ? zy : a.s * v.y) - mx);
    }
    sum = fv_wave_sum_all(sum);
    if (lane == 0) row_loss[i] = mx + log(sum) - zy;
    const double f = a.s / (double)nv, rs = 1.0 / sum;
    for (int c = 2 * lane; c < C; c += 128) {
        const double2 v = *reinterpret_cast<const double2*>(z + c);
        double2 g;
        g.x = c == y ? (exp(zy - mx) * rs - 1.0) * f * dpsi : exp(a.s * v.x - mx) * rs * f;
        g.y = 0.0;                         // the pad column of an odd C
        if (c + 1 < C) g.y = c + 1 == y ? (exp(zy - mx) * rs - 1.0) * f * dpsi : exp(a.s * v.y - mx) * rs * f;
        *reinterpret_cast<double2*>(z + c) = g;
    }
}

__global__ __launch_bounds__(MS_THREADS) void fid_margin_du_kernel(const double* __restrict__ G, const float* __restrict__ W, int M, int C,
                                                                   int ldz, double* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) WTile T;
    __shared__ __attribute__((aligned(16))) double gl[MS_RT][MS_CT];
    const int r0 = blockIdx.y * MS_RT;
    const int k = threadIdx.x & 63, rg = threadIdx.x >> 6;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int tile = 0; tile < MS_DU_TILES; ++tile) {
        const int c0 = (blockIdx.x * MS_DU_TILES + tile) * MS_CT;
        if (c0 >= C) break;                // uniform over the workgroup
        stage_g_tile(gl, G, ldz, r0, M, c0, C);
        stage_w_tile(T, W, c0, C);
#pragma unroll 8
        for (int cc = 0; cc < MS_CT; ++cc) {
            const double w = T.w[cc][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fma(gl[rg * 4 + j][cc], w, acc[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + rg * 4 + j;
        if (r < M) slab[((size_t)blockIdx.x * M + r) * FID_DIM + k] = acc[j];
    }
}

__global__ __launch_bounds__(MS_THREADS) void fid_margin_dw_kernel(const double* __restrict__ G, const float* __restrict__ u,
                                                                   const float* __restrict__ W, int M, int C, int ldz, double loss_weight,
                                                                   float* __restrict__ dW) {
    __shared__ __attribute__((aligned(16))) WTile T;
    __shared__ __attribute__((aligned(16))) double gl[MS_RT][MS_CT];
    __shared__ __attribute__((aligned(16))) double ul[MS_RT][FID_DIM];
    constexpr int PER = MS_CT / (MS_THREADS / 64);      // classes per wave
    const int c0 = blockIdx.x * MS_CT;
    const int k = threadIdx.x & 63, cg = threadIdx.x >> 6;
    stage_w_tile(T, W, c0, C);
    double acc[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j] = 0.0;
    for (int r0 = 0; r0 < M; r0 += MS_RT) {              // the per-class reduction over the rows, in row order
        stage_g_tile(gl, G, ldz, r0, M, c0, C);
        stage_u_tile(ul, u, r0, M);
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < MS_RT; ++r) {
            const double uu = ul[r][k];
#pragma unroll
            for (int j = 0; j < PER; ++j) acc[j] = __builtin_fma(gl[r][cg * PER + j], uu, acc[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int cl = cg * PER + j;
        const double wh = T.w[cl][k];
        const double dot = fv_wave_sum_all(wh * acc[j]);
        const double d = T.live[cl] ? T.inv[cl] * (acc[j] - wh * dot) : acc[j] * 1e6;
        if (c0 + cl < C) dW[(size_t)(c0 + cl) * FID_DIM + k] = (float)(d * loss_weight);
    }
}

__global__ __launch_bounds__(64 * MS_ROW_WAVES) void fid_margin_rows_kernel(const float* __restrict__ pre, const double* __restrict__ slab,
                                                                            int chunks, int M, double loss_weight, float* __restrict__ dE) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * MS_ROW_WAVES + wave;
    if (r >= M) return;                    // wave-uniform: the wave sums below see all 64 lanes
    double du = 0.0;
    for (int ch = 0; ch < chunks; ++ch) du += slab[((size_t)ch * M + r) * FID_DIM + lane];
    dE[(size_t)r * FID_DIM + lane] = l2_relu_bwd(pre[(size_t)r * FID_DIM + lane], du, loss_weight);
}

__global__ __launch_bounds__(256) void fid_margin_finish_kernel(const float* __restrict__ dE, const int* __restrict__ labels,
                                                                const double* __restrict__ row_loss, int M, int C,
                                                                float* __restrict__ loss, float* __restrict__ dbias) {
    __shared__ double part[4][FID_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (M + 3) / 4, lo = wave * per, hi = min(M, lo + per);
    double db = 0.0;
#pragma unroll 8
    for (int r = lo; r < hi; ++r) db += (double)dE[(size_t)r * FID_DIM + lane];
    part[wave][lane] = db;
    __syncthreads();
    if (wave == 0) {
        dbias[lane] = (float)(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
    } else if (wave == 1) {
        int nv = 0;
        double s = 0.0;
        for (int r = lane; r < M; r += 64) {
            const int l = labels[r];
            if (l >= 0 && l < C) { ++nv; s += row_loss[r]; }
        }
        nv = fv_wave_sum(nv);
        s = fv_wave_sum_all(s);
        if (lane == 0) *loss = nv ? (float)(s / (double)nv) : 0.f;
    }
}

int du_chunks(int C) { return (C + MS_CT * MS_DU_TILES - 1) / (MS_CT * MS_DU_TILES); }
size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

static bool margin_shape_ok(int M, int C) { return M >= 1 && M <= FID_BATCH_MAX && C >= 1 && C <= FID_CLASSES_MAX; }

size_t fv_fid_margin_ws_bytes(int M, int C) {
    if (!margin_shape_ok(M, C)) return 0;
    const size_t ldz = ((size_t)C + 1) & ~(size_t)1;
    return up256((size_t)M * ldz * sizeof(double)) + up256((size_t)du_chunks(C) * M * FID_DIM * sizeof(double)) +
           up256((size_t)M * sizeof(double));
}

int fv_fid_margin_check(fv_ctx* ctx, const char* who, int M, int C, int kind, double scale, double margin, double loss_weight) {
    FV_REQUIRE(ctx, M >= 1 && M <= FID_BATCH_MAX, "%s: M %d outside [1, %d]", who, M, FID_BATCH_MAX);
    FV_REQUIRE(ctx, C >= 1 && C <= FID_CLASSES_MAX, "%s: C %d outside [1, %d]", who, C, FID_CLASSES_MAX);
    FV_REQUIRE(ctx, kind == 0 || kind == 1, "%s: kind %d (0 CosFace, 1 ArcFace)", who, kind);
    FV_REQUIRE(ctx, std::isfinite(scale) && scale > 0.0, "%s: scale %g is not finite and > 0", who, scale);
    FV_REQUIRE(ctx, std::isfinite(margin) && margin > 0.0 && margin < (kind == 0 ? 1.0 : M_PI / 2),
               "%s: margin %g outside (0, %s)", who, margin, kind == 0 ? "1" : "pi / 2");
    FV_REQUIRE(ctx, std::isfinite(loss_weight) && loss_weight > 0.0, "%s: loss_weight must be finite and > 0", who);
    return FV_OK;
}

int fv_fid_margin_softmax(fv_ctx* ctx, const float* pre, const float* u, const int32_t* labels, int M, const float* W, int C, int kind,
                          double scale, double margin, double loss_weight, void* workspace, size_t workspace_bytes, float* loss,
                          float* dE, float* dbias, float* dW, int32_t* pred, double* cos_t) {
    FV_REQUIRE(ctx, pre && u && labels && W && workspace && loss && dE && dbias && dW && pred && cos_t, "fid_margin_softmax: NULL buffer");
    if (int rc = fv_fid_margin_check(ctx, "fid_margin_softmax", M, C, kind, scale, margin, loss_weight)) return rc;
    FV_REQUIRE(ctx, (((uintptr_t)u | (uintptr_t)W | (uintptr_t)workspace) & 15) == 0,
               "fid_margin_softmax: u, W and the workspace must be 16-byte aligned");
    const size_t need = fv_fid_margin_ws_bytes(M, C);
    if (need > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_margin_softmax: workspace %zu < %zu bytes", workspace_bytes, need);
    const int ldz = (C + 1) & ~1, chunks = du_chunks(C);
    char* base = (char*)workspace;
    double* Z = (double*)base;
    double* slab = (double*)(base + up256((size_t)M * ldz * sizeof(double)));
    double* row_loss = (double*)((char*)slab + up256((size_t)chunks * M * FID_DIM * sizeof(double)));
    const MarginArgs a{kind, scale, margin, cos(margin), sin(margin), cos(M_PI - margin), sin(M_PI - margin)};
    const unsigned ctiles = (unsigned)((C + MS_CT - 1) / MS_CT), rtiles = (unsigned)((M + MS_RT - 1) / MS_RT);
    const unsigned rblocks = (unsigned)((M + MS_ROW_WAVES - 1) / MS_ROW_WAVES);
    const double mck = (double)M * C * FID_DIM;
    {
        FvProfScope ps(ctx, "fid_margin_cos_kernel", 2.0 * mck, (double)M * C * 8 + (double)rtiles * C * FID_DIM * 4);
        hipLaunchKernelGGL(fid_margin_cos_kernel, dim3(ctiles, rtiles), dim3(MS_THREADS), 0, ctx->stream, u, W, M, C, ldz, Z);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fid_margin_row_kernel", 0.0, (double)M * C * 8 * 4);
        hipLaunchKernelGGL(fid_margin_row_kernel, dim3(rblocks), dim3(64 * MS_ROW_WAVES), 0, ctx->stream, (const int*)labels, M, C, ldz, a, Z,
                           row_loss, (int*)pred, cos_t);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fid_margin_du_kernel", 2.0 * mck, (double)M * C * 8 + (double)rtiles * C * FID_DIM * 4);
        hipLaunchKernelGGL(fid_margin_du_kernel, dim3((unsigned)chunks, rtiles), dim3(MS_THREADS), 0, ctx->stream, (const double*)Z, W, M, C,
                           ldz, slab);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fid_margin_dw_kernel", 2.0 * mck, (double)M * C * 8 + (double)C * FID_DIM * 8);
        hipLaunchKernelGGL(fid_margin_dw_kernel, dim3(ctiles), dim3(MS_THREADS), 0, ctx->stream, (const double*)Z, u, W, M, C, ldz,
                           loss_weight, dW);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fid_margin_rows_kernel", 0.0, (double)M * FID_DIM * (8.0 * chunks + 8));
        hipLaunchKernelGGL(fid_margin_rows_kernel, dim3(rblocks), dim3(64 * MS_ROW_WAVES), 0, ctx->stream, pre, (const double*)slab, chunks, M,
                           loss_weight, dE);
        FV_LAUNCH_CHECK(ctx);
    }
    FvProfScope ps(ctx, "fid_margin_finish_kernel", 0.0, (double)M * (FID_DIM * 4 + 12));
    hipLaunchKernelGGL(fid_margin_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, (const float*)dE, (const int*)labels,
                       (const double*)row_loss, M, C, loss, dbias);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
