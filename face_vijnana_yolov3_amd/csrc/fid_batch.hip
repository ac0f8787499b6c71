// Batch triplet loss with in-batch mining (FaceNet section 3.2 online mining; Hermans et al., "batch hard") over M <= 1024 labelled
// rows of facial IDs: every row of a known subject is an anchor, its positive the farthest row of its subject, its negative mined
// among the other subjects' rows of the same batch.  include/fv_hotpath.h (fv_fid_batch_triplet_loss_grad) has the contract.
//
// Three launches, the later ones reading what the earlier stored (u is at most 256 KB: it stays in L2, nothing is staged whole):
//   select  one wave per anchor, four anchors per workgroup.  The anchor lies in LDS (read as broadcasts); lane l computes D(i, r)
//           of rows r = l, l + 64, ... once (16 float4 loads per row, fid_select.h's chain) and keeps them in registers, since the
//           negative's class needs dap first.  Every choice is an extremum under a total order -- min_less / max_more of
//           block_ops.h -- so it does not depend on the split over lanes.
//   grad    one wave per row r (lane = column), four rows per workgroup: the owner GATHERS its row's total in fp64 -- its own
//           anchor term, then anchors 0 .. M-1 in order, found 64 at a time by a ballot over (pos_index == r, neg_index == r) --
//           and takes it back through l2_normalize and ReLU (l2_relu_bwd).  No atomics, one writer per element.
//   finish  wave 0: dbias = the column sums of the stored dE in row order; wave 1: the loss, hinge terms staged in LDS and summed
//           in anchor order.
#include "fid.h"
#include "fid_select.h"

#include <climits>
#include <cmath>

namespace {

constexpr int BT_WAVES = 4;                       // anchors (rows) per workgroup
constexpr int BT_SLOTS = FID_BATCH_MAX / 64;      // rows per lane at the size limit

__global__ __launch_bounds__(64 * BT_WAVES) void fid_batch_select_kernel(const float* __restrict__ u, const int* __restrict__ subjects,
                                                                         int M, double margin, int mode, int* __restrict__ pos_index,
                                                                         int* __restrict__ neg_index, int* __restrict__ kind,
                                                                         double* __restrict__ d_ap, double* __restrict__ d_an) {
    __shared__ __attribute__((aligned(16))) float as[BT_WAVES][FID_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * BT_WAVES + wave;
    if (i < M) as[wave][lane] = u[(size_t)i * FID_DIM + lane];
    __syncthreads();
    if (i >= M) return;                            // wave-uniform, and no barrier below
    const int sa = subjects[i];

    // D(i, r) of the rows this lane owns; a row that is neither kind of candidate keeps NaN, which no comparison accepts
    double dist[BT_SLOTS];
    int sub[BT_SLOTS];
#pragma unroll
    for (int j = 0; j < BT_SLOTS; ++j) {
        dist[j] = __builtin_nan("");
        sub[j] = -1;
        const int r = 64 * j + lane;
        if (r < M && sa >= 0) {
            sub[j] = subjects[r];
            if (sub[j] >= 0 && r != i) dist[j] = dist_to(as[wave], reinterpret_cast<const float4*>(u + (size_t)r * FID_DIM));
        }
    }

    // the positive: the largest D among the anchor's own subject, the lowest r among equals
    double pd = -__builtin_inf();
    int pi = INT_MAX;
#pragma unroll
    for (int j = 0; j < BT_SLOTS; ++j) {
        const int r = 64 * j + lane;
        if (sub[j] == sa && dist[j] == dist[j] && max_more()(dist[j], r, pd, pi)) { pd = dist[j]; pi = r; }
    }
    fv_wave_best<max_more>(pd, pi);
    const double dap = pd, hi = dap + margin;

    // the negative: [0] band (or, mode 0, all candidates), minimum; [1] D <= dap, maximum; [2] D >= hi, minimum
    double bd[3] = {__builtin_inf(), -__builtin_inf(), __builtin_inf()};
    int bi[3] = {INT_MAX, INT_MAX, INT_MAX};
    if (pi != INT_MAX) {
#pragma unroll
        for (int j = 0; j < BT_SLOTS; ++j) {
            const int r = 64 * j + lane;
            const double d = dist[j];
            if (sub[j] < 0 || sub[j] == sa || d != d) continue;
            if (mode == 0 || (d > dap && d < hi)) {
                if (min_less()(d, r, bd[0], bi[0])) { bd[0] = d; bi[0] = r; }
            } else if (d <= dap) {
                if (max_more()(d, r, bd[1], bi[1])) { bd[1] = d; bi[1] = r; }
            } else if (d >= hi) {
                if (min_less()(d, r, bd[2], bi[2])) { bd[2] = d; bi[2] = r; }
            }
        }
        fv_wave_best<min_less>(bd[0], bi[0]);
        if (mode != 0) { fv_wave_best<max_more>(bd[1], bi[1]); fv_wave_best<min_less>(bd[2], bi[2]); }
    }
    int kd = 3, ni = -1;
    double dn = __builtin_inf();
    if (pi != INT_MAX) {
        if (mode == 0) {
            if (bi[0] != INT_MAX) { ni = bi[0]; dn = bd[0]; kd = class_of(dn, dap, hi); }
        } else {
#pragma unroll
            for (int k = 2; k >= 0; --k)
                if (bi[k] != INT_MAX) { kd = k; ni = bi[k]; dn = bd[k]; }
        }
    }
    if (lane == 0) {
        const bool valid = kd != 3;
        pos_index[i] = valid ? pi : -1;
        neg_index[i] = ni;
        kind[i] = kd;
        d_ap[i] = valid ? dap : __builtin_nan("");   // one quiet NaN, sign and payload clear
        d_an[i] = dn;
    }
}

// 1 / (V d) of a chosen distance, 0 where the distance is exactly 0 (its gradient is defined as 0)
__device__ __forceinline__ double inv_dist(double V, double d) { return d > 0.0 ? 1.0 / (V * d) : 0.0; }

__global__ __launch_bounds__(64 * BT_WAVES) void fid_batch_grad_kernel(const float* __restrict__ pre, const float* __restrict__ u, int M,
                                                                       double margin, double loss_weight,
                                                                       const int* __restrict__ pos_index, const int* __restrict__ neg_index,
                                                                       const int* __restrict__ kind, const double* __restrict__ d_ap,
                                                                       const double* __restrict__ d_an, float* __restrict__ dE) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * BT_WAVES + wave;
    if (r >= M) return;                            // wave-uniform: the wave sums below see all 64 lanes
    int nv = 0;
    for (int i = lane; i < M; i += 64) nv += kind[i] != 3;
    const double V = (double)fv_wave_sum(nv);
    const double ur = (double)u[(size_t)r * FID_DIM + lane];

    double total = 0.0;
    if (kind[r] != 3) {                            // the row's own anchor term
        const double dap = d_ap[r], dan = d_an[r];
        if (dap - dan + margin >= 0.0) {
            const double vp = ur - (double)u[(size_t)pos_index[r] * FID_DIM + lane];
            const double vn = ur - (double)u[(size_t)neg_index[r] * FID_DIM + lane];
            total = inv_dist(V, dap) * vp - inv_dist(V, dan) * vn;
        }
    }
    for (int i0 = 0; i0 < M; i0 += 64) {           // what the anchors i0 .. i0 + 63 send to row r, in anchor order
        const int i = i0 + lane;
        bool hit = false;
        if (i < M) {
            // an invalid anchor has -1 in both; an anchor's positive and negative are different rows, and never itself
            if (pos_index[i] == r || neg_index[i] == r) hit = d_ap[i] - d_an[i] + margin >= 0.0;
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int a = i0 + __builtin_ctzll(mask);
            mask &= mask - 1;
            const double v = (double)u[(size_t)a * FID_DIM + lane] - ur;
            if (pos_index[a] == r) total -= inv_dist(V, d_ap[a]) * v;
            else total += inv_dist(V, d_an[a]) * v;
        }
    }
    dE[(size_t)r * FID_DIM + lane] = l2_relu_bwd(pre[(size_t)r * FID_DIM + lane], total, loss_weight);
}

__global__ __launch_bounds__(128) void fid_batch_finish_kernel(const float* __restrict__ dE, int M, double margin,
                                                               const int* __restrict__ kind, const double* __restrict__ d_ap,
                                                               const double* __restrict__ d_an, float* __restrict__ loss,
                                                               float* __restrict__ dbias) {
    __shared__ double sh[FID_BATCH_MAX];
    const int lane = threadIdx.x & 63;
    int nv = 0;
    if (threadIdx.x >= 64) {
        for (int i = lane; i < M; i += 64) {
            double h = 0.0;
            if (kind[i] != 3) {
                ++nv;
                h = d_ap[i] - d_an[i] + margin;
                h = h > 0.0 ? h : 0.0;
            }
            sh[i] = h;                             // an invalid anchor adds +0: the sum stays what the valid ones give
        }
        nv = fv_wave_sum(nv);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double db = 0.0;
#pragma unroll 8
        for (int r = 0; r < M; ++r) db += (double)dE[(size_t)r * FID_DIM + lane];
        dbias[lane] = (float)db;
    } else if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < M; ++i) s += sh[i];
        *loss = nv ? (float)(s / (double)nv) : 0.f;
    }
}

}  // namespace

int fv_fid_batch_triplet(fv_ctx* ctx, const float* pre, const float* u, const int32_t* subjects, int M, double margin, int mode,
                         double loss_weight, float* loss, float* dE, float* dbias, int32_t* pos_index, int32_t* neg_index, int32_t* kind,
                         double* d_ap, double* d_an) {
    FV_REQUIRE(ctx, pre && u && subjects && loss && dE && dbias && pos_index && neg_index && kind && d_ap && d_an,
               "fid_batch_triplet: NULL buffer");
    FV_REQUIRE(ctx, M >= 1 && M <= FID_BATCH_MAX, "fid_batch_triplet: M %d outside [1, %d]", M, FID_BATCH_MAX);
    FV_REQUIRE(ctx, ((uintptr_t)u & 15) == 0, "fid_batch_triplet: u must be 16-byte aligned");
    FV_REQUIRE(ctx, mode == 0 || mode == 1, "fid_batch_triplet: mode %d (0 batch hard, 1 batch semi-hard)", mode);
    FV_REQUIRE(ctx, std::isfinite(margin) && margin > 0.0, "fid_batch_triplet: margin %g is not finite and > 0", margin);
    FV_REQUIRE(ctx, std::isfinite(loss_weight) && loss_weight > 0.0, "fid_batch_triplet: loss_weight must be finite and > 0");
    const unsigned blocks = (unsigned)((M + BT_WAVES - 1) / BT_WAVES);
    {
        FvProfScope ps(ctx, "fid_batch_select_kernel", 3.0 * M * (double)M * FID_DIM, (double)M * M * (FID_DIM * 4 + 4));
        hipLaunchKernelGGL(fid_batch_select_kernel, dim3(blocks), dim3(64 * BT_WAVES), 0, ctx->stream, u, subjects, M, margin, mode,
                           pos_index, neg_index, kind, d_ap, d_an);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fid_batch_grad_kernel", 0.0, (double)M * (M * 24.0 + 5.0 * FID_DIM * 4));
        hipLaunchKernelGGL(fid_batch_grad_kernel, dim3(blocks), dim3(64 * BT_WAVES), 0, ctx->stream, pre, u, M, margin, loss_weight,
                           (const int*)pos_index, (const int*)neg_index, (const int*)kind, (const double*)d_ap, (const double*)d_an, dE);
        FV_LAUNCH_CHECK(ctx);
    }
    FvProfScope ps(ctx, "fid_batch_finish_kernel", 0.0, (double)M * (FID_DIM * 4 + 20));
    hipLaunchKernelGGL(fid_batch_finish_kernel, dim3(1), dim3(128), 0, ctx->stream, (const float*)dE, M, margin, (const int*)kind,
                       (const double*)d_ap, (const double*)d_an, loss, dbias);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
