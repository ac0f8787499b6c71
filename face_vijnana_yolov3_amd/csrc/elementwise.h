// Internal launch interface of elementwise.hip.
#pragma once
#include "common.h"

// ---- device expressions shared between the BN passes (elementwise.hip) and the halo kernels that apply them on load
// (conv9_mfma.hip, wgrad9_mfma.hip, wgrad0_mfma.hip): one definition each, so the fused and the materialised form give the same
// bits (the library is built with -ffp-contract=off).

// a = LeakyReLU(z * scale + shift)
__device__ __forceinline__ float fv_bn_leaky(float z, float sc, float sh, float leaky) {
    const float v = z * sc + sh;
    return v > 0.f ? v : v * leaky;
}
__device__ __forceinline__ float4 fv_bn_leaky4(float4 v, const float4& sc, const float4& sh, float leaky) {
    v.x = fv_bn_leaky(v.x, sc.x, sh.x, leaky); v.y = fv_bn_leaky(v.y, sc.y, sh.y, leaky);
    v.z = fv_bn_leaky(v.z, sc.z, sh.z, leaky); v.w = fv_bn_leaky(v.w, sc.w, sh.w, leaky);
    return v;
}

// total / M of a published (float) d-beta or d-gamma, rounded once.  A product with float(1 / M) instead carries the rounding of the
// reciprocal (0.8 u at M = 1000) into every element of dz with one sign: at 1000 rows that put dz 2.016 ulp from the float64
// expression (tests/test_exact_bn_gpu.py); with the quotient a CPU emulation gives 1.64.
__device__ __forceinline__ float fv_bn_mean_of(float total, double count) { return (float)((double)total / count); }

// dz = scale * (gy - dbeta/M - xhat * dgamma/M), gy = g * LeakyReLU'(z * scale + shift); mb = fv_bn_mean_of(dbeta, M),
// mg = fv_bn_mean_of(dgamma, M), formed once per channel where the caller has a prologue
__device__ __forceinline__ float fv_bn_bwd_dz(float g, float z, float sc, float sh, float mu, float is, float mb, float mg, float leaky) {
    const float gy = (z * sc + sh) > 0.f ? g : g * leaky;
    return sc * (gy - mb - (z - mu) * is * mg);
}
__device__ __forceinline__ float4 fv_bn_bwd_dz4(const float4& g, const float4& z, const float4& sc, const float4& sh, const float4& mu,
                                                const float4& is, const float4& mb, const float4& mg, float leaky) {
    float4 o;
    o.x = fv_bn_bwd_dz(g.x, z.x, sc.x, sh.x, mu.x, is.x, mb.x, mg.x, leaky);
    o.y = fv_bn_bwd_dz(g.y, z.y, sc.y, sh.y, mu.y, is.y, mb.y, mg.y, leaky);
    o.z = fv_bn_bwd_dz(g.z, z.z, sc.z, sh.z, mu.z, is.z, mb.z, mg.z, leaky);
    o.w = fv_bn_bwd_dz(g.w, z.w, sc.w, sh.w, mu.w, is.w, mb.w, mg.w, leaky);
    return o;
}

// Totals of the [nslot][2][C] fp64 accumulator slots by the first 256 threads of a workgroup of NTH for C < 256: the 256 / C
// thread groups take every (256 / C)-th slot of a channel, thread c < C then adds the groups' partials in ascending order -- one
// fixed order wherever the slots are summed.  (C not dividing 256: the threads behind the last whole group idle.)  Valid in
// threads tid < C on return; contains one barrier, which every thread of the workgroup reaches; s_part is [2][256].
template <int NTH = 256>
__device__ __forceinline__ void fv_bn_slot_totals(const double* __restrict__ slots, int nslot, int C, int tid, double (*s_part)[256],
                                                  double& a, double& b) {
    const int G = 256 / C, g = tid / C, c = tid % C;
    a = 0.0; b = 0.0;
    if (g < G)
        for (int k = g; k < nslot; k += G) { a += slots[(size_t)(2 * k) * C + c]; b += slots[(size_t)(2 * k + 1) * C + c]; }
    if (NTH == 256 || tid < 256) { s_part[0][tid] = a; s_part[1][tid] = b; }
    __syncthreads();
    if (tid < C) {
        a = 0.0; b = 0.0;
        for (int j = 0; j < G; ++j) { a += s_part[0][j * C + tid]; b += s_part[1][j * C + tid]; }
    }
}

// Accumulator slots of the conv epilogue (conv.h stat_slots) -> scale/shift of all C channels in LDS: fixed summation order
// over the slots, fp64, 16 loads per thread.  `publish` (one workgroup per launch): also mean / invstd / scale / shift for the
// backward pass and the update of the moving statistics.  The caller's barrier makes s_sc / s_sh visible.  The first 256 threads
// of a workgroup of NTH do the work (bn_act_stats_kernel, bn_stats_publish_kernel and the BN-input mode of conv1x1_mfma.hip
// share this code, so scale / shift are the same bits wherever they are formed).
template <int NTH = 256>
__device__ __forceinline__ void fv_bn_slots_to_affine(const double* __restrict__ slots, int nslot, double count,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                      float ema_old, float ema_new, float* __restrict__ mean_out,
                                                      float* __restrict__ invstd_out, float* __restrict__ scale_out,
                                                      float* __restrict__ shift_out, float* __restrict__ moving_mean,
                                                      float* __restrict__ moving_var, int C, bool publish, float* s_sc, float* s_sh,
                                                      double (*s_part)[256]) {
    const int tid = threadIdx.x;
    auto finish = [&](int c, double s, double q) {
        const double mean = s / count;
        double var = q / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[c] * invstd, sh = beta[c] - (float)mean * sc;
        s_sc[c] = sc; s_sh[c] = sh;
        if (publish) {
            mean_out[c] = (float)mean; invstd_out[c] = invstd; scale_out[c] = sc; shift_out[c] = sh;
            if (moving_mean) {   // Keras 2.2.4 BatchNormalization: EMA of batch mean and of var * n/(n-(1+eps))
                const double corr = count / (count - (1.0 + (double)eps));
                moving_mean[c] = ema_old * moving_mean[c] + ema_new * (float)mean;
                moving_var[c] = ema_old * moving_var[c] + ema_new * (float)(var * corr);
            }
        }
    };
    if (C >= 256) {
        for (int c = tid; c < C && (NTH == 256 || tid < 256); c += 256) {
            double s = 0.0, q = 0.0;
            for (int k = 0; k < nslot; ++k) { s += slots[(size_t)(2 * k) * C + c]; q += slots[(size_t)(2 * k + 1) * C + c]; }
            finish(c, s, q);
        }
    } else {
        // C < 256 (a power of two >= 32 here): 256 / C thread groups share the slots of a channel
        double s, q;
        fv_bn_slot_totals<NTH>(slots, nslot, C, tid, s_part, s, q);
        if (tid < C) finish(tid, s, q);
    }
}

int fv_ew_bn_finalize(fv_ctx* ctx, const float* psum, const float* psq, int mtiles, int C, double count, const float* gamma,
                      const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale, float* shift,
                      float* moving_mean, float* moving_var);
int fv_ew_bn_fold(fv_ctx* ctx, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
                  float* scale, float* shift);
int fv_ew_bn_act(fv_ctx* ctx, const float* z, const float* scale, const float* shift, const float* skip, float* out,
                 long long rows, int C, float leaky);
int fv_ew_bn_bwd_chunks(long long rows, int C);
int fv_ew_bn_bwd(fv_ctx* ctx, const float* g, const float* z, const float* scale, const float* shift, const float* mean,
                 const float* invstd, long long rows, int C, float leaky, float* pdb, float* pdg, float* dbeta, float* dgamma,
                 float* dz, double* slots = nullptr, int nslot = 0, bool reduced = false, bool accumulate = false);
// accumulate: d-beta / d-gamma are ADDED to what dbeta / dgamma hold (a BN layer shared by several towers of one step, net_fid.hip)
// instead of stored
// part != NULL: multi-workgroup form with fv_ew_mse_scratch_floats() floats of scratch (8-byte aligned); NULL: one workgroup
int fv_ew_mse(fv_ctx* ctx, const float* yp, const float* yt, int rows, int C, int Cpad, float* loss, float* dy, float* dbias,
              double* part = nullptr, double grad_weight = 1.0);
int fv_ew_mse_scratch_floats();
int fv_ew_scale(fv_ctx* ctx, float* v, long long n, float alpha);
int fv_ew_adam(fv_ctx* ctx, float* p, const float* g, float* m, float* v, long long n, float lr_t, float b1, float b2, float eps);
// training-mode BN without a finalize launch: the conv epilogue adds its column sums to
// [nslot][2][C] fp64 accumulator slots (zeroed by the caller); this pass sums them, normalises, and
// publishes mean/invstd/scale/shift (+ moving statistics) for the backward pass
int fv_ew_bn_stat_slots(int C);
// the coefficients of the moving-statistics update under the context's zero-debias step (fv_set_bn_zero_debias_step)
void fv_ew_bn_ema_coeff(const fv_ctx* ctx, float momentum, float* c_old, float* c_new);
int fv_ew_bn_act_stats(fv_ctx* ctx, const float* z, const double* slots, int nslot, double count, const float* gamma,
                       const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale, float* shift,
                       float* moving_mean, float* moving_var, const float* skip, float* out, long long rows, int C, float leaky);
// the statistics part of fv_ew_bn_act_stats alone (one workgroup): for a layer whose consumers apply scale/shift + LeakyReLU on load
int fv_ew_bn_stats_publish(fv_ctx* ctx, const double* slots, int nslot, double count, const float* gamma, const float* beta, float eps,
                           float momentum, float* mean, float* invstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                           int C);
int fv_ew_transpose_ntc(fv_ctx* ctx, const float* src, float* dst, int N, int T, int C, int Npad);
// the same for up to 64 layers in one launch; offsets in floats from the two base pointers
int fv_ew_transpose_all(fv_ctx* ctx, const float* src_base, float* dst_base, int nlayers, const long long* src_off,
                        const long long* dst_off, const int* N, const int* T, const int* C, const int* Npad);
int fv_ew_pad_rows(fv_ctx* ctx, const float* src, float* dst, int N, int K, int Kpad);
int fv_ew_slice_cols(fv_ctx* ctx, const float* src, float* dst, long long rows, int C, int Cpad);
int fv_ew_splitk_finish(fv_ctx* ctx, const float* slabs, int ksplit, long long stride, const float* scale, const float* shift,
                        const float* skip, float* out, long long n, int C, float leaky, int do_leaky);
int fv_ew_bn_fold_all(fv_ctx* ctx, const float* params, const float* state, int nlayers, const int* ch_begin, const long long* gamma_off,
                      const long long* beta_off, const long long* mean_off, const long long* var_off, float eps, int total,
                      float* scale, float* shift);
int fv_ew_fd_loss(fv_ctx* ctx, const float* yp, const float* yt, int cells, int Cpad, float* loss, float* dy);
int fv_ew_upsample_concat(fv_ctx* ctx, const float* src, const float* skip, float* out, int B, int Hs, int Ws, int C1, int C2);
// three-scale training (net_yolov3.hip): backward of upsample+concat, bias-gradient column sums, the per-scale detection loss
int fv_ew_upsample_concat_bwd(fv_ctx* ctx, const float* g, float* g_up, float* g_skip, int B, int Hs, int Ws, int C1, int C2);
int fv_ew_colsum_chunks(long long rows);
int fv_ew_colsum(fv_ctx* ctx, const float* dy, long long rows, int C, int Cpad, double* part /*[chunks][C]*/, float* out);
int fv_ew_yolo_loss_blocks(long long nbox);
int fv_ew_yolo_loss_part(fv_ctx* ctx, const float* t, const float* y, long long cells, int ncls, int A, int Cpad, float* dy, double* part,
                         double grad_weight = 1.0);
int fv_ew_yolo_loss_finish(fv_ctx* ctx, const double* part, const long long* cells3, int A, float* loss);
