// Internal launch interface of fid.hip: the FaceIdentifier's head (reference face_identification.py:318-345): Flatten ->
// Dense(64, relu) -> l2_normalize, the triplet loss (fi.py:72-76) and the dense layer's two gradients.  All fp32 FMA on the vector
// units, every sum in a fixed order (no atomics): the same rows give the same bits, whatever else is in the batch.
#pragma once
#include "block_ops.h"

constexpr int FID_DIM = 64;    // nn_arch.dense1_dim; the loss slices 0:64 / 64:128 / 128:192 are hard-coded in the reference
constexpr int FID_KC = 256;    // F per forward partial: fixed, so a row's summation order does not depend on the batch

// Rows of the dense layer's input (or of its data-gradient): row m lies at p[m / per] + (m % per) * F -- the three towers' feature
// maps [per][F] read (written) in place, tower-major.
struct FidRows { float* p[3]; int per; };

// d pre of one row from d u: back through l2_normalize (the rsqrt factor s is a constant where sum x^2 <= 1e-12) and ReLU (TF's
// ReluGrad: passes only where pre > 0).  `weight` multiplies the fp64 result once, where it is rounded to float: a power of two
// scales the stored value exactly.
__device__ __forceinline__ float l2_relu_bwd(float y, double du, double weight) {
    const double r = y > 0.f ? (double)y : 0.0;
    const double ss = fv_wave_sum_all(r * r);
    double dr;
    if (ss > 1e-12) {
        const double s = 1.0 / sqrt(ss), uu = r * s;
        dr = s * (du - uu * fv_wave_sum_all(uu * du));
    } else {
        dr = du * 1e6;
    }
    return y > 0.f ? (float)(dr * weight) : 0.f;
}

inline long long fv_fid_chunks(long long F) { return F / FID_KC; }
// part [F / FID_KC][M][64]: per-chunk partial products of X . W
int fv_fid_dense_fwd(fv_ctx* ctx, FidRows X, int M, long long F, const float* W, float* part);
// u = l2_normalize(relu(sum of the partials in chunk order + bias)); pre (may be NULL) keeps the pre-activation
int fv_fid_dense_finish(fv_ctx* ctx, const float* part, long long chunks, int M, const float* bias, float* pre, float* u);
// triplet loss over B triplets (rows b, B + b, 2B + b of pre / u): loss = their unweighted mean; dE [3B][64] = loss_weight *
// dL / d pre, dbias [64] = its column sums.  loss_weight must be finite and > 0.
int fv_fid_triplet(fv_ctx* ctx, const float* pre, const float* u, int B, float* loss, float* dE, float* dbias, double loss_weight);
// batch triplet loss over M labelled rows (fid_batch.hip): every row of a known subject is an anchor with its hardest positive and a
// mined negative of the batch (mode 0: the nearest, 1: semi-hard); include/fv_hotpath.h, fv_fid_batch_triplet_loss_grad, has the
// contract.  1 <= M <= FID_BATCH_MAX; u 16-byte aligned.
constexpr int FID_BATCH_MAX = 1024;
int fv_fid_batch_triplet(fv_ctx* ctx, const float* pre, const float* u, const int32_t* subjects, int M, double margin, int mode,
                         double loss_weight, float* loss, float* dE, float* dbias, int32_t* pos_index, int32_t* neg_index, int32_t* kind,
                         double* d_ap, double* d_an);
// additive-margin softmax over the subjects (fid_margin.hip) on M labelled rows and the class kernel W [C][64];
// include/fv_hotpath.h, fv_fid_margin_softmax_loss_grad, has the contract.  1 <= M <= FID_BATCH_MAX, 1 <= C <= FID_CLASSES_MAX; u, W
// and the workspace (fv_fid_margin_ws_bytes; 0 for a shape that is not served) 16-byte aligned.  fv_fid_margin_check: the
// refusals of the scalar arguments alone, for a caller that enqueues other work first.
constexpr int FID_CLASSES_MAX = 32768;
size_t fv_fid_margin_ws_bytes(int M, int C);
int fv_fid_margin_check(fv_ctx* ctx, const char* who, int M, int C, int kind, double scale, double margin, double loss_weight);
int fv_fid_margin_softmax(fv_ctx* ctx, const float* pre, const float* u, const int32_t* labels, int M, const float* W, int C, int kind,
                          double scale, double margin, double loss_weight, void* workspace, size_t workspace_bytes, float* loss,
                          float* dE, float* dbias, float* dW, int32_t* pred, double* cos_t);
// dX = dE . W^T, written (not added) into the rows of dX
int fv_fid_dense_dgrad(fv_ctx* ctx, const float* dE, int M, long long F, const float* W, FidRows dX);
// The reconstruction model's head: u [M][64] = relu(l2_normalize(ids)), x [M][F] = u . W^T + bias (W the dense kernel [F][64])
int fv_fid_recon_head(fv_ctx* ctx, const float* ids, int M, long long F, const float* W, const float* bias, float* u, float* x);
// dW [F][64] = X^T . dE over the M rows, stored
int fv_fid_dense_wgrad(fv_ctx* ctx, FidRows X, const float* dE, int M, long long F, float* dW);
