// Internal launch interface of recon.hip: the two kernels the reconstruction model (reference face_identification.py:1155-1488,
// create_face_reconst_model) adds to the conv data-gradient launchers it otherwise runs on -- the normalise stage in front of
// every transposed conv, and the last transposed conv (32 -> 3 channels), which no training step differentiates.
#pragma once
#include "common.h"

// true for the channel counts the normalise stage is built for: 32, 64, 128, 256, 512, 1024
bool fv_recon_norm_channels_ok(int C);
// rows pixels of C contiguous floats:  d = x - skip (skip == NULL: d = x), l = leaky_relu(d),
//   y = l * (1 / sqrt(max(sum_c l^2, 1e-12))) * scale[c] + shift[c]
// d_out (may be NULL: d is not kept; may be x itself: in place) receives d.  A pixel's result does not depend on rows.
int fv_recon_l2norm_affine(fv_ctx* ctx, const float* x, const float* skip, float* d_out, const float* scale, const float* shift, float* y,
                           long long rows, int C, float leaky);
// out [B][H][W][3] = Conv2DTranspose(3, 3x3, stride 1, 'same') of x [B][H][W][32] with the kernel image w_t [3][9][32]
// (fv_transpose_weights of the layer's [32][9][3] kernel); H % 8 == 0, W % 32 == 0
bool fv_recon_convt_last_ok(int H, int W);
int fv_recon_convt_last(fv_ctx* ctx, const float* x, const float* w_t, int B, int H, int W, float* out);
