// Kernels of the reconstruction model (reference face_identification.py:1155-1488, create_face_reconst_model): facial ID ->
// face image through the Darknet-53 base run backwards as Conv2DTranspose layers.  The transposed convs are the conv
// data-gradients (ops.hip); new here are
//
//  * the stage in front of every transposed conv, LeakyReLU -> per-pixel l2_normalize over the channels -> inference BatchNorm
//    (fi.py:1199-1201), fused with the residual subtract that precedes it (fi.py:1221-1222).  Memory-bound: x (and skip) in, y
//    (and d = x - skip, the next skip) out, 16 bytes per lane.  A pixel's C values stay in registers between the sum of squares
//    and the store.  The sum is per lane in channel order, then an xor butterfly over the lanes of the pixel: one fixed order,
//    whatever the row count.  C <= 128: C / 4 lanes per pixel, several pixels per wave; C >= 256: one wave per pixel, C / 256
//    float4 per lane.
//  * the last layer, Conv2DTranspose(3, 3x3) over 32 channels at full resolution (fi.py:1470-1484): 3 output channels are
//    nothing the matrix-core tiles can use, so it is a direct vector-FMA convolution in the manner of conv0_direct.hip.
#include "recon.h"

namespace {

// ------------------------------------------------------------------------------------------------------- normalise stage
template <int C>
__global__ __launch_bounds__(256) void l2norm_affine_kernel(const float* x, const float* __restrict__ skip, float* d_out,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ y, long long rows, float leaky) {
    constexpr int Q = C / 4;                    // float4 per pixel
    constexpr int LPP = Q < 64 ? Q : 64;        // lanes per pixel
    constexpr int V = Q / LPP;                  // float4 per lane
    constexpr int PPB = 256 / LPP;              // pixels per workgroup pass
    const int lp = threadIdx.x % LPP, pw = threadIdx.x / LPP;
    float4 sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sc[j] = *reinterpret_cast<const float4*>(scale + 4 * (lp + LPP * j));
        sh[j] = *reinterpret_cast<const float4*>(shift + 4 * (lp + LPP * j));
    }
    // every lane of a wave runs the same number of passes (the butterfly needs them all): the bound is per workgroup
    for (long long p0 = (long long)blockIdx.x * PPB; p0 < rows; p0 += (long long)gridDim.x * PPB) {
        const long long p = p0 + pw;
        const bool live = p < rows;
        float4 v[V];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long long e = p * C + 4 * (lp + LPP * j);
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                t = *reinterpret_cast<const float4*>(x + e);
                if (skip) {
                    const float4 k = *reinterpret_cast<const float4*>(skip + e);
                    t.x -= k.x; t.y -= k.y; t.z -= k.z; t.w -= k.w;
                }
                if (d_out) *reinterpret_cast<float4*>(d_out + e) = t;
            }
            t.x = t.x > 0.f ? t.x : t.x * leaky; t.y = t.y > 0.f ? t.y : t.y * leaky;
            t.z = t.z > 0.f ? t.z : t.z * leaky; t.w = t.w > 0.f ? t.w : t.w * leaky;
            v[j] = t;
            s += t.x * t.x; s += t.y * t.y; s += t.z * t.z; s += t.w * t.w;
        }
#pragma unroll
        for (int off = LPP / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        const float r = 1.0f / sqrtf(fmaxf(s, 1e-12f));
        if (live) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float4 t = v[j];
                t.x = t.x * r * sc[j].x + sh[j].x; t.y = t.y * r * sc[j].y + sh[j].y;
                t.z = t.z * r * sc[j].z + sh[j].z; t.w = t.w * r * sc[j].w + sh[j].w;
                *reinterpret_cast<float4*>(y + p * C + 4 * (lp + LPP * j)) = t;
            }
        }
    }
}

template <int C>
void launch_l2norm(fv_ctx* ctx, const float* x, const float* skip, float* d_out, const float* scale, const float* shift, float* y,
                   long long rows, float leaky) {
    constexpr int PPB = 256 / (C / 4 < 64 ? C / 4 : 64);
    const long long passes = (rows + PPB - 1) / PPB;
    const int grid = (int)(passes < 2048 ? passes : 2048);
    hipLaunchKernelGGL(l2norm_affine_kernel<C>, dim3(grid), dim3(256), 0, ctx->stream, x, skip, d_out, scale, shift, y, rows, leaky);
}

// ------------------------------------------------------------------------------------------------------- last layer
// out[b, h, w, ci] = sum_{r, q, co} x[b, h + 1 - r, w + 1 - q, co] * w_t[ci][r * 3 + q][co]   (zero outside the image)
//
// A workgroup owns 8 x 32 output pixels and stages their 10 x 34 halo of 32 channels in LDS, a pixel padded to 36 floats: the
// four lane groups of a ds_read_b128 then cover the 64 banks once.  Thread (strip of 4 pixels along w, q) sums the input channels
// 4 q .. 4 q + 3 and 16 + 4 q .. + 3 for its 4 pixels x 3 output channels: per channel quad 18 float4 of inputs and 27 of weights
// (the same address in every strip: broadcast) feed 432 FMAs.  The four q lanes of a strip are neighbours: two butterfly steps add
// them, lane q = 0 stores 4 pixels x 3 floats as three 16-byte stores.  Summation order: channel quad, tap, channel, then the q
// lanes -- fixed, so an image's result does not depend on the batch.
constexpr int LT_H = 8, LT_W = 32, LT_C = 32;
constexpr int LT_HR = LT_H + 2, LT_HC = LT_W + 2;
constexpr int LT_PS = 36;                         // floats per staged pixel

__global__ __launch_bounds__(256) void convt_last_kernel(const float* __restrict__ x, const float* __restrict__ w_t, float* __restrict__ out,
                                                         int B, int H, int W) {
    __shared__ __attribute__((aligned(16))) float halo[LT_HR * LT_HC * LT_PS];
    __shared__ __attribute__((aligned(16))) float ws[8 * 9 * 4 * 3];      // [channel quad][tap][channel][ci]
    const int tid = threadIdx.x;
    const int tiles_w = W / LT_W, tiles_h = H / LT_H;
    const int tile = blockIdx.x;
    const int tw = tile % tiles_w, th = (tile / tiles_w) % tiles_h, b = tile / (tiles_w * tiles_h);
    const int h0 = th * LT_H, w0 = tw * LT_W;
    for (int i = tid; i < 8 * 9 * 4 * 3; i += 256) {
        const int ci = i % 3, c = (i / 3) % 4, tap = (i / 12) % 9, cq = i / 108;
        ws[i] = w_t[(ci * 9 + tap) * LT_C + cq * 4 + c];
    }
    for (int i = tid; i < LT_HR * LT_HC * (LT_C / 4); i += 256) {
        const int c4 = i % (LT_C / 4), px = i / (LT_C / 4);
        const int hr = px / LT_HC, hc = px - hr * LT_HC;
        const int ih = h0 - 1 + hr, iw = w0 - 1 + hc;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
            v = *reinterpret_cast<const float4*>(x + (((size_t)b * H + ih) * W + iw) * LT_C + 4 * c4);
        *reinterpret_cast<float4*>(&halo[px * LT_PS + 4 * c4]) = v;
    }
    __syncthreads();
    const int strip = tid >> 2, q = tid & 3;
    const int sr = strip >> 3, sc = (strip & 7) * 4;
    float acc[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc[j][0] = 0.f; acc[j][1] = 0.f; acc[j][2] = 0.f; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cq = h * 4 + q;
        float4 in[3][6];
#pragma unroll
        for (int dr = 0; dr < 3; ++dr)
#pragma unroll
            for (int dc = 0; dc < 6; ++dc)
                in[dr][dc] = *reinterpret_cast<const float4*>(&halo[((sr + dr) * LT_HC + sc + dc) * LT_PS + 4 * cq]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, k = tap - r * 3;
            const float* wp = &ws[(cq * 9 + tap) * 12];
            const float4 wa = *reinterpret_cast<const float4*>(wp), wb = *reinterpret_cast<const float4*>(wp + 4),
                         wc = *reinterpret_cast<const float4*>(wp + 8);
            // [channel][ci]: channel 0 = wa.xyz, 1 = wa.w wb.xy, 2 = wb.zw wc.x, 3 = wc.yzw
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = in[2 - r][j + 2 - k];   // halo row (h + 1 - r) - (h0 - 1) = sr + 2 - r, column likewise
                acc[j][0] = fmaf(v.x, wa.x, acc[j][0]); acc[j][1] = fmaf(v.x, wa.y, acc[j][1]); acc[j][2] = fmaf(v.x, wa.z, acc[j][2]);
                acc[j][0] = fmaf(v.y, wa.w, acc[j][0]); acc[j][1] = fmaf(v.y, wb.x, acc[j][1]); acc[j][2] = fmaf(v.y, wb.y, acc[j][2]);
                acc[j][0] = fmaf(v.z, wb.z, acc[j][0]); acc[j][1] = fmaf(v.z, wb.w, acc[j][1]); acc[j][2] = fmaf(v.z, wc.x, acc[j][2]);
                acc[j][0] = fmaf(v.w, wc.y, acc[j][0]); acc[j][1] = fmaf(v.w, wc.z, acc[j][1]); acc[j][2] = fmaf(v.w, wc.w, acc[j][2]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            float a = acc[j][ci];
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            acc[j][ci] = a;
        }
    if (q == 0) {
        float* op = out + (((size_t)b * H + h0 + sr) * W + w0 + sc) * 3;   // 4 pixels x 3 floats: 48 bytes, 16-byte aligned
        *reinterpret_cast<float4*>(op) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[1][0]);
        *reinterpret_cast<float4*>(op + 4) = make_float4(acc[1][1], acc[1][2], acc[2][0], acc[2][1]);
        *reinterpret_cast<float4*>(op + 8) = make_float4(acc[2][2], acc[3][0], acc[3][1], acc[3][2]);
    }
}

}  // namespace

bool fv_recon_norm_channels_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256 || C == 512 || C == 1024; }

int fv_recon_l2norm_affine(fv_ctx* ctx, const float* x, const float* skip, float* d_out, const float* scale, const float* shift, float* y,
                           long long rows, int C, float leaky) {
    FV_REQUIRE(ctx, x && scale && shift && y, "l2norm_affine: NULL buffer");
    FV_REQUIRE(ctx, fv_recon_norm_channels_ok(C), "l2norm_affine: C = %d is not one of 32, 64, 128, 256, 512, 1024", C);
    FV_REQUIRE(ctx, rows >= 1, "l2norm_affine: rows must be >= 1");
    FV_REQUIRE(ctx, y != x && y != skip && y != d_out, "l2norm_affine: y must be a buffer of its own");
    FvProfScope ps(ctx, "l2norm_affine_kernel", "C" + std::to_string(C), 0.0, 4.0 * (double)rows * C * (2 + (skip ? 1 : 0) + (d_out ? 1 : 0)));
    switch (C) {
    case 32: launch_l2norm<32>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    case 64: launch_l2norm<64>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    case 128: launch_l2norm<128>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    case 256: launch_l2norm<256>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    case 512: launch_l2norm<512>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    default: launch_l2norm<1024>(ctx, x, skip, d_out, scale, shift, y, rows, leaky); break;
    }
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

bool fv_recon_convt_last_ok(int H, int W) { return H >= LT_H && W >= LT_W && H % LT_H == 0 && W % LT_W == 0; }

int fv_recon_convt_last(fv_ctx* ctx, const float* x, const float* w_t, int B, int H, int W, float* out) {
    FV_REQUIRE(ctx, x && w_t && out, "conv2d_transpose: NULL buffer");
    FV_REQUIRE(ctx, B >= 1 && fv_recon_convt_last_ok(H, W), "conv2d_transpose: the 32 -> 3 channel layer needs H %% 8 == 0 and W %% 32 == 0 (H=%d, W=%d)", H, W);
    const long long ntiles = (long long)B * (H / LT_H) * (W / LT_W);
    FV_REQUIRE(ctx, ntiles < (1ll << 31) && (long long)B * H * W * LT_C < (1ll << 31), "conv2d_transpose: batch too large");
    FvProfScope ps(ctx, "convt_last_kernel", 2.0 * B * H * W * 3 * 9.0 * LT_C, 4.0 * ((double)B * H * W * (LT_C + 3)));
    hipLaunchKernelGGL(convt_last_kernel, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, x, w_t, out, B, H, W);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
