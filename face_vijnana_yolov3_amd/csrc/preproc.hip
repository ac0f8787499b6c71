// Letterbox preprocessing on the device: uint8 HxWx3 image -> float32 SxSx3 in [0,1]
// (bicubic resize of the /255 image to (w_p, h_p), zero padding to S x S).
//
// Replaces the cv2.resize(INTER_CUBIC) + cv2.copyMakeBorder pair of the reference
// (face_detection.py:112-147 train, 656-694 evaluate, 798-835 test).  Geometry (target size, pad
// split with the odd row/column at the bottom/right) is exact; pixel values follow OpenCV's
// bicubic kernel (a = -0.75, half-pixel centres, replicated border) in float32 -- "parity
// unpinned" against cv2 itself, which is not installed here.
// HBM-bound: reads each source pixel ~(scale^2 x 16) times through L1/L2, writes 12 B per pixel.
#include <cmath>
#include "common.h"

namespace {

__device__ __forceinline__ void cubic_w(float t, float (&w)[4]) {
    const float a = -0.75f;
    w[0] = ((a * (t + 1.f) - 5.f * a) * (t + 1.f) + 8.f * a) * (t + 1.f) - 4.f * a;
    w[1] = ((a + 2.f) * t - (a + 3.f)) * t * t + 1.f;
    w[2] = ((a + 2.f) * (1.f - t) - (a + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ src, int h, int w, int S, int w_p,
                                                        int h_p, int pad_t, int pad_l, float* __restrict__ dst) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= S || y >= S) return;
    float r = 0.f, g = 0.f, b = 0.f;
    const int xi = x - pad_l, yi = y - pad_t;
    if (xi >= 0 && xi < w_p && yi >= 0 && yi < h_p) {
        // source coordinates in double: at 1080p an fp32 coordinate already costs 5e-5 in the weights
        const double fx = (xi + 0.5) * ((double)w / (double)w_p) - 0.5;
        const double fy = (yi + 0.5) * ((double)h / (double)h_p) - 0.5;
        const int sx = (int)floor(fx), sy = (int)floor(fy);
        float wx[4], wy[4];
        cubic_w((float)(fx - sx), wx);
        cubic_w((float)(fy - sy), wy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = min(max(sy - 1 + j, 0), h - 1);
            float rr = 0.f, gg = 0.f, bb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xx = min(max(sx - 1 + i, 0), w - 1);
                const unsigned char* p = src + ((size_t)yy * w + xx) * 3;
                rr += wx[i] * (float)p[0]; gg += wx[i] * (float)p[1]; bb += wx[i] * (float)p[2];
            }
            r += wy[j] * rr; g += wy[j] * gg; b += wy[j] * bb;
        }
        r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); b *= (1.0f / 255.0f);
    }
    float* o = dst + ((size_t)y * S + x) * 3;
    o[0] = r; o[1] = g; o[2] = b;
}

// the same for a whole batch in ONE launch: blockIdx.z = image; the images' bytes sit back to back in one
// buffer (one host-to-device copy per batch), their geometry comes in the kernel arguments
constexpr int LB_MAX = 64;
struct LbTable { long long off[LB_MAX]; int h[LB_MAX], w[LB_MAX], w_p[LB_MAX], h_p[LB_MAX], pad_t[LB_MAX], pad_l[LB_MAX]; };

__global__ __launch_bounds__(256) void letterbox_batch_kernel(const unsigned char* __restrict__ packed, LbTable t, int S,
                                                              float* __restrict__ dst) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= S || y >= S) return;
    const unsigned char* __restrict__ src = packed + t.off[b];
    const int h = t.h[b], w = t.w[b], w_p = t.w_p[b], h_p = t.h_p[b];
    float r = 0.f, g = 0.f, bl = 0.f;
    const int xi = x - t.pad_l[b], yi = y - t.pad_t[b];
    if (xi >= 0 && xi < w_p && yi >= 0 && yi < h_p) {
        const double fx = (xi + 0.5) * ((double)w / (double)w_p) - 0.5;
        const double fy = (yi + 0.5) * ((double)h / (double)h_p) - 0.5;
        const int sx = (int)floor(fx), sy = (int)floor(fy);
        float wx[4], wy[4];
        cubic_w((float)(fx - sx), wx);
        cubic_w((float)(fy - sy), wy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = min(max(sy - 1 + j, 0), h - 1);
            float rr = 0.f, gg = 0.f, bb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xx = min(max(sx - 1 + i, 0), w - 1);
                const unsigned char* p = src + ((size_t)yy * w + xx) * 3;
                rr += wx[i] * (float)p[0]; gg += wx[i] * (float)p[1]; bb += wx[i] * (float)p[2];
            }
            r += wy[j] * rr; g += wy[j] * gg; bl += wy[j] * bb;
        }
        r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); bl *= (1.0f / 255.0f);
    }
    float* o = dst + (((size_t)b * S + y) * S + x) * 3;
    o[0] = r; o[1] = g; o[2] = bl;
}

// many crops (sub-rectangles of the packed images) in one launch: blockIdx.z = crop.  Crop c starts at byte t.off[c] of `packed`
// (its image's offset plus its top-left pixel) and advances t.pitch[c] bytes per row; everything else is letterbox_kernel for a
// contiguous h x w image -- the same expressions in the same order, the border replicated at the CROP's edges (what cv.resize
// sees after the reference's slice), so the pixels are bit-identical to fv_letterbox of a contiguous copy of the crop.
constexpr int LBC_MAX = 64;    // crops per launch: the table travels in the kernel arguments (64 x 36 B); longer lists are chunked
struct LbcTable { long long off[LBC_MAX]; int pitch[LBC_MAX], h[LBC_MAX], w[LBC_MAX], w_p[LBC_MAX], h_p[LBC_MAX], pad_t[LBC_MAX],
                  pad_l[LBC_MAX]; };

__global__ __launch_bounds__(256) void letterbox_crops_kernel(const unsigned char* __restrict__ packed, LbcTable t, int S,
                                                              float* __restrict__ dst) {
    const int c = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= S || y >= S) return;
    const unsigned char* __restrict__ src = packed + t.off[c];
    const int h = t.h[c], w = t.w[c], w_p = t.w_p[c], h_p = t.h_p[c], pitch = t.pitch[c];
    float r = 0.f, g = 0.f, b = 0.f;
    const int xi = x - t.pad_l[c], yi = y - t.pad_t[c];
    if (xi >= 0 && xi < w_p && yi >= 0 && yi < h_p) {
        const double fx = (xi + 0.5) * ((double)w / (double)w_p) - 0.5;
        const double fy = (yi + 0.5) * ((double)h / (double)h_p) - 0.5;
        const int sx = (int)floor(fx), sy = (int)floor(fy);
        float wx[4], wy[4];
        cubic_w((float)(fx - sx), wx);
        cubic_w((float)(fy - sy), wy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = min(max(sy - 1 + j, 0), h - 1);
            float rr = 0.f, gg = 0.f, bb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xx = min(max(sx - 1 + i, 0), w - 1);
                const unsigned char* p = src + (size_t)yy * pitch + (size_t)xx * 3;
                rr += wx[i] * (float)p[0]; gg += wx[i] * (float)p[1]; bb += wx[i] * (float)p[2];
            }
            r += wy[j] * rr; g += wy[j] * gg; b += wy[j] * bb;
        }
        r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); b *= (1.0f / 255.0f);
    }
    float* o = dst + (((size_t)c * S + y) * S + x) * 3;
    o[0] = r; o[1] = g; o[2] = b;
}

// Nearest-neighbour crop + letterbox on uint8 (create_db_fi, fi.py:113-161: cv.resize(INTER_NEAREST) then cv.copyMakeBorder(0)):
// a pure gather.  A crop's S x S x 3 output is one flat run of 16-byte chunks; a workgroup writes CNU_CHUNKS consecutive chunks of
// crop blockIdx.y, one 16-byte store per lane, lanes on consecutive chunks (1 KiB per wave-instruction), the padding written as
// zeros by the same stores.  The fp64 column index (OpenCV's resizeNN: min(floor(x * ifx), w - 1), ifx = 1.0 / (w_p / (double)w))
// is computed once per output column per workgroup and expanded to a per-output-BYTE table of source byte offsets in LDS (3S
// int32, -1 = padding), so a chunk is 4 ds_read_b128 + 16 byte loads; the row index is one fp64 multiply per chunk.
constexpr int CNU_THREADS = 256;
constexpr int CNU_ITERS = 4;                          // chunks per thread: the table build (3S entries) is amortised over 16 KiB of output
constexpr int CNU_CHUNKS = CNU_THREADS * CNU_ITERS;
constexpr int CNU_MAX_S = 4096;                       // 3S int32 of LDS <= 48 KiB

__global__ __launch_bounds__(CNU_THREADS) void crop_nearest_u8_kernel(const unsigned char* __restrict__ packed, LbcTable t, int S,
                                                                      unsigned char* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) int cnu_src[];      // [3S]: source byte offset inside a row of output byte b, or -1
    const int c = blockIdx.y;
    const int h = t.h[c], w = t.w[c], w_p = t.w_p[c], h_p = t.h_p[c], pitch = t.pitch[c], pad_t = t.pad_t[c], pad_l = t.pad_l[c];
    const double ifx = 1.0 / ((double)w_p / (double)w), ify = 1.0 / ((double)h_p / (double)h);
    for (int x = threadIdx.x; x < S; x += CNU_THREADS) {
        const int xi = x - pad_l;
        int o = -1;
        if (xi >= 0 && xi < w_p) o = min((int)floor(xi * ifx), w - 1) * 3;
        cnu_src[3 * x] = o; cnu_src[3 * x + 1] = o < 0 ? -1 : o + 1; cnu_src[3 * x + 2] = o < 0 ? -1 : o + 2;
    }
    __syncthreads();
    const unsigned char* __restrict__ src = packed + t.off[c];
    const int row_chunks = 3 * S / 16, n_chunks = S * row_chunks;
    uint4* __restrict__ out = reinterpret_cast<uint4*>(dst + (size_t)c * S * S * 3);
#pragma unroll
    for (int it = 0; it < CNU_ITERS; ++it) {
        const int q = blockIdx.x * CNU_CHUNKS + it * CNU_THREADS + threadIdx.x;
        if (q >= n_chunks) break;
        const int y = q / row_chunks, j = q - y * row_chunks;
        const int yi = y - pad_t;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        if (yi >= 0 && yi < h_p) {
            const unsigned char* __restrict__ row = src + (size_t)min((int)floor(yi * ify), h - 1) * pitch;
            const int4* tab = reinterpret_cast<const int4*>(cnu_src + 16 * j);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int4 o = tab[k];
                const unsigned b0 = o.x >= 0 ? row[o.x] : 0u, b1 = o.y >= 0 ? row[o.y] : 0u;
                const unsigned b2 = o.z >= 0 ? row[o.z] : 0u, b3 = o.w >= 0 ? row[o.w] : 0u;
                v[k] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            }
        }
        out[q] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// Training augmentation (hps['augment']): letterbox_crops_kernel for ONE crop per image, letterboxed into a T x T box
// at (oy, ox) of the otherwise zero S x S canvas, the finished canvas optionally mirrored (x -> S - 1 - x) and the pixel's colour
// distorted in HSV, in the same pass.  The resampling is letterbox_crops_kernel's -- the same expressions in the same order -- so
// without colour the box holds that kernel's bits.  A workgroup makes LBA_TW x LBA_TH output pixels: the fp64 source coordinate and
// the four weights of each of its columns and rows are computed once (80 threads) into LDS; then every thread makes four pixels
// of one column (64 columns x 4 rows per pass, the passes unrolled so that their loads are in flight together), the tile is staged
// in LDS and stored as 16-byte chunks on consecutive lanes (768 B per row segment).
constexpr int LBA_MAX = 64;         // images per launch: the table travels in the kernel arguments (64 x 52 B); longer batches are chunked
constexpr int LBA_TW = 64, LBA_TH = 16, LBA_ROWS = 4;       // tile; rows per pass (256 threads = 64 columns x 4 rows)
constexpr int LBA_OUT = -2147483647 - 1;  // a column / row outside the placed content
struct LbaTable { long long off[LBA_MAX]; int pitch[LBA_MAX], h[LBA_MAX], w[LBA_MAX], w_p[LBA_MAX], h_p[LBA_MAX], top[LBA_MAX],
                  left[LBA_MAX], mode[LBA_MAX];     // mode: bit 0 = flip, bit 1 = the colour stage runs
                  float dh[LBA_MAX], sat[LBA_MAX], ex[LBA_MAX]; };

// Darknet's distort_image in float32: clamp, RGB -> HSV (h in turns), h += dh (wrapped), s *= sat, v *= ex, HSV -> RGB, clamp
__device__ __forceinline__ void lba_colour(float& r, float& g, float& b, float dh, float sat, float ex) {
    r = fminf(fmaxf(r, 0.f), 1.f); g = fminf(fmaxf(g, 0.f), 1.f); b = fminf(fmaxf(b, 0.f), 1.f);
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b)), d = mx - mn;
    float s = mx == 0.f ? 0.f : d / mx, v = mx, hh = 0.f;
    if (d != 0.f) hh = r == mx ? (g - b) / d : (g == mx ? 2.f + (b - r) / d : 4.f + (r - g) / d);
    hh = hh < 0.f ? hh + 6.f : hh;
    hh = hh / 6.f;
    hh = hh + dh; hh = hh - floorf(hh);
    s = s * sat; v = v * ex;
    const float h6 = 6.f * hh, fl = floorf(h6), f = h6 - fl;
    const int i = (int)fl % 6;
    const float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
    switch (i) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    r = fminf(fmaxf(r, 0.f), 1.f); g = fminf(fmaxf(g, 0.f), 1.f); b = fminf(fmaxf(b, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void letterbox_augment_kernel(const unsigned char* __restrict__ packed, LbaTable t, int S,
                                                                float* __restrict__ dst) {
    __shared__ int col_s[LBA_TW], row_s[LBA_TH];                                  // floor of the source coordinate, or LBA_OUT
    __shared__ __attribute__((aligned(16))) float col_w[LBA_TW][4], row_w[LBA_TH][4];
    __shared__ __attribute__((aligned(16))) float out_s[LBA_TH][LBA_TW * 3];
    const int b = blockIdx.z, x0 = blockIdx.x * LBA_TW, y0 = blockIdx.y * LBA_TH, tid = threadIdx.x;
    const int h = t.h[b], w = t.w[b], w_p = t.w_p[b], h_p = t.h_p[b], pitch = t.pitch[b], mode = t.mode[b];
    if (tid < LBA_TW) {
        const int x = x0 + tid;
        const int xi = ((mode & 1) ? S - 1 - x : x) - t.left[b];                  // undo the flip, then the placement
        int s = LBA_OUT;
        float wx[4] = {0.f, 0.f, 0.f, 0.f};
        if (x < S && xi >= 0 && xi < w_p) {
            const double fx = (xi + 0.5) * ((double)w / (double)w_p) - 0.5;
            s = (int)floor(fx);
            cubic_w((float)(fx - s), wx);
        }
        col_s[tid] = s;
#pragma unroll
        for (int i = 0; i < 4; ++i) col_w[tid][i] = wx[i];
    } else if (tid < LBA_TW + LBA_TH) {
        const int j = tid - LBA_TW, y = y0 + j;
        const int yi = y - t.top[b];
        int s = LBA_OUT;
        float wy[4] = {0.f, 0.f, 0.f, 0.f};
        if (y < S && yi >= 0 && yi < h_p) {
            const double fy = (yi + 0.5) * ((double)h / (double)h_p) - 0.5;
            s = (int)floor(fy);
            cubic_w((float)(fy - s), wy);
        }
        row_s[j] = s;
#pragma unroll
        for (int i = 0; i < 4; ++i) row_w[j][i] = wy[i];
    }
    __syncthreads();
    const unsigned char* __restrict__ src = packed + t.off[b];
    const int lx = tid & (LBA_TW - 1), ly = tid >> 6;
    const int sx = col_s[lx];
    const float4 wxv = *reinterpret_cast<const float4*>(col_w[lx]);
    const float wx[4] = {wxv.x, wxv.y, wxv.z, wxv.w};
    int xo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xo[i] = sx == LBA_OUT ? 0 : min(max(sx - 1 + i, 0), w - 1) * 3;
    // interior columns: the four taps are 12 contiguous bytes of a source row -- one (unaligned) 12-byte load per tap row instead of
    // twelve byte loads; the values, and the arithmetic on them, are the same
    const bool inner = sx != LBA_OUT && sx >= 1 && sx + 2 <= w - 1;
    const float dh = t.dh[b], sat = t.sat[b], ex = t.ex[b];
#pragma unroll
    for (int pass = 0; pass < LBA_TH / LBA_ROWS; ++pass) {
        const int j0 = pass * LBA_ROWS + ly;
        const int sy = row_s[j0];
        float r = 0.f, g = 0.f, bl = 0.f;
        if (sx != LBA_OUT && sy != LBA_OUT) {
            const float4 wyv = *reinterpret_cast<const float4*>(row_w[j0]);
            const float wy[4] = {wyv.x, wyv.y, wyv.z, wyv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = min(max(sy - 1 + j, 0), h - 1);
                const unsigned char* __restrict__ row = src + (size_t)yy * pitch;
                float rr = 0.f, gg = 0.f, bb = 0.f;
                if (inner) {
                    unsigned v[3];
                    __builtin_memcpy(v, row + xo[0], 12);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float p0 = (float)((v[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
                        const float p1 = (float)((v[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
                        const float p2 = (float)((v[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
                        rr += wx[i] * p0; gg += wx[i] * p1; bb += wx[i] * p2;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned char* p = row + xo[i];
                        rr += wx[i] * (float)p[0]; gg += wx[i] * (float)p[1]; bb += wx[i] * (float)p[2];
                    }
                }
                r += wy[j] * rr; g += wy[j] * gg; bl += wy[j] * bb;
            }
            r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); bl *= (1.0f / 255.0f);
            if (mode & 2) lba_colour(r, g, bl, dh, sat, ex);
        }
        out_s[j0][3 * lx] = r; out_s[j0][3 * lx + 1] = g; out_s[j0][3 * lx + 2] = bl;
    }
    __syncthreads();
    // the tile as 16-byte chunks, consecutive lanes on consecutive chunks of a row segment (768 B where the tile is full)
    constexpr int ROW_Q = LBA_TW * 3 / 4;
    const int row_q = 3 * min(LBA_TW, S - x0) / 4;                                 // chunks of this tile's row segment (S % 4 == 0)
#pragma unroll
    for (int q = tid; q < LBA_TH * ROW_Q; q += 256) {
        const int rr = q / ROW_Q, k = q - rr * ROW_Q;
        const int y = y0 + rr;
        if (y < S && k < row_q)
            reinterpret_cast<float4*>(dst + (((size_t)b * S + y) * S + x0) * 3)[k] = reinterpret_cast<const float4*>(out_s[rr])[k];
    }
}

// Mosaic (hps['mosaic']): a canvas is made of up to four TILES.  A tile is letterbox_augment_kernel's placed crop -- the
// ch x cw crop letterboxed into a T x T box at (oy, ox), which may reach beyond the canvas -- seen through a WINDOW [wy0, wy1) x
// [wx0, wx1) of the canvas; a tile's flip mirrors its box in place (local column c -> T - 1 - c).  The windows of a canvas are
// disjoint; a pixel outside every window, or inside a window but outside the tile's content, is +0.  A workgroup makes the same
// 64 x 16 output pixels as letterbox_augment_kernel: it zero-fills its LDS stage, then for every tile of its canvas whose window
// meets its rectangle (a workgroup-uniform test: most workgroups meet one tile, those on a seam two, the one on the centre four)
// builds the column / row tables and evaluates the taps -- letterbox_augment_kernel's expressions in the same order, so a tile
// holds letterbox_crops_kernel's bits at image size T -- writing the lanes inside window and content; one barrier, then the same
// 16-byte row-segment stores.  The tile table travels in the kernel arguments, MOS_TILES tiles (whole canvases) per launch.
constexpr int MOS_TILES = 48;       // tiles per launch (48 x 68 B of kernel arguments); MOS_PER = tiles per canvas at most
constexpr int MOS_PER = 4;
struct MosTable { long long off[MOS_TILES]; int pitch[MOS_TILES], h[MOS_TILES], w[MOS_TILES], w_p[MOS_TILES], h_p[MOS_TILES],
                  top[MOS_TILES],          // canvas row of the content's first row
                  xa[MOS_TILES],           // content column xi of canvas column x: x - xa, under a flip xa - x
                  mode[MOS_TILES],         // bit 0 = flip, bit 1 = the colour stage runs
                  wy0[MOS_TILES], wx0[MOS_TILES], wy1[MOS_TILES], wx1[MOS_TILES];
                  float dh[MOS_TILES], sat[MOS_TILES], ex[MOS_TILES];
                  unsigned char first[MOS_TILES + 1]; };    // canvas z of the launch owns the tiles [first[z], first[z + 1])

__global__ __launch_bounds__(256) void letterbox_mosaic_kernel(const unsigned char* __restrict__ packed, MosTable t, int S,
                                                               float* __restrict__ dst) {
    __shared__ int col_s[LBA_TW], row_s[LBA_TH];                                  // floor of the source coordinate, or LBA_OUT
    __shared__ __attribute__((aligned(16))) float col_w[LBA_TW][4], row_w[LBA_TH][4];
    __shared__ __attribute__((aligned(16))) float out_s[LBA_TH][LBA_TW * 3];
    const int b = blockIdx.z, x0 = blockIdx.x * LBA_TW, y0 = blockIdx.y * LBA_TH, tid = threadIdx.x;
    constexpr int ROW_Q = LBA_TW * 3 / 4;
#pragma unroll
    for (int q = tid; q < LBA_TH * ROW_Q; q += 256) reinterpret_cast<float4*>(&out_s[0][0])[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int lx = tid & (LBA_TW - 1), ly = tid >> 6;
    const int k1 = t.first[b + 1];
    for (int k = t.first[b]; k < k1; ++k) {
        const int wy0 = t.wy0[k], wx0 = t.wx0[k], wy1 = t.wy1[k], wx1 = t.wx1[k];
        if (wx1 <= x0 || wx0 >= x0 + LBA_TW || wy1 <= y0 || wy0 >= y0 + LBA_TH) continue;    // the same in every lane of the workgroup
        const int h = t.h[k], w = t.w[k], w_p = t.w_p[k], h_p = t.h_p[k], pitch = t.pitch[k], mode = t.mode[k];
        __syncthreads();                                                          // the tables of the tile before are read; the stage is zeroed
        if (tid < LBA_TW) {
            const int x = x0 + tid;
            const int xi = (mode & 1) ? t.xa[k] - x : x - t.xa[k];                // undo the window's placement and the in-box flip
            int s = LBA_OUT;
            float wx[4] = {0.f, 0.f, 0.f, 0.f};
            if (x >= wx0 && x < wx1 && xi >= 0 && xi < w_p) {
                const double fx = (xi + 0.5) * ((double)w / (double)w_p) - 0.5;
                s = (int)floor(fx);
                cubic_w((float)(fx - s), wx);
            }
            col_s[tid] = s;
#pragma unroll
            for (int i = 0; i < 4; ++i) col_w[tid][i] = wx[i];
        } else if (tid < LBA_TW + LBA_TH) {
            const int j = tid - LBA_TW, y = y0 + j;
            const int yi = y - t.top[k];
            int s = LBA_OUT;
            float wy[4] = {0.f, 0.f, 0.f, 0.f};
            if (y >= wy0 && y < wy1 && yi >= 0 && yi < h_p) {
                const double fy = (yi + 0.5) * ((double)h / (double)h_p) - 0.5;
                s = (int)floor(fy);
                cubic_w((float)(fy - s), wy);
            }
            row_s[j] = s;
#pragma unroll
            for (int i = 0; i < 4; ++i) row_w[j][i] = wy[i];
        }
        __syncthreads();
        const unsigned char* __restrict__ src = packed + t.off[k];
        const int sx = col_s[lx];
        const float4 wxv = *reinterpret_cast<const float4*>(col_w[lx]);
        const float wx[4] = {wxv.x, wxv.y, wxv.z, wxv.w};
        int xo[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xo[i] = sx == LBA_OUT ? 0 : min(max(sx - 1 + i, 0), w - 1) * 3;
        const bool inner = sx != LBA_OUT && sx >= 1 && sx + 2 <= w - 1;           // the four taps are 12 contiguous bytes of a source row
        const float dh = t.dh[k], sat = t.sat[k], ex = t.ex[k];
#pragma unroll
        for (int pass = 0; pass < LBA_TH / LBA_ROWS; ++pass) {
            const int j0 = pass * LBA_ROWS + ly;
            const int sy = row_s[j0];
            if (sx != LBA_OUT && sy != LBA_OUT) {
                float r = 0.f, g = 0.f, bl = 0.f;
                const float4 wyv = *reinterpret_cast<const float4*>(row_w[j0]);
                const float wy[4] = {wyv.x, wyv.y, wyv.z, wyv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int yy = min(max(sy - 1 + j, 0), h - 1);
                    const unsigned char* __restrict__ row = src + (size_t)yy * pitch;
                    float rr = 0.f, gg = 0.f, bb = 0.f;
                    if (inner) {
                        unsigned v[3];
                        __builtin_memcpy(v, row + xo[0], 12);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float p0 = (float)((v[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
                            const float p1 = (float)((v[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
                            const float p2 = (float)((v[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
                            rr += wx[i] * p0; gg += wx[i] * p1; bb += wx[i] * p2;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const unsigned char* p = row + xo[i];
                            rr += wx[i] * (float)p[0]; gg += wx[i] * (float)p[1]; bb += wx[i] * (float)p[2];
                        }
                    }
                    r += wy[j] * rr; g += wy[j] * gg; bl += wy[j] * bb;
                }
                r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); bl *= (1.0f / 255.0f);
                if (mode & 2) lba_colour(r, g, bl, dh, sat, ex);
                out_s[j0][3 * lx] = r; out_s[j0][3 * lx + 1] = g; out_s[j0][3 * lx + 2] = bl;   // a thread's own pixel in every tile
            }
        }
    }
    __syncthreads();
    const int row_q = 3 * min(LBA_TW, S - x0) / 4;                                 // chunks of this tile's row segment (S % 4 == 0)
#pragma unroll
    for (int q = tid; q < LBA_TH * ROW_Q; q += 256) {
        const int rr = q / ROW_Q, kq = q - rr * ROW_Q;
        const int y = y0 + rr;
        if (y < S && kq < row_q)
            reinterpret_cast<float4*>(dst + (((size_t)b * S + y) * S + x0) * 3)[kq] = reinterpret_cast<const float4*>(out_s[rr])[kq];
    }
}

bool lb_geometry(int h, int w, int S, int* g) {
    int w_p, h_p, pad_t = 0, pad_b = 0, pad_l = 0, pad_r = 0;
    if (w >= h) {   // face_detection.py:120-133
        w_p = S; h_p = (int)((double)h / (double)w * S);
        int pad = S - h_p; pad_t = pad / 2; pad_b = pad - pad_t;
    } else {        // face_detection.py:134-147
        h_p = S; w_p = (int)((double)w / (double)h * S);
        int pad = S - w_p; pad_l = pad / 2; pad_r = pad - pad_l;
    }
    g[0] = w_p; g[1] = h_p; g[2] = pad_t; g[3] = pad_b; g[4] = pad_l; g[5] = pad_r;
    return w_p >= 1 && h_p >= 1;
}

// every record of a crop list (image, y0, x0, h, w) inside its image and letterboxable: checked before anything is enqueued,
// so a bad record leaves dst untouched
int lbc_validate(fv_ctx* ctx, const char* who, const int64_t* offsets, const int32_t* hw, int n_img, const int32_t* crops, int n, int S) {
    for (int c = 0; c < n; ++c) {
        const int* r = crops + 5 * c;
        const int im = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
        FV_REQUIRE(ctx, im >= 0 && im < n_img, "%s: crop %d names image %d of %d", who, c, im, n_img);
        const int H = hw[2 * im], W = hw[2 * im + 1];
        FV_REQUIRE(ctx, H >= 1 && W >= 1 && offsets[im] >= 0, "%s: bad image %d", who, im);
        FV_REQUIRE(ctx, h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= H - h && x0 <= W - w,
                   "%s: crop %d (y0 %d, x0 %d, h %d, w %d) outside image %d (%d x %d)", who, c, y0, x0, h, w, im, H, W);
        int g[6];
        FV_REQUIRE(ctx, lb_geometry(h, w, S, g), "%s: crop %d (%d x %d) too elongated for image_size %d", who, c, h, w, S);
    }
    return FV_OK;
}

// crops [c0, c0 + nc) as the kernels' table; -> source bytes of those crops
double lbc_fill(LbcTable& t, const int64_t* offsets, const int32_t* hw, const int32_t* crops, int c0, int nc, int S) {
    double bytes = 0.0;
    for (int i = 0; i < nc; ++i) {
        const int* r = crops + 5 * (c0 + i);
        const int im = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
        const int W = hw[2 * im + 1];
        int g[6];
        lb_geometry(h, w, S, g);
        t.off[i] = offsets[im] + ((long long)y0 * W + x0) * 3; t.pitch[i] = W * 3;
        t.h[i] = h; t.w[i] = w; t.w_p[i] = g[0]; t.h_p[i] = g[1]; t.pad_t[i] = g[2]; t.pad_l[i] = g[4];
        bytes += (double)h * w * 3;
    }
    return bytes;
}

}  // namespace

extern "C" int fv_letterbox_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                  int image_size, float* dst, int32_t* geom) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && dst && n >= 1 && image_size >= 1, "letterbox_batch: bad arguments");
    const int S = image_size;
    for (int b0 = 0; b0 < n; b0 += LB_MAX) {
        const int nb = n - b0 < LB_MAX ? n - b0 : LB_MAX;
        LbTable t{};
        double bytes = 0.0;
        for (int i = 0; i < nb; ++i) {
            const int h = hw[2 * (b0 + i)], w = hw[2 * (b0 + i) + 1];
            int g[6];
            FV_REQUIRE(ctx, h >= 1 && w >= 1 && offsets[b0 + i] >= 0, "letterbox_batch: bad image %d", b0 + i);
            FV_REQUIRE(ctx, lb_geometry(h, w, S, g), "letterbox_batch: image %d too elongated for image_size %d", b0 + i, S);
            t.off[i] = offsets[b0 + i]; t.h[i] = h; t.w[i] = w; t.w_p[i] = g[0]; t.h_p[i] = g[1]; t.pad_t[i] = g[2]; t.pad_l[i] = g[4];
            if (geom) for (int k = 0; k < 6; ++k) geom[6 * (b0 + i) + k] = g[k];
            bytes += (double)h * w * 3 + 12.0 * S * S;
        }
        FvProfScope ps(ctx, "letterbox_batch_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_batch_kernel, dim3((S + 15) / 16, (S + 15) / 16, nb), dim3(256), 0, ctx->stream, packed, t, S,
                           dst + (size_t)b0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox_crops(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                  const int32_t* crops, int n, int image_size, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && crops && dst && n_img >= 1 && n >= 1 && image_size >= 1, "letterbox_crops: bad arguments");
    const int S = image_size;
    if (int rc = lbc_validate(ctx, "letterbox_crops", offsets, hw, n_img, crops, n, S)) return rc;
    for (int c0 = 0; c0 < n; c0 += LBC_MAX) {
        const int nc = n - c0 < LBC_MAX ? n - c0 : LBC_MAX;
        LbcTable t{};
        const double bytes = lbc_fill(t, offsets, hw, crops, c0, nc, S) + 12.0 * S * S * nc;
        FvProfScope ps(ctx, "letterbox_crops_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_crops_kernel, dim3((S + 15) / 16, (S + 15) / 16, nc), dim3(256), 0, ctx->stream, packed, t, S,
                           dst + (size_t)c0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox_augment_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                          int image_size, const int32_t* place, const float* colour, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && place && dst && n >= 1 && image_size >= 4 && image_size % 4 == 0 && ((uintptr_t)dst & 15) == 0,
               "letterbox_augment_batch: bad arguments (image_size a multiple of 4 and dst 16-byte aligned: rows are stored 16 bytes at a time)");
    const int S = image_size;
    // every record before anything is enqueued: a bad one leaves dst untouched
    for (int i = 0; i < n; ++i) {
        const int H = hw[2 * i], W = hw[2 * i + 1];
        const int* r = place + 8 * i;
        const int cy0 = r[0], cx0 = r[1], ch = r[2], cw = r[3], T = r[4], oy = r[5], ox = r[6], flip = r[7];
        FV_REQUIRE(ctx, H >= 1 && W >= 1 && offsets[i] >= 0, "letterbox_augment_batch: bad image %d", i);
        FV_REQUIRE(ctx, ch >= 1 && cw >= 1 && cy0 >= 0 && cx0 >= 0 && cy0 <= H - ch && cx0 <= W - cw,
                   "letterbox_augment_batch: crop (y0 %d, x0 %d, h %d, w %d) outside image %d (%d x %d)", cy0, cx0, ch, cw, i, H, W);
        FV_REQUIRE(ctx, T >= 1 && T <= S && oy >= 0 && ox >= 0 && oy <= S - T && ox <= S - T,
                   "letterbox_augment_batch: image %d: box of side %d at (y %d, x %d) outside the %d x %d canvas", i, T, oy, ox, S, S);
        int g[6];
        FV_REQUIRE(ctx, lb_geometry(ch, cw, T, g), "letterbox_augment_batch: image %d: crop %d x %d too elongated for a box of side %d", i, ch, cw, T);
        FV_REQUIRE(ctx, flip == 0 || flip == 1, "letterbox_augment_batch: image %d: flip %d is neither 0 nor 1", i, flip);
        if (colour)
            FV_REQUIRE(ctx, std::isfinite(colour[3 * i]) && std::isfinite(colour[3 * i + 1]) && std::isfinite(colour[3 * i + 2]),
                       "letterbox_augment_batch: image %d: colour parameters are not finite", i);
    }
    for (int b0 = 0; b0 < n; b0 += LBA_MAX) {
        const int nb = n - b0 < LBA_MAX ? n - b0 : LBA_MAX;
        LbaTable t{};
        double bytes = 0.0;
        for (int i = 0; i < nb; ++i) {
            const int W = hw[2 * (b0 + i) + 1];
            const int* r = place + 8 * (b0 + i);
            const float* c = colour ? colour + 3 * (b0 + i) : nullptr;
            int g[6];
            lb_geometry(r[2], r[3], r[4], g);
            t.off[i] = offsets[b0 + i] + ((long long)r[0] * W + r[1]) * 3; t.pitch[i] = W * 3;
            t.h[i] = r[2]; t.w[i] = r[3]; t.w_p[i] = g[0]; t.h_p[i] = g[1]; t.top[i] = r[5] + g[2]; t.left[i] = r[6] + g[4];
            const bool col = c && !(c[0] == 0.f && c[1] == 1.f && c[2] == 1.f);       // exactly (0, 1, 1): the stage is skipped
            t.mode[i] = r[7] | (col ? 2 : 0);
            t.dh[i] = col ? c[0] : 0.f; t.sat[i] = col ? c[1] : 1.f; t.ex[i] = col ? c[2] : 1.f;
            bytes += (double)r[2] * r[3] * 3 + 12.0 * S * S;
        }
        FvProfScope ps(ctx, "letterbox_augment_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_augment_kernel, dim3((S + LBA_TW - 1) / LBA_TW, (S + LBA_TH - 1) / LBA_TH, nb), dim3(256), 0,
                           ctx->stream, packed, t, S, dst + (size_t)b0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox_mosaic_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                         int image_size, int n_out, const int32_t* tiles, const float* colour, int n_tiles, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && tiles && dst && n_img >= 1 && n_out >= 1 && n_tiles >= n_out && n_tiles <= MOS_PER * (long long)n_out &&
                        image_size >= 4 && image_size % 4 == 0 && ((uintptr_t)dst & 15) == 0,
               "letterbox_mosaic_batch: bad arguments (1 to 4 tiles per canvas, image_size a multiple of 4 and dst 16-byte aligned: rows are "
               "stored 16 bytes at a time)");
    const int S = image_size;
    // every record before anything is enqueued: a bad one leaves dst untouched
    int canvas = 0, first = 0;                                       // the canvas being read and its first tile
    for (int k = 0; k < n_tiles; ++k) {
        const int* r = tiles + 14 * k;
        const int cv = r[0], im = r[1], cy0 = r[2], cx0 = r[3], ch = r[4], cw = r[5], T = r[6], oy = r[7], ox = r[8], flip = r[9];
        const int wy0 = r[10], wx0 = r[11], wy1 = r[12], wx1 = r[13];
        FV_REQUIRE(ctx, cv >= 0 && cv < n_out && (cv == canvas || (cv == canvas + 1 && k > first)),
                   "letterbox_mosaic_batch: tile %d names canvas %d after canvas %d (of %d): the tiles are sorted by canvas and every canvas "
                   "has at least one", k, cv, canvas, n_out);
        if (cv != canvas) { canvas = cv; first = k; }
        FV_REQUIRE(ctx, k - first < MOS_PER, "letterbox_mosaic_batch: canvas %d has more than %d tiles", cv, MOS_PER);
        FV_REQUIRE(ctx, im >= 0 && im < n_img, "letterbox_mosaic_batch: tile %d names image %d of %d", k, im, n_img);
        const int H = hw[2 * im], W = hw[2 * im + 1];
        FV_REQUIRE(ctx, H >= 1 && W >= 1 && offsets[im] >= 0, "letterbox_mosaic_batch: bad image %d", im);
        FV_REQUIRE(ctx, ch >= 1 && cw >= 1 && cy0 >= 0 && cx0 >= 0 && cy0 <= H - ch && cx0 <= W - cw,
                   "letterbox_mosaic_batch: tile %d: crop (y0 %d, x0 %d, h %d, w %d) outside image %d (%d x %d)", k, cy0, cx0, ch, cw, im, H, W);
        FV_REQUIRE(ctx, T >= 1 && T <= 4LL * S && oy >= -T && ox >= -T && oy <= S && ox <= S,
                   "letterbox_mosaic_batch: tile %d: box of side %d at (y %d, x %d): 1 <= side <= 4 x %d and -side <= y, x <= %d", k, T, oy, ox, S, S);
        int g[6];
        FV_REQUIRE(ctx, lb_geometry(ch, cw, T, g), "letterbox_mosaic_batch: tile %d: crop %d x %d too elongated for a box of side %d", k, ch, cw, T);
        FV_REQUIRE(ctx, flip == 0 || flip == 1, "letterbox_mosaic_batch: tile %d: flip %d is neither 0 nor 1", k, flip);
        FV_REQUIRE(ctx, wy0 >= 0 && wx0 >= 0 && wy0 < wy1 && wx0 < wx1 && wy1 <= S && wx1 <= S,
                   "letterbox_mosaic_batch: tile %d: window rows [%d, %d) columns [%d, %d) is empty or outside the %d x %d canvas", k, wy0, wy1,
                   wx0, wx1, S, S);
        for (int j = first; j < k; ++j) {
            const int* q = tiles + 14 * j;
            FV_REQUIRE(ctx, wy1 <= q[10] || q[12] <= wy0 || wx1 <= q[11] || q[13] <= wx0,
                       "letterbox_mosaic_batch: the windows of tiles %d and %d of canvas %d overlap", j, k, cv);
        }
        if (colour)
            FV_REQUIRE(ctx, std::isfinite(colour[3 * k]) && std::isfinite(colour[3 * k + 1]) && std::isfinite(colour[3 * k + 2]),
                       "letterbox_mosaic_batch: tile %d: colour parameters are not finite", k);
    }
    FV_REQUIRE(ctx, canvas == n_out - 1, "letterbox_mosaic_batch: canvas %d of %d has no tile", canvas + 1, n_out);
    // whole canvases per launch, as many as MOS_TILES tiles hold
    for (int k0 = 0, c0 = 0; k0 < n_tiles;) {
        MosTable t{};
        double bytes = 0.0;
        int nt = 0, nc = 0;
        while (k0 + nt < n_tiles) {
            int m = 1;
            while (k0 + nt + m < n_tiles && tiles[14 * (k0 + nt + m)] == tiles[14 * (k0 + nt)]) ++m;    // the tiles of the next canvas
            if (nt + m > MOS_TILES) break;
            t.first[nc] = (unsigned char)nt;
            for (int i = nt; i < nt + m; ++i) {
                const int* r = tiles + 14 * (k0 + i);
                const float* c = colour ? colour + 3 * (k0 + i) : nullptr;
                const int W = hw[2 * r[1] + 1];
                int g[6];
                lb_geometry(r[4], r[5], r[6], g);
                t.off[i] = offsets[r[1]] + ((long long)r[2] * W + r[3]) * 3; t.pitch[i] = W * 3;
                t.h[i] = r[4]; t.w[i] = r[5]; t.w_p[i] = g[0]; t.h_p[i] = g[1]; t.top[i] = r[7] + g[2];
                t.xa[i] = r[9] ? r[8] + r[6] - 1 - g[4] : r[8] + g[4];
                const bool col = c && !(c[0] == 0.f && c[1] == 1.f && c[2] == 1.f);       // exactly (0, 1, 1): the stage is skipped
                t.mode[i] = r[9] | (col ? 2 : 0);
                t.wy0[i] = r[10]; t.wx0[i] = r[11]; t.wy1[i] = r[12]; t.wx1[i] = r[13];
                t.dh[i] = col ? c[0] : 0.f; t.sat[i] = col ? c[1] : 1.f; t.ex[i] = col ? c[2] : 1.f;
                bytes += (double)r[4] * r[5] * 3;
            }
            nt += m; ++nc;
            t.first[nc] = (unsigned char)nt;
        }
        bytes += 12.0 * S * S * nc;
        FvProfScope ps(ctx, "letterbox_mosaic_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_mosaic_kernel, dim3((S + LBA_TW - 1) / LBA_TW, (S + LBA_TH - 1) / LBA_TH, nc), dim3(256), 0,
                           ctx->stream, packed, t, S, dst + (size_t)c0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
        k0 += nt; c0 += nc;
    }
    return FV_OK;
}

extern "C" int fv_crop_nearest_u8(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                  const int32_t* crops, int n, int image_size, uint8_t* dst) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n >= 0 && image_size >= 16 && image_size % 16 == 0 && image_size <= CNU_MAX_S,
               "crop_nearest_u8: n %d, image_size %d (a multiple of 16 up to %d: rows are stored 16 bytes at a time)", n, image_size,
               CNU_MAX_S);
    if (n == 0) return FV_OK;
    FV_REQUIRE(ctx, packed && offsets && hw && crops && dst && n_img >= 1 && ((uintptr_t)dst & 15) == 0,
               "crop_nearest_u8: bad arguments (dst must be 16-byte aligned)");
    const int S = image_size;
    if (int rc = lbc_validate(ctx, "crop_nearest_u8", offsets, hw, n_img, crops, n, S)) return rc;
    // The crop table travels in the kernel arguments, LBC_MAX crops per launch, as in fv_letterbox_crops: no device allocation, no
    // host-to-device copy of a pageable table (which would block the host) and nothing that has to outlive the call; one launch of
    // 64 crops is already ~2 000 workgroups at 416.
    const int blocks = (S * (3 * S / 16) + CNU_CHUNKS - 1) / CNU_CHUNKS;
    for (int c0 = 0; c0 < n; c0 += LBC_MAX) {
        const int nc = n - c0 < LBC_MAX ? n - c0 : LBC_MAX;
        LbcTable t{};
        const double bytes = lbc_fill(t, offsets, hw, crops, c0, nc, S) + 3.0 * S * S * nc;
        FvProfScope ps(ctx, "crop_nearest_u8_kernel", 0.0, bytes);
        hipLaunchKernelGGL(crop_nearest_u8_kernel, dim3(blocks, nc), dim3(CNU_THREADS), 3 * S * sizeof(int), ctx->stream, packed, t,
                           S, dst + (size_t)c0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox(fv_ctx* ctx, const uint8_t* src, int h, int w, int image_size, float* dst, int32_t* geom) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, src && dst && h >= 1 && w >= 1 && image_size >= 1, "letterbox: bad arguments");
    const int S = image_size;
    int w_p, h_p, pad_t = 0, pad_b = 0, pad_l = 0, pad_r = 0;
    if (w >= h) {   // face_detection.py:120-133
        w_p = S; h_p = (int)((double)h / (double)w * S);
        int pad = S - h_p; pad_t = pad / 2; pad_b = pad - pad_t;
    } else {        // face_detection.py:134-147
        h_p = S; w_p = (int)((double)w / (double)h * S);
        int pad = S - w_p; pad_l = pad / 2; pad_r = pad - pad_l;
    }
    FV_REQUIRE(ctx, w_p >= 1 && h_p >= 1, "letterbox: image too elongated for image_size %d", S);
    if (geom) { geom[0] = w_p; geom[1] = h_p; geom[2] = pad_t; geom[3] = pad_b; geom[4] = pad_l; geom[5] = pad_r; }
    FvProfScope ps(ctx, "letterbox_kernel", 0.0, (double)h * w * 3 + 12.0 * S * S);
    hipLaunchKernelGGL(letterbox_kernel, dim3((S + 15) / 16, (S + 15) / 16), dim3(256), 0, ctx->stream, src, h, w, S, w_p, h_p,
                       pad_t, pad_l, dst);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
