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

// ONE resampling serves every bicubic kernel of this file: lb_axis (an output index -> floor of its source coordinate and four
// weights) and lb_pixel (sixteen taps -> r, g, b).  The kernels below differ only in where a pixel's source and placement come from
// and in how the finished pixels reach memory, so their bits agree by construction (tests/test_letterbox_bits_gpu.py pins them to
// an independent float32 restatement).
struct LbAxis { int s; float w[4]; };

__device__ __forceinline__ LbAxis lb_axis(int i, int n_src, int n_dst) {
    // source coordinates in double: at 1080p an fp32 coordinate already costs 5e-5 in the weights
    const double f = (i + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    LbAxis a;
    a.s = (int)floor(f);
    cubic_w((float)(f - a.s), a.w);
    return a;
}

// the pixel at (sx, sy) of the h x w source at `src` (`pitch` bytes per row), the border replicated at ITS edges (what cv.resize sees
// after the reference's slice).  WIDE: where the four taps of a row are 12 contiguous bytes (an interior column) they come from one
// (unaligned) 12-byte load instead of twelve byte loads; the values, and the arithmetic on them, are the same.
template <bool WIDE>
__device__ __forceinline__ void lb_pixel(const unsigned char* __restrict__ src, int pitch, int h, int w, int sx, const float (&wx)[4],
                                         int sy, const float (&wy)[4], float& r, float& g, float& b) {
    int xo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xo[i] = min(max(sx - 1 + i, 0), w - 1) * 3;
    const bool inner = WIDE && sx >= 1 && sx + 2 <= w - 1;
    r = 0.f; g = 0.f; b = 0.f;
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
        r += wy[j] * rr; g += wy[j] * gg; b += wy[j] * bb;
    }
    r *= (1.0f / 255.0f); g *= (1.0f / 255.0f); b *= (1.0f / 255.0f);
}

// A source: the h x w rectangle that starts at byte `off` of the packed buffer (its image's offset plus its top-left pixel; a whole
// image is the crop with pitch = 3 w at its offset) and advances `pitch` bytes per row, resized to w_p x h_p.  Every table is made of
// these; the tables travel in the kernel arguments (no device allocation, no host-to-device copy of a pageable table, nothing that
// has to outlive the call), so longer lists are chunked.
struct LbSrc { long long off; int pitch, h, w, w_p, h_p; };

// fv_letterbox, fv_letterbox_batch and fv_letterbox_crops: blockIdx.z = entry, one thread per output pixel, any S.  N = the table's
// capacity: LB_MAX for the lists, 1 for fv_letterbox (back-to-back one-image calls are bound by the launch, and 2.5 KB of kernel
// arguments made one 0.6 us longer than 40 B do).
constexpr int LB_MAX = 64;          // entries per launch (64 x 40 B of kernel arguments)
template <int N> struct LbTable { LbSrc src[N]; int pad_t[N], pad_l[N]; };

template <int N>
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ packed, LbTable<N> t, int S, float* __restrict__ dst) {
    const int c = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= S || y >= S) return;
    const LbSrc s = t.src[c];
    float r = 0.f, g = 0.f, b = 0.f;
    const int xi = x - t.pad_l[c], yi = y - t.pad_t[c];
    if (xi >= 0 && xi < s.w_p && yi >= 0 && yi < s.h_p) {
        const LbAxis ax = lb_axis(xi, s.w, s.w_p), ay = lb_axis(yi, s.h, s.h_p);
        lb_pixel<false>(packed + s.off, s.pitch, s.h, s.w, ax.s, ax.w, ay.s, ay.w, r, g, b);
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

__global__ __launch_bounds__(CNU_THREADS) void crop_nearest_u8_kernel(const unsigned char* __restrict__ packed, LbTable<LB_MAX> t, int S,
                                                                      unsigned char* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) int cnu_src[];      // [3S]: source byte offset inside a row of output byte b, or -1
    const int c = blockIdx.y;
    const LbSrc s = t.src[c];
    const int h = s.h, w = s.w, w_p = s.w_p, h_p = s.h_p, pitch = s.pitch, pad_t = t.pad_t[c], pad_l = t.pad_l[c];
    const double ifx = 1.0 / ((double)w_p / (double)w), ify = 1.0 / ((double)h_p / (double)h);
    for (int x = threadIdx.x; x < S; x += CNU_THREADS) {
        const int xi = x - pad_l;
        int o = -1;
        if (xi >= 0 && xi < w_p) o = min((int)floor(xi * ifx), w - 1) * 3;
        cnu_src[3 * x] = o; cnu_src[3 * x + 1] = o < 0 ? -1 : o + 1; cnu_src[3 * x + 2] = o < 0 ? -1 : o + 2;
    }
    __syncthreads();
    const unsigned char* __restrict__ src = packed + s.off;
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

// The tile stage of the training augmentations (hps['augment']; hps['mosaic']).  A TILE is a source
// letterboxed into a T x T box at (oy, ox) of the S x S canvas -- the box may reach beyond the canvas -- optionally mirrored in place
// (local column c -> T - 1 - c), its colour optionally distorted in HSV, all in the pass that resamples it.  The resampling is
// lb_axis / lb_pixel, so without colour a tile holds letterbox_kernel's bits at image size T.  A workgroup makes LBT_W x LBT_H
// canvas pixels: the fp64 source coordinate and the four weights of each of its columns and rows are computed once (80 threads)
// into LDS; then every thread makes four pixels of one column (64 columns x 4 rows per pass, the passes unrolled so that their loads
// are in flight together); the rectangle is staged in LDS and stored as 16-byte chunks on consecutive lanes (768 B per row segment).
constexpr int LBT_W = 64, LBT_H = 16, LBT_ROWS = 4;         // the rectangle; rows per pass (256 threads = 64 columns x 4 rows)
constexpr int LBT_OUT = -2147483647 - 1;                    // a column / row outside the tile's window or content
struct LbPlace { int top,           // canvas row of the content's first row
                     xa,            // content column xi of canvas column x: x - xa, under a flip xa - x
                     mode;          // bit 0 = flip, bit 1 = the colour stage runs
                 float dh, sat, ex; };
struct LbTile { int s[LBT_W + LBT_H];                                    // floor of the source coordinate of the rectangle's columns,
                __attribute__((aligned(16))) float w[LBT_W + LBT_H][4];  // then rows, or LBT_OUT; their weights
                __attribute__((aligned(16))) float out[LBT_H][LBT_W * 3]; };

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

// the tables of the rectangle at (x0, y0) for one tile seen through the window [wy0, wy1) x [wx0, wx1) of the canvas
__device__ __forceinline__ void lbt_tables(LbTile& l, const LbSrc& s, const LbPlace& p, int x0, int y0, int wy0, int wx0, int wy1, int wx1) {
    const int tid = threadIdx.x;
    if (tid >= LBT_W + LBT_H) return;
    const bool col = tid < LBT_W;
    const int at = col ? x0 + tid : y0 + tid - LBT_W;                            // canvas column / row
    const int i = col ? ((p.mode & 1) ? p.xa - at : at - p.xa) : at - p.top;     // undo the placement and the in-box flip
    const int n_src = col ? s.w : s.h, n_dst = col ? s.w_p : s.h_p;
    LbAxis a = {LBT_OUT, {0.f, 0.f, 0.f, 0.f}};
    if (at >= (col ? wx0 : wy0) && at < (col ? wx1 : wy1) && i >= 0 && i < n_dst) a = lb_axis(i, n_src, n_dst);
    l.s[tid] = a.s;
#pragma unroll
    for (int k = 0; k < 4; ++k) l.w[tid][k] = a.w[k];
}

// a thread's four pixels of the rectangle into the stage.  FILL: a pixel outside the tile is written as +0 (the tile is the only
// one of its canvas); otherwise it is left as it is (zeroed before, or another tile's).
template <bool FILL>
__device__ __forceinline__ void lbt_pixels(LbTile& l, const unsigned char* __restrict__ src, const LbSrc& s, const LbPlace& p) {
    const int lx = threadIdx.x & (LBT_W - 1), ly = threadIdx.x >> 6;
    const int sx = l.s[lx];
    const float4 wxv = *reinterpret_cast<const float4*>(l.w[lx]);
    const float wx[4] = {wxv.x, wxv.y, wxv.z, wxv.w};
#pragma unroll
    for (int pass = 0; pass < LBT_H / LBT_ROWS; ++pass) {
        const int j0 = pass * LBT_ROWS + ly;
        const int sy = l.s[LBT_W + j0];
        const bool in = sx != LBT_OUT && sy != LBT_OUT;
        float r = 0.f, g = 0.f, b = 0.f;
        if (in) {
            const float4 wyv = *reinterpret_cast<const float4*>(l.w[LBT_W + j0]);
            const float wy[4] = {wyv.x, wyv.y, wyv.z, wyv.w};
            lb_pixel<true>(src, s.pitch, s.h, s.w, sx, wx, sy, wy, r, g, b);
            if (p.mode & 2) lba_colour(r, g, b, p.dh, p.sat, p.ex);
        }
        if (FILL || in) { l.out[j0][3 * lx] = r; l.out[j0][3 * lx + 1] = g; l.out[j0][3 * lx + 2] = b; }
    }
}

// the stage as 16-byte chunks, consecutive lanes on consecutive chunks of a row segment (768 B where the rectangle is full)
__device__ __forceinline__ void lbt_store(const LbTile& l, float* __restrict__ canvas, int S, int x0, int y0) {
    constexpr int ROW_Q = LBT_W * 3 / 4;
    const int row_q = 3 * min(LBT_W, S - x0) / 4;                                  // chunks of this rectangle's row segment (S % 4 == 0)
#pragma unroll
    for (int q = threadIdx.x; q < LBT_H * ROW_Q; q += 256) {
        const int rr = q / ROW_Q, k = q - rr * ROW_Q;
        const int y = y0 + rr;
        if (y < S && k < row_q)
            reinterpret_cast<float4*>(canvas + ((size_t)y * S + x0) * 3)[k] = reinterpret_cast<const float4*>(l.out[rr])[k];
    }
}

// fv_letterbox_augment_batch: ONE tile per canvas, inside it, seen through the whole canvas; blockIdx.z = canvas
constexpr int LBA_MAX = 64;         // canvases per launch (64 x 56 B of kernel arguments)
struct LbaTable { LbSrc src[LBA_MAX]; LbPlace place[LBA_MAX]; };

__global__ __launch_bounds__(256) void letterbox_augment_kernel(const unsigned char* __restrict__ packed, LbaTable t, int S,
                                                                float* __restrict__ dst) {
    __shared__ LbTile l;
    const int b = blockIdx.z, x0 = blockIdx.x * LBT_W, y0 = blockIdx.y * LBT_H;
    const LbSrc s = t.src[b];
    const LbPlace p = t.place[b];
    lbt_tables(l, s, p, x0, y0, 0, 0, S, S);
    __syncthreads();
    lbt_pixels<true>(l, packed + s.off, s, p);
    __syncthreads();
    lbt_store(l, dst + (size_t)b * S * S * 3, S, x0, y0);
}

// fv_letterbox_mosaic_batch: a canvas is made of up to MOS_PER tiles with disjoint windows; a pixel outside every window, or inside a
// window but outside the tile's content, is +0.  A workgroup zero-fills its stage, then runs the tile stage for every tile of its
// canvas whose window meets its rectangle (a workgroup-uniform test: most workgroups meet one tile, those on a seam two, the one on
// the centre four).  This form measured 5 % slower on one-tile canvases than the kernel above, so both stay.
constexpr int MOS_TILES = 48;       // tiles (whole canvases) per launch (48 x 72 B of kernel arguments); MOS_PER = tiles per canvas at most
constexpr int MOS_PER = 4;
struct MosTable { LbSrc src[MOS_TILES]; LbPlace place[MOS_TILES];
                  int win[MOS_TILES][4];                    // wy0, wx0, wy1, wx1
                  unsigned char first[MOS_TILES + 1]; };    // canvas z of the launch owns the tiles [first[z], first[z + 1])

__global__ __launch_bounds__(256) void letterbox_mosaic_kernel(const unsigned char* __restrict__ packed, MosTable t, int S,
                                                               float* __restrict__ dst) {
    __shared__ LbTile l;
    const int b = blockIdx.z, x0 = blockIdx.x * LBT_W, y0 = blockIdx.y * LBT_H;
#pragma unroll
    for (int q = threadIdx.x; q < LBT_H * LBT_W * 3 / 4; q += 256) reinterpret_cast<float4*>(&l.out[0][0])[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int k1 = t.first[b + 1];
    for (int k = t.first[b]; k < k1; ++k) {
        const int wy0 = t.win[k][0], wx0 = t.win[k][1], wy1 = t.win[k][2], wx1 = t.win[k][3];
        if (wx1 <= x0 || wx0 >= x0 + LBT_W || wy1 <= y0 || wy0 >= y0 + LBT_H) continue;    // the same in every lane of the workgroup
        const LbSrc s = t.src[k];
        const LbPlace p = t.place[k];
        __syncthreads();                                                          // the tables of the tile before are read; the stage is zeroed
        lbt_tables(l, s, p, x0, y0, wy0, wx0, wy1, wx1);
        __syncthreads();
        lbt_pixels<false>(l, packed + s.off, s, p);                               // a thread's own pixel in every tile
    }
    __syncthreads();
    lbt_store(l, dst + (size_t)b * S * S * 3, S, x0, y0);
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

// ---- the host's one path to a source record.  Every record of a call is checked before anything is enqueued, so a bad one
// leaves dst untouched.

// the h x w crop at (y0, x0) of image `im`, to be letterboxed into a side of T: the image exists, the crop lies inside it and its
// letterbox has at least one row and one column.  `rec` k names the record in the messages ("crop 3", "tile 7", "image 0").
int lb_src_check(fv_ctx* ctx, const char* who, const char* rec, int k, const int64_t* offsets, const int32_t* hw, int n_img, int im,
                 int y0, int x0, int h, int w, int T) {
    FV_REQUIRE(ctx, im >= 0 && im < n_img, "%s: %s %d names image %d of %d", who, rec, k, im, n_img);
    const int H = hw[2 * im], W = hw[2 * im + 1];
    FV_REQUIRE(ctx, H >= 1 && W >= 1 && offsets[im] >= 0, "%s: bad image %d", who, im);
    FV_REQUIRE(ctx, h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= H - h && x0 <= W - w,
               "%s: %s %d (y0 %d, x0 %d, h %d, w %d) outside image %d (%d x %d)", who, rec, k, y0, x0, h, w, im, H, W);
    int g[6];
    FV_REQUIRE(ctx, lb_geometry(h, w, T, g), "%s: %s %d (%d x %d) too elongated for a side of %d", who, rec, k, h, w, T);
    return FV_OK;
}

// the checked record as the kernels' source and its letterbox geometry g[6] in T; -> its source bytes
double lb_src_fill(LbSrc& s, int* g, const int64_t* offsets, const int32_t* hw, int im, int y0, int x0, int h, int w, int T) {
    const int W = hw[2 * im + 1];
    lb_geometry(h, w, T, g);
    s.off = offsets[im] + ((long long)y0 * W + x0) * 3; s.pitch = W * 3;
    s.h = h; s.w = w; s.w_p = g[0]; s.h_p = g[1];
    return (double)h * w * 3;
}

// entry k of a list: the crop record (image, y0, x0, h, w) crops + 5 k, or without `crops` the whole image k
struct LbRec { int im, y0, x0, h, w; };
LbRec lb_rec(const int32_t* hw, const int32_t* crops, int k) {
    if (crops) return {crops[5 * k], crops[5 * k + 1], crops[5 * k + 2], crops[5 * k + 3], crops[5 * k + 4]};
    return {k, 0, 0, hw[2 * k], hw[2 * k + 1]};
}

int lb_list_check(fv_ctx* ctx, const char* who, const int64_t* offsets, const int32_t* hw, int n_img, const int32_t* crops, int n, int S) {
    for (int k = 0; k < n; ++k) {
        const LbRec r = lb_rec(hw, crops, k);
        if (int rc = lb_src_check(ctx, who, crops ? "crop" : "image", k, offsets, hw, n_img, r.im, r.y0, r.x0, r.h, r.w, S)) return rc;
    }
    return FV_OK;
}

// entries [k0, k0 + nk) as a table (geom: their 6 geometry values each, or null); -> their source bytes
template <int N>
double lb_list_fill(LbTable<N>& t, const int64_t* offsets, const int32_t* hw, const int32_t* crops, int k0, int nk, int S, int32_t* geom) {
    double bytes = 0.0;
    for (int i = 0; i < nk; ++i) {
        const LbRec r = lb_rec(hw, crops, k0 + i);
        int g[6];
        bytes += lb_src_fill(t.src[i], g, offsets, hw, r.im, r.y0, r.x0, r.h, r.w, S);
        t.pad_t[i] = g[2]; t.pad_l[i] = g[4];
        if (geom) for (int k = 0; k < 6; ++k) geom[6 * (k0 + i) + k] = g[k];
    }
    return bytes;
}

// fv_letterbox, fv_letterbox_batch and fv_letterbox_crops: check, then N entries per launch; `label` is the profile record's
template <int N>
int lb_run(fv_ctx* ctx, const char* who, const char* label, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
           const int32_t* crops, int n, int S, float* dst, int32_t* geom) {
    if (int rc = lb_list_check(ctx, who, offsets, hw, n_img, crops, n, S)) return rc;
    for (int k0 = 0; k0 < n; k0 += N) {
        const int nk = n - k0 < N ? n - k0 : N;
        LbTable<N> t{};
        const double bytes = lb_list_fill(t, offsets, hw, crops, k0, nk, S, geom) + 12.0 * S * S * nk;
        FvProfScope ps(ctx, label, 0.0, bytes);
        hipLaunchKernelGGL(letterbox_kernel<N>, dim3((S + 15) / 16, (S + 15) / 16, nk), dim3(256), 0, ctx->stream, packed, t, S,
                           dst + (size_t)k0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

// a tile's box: side T at (oy, ox), flip, three colour parameters (or null)
int lb_place_check(fv_ctx* ctx, const char* who, const char* rec, int k, int flip, const float* c) {
    FV_REQUIRE(ctx, flip == 0 || flip == 1, "%s: %s %d: flip %d is neither 0 nor 1", who, rec, k, flip);
    FV_REQUIRE(ctx, !c || (std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2])), "%s: %s %d: colour parameters are not finite",
               who, rec, k);
    return FV_OK;
}

// ox is the box's column AFTER an in-place flip; g the content's geometry inside the box
void lb_place_fill(LbPlace& p, const int* g, int T, int oy, int ox, int flip, const float* c) {
    const bool col = c && !(c[0] == 0.f && c[1] == 1.f && c[2] == 1.f);           // exactly (0, 1, 1): the stage is skipped
    p.top = oy + g[2];
    p.xa = flip ? ox + T - 1 - g[4] : ox + g[4];
    p.mode = flip | (col ? 2 : 0);
    p.dh = col ? c[0] : 0.f; p.sat = col ? c[1] : 1.f; p.ex = col ? c[2] : 1.f;
}

}  // namespace

extern "C" int fv_letterbox(fv_ctx* ctx, const uint8_t* src, int h, int w, int image_size, float* dst, int32_t* geom) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, src && dst && image_size >= 1, "letterbox: bad arguments");
    const int64_t off = 0;
    const int32_t hw[2] = {h, w};
    return lb_run<1>(ctx, "letterbox", "letterbox_kernel", src, &off, hw, 1, nullptr, 1, image_size, dst, geom);
}

extern "C" int fv_letterbox_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                  int image_size, float* dst, int32_t* geom) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && dst && n >= 1 && image_size >= 1, "letterbox_batch: bad arguments");
    return lb_run<LB_MAX>(ctx, "letterbox_batch", "letterbox_batch_kernel", packed, offsets, hw, n, nullptr, n, image_size, dst, geom);
}

extern "C" int fv_letterbox_crops(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                  const int32_t* crops, int n, int image_size, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, packed && offsets && hw && crops && dst && n_img >= 1 && n >= 1 && image_size >= 1, "letterbox_crops: bad arguments");
    return lb_run<LB_MAX>(ctx, "letterbox_crops", "letterbox_crops_kernel", packed, offsets, hw, n_img, crops, n, image_size, dst, nullptr);
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
    if (int rc = lb_list_check(ctx, "crop_nearest_u8", offsets, hw, n_img, crops, n, S)) return rc;
    const int blocks = (S * (3 * S / 16) + CNU_CHUNKS - 1) / CNU_CHUNKS;       // one launch of 64 crops is already ~2 000 workgroups at 416
    for (int c0 = 0; c0 < n; c0 += LB_MAX) {
        const int nc = n - c0 < LB_MAX ? n - c0 : LB_MAX;
        LbTable<LB_MAX> t{};
        const double bytes = lb_list_fill(t, offsets, hw, crops, c0, nc, S, nullptr) + 3.0 * S * S * nc;
        FvProfScope ps(ctx, "crop_nearest_u8_kernel", 0.0, bytes);
        hipLaunchKernelGGL(crop_nearest_u8_kernel, dim3(blocks, nc), dim3(CNU_THREADS), 3 * S * sizeof(int), ctx->stream, packed, t,
                           S, dst + (size_t)c0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox_augment_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                          int image_size, const int32_t* place, const float* colour, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    const char* who = "letterbox_augment_batch";
    FV_REQUIRE(ctx, packed && offsets && hw && place && dst && n >= 1 && image_size >= 4 && image_size % 4 == 0 && ((uintptr_t)dst & 15) == 0,
               "%s: bad arguments (image_size a multiple of 4 and dst 16-byte aligned: rows are stored 16 bytes at a time)", who);
    const int S = image_size;
    for (int i = 0; i < n; ++i) {
        const int* r = place + 8 * i;                                    // cy0, cx0, ch, cw, T, oy, ox, flip
        const int T = r[4], oy = r[5], ox = r[6];
        FV_REQUIRE(ctx, T >= 1 && T <= S && oy >= 0 && ox >= 0 && oy <= S - T && ox <= S - T,
                   "%s: image %d: box of side %d at (y %d, x %d) outside the %d x %d canvas", who, i, T, oy, ox, S, S);
        if (int rc = lb_src_check(ctx, who, "crop", i, offsets, hw, n, i, r[0], r[1], r[2], r[3], T)) return rc;
        if (int rc = lb_place_check(ctx, who, "image", i, r[7], colour ? colour + 3 * i : nullptr)) return rc;
    }
    for (int b0 = 0; b0 < n; b0 += LBA_MAX) {
        const int nb = n - b0 < LBA_MAX ? n - b0 : LBA_MAX;
        LbaTable t{};
        double bytes = 12.0 * S * S * nb;
        for (int i = 0; i < nb; ++i) {
            const int* r = place + 8 * (b0 + i);
            int g[6];
            bytes += lb_src_fill(t.src[i], g, offsets, hw, b0 + i, r[0], r[1], r[2], r[3], r[4]);
            // the flip mirrors the canvas: the box in place at the mirrored column
            lb_place_fill(t.place[i], g, r[4], r[5], r[7] ? S - r[4] - r[6] : r[6], r[7], colour ? colour + 3 * (b0 + i) : nullptr);
        }
        FvProfScope ps(ctx, "letterbox_augment_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_augment_kernel, dim3((S + LBT_W - 1) / LBT_W, (S + LBT_H - 1) / LBT_H, nb), dim3(256), 0,
                           ctx->stream, packed, t, S, dst + (size_t)b0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

extern "C" int fv_letterbox_mosaic_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                         int image_size, int n_out, const int32_t* tiles, const float* colour, int n_tiles, float* dst) {
    if (!ctx) return FV_ERR_INVALID;
    const char* who = "letterbox_mosaic_batch";
    FV_REQUIRE(ctx, packed && offsets && hw && tiles && dst && n_img >= 1 && n_out >= 1 && n_tiles >= n_out && n_tiles <= MOS_PER * (long long)n_out &&
                        image_size >= 4 && image_size % 4 == 0 && ((uintptr_t)dst & 15) == 0,
               "%s: bad arguments (1 to 4 tiles per canvas, image_size a multiple of 4 and dst 16-byte aligned: rows are stored 16 bytes at a "
               "time)", who);
    const int S = image_size;
    int canvas = 0, first = 0;                                       // the canvas being read and its first tile
    for (int k = 0; k < n_tiles; ++k) {
        const int* r = tiles + 14 * k;          // canvas, image, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1
        const int cv = r[0], T = r[6], oy = r[7], ox = r[8], wy0 = r[10], wx0 = r[11], wy1 = r[12], wx1 = r[13];
        FV_REQUIRE(ctx, cv >= 0 && cv < n_out && (cv == canvas || (cv == canvas + 1 && k > first)),
                   "%s: tile %d names canvas %d after canvas %d (of %d): the tiles are sorted by canvas and every canvas has at least one", who,
                   k, cv, canvas, n_out);
        if (cv != canvas) { canvas = cv; first = k; }
        FV_REQUIRE(ctx, k - first < MOS_PER, "%s: canvas %d has more than %d tiles", who, cv, MOS_PER);
        FV_REQUIRE(ctx, T >= 1 && T <= 4LL * S && oy >= -T && ox >= -T && oy <= S && ox <= S,
                   "%s: tile %d: box of side %d at (y %d, x %d): 1 <= side <= 4 x %d and -side <= y, x <= %d", who, k, T, oy, ox, S, S);
        if (int rc = lb_src_check(ctx, who, "tile", k, offsets, hw, n_img, r[1], r[2], r[3], r[4], r[5], T)) return rc;
        if (int rc = lb_place_check(ctx, who, "tile", k, r[9], colour ? colour + 3 * k : nullptr)) return rc;
        FV_REQUIRE(ctx, wy0 >= 0 && wx0 >= 0 && wy0 < wy1 && wx0 < wx1 && wy1 <= S && wx1 <= S,
                   "%s: tile %d: window rows [%d, %d) columns [%d, %d) is empty or outside the %d x %d canvas", who, k, wy0, wy1, wx0, wx1, S, S);
        for (int j = first; j < k; ++j) {
            const int* q = tiles + 14 * j;
            FV_REQUIRE(ctx, wy1 <= q[10] || q[12] <= wy0 || wx1 <= q[11] || q[13] <= wx0, "%s: the windows of tiles %d and %d of canvas %d overlap",
                       who, j, k, cv);
        }
    }
    FV_REQUIRE(ctx, canvas == n_out - 1, "%s: canvas %d of %d has no tile", who, canvas + 1, n_out);
    // whole canvases per launch, as many as MOS_TILES tiles hold
    for (int k0 = 0, c0 = 0; k0 < n_tiles;) {
        MosTable t{};
        int nt = 0, nc = 0;
        double bytes = 0.0;
        while (k0 + nt < n_tiles) {
            int m = 1;
            while (k0 + nt + m < n_tiles && tiles[14 * (k0 + nt + m)] == tiles[14 * (k0 + nt)]) ++m;    // the tiles of the next canvas
            if (nt + m > MOS_TILES) break;
            for (int i = nt; i < nt + m; ++i) {
                const int* r = tiles + 14 * (k0 + i);
                int g[6];
                bytes += lb_src_fill(t.src[i], g, offsets, hw, r[1], r[2], r[3], r[4], r[5], r[6]);
                lb_place_fill(t.place[i], g, r[6], r[7], r[8], r[9], colour ? colour + 3 * (k0 + i) : nullptr);
                for (int j = 0; j < 4; ++j) t.win[i][j] = r[10 + j];
            }
            nt += m;
            t.first[++nc] = (unsigned char)nt;
        }
        bytes += 12.0 * S * S * nc;
        FvProfScope ps(ctx, "letterbox_mosaic_kernel", 0.0, bytes);
        hipLaunchKernelGGL(letterbox_mosaic_kernel, dim3((S + LBT_W - 1) / LBT_W, (S + LBT_H - 1) / LBT_H, nc), dim3(256), 0,
                           ctx->stream, packed, t, S, dst + (size_t)c0 * S * S * 3);
        FV_LAUNCH_CHECK(ctx);
        k0 += nt; c0 += nc;
    }
    return FV_OK;
}
