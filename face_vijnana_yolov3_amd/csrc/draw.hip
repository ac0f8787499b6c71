// Drawing onto the packed uint8 RGB frames of a batch, in place (FaceIdentifier.evaluate, fi.py:945-992: draw_boxes_v3's
// ImageDraw.rectangle(width=3) + ImageDraw.text per box, ground truth first, detections second).  Two primitives: an OUTLINE
// (the closed form of a width-w rectangle outline) and a MASK BLEND (an 8-bit coverage mask -- Pillow's rasterised label --
// blended with an ink by Pillow's BLEND8).  The result is that of applying the table one primitive after another.
//
// A launch takes up to DP_MAX consecutive primitives in its kernel arguments (as the crop tables travel, preproc.hip); longer
// tables are cut into consecutive launches on the one stream, which keeps the order.  The host clips every primitive to its image
// and launches, per image the chunk names, only the tiles of the bounding box of its clipped primitives.  A wave owns a 32 x 2
// strip of pixels, one pixel per lane: lane l tests primitive l against the strip, the ballot is the ordered list of the
// primitives that can touch it, and a strip with none returns without touching memory (almost every strip of an 18-megapixel
// frame).  Otherwise the wave walks the set bits in ascending = table order -- the index is wave-uniform, so the primitive is read
// with scalar loads --, every lane keeps its pixel in registers and stores it once, if anything touched it: sequential semantics
// without atomics or passes.  A pixel is three byte stores: rows start at arbitrary byte addresses (3 W bytes per row, images back
// to back), so no wider store is aligned, and the 96 bytes a half-wave writes are contiguous and merge in the L2 write path; the
// pixels drawn per frame are a few thousand, the launch is bound by its latency, not by those stores.
#include "common.h"

namespace {

constexpr int DP_MAX = 32;                 // primitives per launch: one per lane of the cull ballot's low half, 2.6 KB of arguments
constexpr int DP_TW = 32, DP_TH = 8;       // tile: 4 waves x (32 x 2) pixels

struct DrawTable {
    long long img_off[DP_MAX];             // per image slot: byte offset of the image in `packed`
    long long mbase[DP_MAX];               // mask blend: mask byte of image pixel (px, py) = masks[mbase + py * pitch + px]
    int img_w[DP_MAX], tx0[DP_MAX], ty0[DP_MAX], ntx[DP_MAX], nty[DP_MAX];   // per slot: columns, first tile and tile counts of its launch box
    int slot[DP_MAX];                      // per primitive: its image's slot
    int cx0[DP_MAX], cy0[DP_MAX], cx1[DP_MAX], cy1[DP_MAX];   // the primitive clipped to its image (inclusive, never empty)
    int ix0[DP_MAX], iy0[DP_MAX], ix1[DP_MAX], iy1[DP_MAX];   // outline: the interior it leaves alone (inclusive, may be empty)
    int pitch[DP_MAX];                     // mask blend: mw >= 1; outline: -1
    unsigned color[DP_MAX];                // r | g << 8 | b << 16
    int n, n_slots;
};

__global__ __launch_bounds__(256) void draw_prims_kernel(unsigned char* __restrict__ packed, const unsigned char* __restrict__ masks,
                                                         DrawTable t) {
    const int s = blockIdx.z;
    if ((int)blockIdx.x >= t.ntx[s] || (int)blockIdx.y >= t.nty[s]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xa = (t.tx0[s] + (int)blockIdx.x) * DP_TW;                   // the wave's strip: columns xa .. xa + 31, rows ya, ya + 1
    const int ya = (t.ty0[s] + (int)blockIdx.y) * DP_TH + wave * 2;
    bool hit = false;
    if (lane < t.n && t.slot[lane] == s) {
        hit = t.cx0[lane] <= xa + DP_TW - 1 && t.cx1[lane] >= xa && t.cy0[lane] <= ya + 1 && t.cy1[lane] >= ya;
        if (hit && t.pitch[lane] < 0)                                      // an outline whose interior holds the whole strip
            hit = !(xa >= t.ix0[lane] && xa + DP_TW - 1 <= t.ix1[lane] && ya >= t.iy0[lane] && ya + 1 <= t.iy1[lane]);
    }
    unsigned long long live = __ballot(hit);
    if (live == 0ull) return;
    const int x = xa + (lane & 31), y = ya + (lane >> 5);
    // (x, y) may lie outside the image; it is dereferenced only inside a clipped rectangle, which lies inside the image
    unsigned char* __restrict__ p = packed + t.img_off[s] + ((long long)y * t.img_w[s] + x) * 3;
    unsigned r = 0u, g = 0u, b = 0u;
    bool have = false, touched = false;
    while (live != 0ull) {
        const int k = __ffsll(live) - 1;
        live &= live - 1ull;
        if (x < t.cx0[k] || x > t.cx1[k] || y < t.cy0[k] || y > t.cy1[k]) continue;
        const unsigned ink = t.color[k];
        if (t.pitch[k] < 0) {
            if (x >= t.ix0[k] && x <= t.ix1[k] && y >= t.iy0[k] && y <= t.iy1[k]) continue;
            r = ink & 255u; g = (ink >> 8) & 255u; b = (ink >> 16) & 255u;
        } else {
            if (!have) { r = p[0]; g = p[1]; b = p[2]; }
            const unsigned m = masks[t.mbase[k] + (long long)y * t.pitch[k] + x];
            // Pillow's BLEND8: t = old * (255 - m) + ink * m + 128; new = ((t >> 8) + t) >> 8
            unsigned v = r * (255u - m) + (ink & 255u) * m + 128u;          r = ((v >> 8) + v) >> 8;
            v = g * (255u - m) + ((ink >> 8) & 255u) * m + 128u;            g = ((v >> 8) + v) >> 8;
            v = b * (255u - m) + ((ink >> 16) & 255u) * m + 128u;           b = ((v >> 8) + v) >> 8;
        }
        have = true; touched = true;
    }
    if (touched) { p[0] = (unsigned char)r; p[1] = (unsigned char)g; p[2] = (unsigned char)b; }
}

inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// every record of the table checked before anything is enqueued, so a rejected call draws nothing
int draw_validate(fv_ctx* ctx, const int64_t* offsets, const int32_t* hw, int n_img, const fv_draw_prim* prims, int n,
                  int64_t mask_bytes) {
    for (int i = 0; i < n_img; ++i)
        FV_REQUIRE(ctx, hw[2 * i] >= 1 && hw[2 * i] <= 65535 * DP_TH && hw[2 * i + 1] >= 1 && offsets[i] >= 0,
                   "draw_prims_u8: bad image %d (at most %d rows: one grid row per %d)", i, 65535 * DP_TH, DP_TH);
    for (int k = 0; k < n; ++k) {
        const fv_draw_prim& q = prims[k];
        FV_REQUIRE(ctx, q.image >= 0 && q.image < n_img, "draw_prims_u8: primitive %d names image %d of %d", k, q.image, n_img);
        if (q.kind == FV_DRAW_OUTLINE) {
            FV_REQUIRE(ctx, q.width >= 1, "draw_prims_u8: primitive %d: outline width %d", k, q.width);
        } else if (q.kind == FV_DRAW_MASK) {
            FV_REQUIRE(ctx, q.x1 >= 0 && q.y1 >= 0, "draw_prims_u8: primitive %d: mask size %d x %d", k, q.x1, q.y1);
            FV_REQUIRE(ctx, q.mask_off >= 0 && q.mask_off <= mask_bytes && (long long)q.x1 * q.y1 <= mask_bytes - q.mask_off,
                       "draw_prims_u8: primitive %d: mask of %d x %d bytes at %lld runs past the mask buffer (%lld bytes)", k, q.x1,
                       q.y1, (long long)q.mask_off, (long long)mask_bytes);
        } else {
            FV_REQUIRE(ctx, false, "draw_prims_u8: primitive %d: kind %d", k, q.kind);
        }
    }
    return FV_OK;
}

}  // namespace

extern "C" int fv_draw_prims_u8(fv_ctx* ctx, uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                                const fv_draw_prim* prims, int n, const uint8_t* masks, int64_t mask_bytes) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n >= 0 && n_img >= 0 && mask_bytes >= 0, "draw_prims_u8: n %d, n_img %d, mask_bytes %lld", n, n_img,
               (long long)mask_bytes);
    if (n == 0) return FV_OK;
    FV_REQUIRE(ctx, packed && offsets && hw && prims && n_img >= 1 && (masks || mask_bytes == 0), "draw_prims_u8: bad arguments");
    if (int rc = draw_validate(ctx, offsets, hw, n_img, prims, n, mask_bytes)) return rc;
    int k = 0;
    while (k < n) {
        DrawTable t{};
        int slot_img[DP_MAX];
        int bx0[DP_MAX], by0[DP_MAX], bx1[DP_MAX], by1[DP_MAX];           // per slot: bounding box of its clipped primitives
        double bytes = 0.0;
        for (; k < n && t.n < DP_MAX; ++k) {
            const fv_draw_prim& q = prims[k];
            const long long H = hw[2 * q.image], W = hw[2 * q.image + 1];
            const bool outline = q.kind == FV_DRAW_OUTLINE;
            // the pixels the primitive covers, inclusive: the outline's corners, or the mask's rectangle
            const long long X0 = q.x0, Y0 = q.y0;
            const long long X1 = outline ? (long long)q.x1 : X0 + q.x1 - 1, Y1 = outline ? (long long)q.y1 : Y0 + q.y1 - 1;
            const long long cx0 = X0 > 0 ? X0 : 0, cy0 = Y0 > 0 ? Y0 : 0, cx1 = X1 < W - 1 ? X1 : W - 1, cy1 = Y1 < H - 1 ? Y1 : H - 1;
            if (cx0 > cx1 || cy0 > cy1) continue;                          // nothing of it inside the image
            const int i = t.n++;
            int s = 0;
            while (s < t.n_slots && slot_img[s] != q.image) ++s;
            if (s == t.n_slots) {
                slot_img[s] = q.image; t.n_slots++;
                t.img_off[s] = offsets[q.image]; t.img_w[s] = (int)W;
                bx0[s] = (int)cx0; by0[s] = (int)cy0; bx1[s] = (int)cx1; by1[s] = (int)cy1;
            } else {
                if (cx0 < bx0[s]) bx0[s] = (int)cx0;
                if (cy0 < by0[s]) by0[s] = (int)cy0;
                if (cx1 > bx1[s]) bx1[s] = (int)cx1;
                if (cy1 > by1[s]) by1[s] = (int)cy1;
            }
            t.slot[i] = s;
            t.cx0[i] = (int)cx0; t.cy0[i] = (int)cy0; t.cx1[i] = (int)cx1; t.cy1[i] = (int)cy1;
            t.color[i] = (unsigned)q.r | ((unsigned)q.g << 8) | ((unsigned)q.b << 16);
            if (outline) {
                // painted: x - X0 < w or X1 - x < w or y - Y0 < w or Y1 - y < w  <=>  NOT inside [X0 + w, X1 - w] x [Y0 + w, Y1 - w];
                // clamping that interior to the image changes nothing for a pixel of the image
                t.pitch[i] = -1;
                t.ix0[i] = (int)clampll(X0 + q.width, 0, W); t.ix1[i] = (int)clampll(X1 - q.width, -1, W - 1);
                t.iy0[i] = (int)clampll(Y0 + q.width, 0, H); t.iy1[i] = (int)clampll(Y1 - q.width, -1, H - 1);
                bytes += 3.0 * 2.0 * q.width * ((double)(cx1 - cx0 + 1) + (double)(cy1 - cy0 + 1));
            } else {
                t.pitch[i] = q.x1;
                t.mbase[i] = (long long)q.mask_off - Y0 * q.x1 - X0;
                bytes += 7.0 * (double)(cx1 - cx0 + 1) * (double)(cy1 - cy0 + 1);
            }
        }
        if (t.n == 0) break;
        int gx = 1, gy = 1;
        for (int s = 0; s < t.n_slots; ++s) {
            t.tx0[s] = bx0[s] / DP_TW; t.ty0[s] = by0[s] / DP_TH;
            t.ntx[s] = bx1[s] / DP_TW - t.tx0[s] + 1; t.nty[s] = by1[s] / DP_TH - t.ty0[s] + 1;
            if (t.ntx[s] > gx) gx = t.ntx[s];
            if (t.nty[s] > gy) gy = t.nty[s];
        }
        FvProfScope ps(ctx, "draw_prims_kernel", 0.0, bytes);
        hipLaunchKernelGGL(draw_prims_kernel, dim3(gx, gy, t.n_slots), dim3(256), 0, ctx->stream, packed, masks, t);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}
