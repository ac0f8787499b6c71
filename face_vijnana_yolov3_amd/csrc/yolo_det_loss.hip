// YOLOv3 detection loss of the three-scale head and its gradient (include/fv_hotpath.h: fv_yolo_det_loss_grad; DESIGN.md
// section 25).  Not in the reference (yd.py:217-311 is inference only).  A bandwidth-class pass over y, t and dy in three
// launches for the three scales together:
//   det_gather_kernel   one workgroup per image walks the image's slots in slot order and compacts the assigned ones
//                       (t4 == 1) into the image's box list with a ballot prefix -- the list order, and so where the cap cuts
//                       it, does not depend on timing;
//   det_loss_kernel     one workgroup per (image, scale, 85 cells): the image's list staged in LDS; one lane per
//                       (cell, anchor) slot decodes its box, loops over the list for the best IoU and forms the box /
//                       objectness terms; then the workgroup writes its 85 dy rows (contiguous in memory) with the waves
//                       striding over rows and lanes over columns, and only there touches the class entries of the assigned
//                       slots;
//   det_finish_kernel   sums the per-workgroup partials in a fixed order -> loss and stats.
// fp64 arithmetic throughout; every sum is formed in an order fixed by the launch shape.
#include "yolo_det_loss.h"
#include "block_ops.h"

#include <cmath>

namespace {

constexpr int DET_CELLS = 85;   // cells per workgroup: 255 of 256 lanes hold a slot
constexpr int DET_NQ = 9;       // partial sums per workgroup: box, obj, noobj, cls, positives, ignored, sum IoU, IoU > .5, IoU > .75

struct DetArgs {
    const float* y[3];
    const float* t[3];
    float* dy[3];
    double aw[9], ah[9];
    int g[3];     // grid of scale s
    int nc[3];    // workgroups per image at scale s
};

// bce(x, z) = max(x,0) - x z + log1p(e^-|x|) on the logit x and sigma(x) - z without cancellation at the saturated end
__device__ __forceinline__ double det_bce(double x, double z) { return fmax(x, 0.0) - x * z + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double det_q(double x) { const double e = exp(-fabs(x)); return e / (1.0 + e); }   // sigma(-|x|)
__device__ __forceinline__ double det_sigmoid(double x) { const double q = det_q(x); return x >= 0.0 ? 1.0 - q : q; }
__device__ __forceinline__ double det_dbce(double x, double z) { const double q = det_q(x); return x >= 0.0 ? (1.0 - z) - q : q - z; }

__device__ __forceinline__ double det_iou(double px, double py, double pw, double ph, double bx, double by, double bw, double bh) {
    const double iw = fmin(px + 0.5 * pw, bx + 0.5 * bw) - fmax(px - 0.5 * pw, bx - 0.5 * bw);
    const double ih = fmin(py + 0.5 * ph, by + 0.5 * bh) - fmax(py - 0.5 * ph, by - 0.5 * bh);
    const double inter = fmax(iw, 0.0) * fmax(ih, 0.0);
    return inter / (pw * ph + bw * bh - inter);
}

__global__ __launch_bounds__(256) void det_gather_kernel(DetArgs a, int S, int E, int max_boxes, double* __restrict__ boxes,
                                                         int* __restrict__ counts) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.x;
    int running = 0;
    for (int s = 0; s < 3; ++s) {
        const int g = a.g[s], nslot = 3 * g * g;
        const double cell_px = (double)(S / g);
        const float* tb = a.t[s] + (long long)img * nslot * E;
        for (int base = 0; base < nslot; base += 256) {
            const int i = base + tid;
            const bool flag = i < nslot && tb[(long long)i * E + 4] == 1.0f;
            const int off = running + fv_block_compact(flag, s_cnt, lane, wave);
            running += (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            if (flag && off < max_boxes) {
                const float* tp = tb + (long long)i * E;
                const int cell = i / 3, an = i - cell * 3;
                const int row = cell / g, col = cell - row * g;
                double* b = boxes + ((long long)img * max_boxes + off) * 4;
                b[0] = ((double)col + det_sigmoid((double)tp[0])) * cell_px;
                b[1] = ((double)row + det_sigmoid((double)tp[1])) * cell_px;
                b[2] = a.aw[s * 3 + an] * exp((double)tp[2]);
                b[3] = a.ah[s * 3 + an] * exp((double)tp[3]);
            }
            __syncthreads();
        }
    }
    if (tid == 0) counts[img] = running;
}

__global__ __launch_bounds__(256) void det_loss_kernel(DetArgs a, int S, int ncls, int Cpad, int box_loss, double ignore_thresh,
                                                       double box_w, double noobj_w, int max_boxes, double gscale,
                                                       const double* __restrict__ boxes, const int* __restrict__ counts,
                                                       double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double s_box[];   // the image's list, [n][cx, cy, w, h]; a box is read as 2 x 16 bytes
    __shared__ double s_g[5][256];             // d loss / d y of a slot's entries 0..4 (unscaled)
    __shared__ unsigned char s_pos[256];       // slot assigned
    __shared__ double s_red[4][DET_NQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = 5 + ncls;
    const int per = a.nc[0] + a.nc[1] + a.nc[2];
    const int img = blockIdx.x / per;
    int r = blockIdx.x - img * per, s = 0;
    if (r >= a.nc[0]) { r -= a.nc[0]; s = 1; if (r >= a.nc[1]) { r -= a.nc[1]; s = 2; } }
    const int g = a.g[s], cells_img = g * g, c0 = r * DET_CELLS;
    const int nc = cells_img - c0 < DET_CELLS ? cells_img - c0 : DET_CELLS;
    const float* __restrict__ y = a.y[s];
    const float* __restrict__ t = a.t[s];
    float* __restrict__ dy = a.dy[s];
    const int cnt = counts[img], n = cnt < max_boxes ? cnt : max_boxes;
    for (int i = tid; i < 4 * n; i += 256) s_box[i] = boxes[(long long)img * max_boxes * 4 + i];
    __syncthreads();

    double q[DET_NQ];
#pragma unroll
    for (int k = 0; k < DET_NQ; ++k) q[k] = 0.0;
    if (tid < 3 * nc) {
        const int cl = tid / 3, an = tid - cl * 3, cell = c0 + cl;
        const int row = cell / g, col = cell - row * g;
        const long long base = ((long long)img * cells_img + cell) * (3 * E) + (long long)an * E;
        const float* yp = y + base;
        const float* tp = t + base;
        const double y0 = (double)yp[0], y1 = (double)yp[1], y2 = (double)yp[2], y3 = (double)yp[3], y4 = (double)yp[4];
        const bool assigned = tp[4] == 1.0f;
        const double cell_px = (double)(S / g), aw = a.aw[s * 3 + an], ah = a.ah[s * 3 + an];
        const double sx = det_sigmoid(y0), sy = det_sigmoid(y1);
        const double px = ((double)col + sx) * cell_px, py = ((double)row + sy) * cell_px;
        const double pw = aw * exp(fmin(fmax(y2, -20.0), 20.0)), ph = ah * exp(fmin(fmax(y3, -20.0), 20.0));
        double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
        if (!assigned) {
            double best = 0.0;
            for (int j = 0; j < n; ++j)
                best = fmax(best, det_iou(px, py, pw, ph, s_box[4 * j], s_box[4 * j + 1], s_box[4 * j + 2], s_box[4 * j + 3]));
            if (best > ignore_thresh) q[5] = 1.0;
            else { q[2] = noobj_w * det_bce(y4, 0.0); g4 = noobj_w * det_dbce(y4, 0.0); }
        } else {
            const double t0 = (double)tp[0], t1 = (double)tp[1], t2 = (double)tp[2], t3 = (double)tp[3];
            const double zx = det_sigmoid(t0), zy = det_sigmoid(t1);
            const double bx = ((double)col + zx) * cell_px, by = ((double)row + zy) * cell_px;
            const double bw = aw * exp(t2), bh = ah * exp(t3);
            const double iou = det_iou(px, py, pw, ph, bx, by, bw, bh);
            q[4] = 1.0; q[6] = iou; q[7] = iou > 0.5 ? 1.0 : 0.0; q[8] = iou > 0.75 ? 1.0 : 0.0;
            q[1] = det_bce(y4, 1.0); g4 = det_dbce(y4, 1.0);
            if (box_loss == FV_DET_BOX_L2) {
                const double sc = 2.0 - bw * bh / ((double)S * (double)S);
                const double d2 = y2 - t2, d3 = y3 - t3;
                q[0] = box_w * (sc * (det_bce(y0, zx) + det_bce(y1, zy)) + 0.5 * sc * (d2 * d2 + d3 * d3));
                g0 = box_w * sc * det_dbce(y0, zx); g1 = box_w * sc * det_dbce(y1, zy);
                g2 = box_w * sc * d2; g3 = box_w * sc * d3;
            } else {
                // L = 1 - GIoU = 2 - I/U - U/C;  dL = -dI/U + (I/U^2 - 1/C) dU + (U/C^2) dC,  dU = dP - dI
                const double x1 = px - 0.5 * pw, x2 = px + 0.5 * pw, v1 = py - 0.5 * ph, v2 = py + 0.5 * ph;
                const double X1 = bx - 0.5 * bw, X2 = bx + 0.5 * bw, V1 = by - 0.5 * bh, V2 = by + 0.5 * bh;
                const double iw = fmin(x2, X2) - fmax(x1, X1), ih = fmin(v2, V2) - fmax(v1, V1);
                const double iwc = fmax(iw, 0.0), ihc = fmax(ih, 0.0), I = iwc * ihc;
                const double U = pw * ph + bw * bh - I;
                const double cw = fmax(x2, X2) - fmin(x1, X1), ch = fmax(v2, V2) - fmin(v1, V1), C = cw * ch;
                q[0] = box_w * (1.0 - (I / U - (C - U) / C));
                const bool pos = iw > 0.0 && ih > 0.0;
                const double dI_x2 = pos && x2 < X2 ? ihc : 0.0, dI_x1 = pos && x1 > X1 ? -ihc : 0.0;
                const double dI_v2 = pos && v2 < V2 ? iwc : 0.0, dI_v1 = pos && v1 > V1 ? -iwc : 0.0;
                const double dC_x2 = x2 > X2 ? ch : 0.0, dC_x1 = x1 < X1 ? -ch : 0.0;
                const double dC_v2 = v2 > V2 ? cw : 0.0, dC_v1 = v1 < V1 ? -cw : 0.0;
                const double kI = -1.0 / U, kU = I / (U * U) - 1.0 / C, kC = U / (C * C);
                const double L_x2 = kI * dI_x2 + kU * (ph - dI_x2) + kC * dC_x2, L_x1 = kI * dI_x1 + kU * (-ph - dI_x1) + kC * dC_x1;
                const double L_v2 = kI * dI_v2 + kU * (pw - dI_v2) + kC * dC_v2, L_v1 = kI * dI_v1 + kU * (-pw - dI_v1) + kC * dC_v1;
                g0 = box_w * (L_x1 + L_x2) * cell_px * (sx * (1.0 - sx));
                g1 = box_w * (L_v1 + L_v2) * cell_px * (sy * (1.0 - sy));
                g2 = fabs(y2) < 20.0 ? box_w * 0.5 * (L_x2 - L_x1) * pw : 0.0;
                g3 = fabs(y3) < 20.0 ? box_w * 0.5 * (L_v2 - L_v1) * ph : 0.0;
            }
        }
        s_g[0][tid] = g0; s_g[1][tid] = g1; s_g[2][tid] = g2; s_g[3][tid] = g3; s_g[4][tid] = g4;
        s_pos[tid] = assigned ? 1 : 0;
    }
    __syncthreads();

    // the workgroup's dy rows: waves over rows, lanes over columns; class entries of the assigned slots are formed here
    double cls = 0.0;
    for (int cl = wave; cl < nc; cl += 4) {
        const long long cellg = (long long)img * cells_img + c0 + cl;
        const float* yr = y + cellg * (3 * E);
        const float* tr = t + cellg * (3 * E);
        float* gr = dy + cellg * Cpad;
        for (int c = lane; c < Cpad; c += 64) {
            float v = 0.f;
            if (c < 3 * E) {
                const int an = (c >= E ? 1 : 0) + (c >= 2 * E ? 1 : 0), e = c - an * E, slot = cl * 3 + an;
                if (e < 5) v = (float)(s_g[e][slot] * gscale);
                else if (s_pos[slot]) {
                    const double x = (double)yr[c], z = (double)tr[c];
                    cls += det_bce(x, z);
                    v = (float)(det_dbce(x, z) * gscale);
                }
            }
            gr[c] = v;
        }
    }
    q[3] = cls;
#pragma unroll
    for (int k = 0; k < DET_NQ; ++k) {
        const double v = fv_wave_sum(q[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < DET_NQ) part[(long long)blockIdx.x * DET_NQ + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

__global__ __launch_bounds__(256) void det_finish_kernel(const double* __restrict__ part, int nblocks, const int* __restrict__ counts,
                                                         int B, int max_boxes, float* __restrict__ loss, double* __restrict__ stats) {
    __shared__ double s_sum[16][16];
    const int k = threadIdx.x & 15, sub = threadIdx.x >> 4;
    double acc = 0.0;
    if (k < DET_NQ)
        for (int b = sub; b < nblocks; b += 16) acc += part[(long long)b * DET_NQ + k];
    s_sum[sub][k] = acc;
    __syncthreads();
    if (threadIdx.x < DET_NQ) {
        double v = 0.0;
        for (int i = 0; i < 16; ++i) v += s_sum[i][threadIdx.x];
        s_sum[0][threadIdx.x] = threadIdx.x < 4 ? v / (double)B : v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < DET_NQ; ++i) stats[i] = s_sum[0][i];
        *loss = (float)((s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]));
        int mx = 0;
        long long dropped = 0;
        for (int b = 0; b < B; ++b) {
            const int c = counts[b];
            mx = c > mx ? c : mx;
            dropped += c > max_boxes ? c - max_boxes : 0;
        }
        stats[9] = (double)mx; stats[10] = (double)dropped; stats[11] = 0.0;
    }
}

struct DetPlan {
    int g[3], nc[3], per;
    long long nblocks;
    size_t off_part, off_counts, bytes;
};
DetPlan det_plan(int batch, int image_size, int max_boxes) {
    DetPlan p;
    p.per = 0;
    for (int s = 0; s < 3; ++s) {
        p.g[s] = (image_size / 32) << s;
        p.nc[s] = (p.g[s] * p.g[s] + DET_CELLS - 1) / DET_CELLS;
        p.per += p.nc[s];
    }
    p.nblocks = (long long)batch * p.per;
    p.off_part = (size_t)batch * max_boxes * 4 * sizeof(double);
    p.off_counts = p.off_part + (size_t)p.nblocks * DET_NQ * sizeof(double);
    p.bytes = p.off_counts + ((size_t)batch * sizeof(int) + 7) / 8 * 8;
    return p;
}
bool det_shape_ok(int batch, int image_size, int max_boxes) {
    return batch >= 1 && batch <= 65535 && image_size >= 32 && image_size <= 4096 && image_size % 32 == 0 && max_boxes >= 1 && max_boxes <= 1024;
}

}  // namespace

int fv_det_check(fv_ctx* ctx, const char* who, const fv_yolo_det_conf* conf, int batch, int image_size, int ncls, int c_pad,
                 const void* scratch, size_t scratch_bytes, const double* stats) {
    FV_REQUIRE(ctx, conf && scratch && stats, "%s: NULL conf, scratch or stats", who);
    FV_REQUIRE(ctx, conf->box_loss == FV_DET_BOX_L2 || conf->box_loss == FV_DET_BOX_GIOU, "%s: unknown box_loss %d", who, conf->box_loss);
    FV_REQUIRE(ctx, conf->ignore_thresh > 0.f && conf->ignore_thresh <= 1.f, "%s: ignore_thresh must be in (0, 1]", who);
    FV_REQUIRE(ctx, std::isfinite(conf->box_weight) && conf->box_weight > 0.f, "%s: box_weight must be finite and > 0", who);
    FV_REQUIRE(ctx, std::isfinite(conf->noobj_weight) && conf->noobj_weight > 0.f, "%s: noobj_weight must be finite and > 0", who);
    FV_REQUIRE(ctx, conf->max_boxes >= 1 && conf->max_boxes <= 1024, "%s: max_boxes must be in [1, 1024]", who);
    for (int i = 0; i < 18; ++i) FV_REQUIRE(ctx, std::isfinite(conf->anchors[i]) && conf->anchors[i] > 0.f, "%s: anchors must be finite and > 0", who);
    FV_REQUIRE(ctx, det_shape_ok(batch, image_size, conf->max_boxes), "%s: bad batch or image_size (a multiple of 32)", who);
    FV_REQUIRE(ctx, ncls >= 1 && ncls <= 4096 && c_pad >= 3 * (5 + ncls), "%s: c_pad too small (needs 3*(5+ncls)) or bad ncls", who);
    FV_REQUIRE(ctx, ((uintptr_t)scratch & 7) == 0, "%s: scratch must be 8-byte aligned", who);
    const size_t need = det_plan(batch, image_size, conf->max_boxes).bytes;
    FV_REQUIRE(ctx, scratch_bytes >= need, "%s: scratch %zu < %zu bytes", who, scratch_bytes, need);
    return FV_OK;
}

int fv_det_loss_launch(fv_ctx* ctx, const float* const* y3, const float* const* t3, int batch, int image_size, int ncls, int c_pad,
                       const fv_yolo_det_conf* conf, double loss_weight, void* scratch, float* loss, float* const* dy3, double* stats) {
    const DetPlan p = det_plan(batch, image_size, conf->max_boxes);
    DetArgs a;
    for (int s = 0; s < 3; ++s) {
        a.y[s] = y3[s]; a.t[s] = t3[s]; a.dy[s] = dy3[s]; a.g[s] = p.g[s]; a.nc[s] = p.nc[s];
        for (int k = 0; k < 3; ++k) { a.aw[s * 3 + k] = (double)conf->anchors[s * 6 + 2 * k]; a.ah[s * 3 + k] = (double)conf->anchors[s * 6 + 2 * k + 1]; }
    }
    double* boxes = (double*)scratch;
    double* part = (double*)((char*)scratch + p.off_part);
    int* counts = (int*)((char*)scratch + p.off_counts);
    const int E = 5 + ncls;
    const double slots = 63.0 * (image_size / 32) * (image_size / 32) * batch;
    {
        FvProfScope ps(ctx, "det_gather_kernel", 0.0, 4.0 * slots);
        hipLaunchKernelGGL(det_gather_kernel, dim3(batch), dim3(256), 0, ctx->stream, a, image_size, E, conf->max_boxes, boxes, counts);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "det_loss_kernel", 0.0, 4.0 * slots * (6.0 + c_pad / 3.0));
        hipLaunchKernelGGL(det_loss_kernel, dim3((unsigned)p.nblocks), dim3(256), (size_t)conf->max_boxes * 4 * sizeof(double), ctx->stream, a,
                           image_size, ncls, c_pad, (int)conf->box_loss, (double)conf->ignore_thresh, (double)conf->box_weight,
                           (double)conf->noobj_weight, (int)conf->max_boxes, loss_weight / (double)batch, boxes, counts, part);
        FV_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(det_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, part, (int)p.nblocks, counts, batch, (int)conf->max_boxes, loss, stats);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

extern "C" {

size_t fv_yolo_det_scratch_bytes(int batch, int image_size, int max_boxes) {
    if (!det_shape_ok(batch, image_size, max_boxes)) return 0;
    return det_plan(batch, image_size, max_boxes).bytes;
}

int fv_yolo_det_loss_grad(fv_ctx* ctx, const float* const* yp3, const float* const* yt3, int batch, int image_size, int ncls, int c_pad,
                          const fv_yolo_det_conf* conf, double loss_weight, void* scratch, size_t scratch_bytes, float* loss,
                          float* const* dy3, double* stats) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, yp3 && yt3 && dy3 && loss, "yolo_det_loss_grad: NULL buffer");
    for (int s = 0; s < 3; ++s) FV_REQUIRE(ctx, yp3[s] && yt3[s] && dy3[s], "yolo_det_loss_grad: scale %d: NULL buffer", s);
    FV_REQUIRE(ctx, std::isfinite(loss_weight) && loss_weight > 0.0, "yolo_det_loss_grad: loss_weight must be finite and > 0");
    if (int rc = fv_det_check(ctx, "yolo_det_loss_grad", conf, batch, image_size, ncls, c_pad, scratch, scratch_bytes, stats)) return rc;
    return fv_det_loss_launch(ctx, yp3, yt3, batch, image_size, ncls, c_pad, conf, loss_weight, scratch, loss, dy3, stats);
}

}  // extern "C"
