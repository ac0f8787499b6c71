// Tiled inference on gfx950, the step between fv_decode_nms on the tile views and the rows evaluate() / validate() consume: every
// view's detections projected into frame coordinates and one cross-tile greedy NMS per frame.  DESIGN.md section 30, contract in
// tile_merge.h.
//
// One 256-thread workgroup (4 waves) per frame:
//   1. collect: every (view, slot) of the frame with slot < count and score > 0 takes a place in the LDS key array through an
//      integer LDS counter (the order of arrival does not matter: the key carries the candidate's index)
//   2. LDS bitonic sort of 64-bit keys (score bits | ~index) over the next power of two -> descending score, ties: lower view,
//      then lower slot (fv_rank_key, fv_bitonic_sort of block_ops.h)
//   3. project: the candidate at rank p becomes an fp64 box in the frame's slice of the workspace, in rank order (4096 x 32 B does
//      not fit LDS next to the keys; the sweep then reads the slice coalesced)
//   4. greedy walk, at most FV_DET_ROWS rounds: every wave finds the next alive rank from the 64 alive words (one ballot), then
//      the waves sweep the later alive ranks, one ballot per 64 ranks, and clear what the kept box suppresses
//   5. the kept ranks become corners / rows / src
// No float atomics: no float is ever summed.  Every coordinate operation is one IEEE double operation (-ffp-contract=off).
#include <climits>
#include "block_ops.h"
#include "bbox_iou.h"
#include "tile_merge.h"

namespace {

constexpr int ROWS = FV_DET_ROWS;
constexpr int MAXC = FV_TILE_MAX_CANDS;
constexpr int NWORD = MAXC / 64;
static_assert(NWORD == 64, "the alive words are searched with one lane per word");

// overlap(kept a, later b) >= th as do_nms_v2 compares it: nan never, +inf always
__device__ __forceinline__ bool overlap_ge(const double* a, double bx0, double by0, double bx1, double by1, int metric, double th) {
    if (metric == FV_TILE_METRIC_IOU) return bbox_iou_f64(a[0], a[1], a[2], a[3], bx0, by0, bx1, by1) >= th;
    const double iw = interval_overlap_f64(a[0], a[2], bx0, bx1), ih = interval_overlap_f64(a[1], a[3], by0, by1);
    const double inter = iw * ih;
    const double aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (bx1 - bx0) * (by1 - by0);
    return inter / fmin(aa, ab) >= th;
}

__global__ __launch_bounds__(256) void tile_merge_kernel(const int* __restrict__ boxes, const float* __restrict__ score,
                                                         const int* __restrict__ count, const int* __restrict__ tiles,
                                                         const int* __restrict__ frame_off, int T, int K, int S, int metric, double th,
                                                         double* ws, double* __restrict__ corners, double* __restrict__ rows,
                                                         int* __restrict__ nrows, int* __restrict__ src) {
    __shared__ unsigned long long keys[MAXC];
    __shared__ unsigned long long alive[NWORD];
    __shared__ int s_kept[ROWS];
    __shared__ int s_n;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    double* wb = ws + (size_t)f * MAXC * 4;
    const int v0 = frame_off[f], v1 = frame_off[f + 1];
    const bool bad = v0 < 0 || v1 < v0 || v1 > T;

    if (tid == 0) s_n = 0;
    for (int p = tid; p < MAXC; p += 256) keys[p] = 0;
    __syncthreads();

    // ---- 1. collect
    if (!bad) {
        const long long total = (long long)(v1 - v0) * K;          // <= T * K <= INT_MAX (host check)
        for (long long q = tid; q < total; q += 256) {
            const int lv = (int)(q / K), k = (int)(q - (long long)lv * K);
            const int t = v0 + lv;
            const int c = min(max(count[t], 0), K);
            if (k >= c) continue;
            const float s = score[(size_t)t * K + k];
            if (!(s > 0.0f)) continue;                              // nan is never > 0
            const int pos = atomicAdd(&s_n, 1);
            if (pos < MAXC) keys[pos] = fv_rank_key(s, (unsigned)q);
        }
    }
    __syncthreads();
    const int n = s_n;
    if (bad || n > MAXC) {       // the host checks its own bound; what the device finds beyond it is marked, no box of it is read
        for (int r = tid; r < ROWS; r += 256) {
            const size_t o = (size_t)f * ROWS + r;
            for (int c = 0; c < 4; ++c) corners[o * 4 + c] = 0.0;
            for (int c = 0; c < 5; ++c) rows[o * 5 + c] = 0.0;
            src[o] = -1;
        }
        if (tid == 0) nrows[f] = -1;
        return;
    }

    // ---- 2. rank
    int P = 64;
    while (P < n) P <<= 1;
    fv_bitonic_sort<256, true>(keys, P, tid);

    // ---- 3. project, in rank order
    for (int p = tid; p < n; p += 256) {
        const unsigned q = fv_rank_index(keys[p]);
        const int t = v0 + (int)(q / (unsigned)K);
        const int* b = boxes + ((size_t)v0 * K + q) * 4;
        const int* g = tiles + (size_t)t * 5;                       // frame, y0, x0, th, tw
        const int th_ = g[3], tw_ = g[4];
        const double H = (double)th_, W = (double)tw_, Sd = (double)S;
        double x0, x1, y0, y1;
        if (tw_ >= th_) {                                           // int -> double, subtract, max, multiply, divide, min
            const int pad = S - (int)(H / W * Sd);
            const double pt = (double)(pad / 2);
            x0 = fmin((double)b[0] * W / Sd, W);
            x1 = fmin((double)b[2] * W / Sd, W);
            y0 = fmin(fmax((double)b[1] - pt, 0.0) * W / Sd, H);
            y1 = fmin(fmax((double)b[3] - pt, 0.0) * W / Sd, H);
        } else {
            const int pad = S - (int)(W / H * Sd);
            const double pl = (double)(pad / 2);
            x0 = fmin(fmax((double)b[0] - pl, 0.0) * H / Sd, W);
            x1 = fmin(fmax((double)b[2] - pl, 0.0) * H / Sd, W);
            y0 = fmin((double)b[1] * H / Sd, H);
            y1 = fmin((double)b[3] * H / Sd, H);
        }
        const double ox = (double)g[2], oy = (double)g[1];
        wb[p * 4 + 0] = x0 + ox; wb[p * 4 + 1] = y0 + oy; wb[p * 4 + 2] = x1 + ox; wb[p * 4 + 3] = y1 + oy;
    }
    for (int w = tid; w < NWORD; w += 256) {
        const int c = min(max(n - w * 64, 0), 64);
        alive[w] = c == 64 ? ~0ull : ((1ull << c) - 1ull);
    }
    __syncthreads();

    // ---- 4. greedy walk.  Every wave computes the same rank i from the alive words; a wave that already sweeps clears only bits
    // above i, so a slower wave still finds i.  One barrier per round.
    const int nwn = (n + 63) >> 6;
    int cursor = 0, nk = 0;
    while (nk < ROWS) {
        unsigned long long word = alive[lane];
        const int cw = cursor >> 6;
        if (lane < cw) word = 0;
        else if (lane == cw) word &= ~0ull << (cursor & 63);
        const unsigned long long m = __ballot(word != 0);
        if (m == 0) break;
        const int first = __ffsll(m) - 1;
        const unsigned long long w1 = __shfl(word, first);
        const int i = first * 64 + (__ffsll(w1) - 1);
        if (tid == 0) s_kept[nk] = i;
        ++nk;
        cursor = i + 1;
        if (nk == ROWS) break;                                      // nothing after the last row needs deciding
        const double a[4] = {wb[i * 4], wb[i * 4 + 1], wb[i * 4 + 2], wb[i * 4 + 3]};
        for (int c = (cursor >> 6) + wave; c < nwn; c += 4) {
            const int j = (c << 6) + lane;
            const unsigned long long aw = alive[c];
            bool pred = false;
            if (j >= cursor && j < n && ((aw >> lane) & 1ull))
                pred = overlap_ge(a, wb[j * 4], wb[j * 4 + 1], wb[j * 4 + 2], wb[j * 4 + 3], metric, th);
            const unsigned long long kill = __ballot(pred);
            if (lane == 0 && kill) alive[c] = aw & ~kill;
        }
        __syncthreads();
    }
    __syncthreads();

    // ---- 5. output
    for (int r = tid; r < ROWS; r += 256) {
        const size_t o = (size_t)f * ROWS + r;
        if (r < nk) {
            const int i = s_kept[r];
            const unsigned long long key = keys[i];
            const unsigned q = fv_rank_index(key);
            const float s = fv_rank_score(key);
            const double x0 = wb[i * 4], y0 = wb[i * 4 + 1], x1 = wb[i * 4 + 2], y1 = wb[i * 4 + 3];
            corners[o * 4 + 0] = x0; corners[o * 4 + 1] = y0; corners[o * 4 + 2] = x1; corners[o * 4 + 3] = y1;
            rows[o * 5 + 0] = x0; rows[o * 5 + 1] = y0; rows[o * 5 + 2] = x1 - x0; rows[o * 5 + 3] = y1 - y0;
            rows[o * 5 + 4] = (double)fminf(s, 1.0f);
            src[o] = (int)((unsigned)v0 * (unsigned)K + q);
        } else {
            for (int c = 0; c < 4; ++c) corners[o * 4 + c] = 0.0;
            for (int c = 0; c < 5; ++c) rows[o * 5 + c] = 0.0;
            src[o] = -1;
        }
    }
    if (tid == 0) nrows[f] = nk;
}

}  // namespace

extern "C" size_t fv_tile_merge_workspace_bytes(int n_frames) {
    return n_frames < 1 ? 0 : (size_t)n_frames * MAXC * 4 * sizeof(double);
}

extern "C" int fv_tile_merge(fv_ctx* ctx, const int32_t* boxes, const float* score, const int32_t* count, const int32_t* tiles,
                             const int32_t* frame_off, int n_views, int n_frames, int num_cands, int image_size, int metric,
                             double merge_th, void* workspace, size_t workspace_bytes, double* corners, double* rows, int32_t* nrows,
                             int32_t* src) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n_views >= 1 && n_frames >= 1 && num_cands >= 1, "fv_tile_merge: n_views %d, n_frames %d, num_cands %d (all >= 1)",
               n_views, n_frames, num_cands);
    FV_REQUIRE(ctx, num_cands <= FV_TILE_MAX_K, "fv_tile_merge: num_cands %d unsupported (1..%d)", num_cands, FV_TILE_MAX_K);
    FV_REQUIRE(ctx, (long long)n_views * num_cands <= INT_MAX, "fv_tile_merge: n_views %d x num_cands %d is beyond int32", n_views,
               num_cands);
    FV_REQUIRE(ctx, image_size >= 1, "fv_tile_merge: image_size %d", image_size);
    FV_REQUIRE(ctx, metric == FV_TILE_METRIC_IOS || metric == FV_TILE_METRIC_IOU, "fv_tile_merge: metric %d (0 ios, 1 iou)", metric);
    FV_REQUIRE(ctx, merge_th > 0.0 && merge_th <= 1.0, "fv_tile_merge: merge_th %g is outside (0, 1]", merge_th);
    FV_REQUIRE(ctx, boxes && score && count && tiles && frame_off && workspace && corners && rows && nrows && src,
               "fv_tile_merge: NULL buffer");
    FV_REQUIRE(ctx, workspace_bytes >= fv_tile_merge_workspace_bytes(n_frames), "fv_tile_merge: workspace of %zu bytes, %zu needed",
               workspace_bytes, fv_tile_merge_workspace_bytes(n_frames));
    FV_REQUIRE(ctx, ((uintptr_t)workspace & 7) == 0, "fv_tile_merge: workspace must be 8-byte aligned");
    FvProfScope ps(ctx, "tile_merge_kernel", 0.0, (double)n_views * num_cands * 24.0 + (double)n_frames * ROWS * 76.0);
    hipLaunchKernelGGL(tile_merge_kernel, dim3(n_frames), dim3(256), 0, ctx->stream, boxes, score, count, tiles, frame_off, n_views,
                       num_cands, image_size, metric, merge_th, (double*)workspace, corners, rows, nrows, src);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
