// The detection metric of cal_mAP_fd (reference evaluate.py:27-127) on gfx950, for FaceDetector.validate: the rows evaluate() would
// have written from a decode/NMS result, the greedy (ground truth, detection) assignment per image, and the confidence ranking with
// the precision / recall sweep over several IoU thresholds.  DESIGN.md section 28.
//
//   fv_det_rows_from_nms   one thread per (image, row): FaceDetector._project_back's float64 operations in its order
//   fv_det_match_rows      one 256-thread workgroup per image; per ground-truth box the best remaining detection is cached in LDS,
//                          a round takes the largest cached pair and refreshes only the boxes that pointed at the taken detection
//   fv_det_ap_sweep        compaction (integer scan) -> stable LSD radix sort of (key, position), 8 bits per pass over the 64 key
//                          bits, one wave per tile, ranks from ballots -> per threshold a tiled integer scan of "IoU >= th" and the
//                          trapezoid terms summed in a fixed order
//
// No float atomics anywhere: every sum has one order, whatever the launch geometry.  Integer LDS atomics only count.
#include "block_ops.h"
#include "bbox_iou.h"

namespace {

constexpr int ROWS = FV_DET_ROWS;        // rows per image (FaceDetector._write_rows hard-codes boxes[:60])
constexpr int MAX_GT = FV_DET_MAX_GT;    // ground-truth boxes per image the matching kernel caches in LDS
constexpr int TILE = 2048;               // elements per workgroup in the sort and sweep kernels

// ------------------------------------------------------------------------------------------------ rows
__global__ __launch_bounds__(256) void det_rows_kernel(const int* __restrict__ boxes, const float* __restrict__ score,
                                                       const int* __restrict__ count, const int* __restrict__ geom, int nimg, int K,
                                                       int S, double* __restrict__ rows, int* __restrict__ nrows) {
    const long long slot = blockIdx.x * 256ll + threadIdx.x;
    if (slot >= (long long)nimg * ROWS) return;
    const int img = (int)(slot / ROWS), r = (int)(slot - (long long)img * ROWS);
    const int c = min(max(count[img], 0), min(ROWS, K));
    if (r == 0) nrows[img] = c;
    double* o = rows + slot * 5;
    if (r >= c) {
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0;
        return;
    }
    const int* b = boxes + ((long long)img * K + r) * 4;
    const int* g = geom + (long long)img * 6;           // h, w, pad_t, pad_b, pad_l, pad_r
    const double H = (double)g[0], W = (double)g[1], Sd = (double)S;
    double x0, x1, y0, y1;
    if (g[1] >= g[0]) {                                 // int -> double, subtract, max, multiply, divide, min
        x0 = fmin((double)b[0] * W / Sd, W);
        x1 = fmin((double)b[2] * W / Sd, W);
        const double pt = (double)g[2];
        y0 = fmin(fmax((double)b[1] - pt, 0.0) * W / Sd, H);
        y1 = fmin(fmax((double)b[3] - pt, 0.0) * W / Sd, H);
    } else {
        const double pl = (double)g[4];
        x0 = fmin(fmax((double)b[0] - pl, 0.0) * H / Sd, W);
        x1 = fmin(fmax((double)b[2] - pl, 0.0) * H / Sd, W);
        y0 = fmin((double)b[1] * H / Sd, H);
        y1 = fmin((double)b[3] * H / Sd, H);
    }
    o[0] = x0; o[1] = y0; o[2] = x1 - x0; o[3] = y1 - y0;
    o[4] = (double)fminf(score[(long long)img * K + r], 1.0f);
}

// ------------------------------------------------------------------------------------------------ match
__global__ __launch_bounds__(256) void det_match_kernel(const double* __restrict__ rows, const int* __restrict__ nrows,
                                                        const double* __restrict__ gt, const long long* __restrict__ gt_off,
                                                        double* __restrict__ iou_out, int* __restrict__ flag_out) {
    __shared__ double s_best[MAX_GT];          // per ground-truth box: IoU of its best remaining detection, -1 = none / box used
    __shared__ unsigned char s_bd[MAX_GT];     // ... and which detection that is
    __shared__ double s_det[ROWS * 4];         // detection corners
    __shared__ double s_riou[4];
    __shared__ int s_rg[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.x;
    const int D = min(max(nrows[img], 0), ROWS);
    const long long g0 = gt_off[img], G64 = gt_off[img + 1] - g0;
    for (int d = tid; d < ROWS; d += 256) iou_out[(long long)img * ROWS + d] = -1.0;
    if (G64 < 0 || G64 > MAX_GT) {             // the host checks its own bound; what the device finds beyond it is marked, not read
        if (tid == 0) flag_out[img] = -1;
        return;
    }
    const int G = (int)G64;
    if (D == 0 || G == 0) {
        if (tid == 0) flag_out[img] = 0;
        return;
    }
    for (int d = tid; d < D; d += 256) {
        const double* r = rows + ((long long)img * ROWS + d) * 5;
        s_det[d * 4 + 0] = r[0]; s_det[d * 4 + 1] = r[1]; s_det[d * 4 + 2] = r[0] + r[2]; s_det[d * 4 + 3] = r[1] + r[3];
    }
    __syncthreads();

    unsigned long long used_d = 0;             // the same value in every thread
    auto refresh = [&](int g) {
        const double* q = gt + (g0 + g) * 4;
        const double gx0 = q[0], gy0 = q[1], gx1 = q[0] + q[2], gy1 = q[1] + q[3];
        double best = -1.0;
        int bd = 0;
        for (int d = 0; d < D; ++d) {
            if ((used_d >> d) & 1ull) continue;
            const double v = bbox_iou_f64(gx0, gy0, gx1, gy1, s_det[d * 4], s_det[d * 4 + 1], s_det[d * 4 + 2], s_det[d * 4 + 3]);
            if (v > 0.0 && v > best) { best = v; bd = d; }          // nan is never > 0; equal IoUs keep the smaller detection
        }
        s_best[g] = best;
        s_bd[g] = (unsigned char)bd;
    };
    for (int g = tid; g < G; g += 256) refresh(g);
    __syncthreads();

    bool any = false;
    const int rounds = min(D, G);
    for (int round = 0; round < rounds; ++round) {
        double lb = -1.0;
        int lg = 0x7fffffff;
        for (int g = tid; g < G; g += 256) {
            const double v = s_best[g];
            if (v > lb) { lb = v; lg = g; }                          // ascending g: equal IoUs keep the smaller box
        }
        fv_wave_best<max_more>(lb, lg);
        if (lane == 0) { s_riou[wave] = lb; s_rg[wave] = lg; }
        __syncthreads();
        double bb;
        int bg;
        fv_block_best<max_more, 4>(s_riou, s_rg, 1, bb, bg);
        if (!(bb > 0.0)) break;                                      // uniform: every thread computed the same pair
        any = true;
        const int bd = s_bd[bg];
        __syncthreads();                                             // everyone has read the round's tables
        used_d |= 1ull << bd;
        if (tid == 0) {
            iou_out[(long long)img * ROWS + bd] = bb;
            s_best[bg] = -1.0;
        }
        for (int g = tid; g < G; g += 256)
            if (g != bg && s_best[g] > 0.0 && s_bd[g] == bd) refresh(g);
        __syncthreads();
    }
    if (tid == 0) flag_out[img] = any ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ scans
// In-place exclusive scan of data[seg * stride + 0 .. n), the total stored at data[seg * stride + n]; one workgroup per segment.
__global__ __launch_bounds__(1024) void scan_excl_kernel(int* __restrict__ data, long long n, long long stride) {
    __shared__ int s_w[16];
    int* d = data + blockIdx.x * stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + tid;
        const int v = i < n ? d[i] : 0;
        const int inc = fv_wave_incl_scan(v, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const int t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < n) d[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) d[n] = carry;
}

// ------------------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(256) void ap_image_counts_kernel(const int* __restrict__ nrows, const int* __restrict__ flag, int n_img,
                                                              int* __restrict__ img_off) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img < n_img) img_off[img] = flag[img] > 0 ? min(max(nrows[img], 0), ROWS) : 0;
}

// Ascending order of this key = descending confidence (np.argsort(-conf)); -0.0 ranks with 0.0 as it compares.
__device__ __forceinline__ unsigned long long desc_key(double c) {
    if (c == 0.0) c = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(c);
    const unsigned long long asc = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ~asc;
}

__global__ __launch_bounds__(256) void ap_compact_kernel(const double* __restrict__ rows, const int* __restrict__ nrows,
                                                         const double* __restrict__ iou, const int* __restrict__ flag, int n_img,
                                                         const int* __restrict__ img_off, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ idx, double* __restrict__ iou_c) {
    const long long slot = blockIdx.x * 256ll + threadIdx.x;
    if (slot >= (long long)n_img * ROWS) return;
    const int img = (int)(slot / ROWS), r = (int)(slot - (long long)img * ROWS);
    if (flag[img] <= 0 || r >= min(max(nrows[img], 0), ROWS)) return;
    const int pos = img_off[img] + r;
    keys[pos] = desc_key(rows[slot * 5 + 4]);
    idx[pos] = pos;
    iou_c[pos] = iou[slot];
}

// ------------------------------------------------------------------------------------------------ radix sort, one wave per tile
__global__ __launch_bounds__(64) void radix_hist_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ n_ptr,
                                                        int shift, int* __restrict__ hist, int nblk) {
    __shared__ int cnt[256];
    const int lane = threadIdx.x, blk = blockIdx.x;
    const int N = *n_ptr;
    for (int b = lane; b < 256; b += 64) cnt[b] = 0;
    __syncthreads();
    for (int r = 0; r < TILE / 64; ++r) {
        const long long i = (long long)blk * TILE + r * 64 + lane;
        if (i < N) atomicAdd(&cnt[(int)((keys[i] >> shift) & 255ull)], 1);
    }
    __syncthreads();
    for (int b = lane; b < 256; b += 64) hist[(long long)b * nblk + blk] = cnt[b];     // bin-major: one scan gives every tile's bases
}

__global__ __launch_bounds__(64) void radix_scatter_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ idx,
                                                           const int* __restrict__ n_ptr, int shift, const int* __restrict__ hist,
                                                           int nblk, unsigned long long* __restrict__ keys_out,
                                                           int* __restrict__ idx_out) {
    __shared__ int base[256];
    const int lane = threadIdx.x, blk = blockIdx.x;
    const int N = *n_ptr;
    for (int b = lane; b < 256; b += 64) base[b] = hist[(long long)b * nblk + blk];
    __syncthreads();
    for (int r = 0; r < TILE / 64; ++r) {
        const long long i = (long long)blk * TILE + r * 64 + lane;
        if ((long long)blk * TILE + r * 64 >= N) break;              // uniform
        const bool active = i < N;
        unsigned long long key = 0;
        int v = 0;
        if (active) { key = keys[i]; v = idx[i]; }
        const int d = (int)((key >> shift) & 255ull);
        unsigned long long peers = __ballot(active);                 // lanes of this round with the same digit
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long m = __ballot(active && bit);
            peers &= bit ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        const int pos = base[d] + rank;
        __syncthreads();
        if (active && rank == 0) base[d] += __popcll(peers);
        __syncthreads();
        if (active && pos < N) { keys_out[pos] = key; idx_out[pos] = v; }
    }
}

// ------------------------------------------------------------------------------------------------ sweep
struct Thresholds {
    double th[FV_DET_MAX_TH];
};

// flags of the 8 consecutive ranks a thread owns: bit e <=> rank k0 + e exists and its IoU >= th
__device__ __forceinline__ unsigned tp_bits(const int* __restrict__ idx, const double* __restrict__ iou_c, long long k0, int N, double th) {
    unsigned bits = 0;
    for (int e = 0; e < 8; ++e)
        if (k0 + e < N && iou_c[idx[k0 + e]] >= th) bits |= 1u << e;
    return bits;
}

__global__ __launch_bounds__(256) void ap_tp_count_kernel(const int* __restrict__ idx, const double* __restrict__ iou_c,
                                                          const int* __restrict__ n_ptr, Thresholds ths, int* __restrict__ blk_cnt,
                                                          int nblk) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x, t = blockIdx.y;
    const int N = *n_ptr;
    int c = __popc(tp_bits(idx, iou_c, (long long)blk * TILE + tid * 8, N, ths.th[t]));
    c = fv_wave_incl_scan(c, lane);
    if (lane == 63) s_w[wave] = c;
    __syncthreads();
    if (tid == 0) blk_cnt[(long long)t * (nblk + 1) + blk] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(256) void ap_sweep_kernel(const int* __restrict__ idx, const double* __restrict__ iou_c,
                                                       const int* __restrict__ n_ptr, Thresholds ths, double gt_count,
                                                       const int* __restrict__ blk_cnt, int nblk, double* __restrict__ blk_ap,
                                                       int* __restrict__ order, int* __restrict__ counts, long long counts_stride) {
    __shared__ int s_w[4];
    __shared__ double s_a[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x, t = blockIdx.y;
    const int N = *n_ptr;
    const long long k0 = (long long)blk * TILE + tid * 8;
    const unsigned bits = tp_bits(idx, iou_c, k0, N, ths.th[t]);
    const int mine = __popc(bits);
    const int inc = fv_wave_incl_scan(mine, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int tp = blk_cnt[(long long)t * (nblk + 1) + blk] + inc - mine;          // true positives among the ranks before k0
    for (int w = 0; w < wave; ++w) tp += s_w[w];
    double sum = 0.0;
    for (int e = 0; e < 8; ++e) {
        const long long k = k0 + e;
        if (k >= N) break;
        const int f = (bits >> e) & 1u;
        const int prev = tp;
        tp += f;
        if (counts) counts[t * counts_stride + k] = tp;
        if (order && t == 0) order[k] = idx[k];
        if (k >= 1) {
            // (r_k - r_{k-1}) * (p_k + p_{k-1}) / 2 with p = tp / (k + 1), r = tp / gt_count: pr_curve's divisions
            const double rk = (double)tp / gt_count, rp = (double)prev / gt_count;
            const double pk = (double)tp / (double)(k + 1), pp = (double)prev / (double)k;
            sum += (rk - rp) * (pk + pp) / 2.0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);   // lane 0 holds fv_wave_sum's tree
    if (lane == 0) s_a[wave] = sum;
    __syncthreads();
    if (tid == 0) blk_ap[(long long)t * nblk + blk] = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
}

__global__ __launch_bounds__(64) void ap_final_kernel(const int* __restrict__ n_ptr, double gt_count, const int* __restrict__ blk_cnt,
                                                      const double* __restrict__ blk_ap, int nblk, int T, double* __restrict__ result,
                                                      int* __restrict__ n_det) {
    const int lane = threadIdx.x, t = blockIdx.x;
    const int N = *n_ptr;
    double sum = 0.0;
    for (int b = lane; b < nblk; b += 64) sum += blk_ap[(long long)t * nblk + b];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if (lane == 0) {
        const int tp = blk_cnt[(long long)t * (nblk + 1) + nblk];
        result[t] = sum;
        result[T + t] = N > 0 ? (double)tp / (double)N : 0.0;
        result[2 * T + t] = N > 0 ? (double)tp / gt_count : 0.0;
        if (t == 0) n_det[0] = N;
    }
}

struct SweepLayout {
    size_t img_off, keys_a, keys_b, idx_a, idx_b, iou_c, hist, blk_cnt, blk_ap, bytes;
    long long slots;
    int nblk;
};

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

SweepLayout sweep_layout(int n_img) {
    SweepLayout L;
    L.slots = (long long)n_img * ROWS;
    L.nblk = (int)((L.slots + TILE - 1) / TILE);
    size_t o = 0;
    L.img_off = o; o = align_up(o + ((size_t)n_img + 1) * 4);
    L.keys_a = o; o = align_up(o + (size_t)L.slots * 8);
    L.keys_b = o; o = align_up(o + (size_t)L.slots * 8);
    L.idx_a = o; o = align_up(o + (size_t)L.slots * 4);
    L.idx_b = o; o = align_up(o + (size_t)L.slots * 4);
    L.iou_c = o; o = align_up(o + (size_t)L.slots * 8);
    L.hist = o; o = align_up(o + ((size_t)256 * L.nblk + 1) * 4);
    L.blk_cnt = o; o = align_up(o + (size_t)FV_DET_MAX_TH * (L.nblk + 1) * 4);
    L.blk_ap = o; o = align_up(o + (size_t)FV_DET_MAX_TH * L.nblk * 8);
    L.bytes = o;
    return L;
}

constexpr int MAX_IMAGES = 1 << 24;      // 60 rows each: positions and counts stay inside int32

}  // namespace

extern "C" int fv_det_rows_from_nms(fv_ctx* ctx, const int32_t* boxes, const float* score, const int32_t* count, const int32_t* geom,
                                    int nimg, int num_cands, int image_size, double* rows, int32_t* nrows) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, nimg >= 0 && nimg <= MAX_IMAGES, "fv_det_rows_from_nms: nimg %d unsupported", nimg);
    if (nimg == 0) return FV_OK;
    FV_REQUIRE(ctx, boxes && score && count && geom && rows && nrows, "fv_det_rows_from_nms: NULL buffer");
    FV_REQUIRE(ctx, num_cands >= 1 && image_size >= 1, "fv_det_rows_from_nms: num_cands %d / image_size %d", num_cands, image_size);
    const long long slots = (long long)nimg * ROWS;
    FvProfScope ps(ctx, "det_rows_kernel", 0.0, (double)slots * (16.0 + 4.0 + 40.0));
    hipLaunchKernelGGL(det_rows_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, ctx->stream, boxes, score, count, geom,
                       nimg, num_cands, image_size, rows, nrows);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

extern "C" int fv_det_match_rows(fv_ctx* ctx, const double* rows, const int32_t* nrows, const double* gt, const int64_t* gt_off,
                                 int nimg, int max_gt, double* iou, int32_t* flag) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, nimg >= 0 && nimg <= MAX_IMAGES, "fv_det_match_rows: nimg %d unsupported", nimg);
    FV_REQUIRE(ctx, max_gt >= 0 && max_gt <= MAX_GT, "fv_det_match_rows: %d ground-truth boxes on one image (at most %d)", max_gt,
               MAX_GT);
    if (nimg == 0) return FV_OK;
    FV_REQUIRE(ctx, rows && nrows && gt_off && iou && flag && (gt || max_gt == 0), "fv_det_match_rows: NULL buffer");
    FvProfScope ps(ctx, "det_match_kernel", 0.0, (double)nimg * (ROWS * 48.0 + max_gt * 32.0));
    hipLaunchKernelGGL(det_match_kernel, dim3(nimg), dim3(256), 0, ctx->stream, rows, nrows, gt, (const long long*)gt_off, iou, flag);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

extern "C" size_t fv_det_ap_sweep_workspace_bytes(int n_img) {
    if (n_img < 0 || n_img > MAX_IMAGES) return 0;
    return sweep_layout(n_img).bytes;
}

extern "C" int fv_det_ap_sweep(fv_ctx* ctx, const double* rows, const int32_t* nrows, const double* iou, const int32_t* flag, int n_img,
                               const double* thresholds, int n_th, int64_t gt_count, void* workspace, size_t workspace_bytes,
                               double* result, int32_t* n_det, int32_t* order, int32_t* counts) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n_img >= 0 && n_img <= MAX_IMAGES, "fv_det_ap_sweep: n_img %d unsupported", n_img);
    FV_REQUIRE(ctx, thresholds && n_th >= 1 && n_th <= FV_DET_MAX_TH, "fv_det_ap_sweep: %d thresholds (1..%d)", n_th, FV_DET_MAX_TH);
    FV_REQUIRE(ctx, gt_count >= 1, "fv_det_ap_sweep: gt_count %lld (the recall denominator) must be >= 1", (long long)gt_count);
    FV_REQUIRE(ctx, result && n_det, "fv_det_ap_sweep: NULL result");
    const SweepLayout L = sweep_layout(n_img);
    FV_REQUIRE(ctx, workspace_bytes >= L.bytes && (workspace || L.bytes == 0), "fv_det_ap_sweep: workspace %zu bytes < %zu", workspace_bytes,
               L.bytes);
    FV_REQUIRE(ctx, ((uintptr_t)workspace & 7) == 0, "fv_det_ap_sweep: workspace must be 8-byte aligned");
    if (n_img == 0) {
        FV_HIP(ctx, hipMemsetAsync(result, 0, (size_t)3 * n_th * sizeof(double), ctx->stream));
        FV_HIP(ctx, hipMemsetAsync(n_det, 0, sizeof(int32_t), ctx->stream));
        return FV_OK;
    }
    FV_REQUIRE(ctx, rows && nrows && iou && flag, "fv_det_ap_sweep: NULL buffer");
    Thresholds ths;
    for (int t = 0; t < FV_DET_MAX_TH; ++t) ths.th[t] = t < n_th ? thresholds[t] : 0.0;
    char* ws = (char*)workspace;
    int* img_off = (int*)(ws + L.img_off);
    unsigned long long* keys[2] = {(unsigned long long*)(ws + L.keys_a), (unsigned long long*)(ws + L.keys_b)};
    int* idx[2] = {(int*)(ws + L.idx_a), (int*)(ws + L.idx_b)};
    double* iou_c = (double*)(ws + L.iou_c);
    int* hist = (int*)(ws + L.hist);
    int* blk_cnt = (int*)(ws + L.blk_cnt);
    double* blk_ap = (double*)(ws + L.blk_ap);
    const int* n_ptr = img_off + n_img;
    const int nblk = L.nblk;
    const unsigned slot_blocks = (unsigned)((L.slots + 255) / 256);
    hipStream_t st = ctx->stream;
    {
        FvProfScope ps(ctx, "det_ap_compact", 0.0, (double)L.slots * 40.0);
        hipLaunchKernelGGL(ap_image_counts_kernel, dim3((n_img + 255) / 256), dim3(256), 0, st, nrows, flag, n_img, img_off);
        hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, st, img_off, (long long)n_img, 0ll);
        hipLaunchKernelGGL(ap_compact_kernel, dim3(slot_blocks), dim3(256), 0, st, rows, nrows, iou, flag, n_img, img_off, keys[0], idx[0],
                           iou_c);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "det_ap_radix_sort", 0.0, (double)L.slots * 8.0 * 36.0);
        for (int pass = 0; pass < 8; ++pass) {
            const int a = pass & 1, b = a ^ 1;
            hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(64), 0, st, keys[a], n_ptr, pass * 8, hist, nblk);
            hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, st, hist, 256ll * nblk, 0ll);
            hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(64), 0, st, keys[a], idx[a], n_ptr, pass * 8, hist, nblk, keys[b],
                               idx[b]);
        }
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "det_ap_sweep", 0.0, (double)L.slots * n_th * 24.0);
        hipLaunchKernelGGL(ap_tp_count_kernel, dim3(nblk, n_th), dim3(256), 0, st, idx[0], iou_c, n_ptr, ths, blk_cnt, nblk);
        hipLaunchKernelGGL(scan_excl_kernel, dim3(n_th), dim3(1024), 0, st, blk_cnt, (long long)nblk, (long long)(nblk + 1));
        hipLaunchKernelGGL(ap_sweep_kernel, dim3(nblk, n_th), dim3(256), 0, st, idx[0], iou_c, n_ptr, ths, (double)gt_count, blk_cnt,
                           nblk, blk_ap, order, counts, L.slots);
        hipLaunchKernelGGL(ap_final_kernel, dim3(n_th), dim3(64), 0, st, n_ptr, (double)gt_count, blk_cnt, blk_ap, nblk, n_th, result,
                           n_det);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}
