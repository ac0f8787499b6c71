// Three-scale head on gfx950, the step between fv_yolo_decode_nms_batch and everything that reads fv_decode_nms' layout: the tail
// of the reference's detect() (score > 0, ascending stable argsort, the first num_cands) per image.  DESIGN.md section 33,
// contract in yolo_select.h.
//
// One 1024-thread workgroup (16 waves) per image:
//   1. strided pass over the rows: the class maximum as np.argmax finds it, on the bit patterns (integer compares only, so the
//      denormal mode cannot matter), and the kept rows' keys (score bits << 32) | r compacted in row order into LDS
//      (fv_block_compact).  Positive floats order as their bit patterns; an ascending key breaks ties toward the lower r.
//   2. LDS bitonic sort (fv_bitonic_sort of block_ops.h), ascending, over P = the next power of two >= max(kept, 2), padded with
//      ~0ull.  P follows the kept rows, not the capacity: a sparse image costs little.
//   3. the first num_cands keys drive the gather of boxes, objectness and classes; the rest of the slots are filled.
// Every output value is a copy of an input or min(bits, bits of 1.0f): no float arithmetic, no float atomics.
#include <climits>
#include "block_ops.h"
#include "yolo_select.h"

namespace {

constexpr unsigned INF_BITS = 0x7F800000u, ONE_BITS = 0x3F800000u;

__global__ __launch_bounds__(1024) void yolo_select_kernel(const int* __restrict__ boxes_all, const unsigned* __restrict__ obj_all,
                                                           const unsigned* __restrict__ classes_all, const int* __restrict__ count,
                                                           int capacity, int nclass, int refuse_at, int K, int* __restrict__ out_boxes,
                                                           int* __restrict__ out_src, unsigned* __restrict__ out_obj,
                                                           unsigned* __restrict__ out_score, unsigned* __restrict__ out_classes,
                                                           int* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);      // [next power of two >= max(capacity, 2)]
    __shared__ int wave_cnt[16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t img = blockIdx.x;
    const int c = count[img];
    const bool refused = c >= refuse_at;
    const int n = refused ? 0 : min(max(c, 0), capacity);                        // uniform; a refused image's rows are not read
    const int* __restrict__ boxes = boxes_all + img * capacity * 4;
    const unsigned* __restrict__ obj = obj_all + img * capacity;
    const unsigned* __restrict__ classes = classes_all + img * capacity * nclass;

    // ---- 1. class maximum and ordered compaction of the kept rows
    int kept = 0;
    for (int r0 = 0; r0 < n; r0 += 1024) {
        const int r = r0 + tid;
        unsigned best = 0;                                                       // largest positive pattern of the row; 0: none
        bool nan = false;
        if (r < n) {
            const unsigned* row = classes + (size_t)r * nclass;
            for (int k = 0; k < nclass; ++k) {
                const unsigned u = row[k];
                nan |= (u & 0x7FFFFFFFu) > INF_BITS;
                if ((int)u > 0 && u > best) best = u;                            // sign clear and not +0.0: ordered as the floats are
            }
        }
        const bool keep = r < n && !nan && best != 0;                            // score > 0; a NaN row's arg-max is its first NaN
        const int pos = kept + fv_block_compact(keep, wave_cnt, lane, wave);
        if (keep) keys[pos] = ((unsigned long long)min(best, ONE_BITS) << 32) | (unsigned)r;      // pos <= r < capacity
        int tot = 0;
        for (int w = 0; w < 16; ++w) tot += wave_cnt[w];
        kept += tot;
        __syncthreads();                                                         // wave_cnt is written again in the next round
    }

    // ---- 2. ascending sort of the kept keys
    if (kept > 1) {                                                              // uniform
        int P = 2;
        while (P < kept) P <<= 1;
        for (int p = kept + tid; p < P; p += 1024) keys[p] = ~0ull;
        __syncthreads();
        fv_bitonic_sort<1024, false>(keys, P, tid);
    }                                                                            // else: the loop's last barrier covers keys[0]

    // ---- 3. gather
    const int m = min(kept, K);
    const size_t o0 = img * K;
    for (int s = tid; s < K; s += 1024) {
        int4 bx = make_int4(-1, -1, -1, -1);
        int src = -1;
        unsigned ob = 0, sc = 0;
        if (s < m) {
            const unsigned long long key = keys[s];
            src = (int)(unsigned)(key & 0xFFFFFFFFull);
            sc = (unsigned)(key >> 32);
            const int* b = boxes + (size_t)src * 4;
            bx = make_int4(b[0], b[1], b[2], b[3]);
            ob = obj[src];
        }
        int* ob4 = out_boxes + (o0 + s) * 4;
        ob4[0] = bx.x; ob4[1] = bx.y; ob4[2] = bx.z; ob4[3] = bx.w;
        out_src[o0 + s] = src;
        out_obj[o0 + s] = ob;
        out_score[o0 + s] = sc;
    }
    if (out_classes) {
        for (int i = tid; i < K * nclass; i += 1024) {                           // K * nclass <= 512 * nclass: int32 (host check)
            const int s = i / nclass, k = i - s * nclass;
            unsigned v = 0;
            if (s < m) v = classes[(size_t)(unsigned)(keys[s] & 0xFFFFFFFFull) * nclass + k];
            out_classes[o0 * nclass + i] = v;
        }
    }
    if (tid == 0) out_count[img] = refused ? -1 : m;
}

}  // namespace

extern "C" int fv_yolo_select_cands(fv_ctx* ctx, const int32_t* boxes, const float* objness, const float* classes, const int32_t* count,
                                    int nimg, int capacity, int nclass, int refuse_at, int num_cands, int32_t* out_boxes,
                                    int32_t* out_src, float* out_obj, float* out_score, float* out_classes, int32_t* out_count) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, nimg >= 1, "fv_yolo_select_cands: nimg %d (>= 1)", nimg);
    FV_REQUIRE(ctx, capacity >= 1 && capacity <= FV_YOLO_SELECT_MAX_CAPACITY, "fv_yolo_select_cands: capacity %d unsupported (1..%d)",
               capacity, FV_YOLO_SELECT_MAX_CAPACITY);
    FV_REQUIRE(ctx, nclass >= 1 && nclass <= INT_MAX / FV_YOLO_SELECT_MAX_K, "fv_yolo_select_cands: nclass %d (>= 1)", nclass);
    FV_REQUIRE(ctx, num_cands >= 1 && num_cands <= FV_YOLO_SELECT_MAX_K, "fv_yolo_select_cands: num_cands %d unsupported (1..%d)",
               num_cands, FV_YOLO_SELECT_MAX_K);
    FV_REQUIRE(ctx, refuse_at >= 1, "fv_yolo_select_cands: refuse_at %d (>= 1)", refuse_at);
    FV_REQUIRE(ctx, boxes && objness && classes && count && out_boxes && out_src && out_obj && out_score && out_count,
               "fv_yolo_select_cands: NULL buffer");
    int P = 2;
    while (P < capacity) P <<= 1;
    const size_t lds = (size_t)P * 8;                                            // 64 KB at 8192 keys
    if (lds > 32 * 1024)
        FV_HIP(ctx, hipFuncSetAttribute((const void*)yolo_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FvProfScope ps(ctx, "yolo_select_kernel", 0.0,
                   (double)nimg * ((double)capacity * nclass * 4.0 + (double)num_cands * (28.0 + 8.0 * nclass)));
    hipLaunchKernelGGL(yolo_select_kernel, dim3(nimg), dim3(1024), lds, ctx->stream, boxes, reinterpret_cast<const unsigned*>(objness),
                       reinterpret_cast<const unsigned*>(classes), count, capacity, nclass, refuse_at, num_cands, out_boxes, out_src,
                       reinterpret_cast<unsigned*>(out_obj), reinterpret_cast<unsigned*>(out_score),
                       reinterpret_cast<unsigned*>(out_classes), out_count);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
