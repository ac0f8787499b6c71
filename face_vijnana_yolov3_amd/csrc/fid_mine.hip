// Triplet negatives from the model's own facial IDs (semi-hard mining, FaceNet section 3.2): for every (anchor, positive) pair
// of a group table the row of ids that the chosen mode picks among the rows of other, known subjects.
//
// Exact by construction: D(i, r) is sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences (no FMA
// contraction: -ffp-contract=off) -- fid_match.hip's numerics, and the anchor-positive distance goes through the same function.
// Every choice is an extremum under a total order -- the minimum of (D, r), or the maximum of D with the lowest r among equals --
// so it does not depend on how rows are split over lanes, waves and workgroups, on the grouping or on the other triplets.  No
// atomics.
//
// One workgroup serves one anchor and up to PB of its positives (a longer group is cut by the launcher): the anchor is staged in
// LDS and read as broadcasts, thread t scans rows t, t + 256, ... (16 float4 loads per row), so each D(a, r) is computed once and
// then tested against the PB (dap, hi) pairs, which lie in LDS too.  Per positive a thread keeps three running (double, int) bests,
// one per class; then fv_wave_best and, over the four waves in LDS, fv_block_best (block_ops.h).  Work: chunks * n * 64 * 3 fp64
// vector ops for the distances plus about 12 compares per (row, positive).
#include "fid_select.h"
#include <climits>
#include <cmath>
#include <cstring>

namespace {

constexpr int MN_DIM = 64;
constexpr int MN_THREADS = 256;
constexpr int MN_WAVES = MN_THREADS / 64;
constexpr int MN_PB = FV_MINE_PB;

struct MineChunk {
    int anchor, first, count;   // triplets first .. first + count - 1 (count <= PB) share this anchor
};

// MODE 0 (semi-hard): NB = 3 bests per positive -- [0] band, minimum; [1] D <= dap, maximum; [2] D >= hi, minimum.
// MODE 1 (hardest): one best per thread, the minimum over the eligible rows, whatever the positive.
template <int PB, int MODE>
__global__ __launch_bounds__(MN_THREADS) void fid_mine_kernel(const float* __restrict__ ids, const int* __restrict__ subjects, int n,
                                                              const MineChunk* __restrict__ chunks, const int* __restrict__ positives,
                                                              double margin, int* __restrict__ neg_index, int* __restrict__ kind,
                                                              double* __restrict__ d_ap, double* __restrict__ d_an) {
    constexpr int NB = MODE == 0 ? 3 * PB : 1;
    __shared__ __attribute__((aligned(16))) float as[MN_DIM];
    __shared__ double sdap[PB], shi[PB];
    __shared__ double wd[MN_WAVES][NB];
    __shared__ int wi[MN_WAVES][NB];
    const int tid = threadIdx.x;
    const MineChunk c = chunks[blockIdx.x];
    const int sa = subjects[c.anchor];
    if (tid < MN_DIM) as[tid] = ids[(size_t)c.anchor * MN_DIM + tid];
    __syncthreads();
    if (tid < PB) {
        double dap = __builtin_nan("");               // a slot past the chunk: no comparison with it holds
        if (tid < c.count)
            dap = dist_to(as, reinterpret_cast<const float4*>(ids + (size_t)positives[c.first + tid] * MN_DIM));
        sdap[tid] = dap;
        shi[tid] = dap + margin;
    }
    __syncthreads();

    double bd[NB];
    int bi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { bd[b] = (MODE == 0 && b % 3 == 1) ? -__builtin_inf() : __builtin_inf(); bi[b] = INT_MAX; }
    for (int r = tid; r < n; r += MN_THREADS) {
        const int s = subjects[r];
        if (s < 0 || s == sa) continue;
        const double dist = dist_to(as, reinterpret_cast<const float4*>(ids + (size_t)r * MN_DIM));
        if (dist != dist) continue;                    // a NaN distance belongs to no class
        if (MODE == 1) {
            if (min_less()(dist, r, bd[0], bi[0])) { bd[0] = dist; bi[0] = r; }
            continue;
        }
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            if (j >= c.count) continue;                // uniform
            const double dap = sdap[j], hi = shi[j];
            if (dist > dap && dist < hi) {
                if (min_less()(dist, r, bd[3 * j], bi[3 * j])) { bd[3 * j] = dist; bi[3 * j] = r; }
            } else if (dist <= dap) {
                if (max_more()(dist, r, bd[3 * j + 1], bi[3 * j + 1])) { bd[3 * j + 1] = dist; bi[3 * j + 1] = r; }
            } else if (dist >= hi) {
                if (min_less()(dist, r, bd[3 * j + 2], bi[3 * j + 2])) { bd[3 * j + 2] = dist; bi[3 * j + 2] = r; }
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (MODE == 0 && b / 3 >= c.count) continue;   // uniform
        if (MODE == 0 && b % 3 == 1) fv_wave_best<max_more>(bd[b], bi[b]); else fv_wave_best<min_less>(bd[b], bi[b]);
        if (lane == 0) { wd[wave][b] = bd[b]; wi[wave][b] = bi[b]; }
    }
    __syncthreads();
    if (tid < c.count) {
        const double dap = sdap[tid], hi = shi[tid];
        double best_d[3];
        int best_i[3];
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double* sd = &wd[0][3 * tid + k];
                const int* si = &wi[0][3 * tid + k];
                if (k == 1) fv_block_best<max_more, MN_WAVES>(sd, si, NB, best_d[k], best_i[k]);
                else fv_block_best<min_less, MN_WAVES>(sd, si, NB, best_d[k], best_i[k]);
            }
        } else {
            fv_block_best<min_less, MN_WAVES>(&wd[0][0], &wi[0][0], NB, best_d[0], best_i[0]);
        }
        int kd = 3, ni = -1;
        double dn = __builtin_inf();
        if (dap == dap) {
            if (MODE == 0) {
                for (int k = 2; k >= 0; --k)
                    if (best_i[k] != INT_MAX) { kd = k; ni = best_i[k]; dn = best_d[k]; }
            } else if (best_i[0] != INT_MAX) {
                kd = class_of(best_d[0], dap, hi); ni = best_i[0]; dn = best_d[0];
            }
        }
        const int t = c.first + tid;
        neg_index[t] = ni;
        kind[t] = kd;
        d_ap[t] = dap == dap ? dap : __builtin_nan("");   // one NaN, whatever the operands' payloads were
        d_an[t] = dn;
    }
}

template <int PB, int MODE>
void launch_mine(fv_ctx* ctx, const float* ids, const int* subjects, int n, const MineChunk* chunks, int n_chunks,
                 const int* positives, double margin, int* neg_index, int* kind, double* d_ap, double* d_an) {
    FvProfScope ps(ctx, PB == 1 ? "fid_mine_kernel<1>" : "fid_mine_kernel", 3.0 * n_chunks * (double)n * MN_DIM,
                   (double)n_chunks * n * (MN_DIM * 4 + 4));
    hipLaunchKernelGGL((fid_mine_kernel<PB, MODE>), dim3((unsigned)n_chunks), dim3(MN_THREADS), 0, ctx->stream, ids, subjects, n,
                       chunks, positives, margin, neg_index, kind, d_ap, d_an);
}

}  // namespace

extern "C" int fv_fid_mine_negatives(fv_ctx* ctx, const float* ids, const int32_t* subjects, int n, const int32_t* anchors,
                                     const int32_t* pos_off, int g, const int32_t* positives, int t, double margin, int mode,
                                     int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, ids && subjects && pos_off, "fid_mine_negatives: bad arguments");
    FV_REQUIRE(ctx, n >= 1 && g >= 0 && t >= 0, "fid_mine_negatives: n %d < 1, g %d < 0 or t %d < 0", n, g, t);
    // nothing to write: the outputs (and an empty table's arrays) may be NULL
    FV_REQUIRE(ctx, (anchors || g == 0) && (t == 0 || (positives && neg_index && kind && d_ap && d_an)), "fid_mine_negatives: bad arguments");
    FV_REQUIRE(ctx, ((uintptr_t)ids & 15) == 0, "fid_mine_negatives: ids must be 16-byte aligned");
    FV_REQUIRE(ctx, mode == 0 || mode == 1, "fid_mine_negatives: mode %d (0 semi-hard, 1 hardest)", mode);
    FV_REQUIRE(ctx, std::isfinite(margin) && margin > 0.0, "fid_mine_negatives: margin %g is not finite and > 0", margin);
    // validate the whole table before anything is enqueued: a bad entry leaves the outputs untouched
    FV_REQUIRE(ctx, pos_off[0] == 0 && pos_off[g] == t, "fid_mine_negatives: pos_off runs from %d to %d, not from 0 to t = %d",
               pos_off[0], pos_off[g], t);
    int longest = 0;
    long long n_chunks = 0;
    for (int q = 0; q < g; ++q) {
        FV_REQUIRE(ctx, pos_off[q] <= pos_off[q + 1], "fid_mine_negatives: pos_off descends at group %d (%d, %d)", q, pos_off[q],
                   pos_off[q + 1]);
        FV_REQUIRE(ctx, anchors[q] >= 0 && anchors[q] < n, "fid_mine_negatives: anchor %d of group %d outside [0, %d)", anchors[q], q, n);
        const int len = pos_off[q + 1] - pos_off[q];
        longest = len > longest ? len : longest;
    }
    for (int j = 0; j < t; ++j)
        FV_REQUIRE(ctx, positives[j] >= 0 && positives[j] < n, "fid_mine_negatives: positive %d of triplet %d outside [0, %d)",
                   positives[j], j, n);
    if (t == 0) return FV_OK;

    // all groups singletons: the one-positive kernel; otherwise chunks of up to MN_PB positives
    const int pb = longest > 1 ? MN_PB : 1;
    std::vector<MineChunk> chunks;
    chunks.reserve((size_t)t / pb + g);
    for (int q = 0; q < g; ++q)
        for (int j = pos_off[q]; j < pos_off[q + 1]; j += pb) {
            const int left = pos_off[q + 1] - j;
            chunks.push_back(MineChunk{anchors[q], j, left < pb ? left : pb});
        }
    n_chunks = (long long)chunks.size();

    // one device copy of the chunk table and the positives (pageable source: consumed before the call returns)
    const size_t cb = sizeof(MineChunk) * chunks.size(), pbytes = sizeof(int32_t) * (size_t)t;
    std::vector<unsigned char> host(cb + pbytes);
    memcpy(host.data(), chunks.data(), cb);
    memcpy(host.data() + cb, positives, pbytes);
    void* dev = nullptr;
    FV_HIP(ctx, hipMallocAsync(&dev, host.size(), ctx->stream));
    const hipError_t ce = hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream);
    const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(ctx->stream) : ce;
    if (se != hipSuccess) {
        (void)hipFreeAsync(dev, ctx->stream);
        return fv_fail(ctx, FV_ERR_HIP, "fid_mine_negatives: table upload failed: %s", hipGetErrorString(se));
    }
    const MineChunk* dc = reinterpret_cast<const MineChunk*>(dev);
    const int* dp = reinterpret_cast<const int*>(reinterpret_cast<unsigned char*>(dev) + cb);
    if (pb == 1) {
        if (mode == 0) launch_mine<1, 0>(ctx, ids, subjects, n, dc, (int)n_chunks, dp, margin, neg_index, kind, d_ap, d_an);
        else launch_mine<1, 1>(ctx, ids, subjects, n, dc, (int)n_chunks, dp, margin, neg_index, kind, d_ap, d_an);
    } else {
        if (mode == 0) launch_mine<MN_PB, 0>(ctx, ids, subjects, n, dc, (int)n_chunks, dp, margin, neg_index, kind, d_ap, d_an);
        else launch_mine<MN_PB, 1>(ctx, ids, subjects, n, dc, (int)n_chunks, dp, margin, neg_index, kind, d_ap, d_an);
    }
    const hipError_t le = hipGetLastError();
    (void)hipFreeAsync(dev, ctx->stream);
    if (le != hipSuccess) return fv_fail(ctx, FV_ERR_HIP, "fid_mine_kernel launch failed: %s", hipGetErrorString(le));
    return FV_OK;
}
