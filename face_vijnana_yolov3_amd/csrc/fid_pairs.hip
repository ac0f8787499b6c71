// Face-verification pair distances (reference evaluate.py:129-223, cal_face_pairs_dists / cal_VAL_FAR): the Euclidean distance of
// every facial-ID pair of a block table -- i < j triangles (same-identity pairs of one subject) and na x nb rectangles
// (different-identity pairs of two subjects) -- written in the reference's append order, and per kind the number of pairs at or
// below each threshold.
//
// Exact by construction: each distance is sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences (no FMA
// contraction: -ffp-contract=off), rounded to float32 -- fid_match.hip's numerics.  A pair's bits do not depend on its tile, its
// block's position in the table or the launch split.  The counts are integer sums (LDS histogram per workgroup, one integer
// global atomic per non-empty bin per workgroup, then a cumulative pass), so they are deterministic too.  No float atomics.
//
// Work: 3 * 64 fp64 vector ops per pair (2.2e11 at VGGFace2 size, ~1.1e9 pairs) on 64 x 64 pair tiles.  A workgroup stages the
// tile's A and B rows in LDS transposed ([k][row], row stride 68 floats) and each thread register-blocks 4 x 4 pairs: per
// dimension two ds_read_b128 (A broadcast, B contiguous) feed 8 conversions and 48 fp64 ops.  Tiles of every block are numbered
// by a per-block prefix (built on the host); a fixed grid walks them grid-stride, each tile found by a binary search of the
// prefix.  Every tile costs the same (masked pairs are computed and dropped), so the walk is even whatever the block sizes.
#include "common.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int FP_DIM = 64;
constexpr int FP_TILE = 64;
constexpr int FP_THREADS = 256;
constexpr int FP_STRIDE = FP_TILE + 4;              // LDS row stride of the transposed tiles (floats; keeps b128 reads aligned)
constexpr int FP_MAX_TH = 4096;
constexpr long long FP_MAX_TILES_PER_WG = 1 << 18;  // 2^18 tiles * 4096 pairs < 2^32: the LDS histogram stays in uint32
constexpr int FP_GRID = 4096;

struct PairArgs {
    const float* ids;
    const fv_pair_block* blocks;
    const long long* prefix;     // [n_blocks + 1] tiles before each block
    const float* th;             // [n_th] ascending
    int n_blocks, n_th;
    long long n_tiles;
    float* dists;                // NULL: counts only
    unsigned long long* counts;  // [2][n_th]: histogram (bin = first threshold >= d), made cumulative by pair_counts_finish
};

__host__ __device__ inline long long tri_tiles(long long n) {
    const long long t = (n + FP_TILE - 1) / FP_TILE;
    return n >= 2 ? t * (t + 1) / 2 : 0;
}

__host__ __device__ inline long long block_tiles(const fv_pair_block& b) {
    if (b.kind == 0) return tri_tiles(b.na);
    return b.na >= 1 && b.nb >= 1 ? ((b.na + FP_TILE - 1) / FP_TILE) * ((b.nb + FP_TILE - 1) / FP_TILE) : 0;
}

__device__ inline void locate(const PairArgs& p, long long t, int& blk, long long& ti, long long& tj) {
    int lo = 0, hi = p.n_blocks;                    // last block whose prefix <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.prefix[mid] <= t) lo = mid; else hi = mid;
    }
    blk = lo;
    long long u = t - p.prefix[lo];
    const fv_pair_block& b = p.blocks[lo];
    if (b.kind == 1) {
        const long long tb = (b.nb + FP_TILE - 1) / FP_TILE;
        ti = u / tb; tj = u % tb;
        return;
    }
    // upper triangle of T x T tiles, row ti holding T - ti of them: closed-form estimate, then exact integer fix-up
    const long long T = (b.na + FP_TILE - 1) / FP_TILE;
    const double c = 2.0 * (double)T + 1.0;
    long long r = (long long)((c - sqrt(c * c - 8.0 * (double)u)) * 0.5);
    if (r < 0) r = 0;
    if (r > T - 1) r = T - 1;
    auto before = [T](long long row) { return row * T - row * (row - 1) / 2; };
    while (r > 0 && before(r) > u) --r;
    while (r + 1 < T && before(r + 1) <= u) ++r;
    ti = r; tj = r + (u - before(r));
}

__device__ inline void stage(float (*s)[FP_STRIDE], const float* ids, long long row0, long long rows, int tid) {
    // 64 rows x 16 float4, four per thread; rows past the block are zeros (never read from memory)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + q * FP_THREADS;
        const int row = e >> 4, k4 = e & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < rows) v = *reinterpret_cast<const float4*>(ids + (row0 + row) * FP_DIM + 4 * k4);
        s[4 * k4 + 0][row] = v.x; s[4 * k4 + 1][row] = v.y; s[4 * k4 + 2][row] = v.z; s[4 * k4 + 3][row] = v.w;
    }
}

__global__ __launch_bounds__(FP_THREADS) void pair_dists_kernel(PairArgs p) {
    __shared__ __attribute__((aligned(16))) float As[FP_DIM][FP_STRIDE];
    __shared__ __attribute__((aligned(16))) float Bs[FP_DIM][FP_STRIDE];
    extern __shared__ unsigned int dyn[];            // th[n_th] (as floats), hist[2][n_th]
    float* th = reinterpret_cast<float*>(dyn);
    unsigned int* hist = dyn + p.n_th;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    for (int i = tid; i < p.n_th; i += FP_THREADS) { th[i] = p.th[i]; hist[i] = 0u; hist[p.n_th + i] = 0u; }

    for (long long t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        int bi;
        long long ti, tj;
        locate(p, t, bi, ti, tj);
        const fv_pair_block b = p.blocks[bi];
        const long long i0 = ti * FP_TILE, j0 = tj * FP_TILE;
        const long long nb = b.kind == 0 ? b.na : b.nb;
        __syncthreads();                              // previous tile's LDS reads (and the threshold fill) are done
        stage(As, p.ids, b.a0 + i0, b.na - i0, tid);
        stage(Bs, p.ids, b.b0 + j0, nb - j0, tid);
        __syncthreads();

        double s[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) s[r][c] = 0.0;
#pragma unroll 4
        for (int k = 0; k < FP_DIM; ++k) {
            const float4 av = *reinterpret_cast<const float4*>(&As[k][4 * ty]);
            const float4 bv = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
            const double a[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
            const double bb[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = a[r] - bb[c];
                    s[r][c] += d * d;
                }
        }

        unsigned int* h = hist + b.kind * p.n_th;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = i0 + 4 * ty + r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long j = j0 + 4 * tx + c;
                const bool ok = b.kind == 0 ? (j < b.na && j > i) : (i < b.na && j < b.nb);
                if (!ok) continue;
                const float dist = (float)sqrt(s[r][c]);
                if (p.dists) {
                    const long long rank = b.kind == 0 ? i * b.na - i * (i + 1) / 2 + (j - i - 1) : i * b.nb + j;
                    p.dists[b.out_off + rank] = dist;
                }
                int lo = 0, hi = p.n_th;              // first threshold >= dist; NaN finds none
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (th[mid] >= dist) hi = mid; else lo = mid + 1;
                }
                if (lo < p.n_th) atomicAdd(&h[lo], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * p.n_th; i += FP_THREADS)
        if (hist[i]) atomicAdd(&p.counts[i], (unsigned long long)hist[i]);
}

// counts[kind][t] = sum of histogram bins 0..t, one workgroup per kind: 16 consecutive bins per thread, then a workgroup scan
__global__ __launch_bounds__(FP_THREADS) void pair_counts_finish(unsigned long long* counts, int n_th) {
    __shared__ unsigned long long part[FP_THREADS];
    unsigned long long* c = counts + (size_t)blockIdx.x * n_th;
    const int tid = threadIdx.x;
    constexpr int PER = FP_MAX_TH / FP_THREADS;
    unsigned long long v[PER], run = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid * PER + q;
        run += i < n_th ? c[i] : 0ull;
        v[q] = run;
    }
    part[tid] = run;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < tid; ++w) base += part[w];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid * PER + q;
        if (i < n_th) c[i] = base + v[q];
    }
}

}  // namespace

extern "C" int fv_fid_pair_dists(fv_ctx* ctx, const float* ids, int64_t n_ids, const fv_pair_block* blocks, int n_blocks,
                                 const float* thresholds, int n_th, float* dists, int64_t n_dists, int64_t* counts) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, ids && blocks && thresholds && counts && n_blocks >= 1, "fid_pair_dists: bad arguments");
    FV_REQUIRE(ctx, n_ids >= 1 && n_ids < (1ll << 31), "fid_pair_dists: n_ids %lld outside [1, 2^31)", (long long)n_ids);
    FV_REQUIRE(ctx, ((uintptr_t)ids & 15) == 0, "fid_pair_dists: ids must be 16-byte aligned");
    FV_REQUIRE(ctx, n_th >= 1 && n_th <= FP_MAX_TH, "fid_pair_dists: n_th %d outside [1, %d]", n_th, FP_MAX_TH);
    for (int t = 1; t < n_th; ++t)
        FV_REQUIRE(ctx, thresholds[t - 1] <= thresholds[t], "fid_pair_dists: thresholds not ascending at %d (%g, %g)", t,
                   (double)thresholds[t - 1], (double)thresholds[t]);
    FV_REQUIRE(ctx, !(thresholds[0] != thresholds[0]), "fid_pair_dists: threshold 0 is NaN");
    FV_REQUIRE(ctx, !dists || n_dists >= 0, "fid_pair_dists: n_dists %lld < 0", (long long)n_dists);
    // validate the whole table before anything is enqueued: a bad record leaves dists and counts untouched
    std::vector<long long> prefix(n_blocks + 1);
    prefix[0] = 0;
    for (int k = 0; k < n_blocks; ++k) {
        const fv_pair_block& b = blocks[k];
        FV_REQUIRE(ctx, b.kind == 0 || b.kind == 1, "fid_pair_dists: block %d has kind %d (0 triangle, 1 rectangle)", k, b.kind);
        FV_REQUIRE(ctx, b.a0 >= 0 && b.na >= 0 && b.na <= n_ids - b.a0, "fid_pair_dists: block %d rows a [%lld, +%lld) outside %lld ids",
                   k, (long long)b.a0, (long long)b.na, (long long)n_ids);
        FV_REQUIRE(ctx, b.b0 >= 0 && b.nb >= 0 && b.nb <= n_ids - b.b0, "fid_pair_dists: block %d rows b [%lld, +%lld) outside %lld ids",
                   k, (long long)b.b0, (long long)b.nb, (long long)n_ids);
        FV_REQUIRE(ctx, b.kind == 1 || (b.b0 == b.a0 && b.nb == b.na), "fid_pair_dists: triangle block %d needs b0 == a0 and nb == na", k);
        FV_REQUIRE(ctx, b.out_off >= 0, "fid_pair_dists: block %d out_off %lld < 0", k, (long long)b.out_off);
        const long long pairs = b.kind == 0 ? b.na * (b.na - 1) / 2 : b.na * b.nb;
        FV_REQUIRE(ctx, !dists || pairs <= n_dists - b.out_off, "fid_pair_dists: block %d writes [%lld, %lld) past n_dists %lld", k,
                   (long long)b.out_off, (long long)b.out_off + pairs, (long long)n_dists);
        prefix[k + 1] = prefix[k] + block_tiles(b);
    }
    const long long n_tiles = prefix[n_blocks];

    FV_HIP(ctx, hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * n_th, ctx->stream));
    if (n_tiles > 0) {
        // one device copy of the table, its tile prefix and the thresholds (pageable source: consumed before the call returns)
        const size_t bb = sizeof(fv_pair_block) * n_blocks, pb = sizeof(long long) * (n_blocks + 1), tb = sizeof(float) * n_th;
        std::vector<unsigned char> host(bb + pb + tb);
        memcpy(host.data(), blocks, bb);
        memcpy(host.data() + bb, prefix.data(), pb);
        memcpy(host.data() + bb + pb, thresholds, tb);
        void* dev = nullptr;
        FV_HIP(ctx, hipMallocAsync(&dev, host.size(), ctx->stream));
        const hipError_t ce = hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream);
        const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(ctx->stream) : ce;
        if (se != hipSuccess) {
            (void)hipFreeAsync(dev, ctx->stream);
            return fv_fail(ctx, FV_ERR_HIP, "fid_pair_dists: table upload failed: %s", hipGetErrorString(se));
        }
        PairArgs a;
        a.ids = ids;
        a.blocks = reinterpret_cast<const fv_pair_block*>(dev);
        a.prefix = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(dev) + bb);
        a.th = reinterpret_cast<const float*>(reinterpret_cast<unsigned char*>(dev) + bb + pb);
        a.n_blocks = n_blocks;
        a.n_th = n_th;
        a.n_tiles = n_tiles;
        a.dists = dists;
        a.counts = reinterpret_cast<unsigned long long*>(counts);
        long long grid = n_tiles < FP_GRID ? n_tiles : FP_GRID;
        if ((n_tiles + grid - 1) / grid > FP_MAX_TILES_PER_WG) grid = (n_tiles + FP_MAX_TILES_PER_WG - 1) / FP_MAX_TILES_PER_WG;
        const double pairs_est = (double)n_tiles * FP_TILE * FP_TILE;
        // up to 48 KiB of thresholds and histogram next to the 34 KiB of tiles: past the default 64 KiB limit of one workgroup
        const size_t dyn = sizeof(float) * 3 * n_th;
        const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(pair_dists_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        if (ae != hipSuccess) {
            (void)hipFreeAsync(dev, ctx->stream);
            return fv_fail(ctx, FV_ERR_HIP, "fid_pair_dists: hipFuncSetAttribute failed: %s", hipGetErrorString(ae));
        }
        {
            FvProfScope ps(ctx, "pair_dists_kernel", 3.0 * FP_DIM * pairs_est,
                           (double)n_tiles * 2 * FP_TILE * FP_DIM * 4 + (dists ? 4.0 * pairs_est : 0.0));
            hipLaunchKernelGGL(pair_dists_kernel, dim3((unsigned)grid), dim3(FP_THREADS), dyn, ctx->stream, a);
        }
        const hipError_t le = hipGetLastError();
        (void)hipFreeAsync(dev, ctx->stream);
        if (le != hipSuccess) return fv_fail(ctx, FV_ERR_HIP, "pair_dists_kernel launch failed: %s", hipGetErrorString(le));
    }
    hipLaunchKernelGGL(pair_counts_finish, dim3(2), dim3(FP_THREADS), 0, ctx->stream, reinterpret_cast<unsigned long long*>(counts),
                       n_th);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}
