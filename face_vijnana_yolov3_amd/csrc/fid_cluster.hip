// DBSCAN over facial IDs on gfx950 (contract in fid_cluster.h): which unlabelled faces are the same person.
//
// NP = n rounded up to 64, W = NP / 64.  The workspace holds the neighbour relation as a bit matrix in word-column-major order,
// adj[w * NP + i] = the neighbours of row i among rows 64 w .. 64 w + 63, so that the 64 rows of a wave store and load one
// contiguous 512 B run per word column.  Four passes, seven launches, all on the context's stream:
//   1. neighbours   fidc_neighbours_kernel: one anchor row per thread, held as 64 doubles in registers; 64 rows at a time staged
//                   in LDS as doubles and read as broadcasts (every lane the same address).  D(i, r) == D(r, i) bit for bit, so a
//                   wave computes only the 64 x 64 tiles on and above the diagonal and stores the mirrored tile from 64 ballots.
//                   No sqrt in the loop: sqrt is monotone and correctly rounded, so sqrt(s) <= eps <=> s <= T for the largest
//                   double T with sqrt(T) <= eps, which the host finds.  fidc_count_kernel: popcounts -> n_nbr, core, the core
//                   bitmask (one ballot per wave), and every row its own parent.  No atomics in this pass.
//   2. components   fidc_unite_kernel: a lock-free union-find over the core rows; row i unites with its core neighbours r < i.
//                   A root is only ever hooked under a smaller index (compare-and-swap on parent[larger root]), so parent[x] <= x
//                   always holds and the root of a component is its smallest row, whatever the order.  A failed compare-and-swap
//                   means another thread hooked that root: progress, never a wait on another workgroup.  Path halving through an
//                   integer atomic minimum (a parent only ever moves to a smaller ancestor).  fidc_flatten_kernel: root[i] and
//                   the bitmask of the roots.
//   3. borders      fidc_border_kernel: one workgroup per non-core row; distances recomputed (dist_to, with sqrt) for the set bits
//                   of (row AND core mask) only; the minimum of (D, r) under min_less.
//   4. relabel      fidc_scan_kernel: exclusive scan of the root words' popcounts (one workgroup) -> the number of every root and
//                   n_clusters; fidc_label_kernel: labels and via.
// Every word of the workspace that is read has been written by an earlier launch of the same call.
#include <cfloat>
#include <climits>
#include <cmath>
#include "fid_select.h"
#include "fid_cluster.h"

namespace {

constexpr int FC_DIM = 64;
constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / 64;
constexpr int FC_COL_TILES = 8;                       // column tiles (of 64 rows) one neighbours workgroup walks
constexpr int FC_MAX_W = FV_FID_CLUSTER_MAX_N / 64;
static_assert(FC_MAX_W == 4 * FC_THREADS, "fidc_scan_kernel: one workgroup, four words per thread");

typedef unsigned long long u64;

struct FcWorkspace {
    u64* adj;          // [W][NP]
    u64* core_mask;    // [W]
    u64* root_mask;    // [W]
    int* word_pref;    // [W] roots in the words before this one
    int* parent;       // [NP]
    int* root;         // [NP]
};

__host__ __device__ inline int fc_np(int n) { return (n + 63) & ~63; }

size_t fc_layout(int n, void* base, FcWorkspace* ws) {
    const size_t NP = fc_np(n), W = NP / 64;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 7) & ~(size_t)7; return (char*)base + o; };
    char* adj = take(W * NP * 8);
    char* cm = take(W * 8);
    char* rm = take(W * 8);
    char* wp = take(W * 4);
    char* pa = take(NP * 4);
    char* ro = take(NP * 4);
    if (ws) *ws = FcWorkspace{(u64*)adj, (u64*)cm, (u64*)rm, (int*)wp, (int*)pa, (int*)ro};
    return off;
}

// ---- 1. neighbours.  Workgroup (bx, by): row tiles 4 bx .. 4 bx + 3 (one per wave), column tiles 8 by .. 8 by + 7.
__global__ __launch_bounds__(FC_THREADS) void fidc_neighbours_kernel(const float* __restrict__ ids, int n, double T, u64* __restrict__ adj) {
    __shared__ __attribute__((aligned(16))) double xs[64][FC_DIM];
    const int NP = fc_np(n), W = NP >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J0 = blockIdx.y * FC_COL_TILES;
    if (J0 + FC_COL_TILES - 1 < (int)blockIdx.x * FC_WAVES) return;      // wholly below the diagonal: the mirrored stores cover it
    const int I = blockIdx.x * FC_WAVES + wave;                        // this wave's row tile
    const int i = I * 64 + lane;
    double a[FC_DIM];
    {
        const float4* ap = reinterpret_cast<const float4*>(ids + (size_t)(i < n ? i : 0) * FC_DIM);
#pragma unroll
        for (int k4 = 0; k4 < FC_DIM / 4; ++k4) {
            const float4 v = i < n ? ap[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
            a[4 * k4] = v.x; a[4 * k4 + 1] = v.y; a[4 * k4 + 2] = v.z; a[4 * k4 + 3] = v.w;
        }
    }
    for (int J = J0; J < J0 + FC_COL_TILES && J < W; ++J) {
        __syncthreads();                                               // the previous tile has been read
        for (int e = tid; e < 64 * FC_DIM / 4; e += FC_THREADS) {
            const int c = e / (FC_DIM / 4), k4 = e % (FC_DIM / 4);
            const int r = J * 64 + c;
            const float4 v = r < n ? reinterpret_cast<const float4*>(ids + (size_t)r * FC_DIM)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
            xs[c][4 * k4] = v.x; xs[c][4 * k4 + 1] = v.y; xs[c][4 * k4 + 2] = v.z; xs[c][4 * k4 + 3] = v.w;
        }
        __syncthreads();
        if (I >= W || J < I) continue;                                 // wave-uniform
        u64 word = 0;
        for (int c = 0; c < 64; c += 4) {                              // four rows at a time: four independent sums
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int k = 0; k < FC_DIM; k += 2) {
                const double2 x0 = *reinterpret_cast<const double2*>(&xs[c][k]);
                const double2 x1 = *reinterpret_cast<const double2*>(&xs[c + 1][k]);
                const double2 x2 = *reinterpret_cast<const double2*>(&xs[c + 2][k]);
                const double2 x3 = *reinterpret_cast<const double2*>(&xs[c + 3][k]);
                double d;
                d = a[k] - x0.x; s0 += d * d; d = a[k + 1] - x0.y; s0 += d * d;
                d = a[k] - x1.x; s1 += d * d; d = a[k + 1] - x1.y; s1 += d * d;
                d = a[k] - x2.x; s2 += d * d; d = a[k + 1] - x2.y; s2 += d * d;
                d = a[k] - x3.x; s3 += d * d; d = a[k + 1] - x3.y; s3 += d * d;
            }
            // a NaN sum compares false; rows past n are masked below
            word |= (u64)((s0 <= T ? 1u : 0u) | (s1 <= T ? 2u : 0u) | (s2 <= T ? 4u : 0u) | (s3 <= T ? 8u : 0u)) << c;
        }
        const int cols = n - J * 64;                                   // >= 1: J < W
        if (cols < 64) word &= (1ull << cols) - 1ull;
        if (i >= n) word = 0;
        adj[(size_t)J * NP + i] = word;
        if (J > I) {                                                   // the mirrored tile: lane b takes bit b of every lane's word
            u64 tw = 0;
            for (int b = 0; b < 64; ++b) {
                const u64 m = __ballot((word >> b) & 1ull);
                if (lane == b) tw = m;
            }
            adj[(size_t)I * NP + J * 64 + lane] = tw;
        }
    }
}

// n_nbr, core, the core bitmask, parent = self.  One thread per row of NP; the loads of a wave are contiguous per word column.
__global__ __launch_bounds__(FC_THREADS) void fidc_count_kernel(const u64* __restrict__ adj, int n, int min_pts, int* __restrict__ n_nbr,
                                                                uint8_t* __restrict__ core, u64* __restrict__ core_mask,
                                                                int* __restrict__ parent) {
    const int NP = fc_np(n), W = NP >> 6;
    const int i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i >= NP) return;                                               // NP is a multiple of 64: whole waves
    int cnt = 0;
    for (int w = 0; w < W; ++w) cnt += __popcll(adj[(size_t)w * NP + i]);
    const bool is_core = i < n && cnt >= min_pts;
    const u64 m = __ballot(is_core);
    if ((threadIdx.x & 63) == 0) core_mask[i >> 6] = m;
    parent[i] = i;
    if (i < n) { n_nbr[i] = cnt; core[i] = is_core ? 1 : 0; }
}

// ---- 2. components
__device__ __forceinline__ int fc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as it stands; every step moves x to a smaller index, so the walk ends
__device__ __forceinline__ int fc_find(int* parent, int x) {
    int p = fc_ld(parent + x);
    while (p != x) {
        const int gp = fc_ld(parent + p);
        if (gp < p) atomicMin(parent + x, gp);                         // path halving: gp is an ancestor of x and smaller than p
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void fc_unite(int* parent, int a, int b) {
    for (;;) {
        a = fc_find(parent, a);
        b = fc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                                       // someone else hooked hi (under old < hi): go on from there
        b = lo;
    }
}

__global__ __launch_bounds__(FC_THREADS) void fidc_unite_kernel(const u64* __restrict__ adj, const u64* __restrict__ core_mask, int n,
                                                                int* parent) {
    const int NP = fc_np(n);
    const int i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i >= n || !((core_mask[i >> 6] >> (i & 63)) & 1ull)) return;
    for (int w = 0; w <= (i >> 6); ++w) {
        u64 bits = adj[(size_t)w * NP + i] & core_mask[w];
        if (w == (i >> 6)) bits &= (1ull << (i & 63)) - 1ull;           // r < i: the pair (r, i) is r's neighbour i > r seen from i
        while (bits) {
            const int r = w * 64 + __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            if (fc_ld(parent + r) != fc_ld(parent + i)) fc_unite(parent, i, r);
        }
    }
}

__global__ __launch_bounds__(FC_THREADS) void fidc_flatten_kernel(const u64* __restrict__ core_mask, int n, const int* __restrict__ parent,
                                                                  int* __restrict__ root, u64* __restrict__ root_mask) {
    const int NP = fc_np(n);
    const int i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i >= NP) return;
    int r = -1;
    if (i < n && ((core_mask[i >> 6] >> (i & 63)) & 1ull)) {
        r = i;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;
    }
    root[i] = r;
    const u64 m = __ballot(r == i);
    if ((threadIdx.x & 63) == 0) root_mask[i >> 6] = m;
}

// ---- 3. borders: workgroup i serves row i; via[i] = the nearest core neighbour of a non-core row, -1 when it has none
__global__ __launch_bounds__(FC_THREADS) void fidc_border_kernel(const float* __restrict__ ids, const u64* __restrict__ adj,
                                                                 const u64* __restrict__ core_mask, int n, int* __restrict__ via) {
    __shared__ __attribute__((aligned(16))) float as[FC_DIM];
    __shared__ double wd[FC_WAVES];
    __shared__ int wi[FC_WAVES];
    const int NP = fc_np(n), W = NP >> 6;
    const int i = blockIdx.x, tid = threadIdx.x;
    if ((core_mask[i >> 6] >> (i & 63)) & 1ull) return;                // a core row (the same answer in the whole workgroup)
    if (tid < FC_DIM) as[tid] = ids[(size_t)i * FC_DIM + tid];
    __syncthreads();
    double bd = __builtin_inf();
    int bi = INT_MAX;
    for (int w = tid; w < W; w += FC_THREADS) {
        u64 bits = adj[(size_t)w * NP + i] & core_mask[w];
        while (bits) {
            const int r = w * 64 + __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            const double d = dist_to(as, reinterpret_cast<const float4*>(ids + (size_t)r * FC_DIM));
            if (min_less()(d, r, bd, bi)) { bd = d; bi = r; }
        }
    }
    fv_wave_best<min_less>(bd, bi);
    if ((tid & 63) == 0) { wd[tid >> 6] = bd; wi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        fv_block_best<min_less, FC_WAVES>(wd, wi, 1, bd, bi);
        via[i] = bi == INT_MAX ? -1 : bi;
    }
}

// ---- 4. relabel.  One workgroup: word_pref[w] = the roots in the words before w; n_clusters = all of them.
__global__ __launch_bounds__(FC_THREADS) void fidc_scan_kernel(const u64* __restrict__ root_mask, int W, int* __restrict__ word_pref,
                                                               int* __restrict__ n_clusters) {
    __shared__ int s_wave[FC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int w = 4 * tid + j;
        c[j] = w < W ? __popcll(root_mask[w]) : 0;
        sum += c[j];
    }
    const int incl = fv_wave_incl_scan(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int off = incl - sum;
    for (int v = 0; v < wave; ++v) off += s_wave[v];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int w = 4 * tid + j;
        if (w < W) word_pref[w] = off;
        off += c[j];
    }
    if (tid == FC_THREADS - 1) n_clusters[0] = off;
}

__global__ __launch_bounds__(FC_THREADS) void fidc_label_kernel(const int* __restrict__ root, const u64* __restrict__ root_mask,
                                                                const int* __restrict__ word_pref, int n, int* __restrict__ labels,
                                                                int* via) {
    const int i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i >= n) return;
    int r = root[i];
    if (r >= 0) {
        via[i] = i;
    } else {
        const int v = via[i];                                          // fidc_border_kernel's
        if (v < 0) { labels[i] = -1; return; }
        r = root[v];
    }
    labels[i] = word_pref[r >> 6] + __popcll(root_mask[r >> 6] & ((1ull << (r & 63)) - 1ull));
}

// the largest double T with sqrt(T) <= eps (eps finite, >= 0): sqrt is monotone and correctly rounded, so s <= T <=> sqrt(s) <= eps
double fc_sq_threshold(double eps) {
    double t = eps * eps;
    if (!(t <= DBL_MAX)) t = DBL_MAX;
    while (std::sqrt(t) > eps) t = std::nextafter(t, 0.0);
    while (t < DBL_MAX && std::sqrt(std::nextafter(t, (double)INFINITY)) <= eps) t = std::nextafter(t, (double)INFINITY);
    return t;
}

}  // namespace

extern "C" size_t fv_fid_cluster_workspace_bytes(int n) {
    if (n < 1 || n > FV_FID_CLUSTER_MAX_N) return 0;
    return fc_layout(n, nullptr, nullptr);
}

extern "C" int fv_fid_cluster(fv_ctx* ctx, const float* ids, int n, double eps, int min_pts, void* workspace, int32_t* labels,
                              int32_t* via, int32_t* n_nbr, uint8_t* core, int32_t* n_clusters) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, ids && workspace && labels && via && n_nbr && core && n_clusters, "fid_cluster: NULL pointer");
    FV_REQUIRE(ctx, n >= 1 && n <= FV_FID_CLUSTER_MAX_N, "fid_cluster: n = %d is outside 1..%d", n, FV_FID_CLUSTER_MAX_N);
    FV_REQUIRE(ctx, std::isfinite(eps) && eps >= 0.0, "fid_cluster: eps must be finite and >= 0");
    FV_REQUIRE(ctx, min_pts >= 1, "fid_cluster: min_pts must be >= 1");
    FV_REQUIRE(ctx, ((uintptr_t)ids & 15) == 0, "fid_cluster: ids must be 16-byte aligned");
    FV_REQUIRE(ctx, ((uintptr_t)workspace & 7) == 0, "fid_cluster: workspace must be 8-byte aligned");
    FcWorkspace ws;
    fc_layout(n, workspace, &ws);
    const int NP = fc_np(n), W = NP / 64;
    const double T = fc_sq_threshold(eps);
    const dim3 rows((NP + FC_THREADS - 1) / FC_THREADS), block(FC_THREADS);
    const double adj_bytes = (double)W * NP * 8;
    {
        FvProfScope ps(ctx, "fidc_neighbours_kernel", 1.5 * n * (double)n * FC_DIM, (double)n * FC_DIM * 4 + adj_bytes);
        hipLaunchKernelGGL(fidc_neighbours_kernel, dim3(rows.x, (W + FC_COL_TILES - 1) / FC_COL_TILES), block, 0, ctx->stream, ids, n, T,
                           ws.adj);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_count_kernel", 0.0, adj_bytes);
        hipLaunchKernelGGL(fidc_count_kernel, rows, block, 0, ctx->stream, ws.adj, n, min_pts, n_nbr, core, ws.core_mask, ws.parent);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_unite_kernel", 0.0, adj_bytes / 2);
        hipLaunchKernelGGL(fidc_unite_kernel, rows, block, 0, ctx->stream, ws.adj, ws.core_mask, n, ws.parent);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_flatten_kernel", 0.0, 8.0 * NP);
        hipLaunchKernelGGL(fidc_flatten_kernel, rows, block, 0, ctx->stream, ws.core_mask, n, ws.parent, ws.root, ws.root_mask);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_border_kernel", 0.0, 0.0);
        hipLaunchKernelGGL(fidc_border_kernel, dim3(n), block, 0, ctx->stream, ids, ws.adj, ws.core_mask, n, via);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_scan_kernel", 0.0, 12.0 * W);
        hipLaunchKernelGGL(fidc_scan_kernel, dim3(1), block, 0, ctx->stream, ws.root_mask, W, ws.word_pref, n_clusters);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "fidc_label_kernel", 0.0, 16.0 * n);
        hipLaunchKernelGGL(fidc_label_kernel, rows, block, 0, ctx->stream, ws.root, ws.root_mask, ws.word_pref, n, labels, via);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}
