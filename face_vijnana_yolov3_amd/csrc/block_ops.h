// Wave (64 lanes) and workgroup steps shared by the kernels off the matrix path.  DESIGN.md section 32 states for each the property
// its callers rely on: the addition tree, the tie rule, which lane holds the result.
#pragma once
#include "common.h"

// ---- wave sums and maxima: xor butterfly, o = 32, 16, 8, 4, 2, 1 with v = v + partner.  Lane 0 holds ((v0 + v32) + (v16 + v48)) + ...
// Every lane adds the same pairs, so an integer total is in every lane; a floating-point caller that needs one value in all lanes
// takes fv_wave_sum_all, which broadcasts lane 0's.
template <typename T>
__device__ __forceinline__ T fv_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double fv_wave_sum_all(double v) { return __shfl(fv_wave_sum(v), 0); }
__device__ __forceinline__ double fv_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// ---- extrema of (value, index).  The three orders every choice is an extremum of, as function objects: Order()(d0, i0, d1, i1) <=>
// (d0, i0) comes before (d1, i1); the lowest index wins among equals.  Total on the values their callers feed them, so an extremum
// does not depend on the reduction tree.
// minimum of (value, index); an empty best is (+inf, INT_MAX), which every row beats.  No NaN operands.
struct min_less {
    __device__ __forceinline__ bool operator()(double d0, int i0, double d1, int i1) const { return d0 < d1 || (d0 == d1 && i0 < i1); }
};
// maximum value, the lowest index among equals; an empty best is (-inf, INT_MAX).  No NaN operands.
struct max_more {
    __device__ __forceinline__ bool operator()(double d0, int i0, double d1, int i1) const { return d0 > d1 || (d0 == d1 && i0 < i1); }
};
// the order np.argmin uses: NaN before every number (the first NaN wins), otherwise by value, then by index
struct lex_less {
    __device__ __forceinline__ bool operator()(double d0, int i0, double d1, int i1) const {
        const bool n0 = d0 != d0, n1 = d1 != d1;
        if (n0 != n1) return n0;
        if (n0) return i0 < i1;
        return d0 < d1 || (d0 == d1 && i0 < i1);
    }
};
// the wave's best under Order, in every lane
template <typename Order>
__device__ __forceinline__ void fv_wave_best(double& d, int& i) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (Order()(od, oi, d, i)) { d = od; i = oi; }
    }
}
// the best of the NWAVES per-wave bests wd[w * stride], wi[w * stride] that lane 0 of each wave stored; the caller places the barrier
template <typename Order, int NWAVES>
__device__ __forceinline__ void fv_block_best(const double* wd, const int* wi, int stride, double& d, int& i) {
    d = wd[0];
    i = wi[0];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) {
        const double od = wd[w * stride];
        const int oi = wi[w * stride];
        if (Order()(od, oi, d, i)) { d = od; i = oi; }
    }
}

// ---- rank keys: 64-bit key of a positive float score and an index; descending key order = descending score, ties toward the lower index
__device__ __forceinline__ unsigned long long fv_rank_key(float score, unsigned index) {
    return ((unsigned long long)__float_as_uint(score) << 32) | (0xFFFFFFFFu - index);
}
__device__ __forceinline__ unsigned fv_rank_index(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull); }
__device__ __forceinline__ float fv_rank_score(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// LDS bitonic sort of keys[0 .. P), P a power of two >= 2, by a workgroup of THREADS; ends with a barrier.  Equal keys (the padding
// value) may land in any order.
template <int THREADS, bool DESC>
__device__ __forceinline__ void fv_bitonic_sort(unsigned long long* keys, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i + j;
                const unsigned long long a = keys[i], b = keys[l];
                const bool up = ((i & k) == 0) != DESC;  // ascending run?
                if (up ? (a > b) : (a < b)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
}

// ---- integer boxes: the length of [x1, x2] n [x3, x4] as the reference's _interval_overlap computes it
__device__ __forceinline__ int fv_interval_overlap_i32(int x1, int x2, int x3, int x4) {
    if (x3 < x1) {
        if (x4 < x1) return 0;
        return min(x2, x4) - x1;
    } else {
        if (x2 < x3) return 0;
        return min(x2, x4) - x3;
    }
}
// intersection and union areas of two (x0, y0, x1, y1) boxes; what a zero union means is the caller's policy
__device__ __forceinline__ void fv_box_inter_union(const int4& a, const int4& b, long long& inter, long long& uni) {
    const long long iw = fv_interval_overlap_i32(a.x, a.z, b.x, b.z);
    const long long ih = fv_interval_overlap_i32(a.y, a.w, b.y, b.w);
    inter = iw * ih;
    uni = (long long)(a.z - a.x) * (a.w - a.y) + (long long)(b.z - b.x) * (b.w - b.y) - inter;
}

// ---- scans and ordered compaction
__device__ __forceinline__ int fv_wave_incl_scan(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// This thread's place among the workgroup's set flags in thread order.  s_cnt: one int of LDS per wave, left holding the waves'
// counts (their sum is the workgroup's total); one barrier inside, and the caller places one before s_cnt is used again.
__device__ __forceinline__ int fv_block_compact(bool flag, int* s_cnt, int lane, int wave) {
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += s_cnt[w];
    return off + __popcll(mask & ((1ull << lane) - 1ull));
}

// ---- fixed-order LDS tree sums: s[0] = the sum of s[0 .. N) by halving, s[t] += s[t + st] for st = N/2 .. 1.  The caller has stored
// s and placed a barrier; ends with a barrier.
template <int N>
__device__ __forceinline__ void fv_block_tree_sum(double* s, int tid) {
    for (int st = N / 2; st > 0; st >>= 1) {
        if (tid < st) s[tid] += s[tid + st];
        __syncthreads();
    }
}
// the same down the 128 rows of two [128][9] arrays at once (thread = row rl, column cl of 8): a[0][cl], b[0][cl] hold the sums
__device__ __forceinline__ void fv_block_tree_sum2(double (*a)[9], double (*b)[9], int rl, int cl) {
    for (int st = 64; st > 0; st >>= 1) {
        if (rl < st) { a[rl][cl] += a[rl + st][cl]; b[rl][cl] += b[rl + st][cl]; }
        __syncthreads();
    }
}
