// Selection primitives shared by fid_mine.hip and fid_batch.hip: the exact distance D(i, r) between two rows of facial IDs and the
// two total orders every choice is an extremum of.  D is sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64
// differences (no FMA contraction: -ffp-contract=off) -- fid_match.hip's numerics.
#pragma once
#include "common.h"

// minimum of (distance, index); an empty best is (+inf, INT_MAX), which every row beats
__device__ __forceinline__ bool min_less(double d0, int i0, double d1, int i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }
// maximum distance, the lowest index among equals; an empty best is (-inf, INT_MAX)
__device__ __forceinline__ bool max_more(double d0, int i0, double d1, int i1) { return d0 > d1 || (d0 == d1 && i0 < i1); }

// a: the anchor in LDS (the same address in every lane: a broadcast), rp: one row of ids
__device__ __forceinline__ double dist_to(const float* a, const float4* rp) {
    double s = 0.0;
#pragma unroll 4
    for (int k4 = 0; k4 < 64 / 4; ++k4) {
        const float4 v = rp[k4];
        const float4 x = *reinterpret_cast<const float4*>(a + 4 * k4);
        double d;
        d = (double)x.x - (double)v.x; s += d * d;
        d = (double)x.y - (double)v.y; s += d * d;
        d = (double)x.z - (double)v.z; s += d * d;
        d = (double)x.w - (double)v.w; s += d * d;
    }
    return sqrt(s);
}

template <bool MAX>
__device__ __forceinline__ void wave_best(double& d, int& i) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (MAX ? max_more(od, oi, d, i) : min_less(od, oi, d, i)) { d = od; i = oi; }
    }
}

// class of a negative at distance dist for a positive at dap, hi = dap + margin (none of them NaN): exactly one holds
__device__ __forceinline__ int class_of(double dist, double dap, double hi) {
    if (dist > dap && dist < hi) return 0;
    return dist <= dap ? 1 : 2;
}
