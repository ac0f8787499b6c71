// Selection primitives shared by fid_mine.hip and fid_batch.hip: the exact distance D(i, r) between two rows of facial IDs and the
// class of a negative.  Every choice is an extremum under min_less / max_more of block_ops.h.  D is sqrt of the fp64 sum, in
// dimension order 0..63, of the squared fp64 differences (no FMA contraction: -ffp-contract=off) -- fid_match.hip's numerics.
#pragma once
#include "block_ops.h"

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

// class of a negative at distance dist for a positive at dap, hi = dap + margin (none of them NaN): exactly one holds
__device__ __forceinline__ int class_of(double dist, double dap, double hi) {
    if (dist > dap && dist < hi) return 0;
    return dist <= dap ? 1 : 2;
}
