// The input of a FaceIdentifier training step from a device-resident store of uint8 face crops (crop_store.py): slot idx[j] of
// the store becomes row j of a float32 batch, every byte divided by 255 -- what the reference's TrainingSequence does on the host
// per file (fi.py:1577, `img.astype(np.float32) / 255.0`).  A pure streaming conversion, 1 byte read and 4 written per element.
//
// The index list travels in the kernel arguments, CG_MAX indices per launch (as the crop tables travel, preproc.hip): no device
// allocation, no host-to-device copy of a pageable table and nothing that has to outlive the call.  blockIdx.y is the row of the
// chunk, so the slot index is wave-uniform and read with scalar loads.  Every byte offset is 64-bit: a store of 416 x 416 crops
// passes 4 GiB at slot 8 273.
//
// Four fifths of the traffic are the float stores, so the shape is chosen for them: a lane loads ONE dword (the wave 256
// contiguous bytes) and stores its four floats as one float4, which makes every store instruction of a wave 1 KiB of contiguous
// memory; CG_WORDS such dwords per lane, all loaded before the first store.  The shape that loads 16 bytes per lane and stores
// four float4 at a 64-byte lane stride ran at 3.6 / 3.9 TB/s (n = 39 / 120 crops of 416 x 416) where this one runs at 6.7 / 6.1
// and a device copy of the same bytes at 7.9 / 5.5.
#include "common.h"

namespace {

constexpr int CG_MAX = FV_GATHER_CHUNK;    // indices per launch: 512 bytes of kernel arguments
constexpr int CG_THREADS = 256;
constexpr int CG_WORDS = 8;                // dwords per lane: a workgroup converts 8 KiB of a slot

struct GatherTable {
    int slot[CG_MAX];
};

// (float)b / 255.0f, correctly rounded, for b = 0 .. 255 without a divide instruction: q0 = b * r with r = fl(1 / 255), the exact
// residual b - 255 * q0 by one fma, and one fma to add its quotient (the Newton step every IEEE divide ends in).  Checked against
// the exactly rounded quotient for all 256 values (tests/test_crop_store_gpu.py runs every byte value through the kernel).  The
// pragmas pin the three operations whatever -ffast-math / -ffp-contract the file is built with.
__device__ __forceinline__ float byte_over_255(unsigned b) {
#pragma clang fp reassociate(off) contract(off)
    const float x = (float)b, r = 0x1.010102p-8f;
    const float q0 = x * r;
    const float e = __builtin_fmaf(-255.0f, q0, x);
    return __builtin_fmaf(e, r, q0);
}

__device__ __forceinline__ float4 word_over_255(unsigned w) {
    return make_float4(byte_over_255(w & 255u), byte_over_255((w >> 8) & 255u), byte_over_255((w >> 16) & 255u),
                       byte_over_255(w >> 24));
}

// grid (ceil(words / (CG_THREADS * CG_WORDS)), rows of the chunk); words = elems / 4
__global__ __launch_bounds__(CG_THREADS) void crop_gather_kernel(const unsigned char* __restrict__ store, GatherTable t, long long words,
                                                                 float* __restrict__ dst) {
    const long long w0 = (long long)blockIdx.x * (CG_THREADS * CG_WORDS) + threadIdx.x;
    const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(store) + (long long)t.slot[blockIdx.y] * words;
    float4* __restrict__ out = reinterpret_cast<float4*>(dst) + (long long)blockIdx.y * words;
    unsigned v[CG_WORDS];
#pragma unroll
    for (int i = 0; i < CG_WORDS; ++i) {
        const long long w = w0 + i * CG_THREADS;
        if (w < words) v[i] = src[w];
    }
#pragma unroll
    for (int i = 0; i < CG_WORDS; ++i) {
        const long long w = w0 + i * CG_THREADS;
        if (w < words) out[w] = word_over_255(v[i]);
    }
}

}  // namespace

extern "C" int fv_gather_u8_f32(fv_ctx* ctx, const uint8_t* store, int64_t n_slots, int64_t elems, const int32_t* idx, int n,
                                float* dst) {
    // the arguments first (they need no context: with ctx NULL the reason is left where fv_create leaves its own)
    FV_REQUIRE(ctx, n >= 0 && n_slots >= 0, "gather_u8_f32: n %d, n_slots %lld", n, (long long)n_slots);
    FV_REQUIRE(ctx, elems >= 16 && elems % 16 == 0 && elems <= ((int64_t)1 << 36),
               "gather_u8_f32: elems %lld (a multiple of 16, from 16 to 2^36)", (long long)elems);
    FV_REQUIRE(ctx, n_slots <= INT64_MAX / elems, "gather_u8_f32: %lld slots of %lld bytes", (long long)n_slots, (long long)elems);
    if (n > 0) {
        FV_REQUIRE(ctx, store && idx && dst, "gather_u8_f32: null pointer with n %d", n);
        FV_REQUIRE(ctx, ((uintptr_t)store & 15) == 0 && ((uintptr_t)dst & 15) == 0, "gather_u8_f32: store and dst must be 16-byte aligned");
        for (int j = 0; j < n; ++j)
            FV_REQUIRE(ctx, idx[j] >= 0 && idx[j] < n_slots, "gather_u8_f32: index %d is %d, outside [0, %lld)", j, idx[j],
                       (long long)n_slots);
    }
    if (!ctx) return FV_ERR_INVALID;
    if (n == 0) return FV_OK;
    const long long words = elems / 4, per_block = (long long)CG_THREADS * CG_WORDS;
    const unsigned blocks = (unsigned)((words + per_block - 1) / per_block);          // elems <= 2^36: below 2^23
    for (int j0 = 0; j0 < n; j0 += CG_MAX) {
        const int nj = n - j0 < CG_MAX ? n - j0 : CG_MAX;
        GatherTable t{};
        for (int i = 0; i < nj; ++i) t.slot[i] = idx[j0 + i];
        FvProfScope ps(ctx, "crop_gather_kernel", 0.0, 5.0 * (double)elems * nj);
        hipLaunchKernelGGL(crop_gather_kernel, dim3(blocks, nj), dim3(CG_THREADS), 0, ctx->stream, store, t, words,
                           dst + (size_t)j0 * (size_t)elems);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}
