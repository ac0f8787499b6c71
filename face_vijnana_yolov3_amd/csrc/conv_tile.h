// The tile machinery of the fp32-MFMA convolutions, written once: conv_kernel / conv_tail_fixup_kernel (conv_mfma.hip), the
// persistent 1x1 form (conv1x1_mfma.hip) and the small-M kernel (conv_small_mfma.hip) are assembled from these parts, so "the same
// K order and epilogue as the tile kernel" is the same code and not a copy kept in step by hand.  In order: tile constants and the
// XCD-aware workgroup remap; lattice addressing (row-offset table entry, LatticeRows with set_tap); the operand register set
// (OperandRegs: load / stage); the K step (readfrag, mfma_chunk, the scheduling-barrier-pinned k_step); the accumulator helpers
// (acc_zero, acc_row, acc_to_lds, tile_stats); the per-piece output transform (piece_transform); the fused BN-backward reduction
// (BnRedAcc, bnred_flush); the statistics store; the grouped 16-byte store loop (wide_store with RowTable / RowLinear).  What a
// kernel keeps to itself is policy: which K step to load next and when, and how its tiles are dealt.  Everything is forced
// inline -- the kernels' generated code is what it was when each held its own copy (tools/kernel_histogram.py, kernel_resources.sh).
// Device code in an anonymous namespace: include from a .hip file only.
#pragma once
#include "conv.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDT = BK + 4;  // padded LDS row (dwords)

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    int q = nwg >> 3, r = nwg & 7, x = bid & 7, pos = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + pos;
}

// ---------------------------------------------------------------------------------------------- lattice addressing
// Output offset (in elements) of lattice row m of parity class cls, -1 = row outside the problem.
__device__ __forceinline__ int lattice_rowoff(const FvConvArgs& a, int cls, int m, int HWl) {
    int off = -1;
    if (m < a.M) {
        int b = m / HWl, rem = m - b * HWl, oh = rem / a.Wl, ow = rem - oh * a.Wl;
        off = ((b * a.Hout + oh * a.os + a.oph[cls]) * a.Wout + ow * a.os + a.opw[cls]) * a.Nout;
    }
    return off;
}

constexpr unsigned OOB = 0x80000000u;  // buffer offset >= num_records for every tensor we accept (< 2^31 bytes): the load returns zeros

// The APT lattice rows whose A operand a thread loads (rows m_first + rstep * p): image row base and input row / column of tap
// (0, 0), worked out once; set_tap turns them into the byte offsets of one tap (OOB where the tap falls outside the image).
template <int APT>
struct LatticeRows {
    int pix[APT], oh[APT], ow[APT];
    unsigned off[APT];
    __device__ __forceinline__ void init(const FvConvArgs& a, int m_first, int rstep, int HWl) {
#pragma unroll
        for (int p = 0; p < APT; ++p) {
            const int m = m_first + rstep * p;
            if (m < a.M) {
                const int b = m / HWl, rem = m - b * HWl, h = rem / a.Wl, w = rem - h * a.Wl;
                pix[p] = b * a.Hin; oh[p] = h * a.is; ow[p] = w * a.is;
            } else {
                pix[p] = 0; oh[p] = -(1 << 28); ow[p] = 0;          // every tap lands outside the image: zeros
            }
        }
    }
    __device__ __forceinline__ void set_tap(const FvConvArgs& a, const FvTaps& taps, int tp, int col4) {
        const int dh = taps.dh[tp], dw = taps.dw[tp];
#pragma unroll
        for (int p = 0; p < APT; ++p) {
            const int ih = oh[p] + dh, iw = ow[p] + dw;
            const bool ok = (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
            off[p] = ok ? (unsigned)(((pix[p] + ih) * a.Win + iw) * a.Cin + col4) * 4u : OOB;
        }
    }
};

// ---------------------------------------------------------------------------------------------- operand register set
// One K step's operand rows of a thread on their way HBM -> registers -> LDS: APT 16-byte pieces of A rows, BL of B rows.  Rows
// come through buffer descriptors: an out-of-range offset (row outside the image / the problem) returns zeros in hardware, so the
// K loop has no per-load branches.  stage() writes them to one LDS buffer pair (thread row r0, rows RSTEP apart).
template <int APT, int BL>
struct OperandRegs {
    u32x4 ra[APT], rb[BL];
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t wr, const unsigned (&a_off)[APT],
                                         const unsigned (&b_row)[BL], int aofs, int wofs) {
#pragma unroll
        for (int p = 0; p < APT; ++p) ra[p] = __builtin_amdgcn_raw_buffer_load_b128(xr, a_off[p], aofs, 0);
#pragma unroll
        for (int p = 0; p < BL; ++p) rb[p] = __builtin_amdgcn_raw_buffer_load_b128(wr, b_row[p], wofs, 0);
    }
    template <int RSTEP>
    __device__ __forceinline__ void stage(float* As, float* Bs, int r0, int col4) const {
#pragma unroll
        for (int p = 0; p < APT; ++p) *reinterpret_cast<u32x4*>(&As[(r0 + RSTEP * p) * LDT + col4]) = ra[p];
#pragma unroll
        for (int p = 0; p < BL; ++p) *reinterpret_cast<u32x4*>(&Bs[(r0 + RSTEP * p) * LDT + col4]) = rb[p];
    }
};

// ---------------------------------------------------------------------------------------------- K step
// Fragments of K chunk kc (8 deep) for a wave's MB x NB blocks of 32 x 32: arow / brow = the lane's row and lane-half column.
template <int MB, int NB>
__device__ __forceinline__ void readfrag(const float* __restrict__ Asm, const float* __restrict__ Bsm, int arow, int brow, int kc,
                                         float4 (&af)[MB], float4 (&bf)[NB]) {
#pragma unroll
    for (int i = 0; i < MB; ++i) af[i] = *reinterpret_cast<const float4*>(&Asm[arow + i * 32 * LDT + kc * 8]);
#pragma unroll
    for (int j = 0; j < NB; ++j) bf[j] = *reinterpret_cast<const float4*>(&Bsm[brow + j * 32 * LDT + kc * 8]);
}
// The one MFMA chunk: within an 8-deep chunk lane-half h supplies k = 4h + e to MFMA e.  k-major order: consecutive MFMAs rotate
// over all MB*NB accumulators, so an accumulator is re-used only every MB*NB-th instruction (dependent-accumulator latency never
// on the issue path).
template <int MB, int NB>
__device__ __forceinline__ void mfma_chunk(f32x16 (&acc)[MB][NB], const float4 (&af)[MB], const float4 (&bf)[NB]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float av = e == 0 ? af[i].x : e == 1 ? af[i].y : e == 2 ? af[i].z : af[i].w;
                const float bv = e == 0 ? bf[j].x : e == 1 ? bf[j].y : e == 2 ? bf[j].z : bf[j].w;
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
            }
}
// One K step (32 deep, four chunks) from the staged LDS tiles Ac / Bc.  Fragment double-buffering: the LDS reads of chunk c + 1
// are issued before the MFMAs of chunk c, and stage_next() -- the caller's "write the next step's rows to the other LDS buffer"
// -- runs between chunks 2 and 3.  The scheduling barriers pin exactly this order (a variant that differed only in
// s_waitcnt placement lost 2 %).  The caller issues its global loads before and its workgroup barrier after.
template <int MB, int NB, class StageNext>
__device__ __forceinline__ void k_step(f32x16 (&acc)[MB][NB], const float* Ac, const float* Bc, int arow, int brow, StageNext&& stage_next) {
    float4 af0[MB], bf0[NB], af1[MB], bf1[NB];
    readfrag<MB, NB>(Ac, Bc, arow, brow, 0, af0, bf0);
    readfrag<MB, NB>(Ac, Bc, arow, brow, 1, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_chunk<MB, NB>(acc, af0, bf0);
    __builtin_amdgcn_sched_barrier(0);
    readfrag<MB, NB>(Ac, Bc, arow, brow, 2, af0, bf0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_chunk<MB, NB>(acc, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    readfrag<MB, NB>(Ac, Bc, arow, brow, 3, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_chunk<MB, NB>(acc, af0, bf0);
    __builtin_amdgcn_sched_barrier(0);
    stage_next();
    __builtin_amdgcn_sched_barrier(0);
    mfma_chunk<MB, NB>(acc, af1, bf1);
}

// ---------------------------------------------------------------------------------------------- accumulator helpers
template <int MB, int NB>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[MB][NB]) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
}
// Row (inside its 32 x 32 block) of accumulator register r of a lane in lane-half `half`; the lane's column is lane & 31.
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// Accumulator layout -> row-major tile [..][LD] in LDS; row0 / col0: the wave's corner in the tile.  Barriers are the caller's.
template <int LD, int MB, int NB>
__device__ __forceinline__ void acc_to_lds(float* Cs, const f32x16 (&acc)[MB][NB], int row0, int col0, int half, int lc) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) Cs[(row0 + i * 32 + acc_row(r, half)) * LD + col0 + j * 32 + lc] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------- fused reductions
// Fused BatchNorm-backward reduction (FV_EPI_BNRED): the tile just produced is the gradient g w.r.t. the
// OUTPUT of a BN+LeakyReLU layer; with that layer's pre-BN tensor z the epilogue also forms
// gy = g * leaky'(z*scale+shift) and accumulates the column sums of gy and gy * xhat (d-beta, d-gamma)
// into that layer's fp64 slots -- the separate reduction pass over (g, z) disappears.
struct BnRedAcc {
    float4 sc, sh, mu, is, db, dg;
    __device__ __forceinline__ void init(const FvConvArgs& a, int n, bool on) {
        db = make_float4(0.f, 0.f, 0.f, 0.f); dg = db;
        sc = sh = mu = is = db;
        if (on) {
            sc = *reinterpret_cast<const float4*>(a.bn_scale + n); sh = *reinterpret_cast<const float4*>(a.bn_shift + n);
            mu = *reinterpret_cast<const float4*>(a.bn_mean + n); is = *reinterpret_cast<const float4*>(a.bn_invstd + n);
        }
    }
    __device__ __forceinline__ void add(const float4& g, const float4& z, float leaky) {
        float gy;
        gy = (z.x * sc.x + sh.x) > 0.f ? g.x : g.x * leaky; db.x += gy; dg.x += gy * ((z.x - mu.x) * is.x);
        gy = (z.y * sc.y + sh.y) > 0.f ? g.y : g.y * leaky; db.y += gy; dg.y += gy * ((z.y - mu.y) * is.y);
        gy = (z.z * sc.z + sh.z) > 0.f ? g.z : g.z * leaky; db.z += gy; dg.z += gy * ((z.z - mu.z) * is.z);
        gy = (z.w * sc.w + sh.w) > 0.f ? g.w : g.w * leaky; db.w += gy; dg.w += gy * ((z.w - mu.w) * is.w);
    }
};
// reduce the per-thread sums over the row lanes through LDS (scratch: 2 * RL * BN floats) and add the tile's column sums to
// slot `row_id % nslot`.  With more than 256 threads the two row lanes that share a wave (lanes l and l ^ 32 hold the same
// four columns when BN = 128) are combined by a shuffle first, so that the scratch still fits behind the output tile.
template <int BN, int NTH>
__device__ __forceinline__ void bnred_flush(const FvConvArgs& a, const BnRedAcc& r, float* scratch, int n0, int row_id, int tid) {
    constexpr int C4 = BN / 4;
    constexpr bool PAIR = NTH > 256;          // pre-reduce the row lanes that share a wave: one scratch row per wave
    static_assert(!PAIR || (64 % C4 == 0), "the in-wave pre-reduction needs the column groups to tile a wave");
    constexpr int RL = PAIR ? NTH / 64 : NTH / C4;
    const int c4 = (tid % C4) * 4;       // tid: threadIdx.x (a persistent caller passes an opaque copy, so that nothing here is hoisted out of its tile loop)
    float4 db = r.db, dg = r.dg;
    int rl = tid / C4;
    bool writer = true;
    if constexpr (PAIR) {
#pragma unroll
        for (int o = C4; o < 64; o <<= 1) {   // lanes l and l ^ o hold the same four columns
            db.x += __shfl_xor(db.x, o); db.y += __shfl_xor(db.y, o); db.z += __shfl_xor(db.z, o); db.w += __shfl_xor(db.w, o);
            dg.x += __shfl_xor(dg.x, o); dg.y += __shfl_xor(dg.y, o); dg.z += __shfl_xor(dg.z, o); dg.w += __shfl_xor(dg.w, o);
        }
        writer = (tid & 63) < C4;
        rl = tid >> 6;
    }
    float (*red)[RL][BN] = reinterpret_cast<float (*)[RL][BN]>(scratch);
    __syncthreads();
    if (writer) {
        *reinterpret_cast<float4*>(&red[0][rl][c4]) = db;
        *reinterpret_cast<float4*>(&red[1][rl][c4]) = dg;
    }
    __syncthreads();
    if (tid < BN && n0 + tid < a.Nout) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < RL; ++w) { s += red[0][w][tid]; q += red[1][w][tid]; }
        double* sl = a.bn_slots + (size_t)(row_id % a.bn_nslot) * 2 * a.Nout;
        unsafeAtomicAdd(sl + n0 + tid, (double)s);
        unsafeAtomicAdd(sl + a.Nout + n0 + tid, (double)q);
    }
}

// Column sum / sum of squares of one tile: either its own partial row (deterministic; reduced later by
// bn_finalize) or added to one of a few fp64 accumulator slots (fp32 partials are exact in fp64; only
// the order of the fp64 additions varies, far below fp32 resolution) which the consumer kernel sums
// itself -- that saves the finalize launch between the conv and the normalise pass.
__device__ __forceinline__ void stat_store(const FvConvArgs& a, int mt, int n, float s, float q) {
    if (a.stat_slots) {
        double* sl = a.stat_slots + (size_t)(mt % a.stat_nslot) * 2 * a.Nout;
        unsafeAtomicAdd(sl + n, (double)s);
        unsafeAtomicAdd(sl + a.Nout + n, (double)q);
    } else {
        a.psum[(size_t)mt * a.Nout + n] = s;
        a.psq[(size_t)mt * a.Nout + n] = q;
    }
}

// Column sum / sum of squares of the tile in the accumulators (training-mode BatchNorm), reduced over the WAVES_M wave rows
// through `red` and handed to stat_store as tile row mt.
template <int BN, int WAVES_M, int MB, int NB>
__device__ __forceinline__ void tile_stats(const FvConvArgs& a, const f32x16 (&acc)[MB][NB], float (&red)[2][WAVES_M][BN], int wm, int col0,
                                           int half, int lc, int tid, int n0, int mt) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { float v = acc[i][j][r]; s += v; q += v * v; }
        s += __shfl_xor(s, 32);
        q += __shfl_xor(q, 32);
        if (half == 0) { red[0][wm][col0 + j * 32 + lc] = s; red[1][wm][col0 + j * 32 + lc] = q; }
    }
    __syncthreads();
    if (tid < BN && n0 + tid < a.Nout) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_M; ++w) { s += red[0][w][tid]; q += red[1][w][tid]; }
        stat_store(a, mt, n0 + tid, s, q);
    }
}

// ---------------------------------------------------------------------------------------------- output
// What happens to one 16-byte piece (output channels n .. n + 3) on its way out: per-channel affine -> LeakyReLU -> residual add.
// addend points to the piece's addend; it is read only with FV_EPI_ADD (addon).
__device__ __forceinline__ void piece_transform(const FvConvArgs& a, float4& v, int n, bool addon, const float4* addend) {
    if (a.epi & FV_EPI_AFFINE) {
        if (a.scale) { const float4 s = *reinterpret_cast<const float4*>(a.scale + n); v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w; }
        if (a.shift) { const float4 s = *reinterpret_cast<const float4*>(a.shift + n); v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w; }
    }
    if (a.epi & FV_EPI_LEAKY) {
        v.x = v.x > 0.f ? v.x : v.x * a.leaky; v.y = v.y > 0.f ? v.y : v.y * a.leaky;
        v.z = v.z > 0.f ? v.z : v.z * a.leaky; v.w = v.w > 0.f ? v.w : v.w * a.leaky;
    }
    if (addon) { const float4 s = *addend; v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w; }
}

// How a tile row maps to an output offset (in elements): through the row-offset table of the gather kernels, or linearly
// (row m of the lattice = row m of out) for the persistent 1x1 form.
struct RowTable {
    const int* rowoff;
    __device__ __forceinline__ bool ok(int row) const { return rowoff[row] >= 0; }
    __device__ __forceinline__ int off(int row) const { return rowoff[row]; }
};
struct RowLinear {
    int m0, M, Nout;
    __device__ __forceinline__ bool ok(int row) const { return m0 + row < M; }
    __device__ __forceinline__ int off(int row) const { return (m0 + row) * Nout; }
};

// Wide store of the BM_ x BN tile that acc_to_lds left in Cs (16-byte output rows).  In the accumulator layout a lane owns one
// output column and 16 scattered rows, i.e. 64 four-byte stores per lane and tile -- a store-issue-bound tail of ~10 us per tile;
// from the transposed tile whole 16-byte pieces leave: 4x fewer store instructions, every wave instruction covers two full
// 512-byte rows.  The tile leaves in groups of four pieces per thread: the global loads of a group (the residual addend; z of the
// fused BN-backward reduction) are ALL issued before the first of them is used.  Piece by piece -- load, wait, combine, store --
// every one of the BM_ * C4 / NTH pieces paid a full memory round trip (eight s_waitcnt vmcnt(0) in a row): ~10 us per tile, which
// is most of a 1x1 data-gradient tile's life (4 - 8 K steps).  Rows outside the problem load from offset 0 (in range, unused).
// With bnred the pieces also feed the fused BN-backward reduction, flushed to slot row_id through the LDS behind the tile.
// tid: threadIdx.x (a persistent caller passes an opaque copy, so that nothing here is hoisted out of its tile loop).
template <int BM_, int BN, int NTH, class RowMap>
__device__ __forceinline__ void wide_store(const FvConvArgs& a, float* Cs, float* outp, const RowMap& rows, int n0, int row_id, int tid, bool bnred) {
    constexpr int C4 = BN / 4;                   // float4 pieces per tile row
    BnRedAcc br;                                 // NTH % C4 == 0: a thread keeps its 4 columns over the rows
    br.init(a, n0 + (tid % C4) * 4, bnred && n0 + (tid % C4) * 4 < a.Nout);
    constexpr int NP = BM_ * C4 / NTH, GP = NP < 4 ? NP : 4;
    static_assert(NP % GP == 0, "epilogue grouping");
    const bool addon = (a.epi & FV_EPI_ADD) != 0;
#pragma unroll
    for (int p0 = 0; p0 < NP; p0 += GP) {
        int offn[GP]; bool okp[GP];
        float4 zq[GP], aq[GP];
#pragma unroll
        for (int q = 0; q < GP; ++q) {
            const int f = tid + NTH * (p0 + q), row = f / C4, c4 = (f % C4) * 4;
            const int n = n0 + c4;
            okp[q] = rows.ok(row) && n < a.Nout;
            offn[q] = okp[q] ? rows.off(row) + n : 0;
        }
        if (bnred) {
#pragma unroll
            for (int q = 0; q < GP; ++q) zq[q] = *reinterpret_cast<const float4*>(a.bn_z + offn[q]);
        }
        if (addon) {
#pragma unroll
            for (int q = 0; q < GP; ++q) aq[q] = *reinterpret_cast<const float4*>(a.addend + offn[q]);
        }
#pragma unroll
        for (int q = 0; q < GP; ++q) {
            const int f = tid + NTH * (p0 + q), row = f / C4, c4 = (f % C4) * 4;
            if (okp[q]) {
                float4 v = *reinterpret_cast<const float4*>(&Cs[row * BN + c4]);
                piece_transform(a, v, n0 + c4, addon, &aq[q]);
                *reinterpret_cast<float4*>(outp + offn[q]) = v;
                if (bnred) br.add(v, zq[q], a.bn_leaky);
            }
        }
    }
    if (bnred) bnred_flush<BN, NTH>(a, br, Cs + BM_ * BN, n0, row_id, tid);
}

}  // namespace
