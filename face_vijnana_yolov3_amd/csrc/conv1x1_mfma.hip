// Persistent form of the 1x1 stride-1 convolution (forward of the 23 1x1 layers of yolov3_detect.py:221-267 and their
// data-gradients): a plain GEMM out[M][N] = x[M][K] . w[N][K]^T on the tile machinery of conv_mfma.hip.
//
// Why a second kernel (tools/conv_phases.py, round 5): a 1x1 tile lives 4 .. 16 K steps.  In the one-tile-per-workgroup launch
// all 512 resident workgroups run IN PHASE -- prologue (operand latency, nothing to multiply), K loop, epilogue -- over the
// whole chip: the matrix pipes idle during every prologue and epilogue, the memory system idles during every K loop (the
// data-gradients with the fused BN-backward reduction move 192 KB per tile in their epilogue), and a round of tiles costs
// prologue + K loop + epilogue although the 3x3 layers show that a workgroup's epilogue hides behind its CU partner's K loop
// once the two are out of phase.  Here a workgroup walks several tiles:
//  * the operand rows of tile i+1 (first two K steps) are in flight while tile i's epilogue runs -- no prologue latency after
//    the first tile, no workgroup launch between tiles;
//  * the two workgroups of a CU fall out of phase after their first tile (one wins the matrix pipe) and stay so:
//    one multiplies while the other stores;
//  * addressing is linear (row m of the lattice = row m of x and of out): no divisions, no row-offset table.
// The K step, the accumulator helpers and the store epilogue are the ones conv_kernel<BN, ...> uses (conv_tile.h), so the results
// are bit-identical (tests/test_ops_gpu.py).  Tiles are dealt round-robin (workgroup b takes b, b + G, ...; the XCD remap keeps the N tiles of one
// A panel on one L2 at the same time).
#include <string>
#include <type_traits>
#include "conv_tile.h"
#include "elementwise.h"

namespace {

constexpr int BI_CMAX = 512;   // BN-input mode: input channels whose scale / shift a workgroup keeps in LDS (2 x 2 KB; two workgroups per CU fill the LDS)

#ifndef PF_BNRED
#define PF_BNRED 0
#endif

// PF: K steps of the NEXT tile whose operand loads are issued before the epilogue (0 .. 2; the rest right after it).  BNRED: the epilogue
// with the fused BN-backward reduction (its z / addend rows and per-channel vectors need the registers a deep prefetch would hold).
//
// BNIN (1, or 2 with a skip tensor): the BN-input mode of conv.h.  x is z(l) of the producing layer: after the workgroup has
// turned that layer's statistics slots into scale / shift (the prologue of bn_act_stats_kernel, same code), the step that moves an
// A piece from registers to LDS writes LeakyReLU(z * scale + shift) (+ skip) -- the expression and order of the normalise pass,
// so a(l) and this launch's z are the bits of the two-launch form -- and, in the workgroups of N tile 0, stores the piece to a(l).
// Rows beyond M stage 0.0 (the descriptor's zero would come out as LeakyReLU(shift)) and store nothing.  The skip piece of K step
// s + 1 is loaded at the start of K step s, one step later than z: one register set for it instead of two.
template <int BN, int WAVES_M, int WAVES_N, int PF, bool BNRED, int BNIN = 0>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 4) void conv1x1_persist_kernel(const FvConvArgs a, const int ntiles) {
    constexpr int NTH = 64 * WAVES_M * WAVES_N;
    constexpr int APT = BM * 8 / NTH;
    constexpr int RSTEP = NTH / 8;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int MB = WTM / 32, NB = WTN / 32;
    constexpr int BL = BN * 8 / NTH;
    static_assert(NTH == 512 && MB >= 1 && NB >= 1 && BL >= 1 && APT >= 1, "bad tiling");

    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * LDT];
    static_assert(2 * (BM + BN) * LDT >= BM * BN + 2 * (NTH / 64) * BN, "operand LDS must hold the output tile + the BN-backward reduction scratch");
    float (*As)[BM * LDT] = reinterpret_cast<float (*)[BM * LDT]>(smem);
    float (*Bs)[BN * LDT] = reinterpret_cast<float (*)[BN * LDT]>(smem + 2 * BM * LDT);
    __shared__ float red[2][WAVES_M][BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int NT = (a.Nout + BN - 1) / BN;
    const int nk = a.Cin / BK;

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)((unsigned)a.M * a.Cin * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, (int)((unsigned)a.Nout * a.Cin * 4u), 0x00020000);
    const int col4 = (tid & 7) * 4, r0 = tid >> 3;
    unsigned a_off[APT], b_row[BL];
    OperandRegs<APT, BL> regs0, regs1;         // even / odd K steps
    u32x4 sk[APT];                             // BNIN == 2: the skip pieces of the K step staged next
    float *s_sc = nullptr, *s_sh = nullptr;
    bool store_a = false;
    __amdgpu_buffer_rsrc_t sr = xr, ar = xr;
    if constexpr (BNIN != 0) {
        __shared__ __attribute__((aligned(16))) float s_aff[2][BI_CMAX];
        s_sc = s_aff[0]; s_sh = s_aff[1];
        ar = __builtin_amdgcn_make_buffer_rsrc((void*)a.bi_a, 0, (int)((unsigned)a.M * a.Cin * 4u), 0x00020000);
        if constexpr (BNIN == 2) sr = __builtin_amdgcn_make_buffer_rsrc((void*)a.bi_skip, 0, (int)((unsigned)a.M * a.Cin * 4u), 0x00020000);
    }

    auto set_tile = [&](int w, int& mt, int& nt) {
        const int tile = xcd_remap(w, ntiles);
        mt = tile / NT; nt = tile - mt * NT;
#pragma unroll
        for (int p = 0; p < APT; ++p) {
            const int m = mt * BM + r0 + RSTEP * p;
            a_off[p] = m < a.M ? (unsigned)(m * a.Cin + col4) * 4u : OOB;
        }
#pragma unroll
        for (int p = 0; p < BL; ++p) {
            const int n = nt * BN + r0 + RSTEP * p;
            b_row[p] = n < a.Nout ? (unsigned)(n * a.Cin + col4) * 4u : OOB;
        }
        store_a = nt == 0;
    };
    auto load = [&](OperandRegs<APT, BL>& regs, int step) { regs.load(xr, wr, a_off, b_row, step * BK * 4, step * BK * 4); };
    auto load_skip = [&](int step) {
        if constexpr (BNIN == 2) {
#pragma unroll
            for (int p = 0; p < APT; ++p) sk[p] = __builtin_amdgcn_raw_buffer_load_b128(sr, a_off[p], step * BK * 4, 0);
        }
    };
    // registers -> LDS of K step `step` (a_off, store_a: the tile these rows belong to)
    auto stage = [&](OperandRegs<APT, BL>& regs, float* Asb, float* Bsb, int step) {
        if constexpr (BNIN != 0) {
            const float4 sc = *reinterpret_cast<const float4*>(s_sc + step * BK + col4), sh = *reinterpret_cast<const float4*>(s_sh + step * BK + col4);
#pragma unroll
            for (int p = 0; p < APT; ++p) {
                float4 v = fv_bn_leaky4(__builtin_bit_cast(float4, regs.ra[p]), sc, sh, a.bi_leaky);
                if constexpr (BNIN == 2) { const float4 q = __builtin_bit_cast(float4, sk[p]); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
                const bool ok = a_off[p] != OOB;
                if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
                regs.ra[p] = __builtin_bit_cast(u32x4, v);
                if (store_a && ok) __builtin_amdgcn_raw_buffer_store_b128(regs.ra[p], ar, a_off[p], step * BK * 4, 0);
            }
        }
        regs.template stage<RSTEP>(Asb, Bsb, r0, col4);
    };
    const int arow = (wm * WTM + (lane & 31)) * LDT + (lane >> 5) * 4;
    const int brow = (wn * WTN + (lane & 31)) * LDT + (lane >> 5) * 4;

    int w = blockIdx.x, mt, nt;
    set_tile(w, mt, nt);
    load(regs0, 0);
    if (nk > 1) load(regs1, 1);
    load_skip(0);
    if constexpr (BNIN != 0) {
        // the operand buffers are not in use yet: the slot partials go through them
        fv_bn_slots_to_affine<NTH>(a.bi_slots, a.bi_nslot, a.bi_count, a.bi_gamma, a.bi_beta, a.bi_eps, a.bi_ema_old, a.bi_ema_new, a.bi_mean,
                                   a.bi_invstd, a.bi_scale, a.bi_shift, a.bi_mmean, a.bi_mvar, a.Cin, blockIdx.x == 0, s_sc, s_sh,
                                   reinterpret_cast<double (*)[256]>(smem));
        __syncthreads();
    }

    for (;;) {
        f32x16 acc[MB][NB];
        acc_zero(acc);
        stage(regs0, As[0], Bs[0], 0);      // K step 0 of this tile: loaded before the previous tile's epilogue (or above)
        __syncthreads();
        auto body = [&](int s, auto odd) {
            constexpr int ODD = decltype(odd)::value;
            if (s + 1 < nk) load_skip(s + 1);
            if (s + 2 < nk) load(ODD ? regs1 : regs0, s + 2);
            k_step(acc, As[ODD], Bs[ODD], arow, brow, [&] {
                if (s + 1 < nk) stage(ODD ? regs0 : regs1, As[1 - ODD], Bs[1 - ODD], s + 1);
            });
            __syncthreads();
        };
        for (int s = 0; s < nk; s += 2) {
            body(s, std::false_type{});
            if (s + 1 < nk) body(s + 1, std::true_type{});
        }

        // the next tile's first operand rows go out now and land while this tile is on its way out
        const int mt_c = mt, nt_c = nt;
        const int wnext = w + (int)gridDim.x;
        const bool more = wnext < ntiles;
        if (more) {
            set_tile(wnext, mt, nt);
            if constexpr (PF >= 1) load(regs0, 0);
            if constexpr (PF >= 2) { if (nk > 1) load(regs1, 1); }
            load_skip(0);
        }

        // ------------------------------------------------------------------ epilogue of tile (mt_c, nt_c)
        const int m0 = mt_c * BM, n0 = nt_c * BN;
        // the piece coordinates below depend on the thread id alone: left to itself the compiler hoists all of them out of the tile loop
        // and keeps ~40 VGPRs live through the K loop (164 instead of 122: one workgroup per CU).  An opaque copy of the thread id
        // makes them this iteration's values again.
        int te = tid;
        asm volatile("" : "+v"(te));
        const int lane_e = te & 63, half_e = lane_e >> 5, lc_e = lane_e & 31, wave_e = te >> 6;
        const int wm_e = wave_e / WAVES_N, wn_e = wave_e % WAVES_N;
        if (a.epi & FV_EPI_STATS) tile_stats(a, acc, red, wm_e, wn_e * WTN, half_e, lc_e, te, n0, mt_c);
        float* Cs = smem;
        __syncthreads();         // (the K loop's last barrier already separates the operand reads from these writes; kept for the `red` reads above)
        acc_to_lds<BN>(Cs, acc, wm_e * WTM, wn_e * WTN, half_e, lc_e);
        __syncthreads();
        wide_store<BM, BN, NTH>(a, Cs, a.out, RowLinear{m0, a.M, a.Nout}, n0, mt_c, te, BNRED);
        if (!more) break;
        w = wnext;
        if constexpr (PF < 1) load(regs0, 0);
        if constexpr (PF < 2) { if (nk > 1) load(regs1, 1); }
        __syncthreads();         // the output tile (and the reduction scratch behind it) has been read: the operand buffers are free again
    }
}

template <int BN, int WM_, int WN_>
int launch_persist(fv_ctx* ctx, const FvConvArgs& a) {
    const bool bnred = (a.epi & FV_EPI_BNRED) != 0;
    const int bnin = a.bi_slots ? (a.bi_skip ? 2 : 1) : 0;
    const int MT = (a.M + BM - 1) / BM, NT = (a.Nout + BN - 1) / BN;
    const int ntiles = MT * NT;
    const int grid = ntiles < 512 ? ntiles : 512;        // two workgroups per CU; a multiple of 8 whenever a workgroup takes a second tile
    static const std::string name_s = "conv1x1_persist_kernel<" + std::to_string(BN) + ">";
    static const char* name = name_s.c_str();
    FvProfScope ps(ctx, name, "M" + std::to_string(a.M) + " N" + std::to_string(a.Nout) + " K" + std::to_string(a.Cin) + ((a.epi & FV_EPI_BNRED) ? " r" : "") +
                       (bnin == 2 ? " bn+skip" : bnin ? " bn" : ""),
                   a.alg_flops, 4.0 * ((double)a.M * a.Cin * (1 + bnin) + (double)a.Nout * a.Cin + (double)a.M * a.Nout * ((a.epi & FV_EPI_ADD) ? 2 : 1)));
    if (bnin == 2) hipLaunchKernelGGL((conv1x1_persist_kernel<BN, WM_, WN_, 2, false, 2>), dim3(grid), dim3(64 * WM_ * WN_), 0, ctx->stream, a, ntiles);
    else if (bnin) hipLaunchKernelGGL((conv1x1_persist_kernel<BN, WM_, WN_, 2, false, 1>), dim3(grid), dim3(64 * WM_ * WN_), 0, ctx->stream, a, ntiles);
    else if (bnred) hipLaunchKernelGGL((conv1x1_persist_kernel<BN, WM_, WN_, PF_BNRED, true>), dim3(grid), dim3(64 * WM_ * WN_), 0, ctx->stream, a, ntiles);
    else hipLaunchKernelGGL((conv1x1_persist_kernel<BN, WM_, WN_, 2, false>), dim3(grid), dim3(64 * WM_ * WN_), 0, ctx->stream, a, ntiles);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

}  // namespace

// A 1x1 stride-1 launch over the whole lattice with 16-byte output rows
static bool gemm_shape_ok(const FvConvArgs& a) {
    if (a.nclass != 1 || a.taps[0].n != 1 || a.taps[0].dh[0] != 0 || a.taps[0].dw[0] != 0 || a.taps[0].wslot[0] != 0 || a.Tw != 1) return false;
    if (a.is != 1 || a.os != 1 || a.Hl != a.Hin || a.Wl != a.Win || a.Hout != a.Hl || a.Wout != a.Wl || a.oph[0] || a.opw[0]) return false;
    return a.Cin % BK == 0 && !(a.Nout & 3) && a.Nout > 32 && a.ksplit <= 1 && !a.narrow;
}

// ... and more tiles than the 512 resident slots: the case in which a workgroup of the persistent form gets a second tile.
// (Fewer tiles: the one-tile kernel with its K split / tail split.)
bool fv_conv1x1_persist_ok(const FvConvArgs& a) {
    if (!gemm_shape_ok(a)) return false;
    const int bn = a.Nout > 64 ? 128 : 64;
    const long long tiles = (long long)((a.M + BM - 1) / BM) * ((a.Nout + bn - 1) / bn);
    return tiles > 512;
}

// The BN-input mode exists in this kernel alone, so it takes the launch at any number of tiles (grid = tiles below 512): a training
// forward (statistics epilogue, nothing else) whose input channels fit the scale / shift vectors in LDS.
bool fv_conv1x1_bn_in_ok(const FvConvArgs& a) {
    return gemm_shape_ok(a) && a.epi == FV_EPI_STATS && a.Cin <= BI_CMAX && !a.small && !a.bm64;
}

// Where the fused launch is taken by default.  Every class of the 40 x 416^2 step that the kernel takes measured below normalise
// pass + plain conv, with and without skip: 104^2 (3380 tiles), 52^2 (845) and 26^2 (212 M tiles x 2 N tiles = 424,
// fewer than the 512 resident slots: the persistent kernel at grid = tiles).  Launches with fewer than 256 tiles -- half the
// resident slots idle in either form -- were not measured and keep the two launches.
bool fv_conv1x1_bn_in_wins(const FvConvArgs& a, bool with_skip) {
    (void)with_skip;
    const int bn = a.Nout > 64 ? 128 : 64;
    return (long long)((a.M + BM - 1) / BM) * ((a.Nout + bn - 1) / bn) >= 256;
}

int fv_conv1x1_persist_launch(fv_ctx* ctx, const FvConvArgs& a) {
    if (a.Nout > 64) return launch_persist<128, 2, 4>(ctx, a);
    return launch_persist<64, 4, 2>(ctx, a);
}
