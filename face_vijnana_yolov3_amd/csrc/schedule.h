// Host-side pieces shared by the network schedules (net.hip: FaceDetector, net_yolov3.hip: the three-scale graph, net_fid.hip:
// the FaceIdentifier's towers): workspace carving and sizing, the batch check, the inference conv dispatch, a training step's
// preamble, the training forward of a BN layer and of the base, and the backward pass with its side-stream weight-gradient
// pipeline.  No kernels here: every helper enqueues operator launches.  Included by the schedule files only.
#pragma once
#include <algorithm>
#include <vector>
#include "conv.h"
#include "elementwise.h"
#include "ops.h"

namespace {

constexpr float BN_EPS = 1e-3f;       // yd.py:212
constexpr float BN_MOMENTUM = 0.99f;  // Keras BatchNormalization default
constexpr float LEAKY = 0.1f;         // yd.py:213

using Layers = std::vector<fv_layer_desc>;

struct Carver {
    char* base; size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    float* take(size_t floats) {
        float* p = base ? (float*)(base + off) : nullptr;
        off += (floats * sizeof(float) + 255) & ~(size_t)255;
        return p;
    }
    float* take_some(size_t floats) { return floats ? take(floats) : nullptr; }   // NULL (and nothing carved) for none
};

// Lends the plan's tail-split scratch to the conv launcher for the duration of one network call.
struct TailLend {
    fv_ctx* ctx;
    float* prev; long long prev_floats;
    TailLend(fv_ctx* c, float* tail, size_t tail_floats) : ctx(c), prev(c->tail_slab), prev_floats(c->tail_slab_floats) {
        c->tail_slab = nullptr; c->tail_slab_floats = 0;
        if (c->tail_split && tail) { c->tail_slab = tail; c->tail_slab_floats = (long long)tail_floats; }
    }
    ~TailLend() { ctx->tail_slab = prev; ctx->tail_slab_floats = prev_floats; }
};

// fv_set_bn_zero_debias_step applies to ONE training step: later per-operator BN calls on this context use their own momentum
struct EmaReset { fv_ctx* c; ~EmaReset() { c->bn_ema_step = 0; } };

// Every tensor is addressed through one 2 GiB buffer descriptor (fv_conv_launch): the largest, the first layer's output of
// batch*S*S*32 floats, must stay below 2^29.  Checked before anything is enqueued, so a refused call changes nothing.
int check_batch(fv_ctx* ctx, const char* who, int batch, int S) {
    FV_REQUIRE(ctx, batch >= 1 && S >= 32 && S % 32 == 0, "%s: image_size must be a positive multiple of 32 (got %d), batch >= 1", who, S);
    const long long elems = (long long)batch * S * S * 32;
    FV_REQUIRE(ctx, elems < (1ll << 29), "%s: batch*S*S*32 = %lld reaches 2^29 elements (2 GiB buffer descriptor); reduce the batch",
               who, elems);
    return FV_OK;
}

// K-split partial slabs of the small-M inference launches of layers 1.. (batch-1 latency path), under either setting of
// option "conv_bm64"
size_t ksplit_slab_floats(const Layers& L, int B, int S) {
    size_t max_slab = 0;
    for (size_t l = 1; l < L.size(); ++l) {
        const auto& d = L[l];
        size_t rows = (size_t)B * (S / d.out_div) * (S / d.out_div);
        for (int bm64 = 0; bm64 < 2; ++bm64) {
            const int ks = fv_conv_choose_ksplit((int)rows, d.cout, d.ksize * d.ksize * d.cin / 32, bm64 != 0);
            if (ks > 1 && ks * rows * d.cout > max_slab) max_slab = ks * rows * d.cout;
        }
    }
    return max_slab;
}

// Tail-split scratch: the largest need over the forward and (training) stride-1 data-gradient launches of layers 1..; the
// data-gradient of a layer without BN reads its output gradient padded to cpad channels.
size_t tail_split_floats(const Layers& L, int B, int S, bool training, int cpad) {
    long long need = 0;
    for (size_t l = 1; l < L.size(); ++l) {
        const auto& d = L[l];
        const int Hi = S / d.in_div, Ho = Hi / d.stride;
        int tf, full; long long n;
        fv_conv_tail_plan(B * Ho * Ho, d.cout, d.ksize * d.ksize * d.cin / 32, &tf, &full, &n);
        need = std::max(need, n);
        if (training && d.stride == 1) {
            fv_conv_tail_plan(B * Hi * Hi, d.cin, d.ksize * d.ksize * (d.has_bn ? d.cout : cpad) / 32, &tf, &full, &n);
            need = std::max(need, n);
        }
    }
    return (size_t)need;
}

// Chunks of at most the 64 layers the fold / transpose kernels take per launch, of equal size.
int chunk_size(int n) { const int chunks = (n + 63) / 64; return (n + chunks - 1) / chunks; }

// Fold the moving statistics of every BN layer into scale/shift (all channels, channel offset = mean_off / 2).
int fold_bn(fv_ctx* ctx, const Layers& L, const float* params, const float* bn_state, float* scale, float* shift) {
    std::vector<const fv_layer_desc*> bn;
    for (const auto& d : L) if (d.has_bn) bn.push_back(&d);
    const int n = (int)bn.size(), per = chunk_size(n);
    for (int i0 = 0; i0 < n; i0 += per) {
        const int cnt = std::min(per, n - i0), c0 = (int)(bn[i0]->mean_off / 2);
        int chb[64]; long long go[64], bo[64], mo[64], vo[64];
        for (int i = 0; i < cnt; ++i) {
            const auto& d = *bn[i0 + i];
            chb[i] = (int)(d.mean_off / 2) - c0; go[i] = d.gamma_off; bo[i] = d.beta_off; mo[i] = d.mean_off; vo[i] = d.var_off;
        }
        const auto& last = *bn[i0 + cnt - 1];
        if (int rc = fv_ew_bn_fold_all(ctx, params, bn_state, cnt, chb, go, bo, mo, vo, BN_EPS, (int)(last.mean_off / 2) + last.cout - c0,
                                       scale + c0, shift + c0)) return rc;
    }
    return FV_OK;
}

// Transposed kernels [cin][tap][cout] of layers 1.. into wt[l] for the data-gradients; a layer without BN is padded to cpad.
int transpose_weights(fv_ctx* ctx, const Layers& L, const float* params, const std::vector<float*>& wt, int cpad) {
    const int n = (int)L.size() - 1, per = chunk_size(n);
    for (int l0 = 1; l0 <= n; l0 += per) {
        const int cnt = std::min(per, n + 1 - l0);
        long long so[64], dof[64]; int tn[64], tt[64], tc[64], tp[64];
        for (int i = 0; i < cnt; ++i) {
            const auto& d = L[l0 + i];
            so[i] = d.w_off; dof[i] = wt[l0 + i] - wt[l0];
            tn[i] = d.cout; tt[i] = d.ksize * d.ksize; tc[i] = d.cin; tp[i] = d.has_bn ? d.cout : cpad;
        }
        if (int rc = fv_ew_transpose_all(ctx, params, wt[l0], cnt, so, dof, tn, tt, tc, tp)) return rc;
    }
    return FV_OK;
}

// ------------------------------------------------------------------------------------------------------------ inference
// One inference pass: BN folded into scale/shift (all channels, offset mean_off / 2), the first layer's kernel packed.
struct Infer {
    fv_ctx* ctx; const float* params; int B, S;
    const float *w0p, *scale, *shift;
    float* slab;   // K-split partial slabs
};

// Conv of layer d: BN + LeakyReLU (or bias alone without BN), then + skip.  A small-M launch (batch-1 latency) is K-split into
// partial slabs that the finish kernel sums in fixed order -- unless conv_small splits K inside the workgroup; the first layer
// (3 input channels, packed kernel) never splits.
int infer_conv(const Infer& f, const fv_layer_desc& d, const float* in, const float* skip, float* out) {
    fv_ctx* ctx = f.ctx;
    const int H = f.S / d.in_div;
    const long long rows = (long long)f.B * (H / d.stride) * (H / d.stride);
    const float* w = d.cin % 32 ? f.w0p : f.params + d.w_off;
    const float* sc = d.has_bn ? f.scale + d.mean_off / 2 : nullptr;
    const float* sh = d.has_bn ? f.shift + d.mean_off / 2 : f.params + d.beta_off;
    const int ks = d.cin % 32 || (ctx->conv_small && fv_conv_small_plan((int)rows, d.cout, d.cin, d.ksize * d.ksize)) ? 1
                   : fv_conv_choose_ksplit((int)rows, d.cout, d.ksize * d.ksize * d.cin / 32, ctx->conv_bm64);
    if (ks > 1) {
        if (int rc = fv_op_conv_forward(ctx, in, w, f.B, H, H, d.cin, d.cout, d.ksize, d.stride, 0, nullptr, nullptr, 0.f, nullptr,
                                        f.slab, nullptr, nullptr, ks)) return rc;
        return fv_ew_splitk_finish(ctx, f.slab, ks, rows * d.cout, sc, sh, skip, out, rows * d.cout, d.cout, LEAKY, d.has_bn);
    }
    const int epi = FV_EPI_AFFINE | (d.has_bn ? FV_EPI_LEAKY : 0) | (skip ? FV_EPI_ADD : 0);
    return fv_op_conv_forward(ctx, in, w, f.B, H, H, d.cin, d.cout, d.ksize, d.stride, epi, sc, sh, LEAKY, skip, out, nullptr, nullptr);
}

// The Darknet-53 base L[0, nb) over three rotating buffers G (the input, the skip kept while a residual block runs, the output).
// out_at[l] (when given) takes layer l's output instead: a tensor the caller keeps.  Returns the last output and its buffer.
int base_infer(const Infer& f, const Layers& L, int nb, const float* x, float* const G[3], const std::vector<float*>& out_at,
               const float** last, int* ilast) {
    const float* cur = x;
    int icur = -1, iskip = -1;
    const float* skip = nullptr;
    for (int l = 0; l < nb; ++l) {
        const auto& d = L[l];
        if (d.role == 1) { skip = cur; iskip = icur; }
        int iout = 0;
        while (iout == icur || (iout == iskip && (d.role == 1 || d.role == 2))) ++iout;
        float* out = G[iout];
        if (!out_at.empty() && out_at[l]) { out = out_at[l]; iout = -1; }
        if (int rc = infer_conv(f, d, cur, d.role == 2 ? skip : nullptr, out)) return rc;
        cur = out; icur = iout;
        if (d.role == 2) { skip = nullptr; iskip = -1; }
    }
    *last = cur; *ilast = icur;
    return FV_OK;
}

// ------------------------------------------------------------------------------------------------------------- training
// The per-layer tensors a training step keeps (entries of the layers without BN stay NULL; wt[0] is unused: the first layer
// has no data-gradient).
struct Kept {
    std::vector<float*> z, a, mean, invstd, scale, shift, wt;
    std::vector<double*> slots, bslots;   // per layer [nslot][2][cout] fp64 accumulators, forward statistics and backward
    size_t slots_bytes = 0;               // d-beta/d-gamma (one contiguous range over all layers, zeroed by one memset)
    void resize(size_t n) {
        for (auto* v : {&z, &a, &mean, &invstd, &scale, &shift, &wt}) v->resize(n);
        slots.resize(n); bslots.resize(n);
    }
    void carve_slots(Carver& c, const Layers& L) {   // the BN layers' slots in one range, zeroed by one memset per step
        size_t tot = 0;
        for (const auto& d : L) if (d.has_bn) tot += (size_t)fv_ew_bn_stat_slots(d.cout) * 2 * d.cout;
        double* base = (double*)c.take(tot * 4);
        slots_bytes = 2 * tot * sizeof(double);
        for (size_t l = 0, off = 0; l < L.size(); ++l) {
            if (!L[l].has_bn) continue;
            slots[l] = base ? base + off : nullptr; bslots[l] = base ? base + tot + off : nullptr;
            off += (size_t)fv_ew_bn_stat_slots(L[l].cout) * 2 * L[l].cout;
        }
    }
};

// fv_*_train_workspace_tensor: where tensor `which` (z, a, mean, invstd, scale, shift) of layer l lies in the workspace
int kept_tensor(const Kept& k, const char* base, const fv_layer_desc& d, int l, int which, int B, int S, size_t* offset_bytes,
                int64_t* count) {
    const float* t = which == 0 ? k.z[l] : which == 1 ? k.a[l] : which == 2 ? k.mean[l]
                   : which == 3 ? k.invstd[l] : which == 4 ? k.scale[l] : k.shift[l];
    const int Ho = S / d.out_div;
    *offset_bytes = (size_t)((const char*)t - base);
    *count = which <= 1 ? (int64_t)B * Ho * Ho * d.cout : d.cout;
    return FV_OK;
}

// One training step: what the forward and backward helpers read.
struct Train {
    fv_ctx* ctx; const Layers& L; const Kept& k; int B, S;
    const float* params; float* bn_state; float* grads;
    bool accumulate_bn = false;   // d-beta / d-gamma are added to `grads` (towers sharing one BN layer), not stored
    // forward pass: the layer whose normalise pass waits for the next layer's forward (bn_in_next), and that pass's skip
    mutable int deferred = -1;
    mutable const float* deferred_skip = nullptr;
};

// Option "early_bn_fused" (DESIGN.md 4.3): where the readers of a(l - 1) are halo kernels, which stage every input element once,
// they apply layer l - 1's scale/shift + LeakyReLU while staging z(l - 1), and a(l - 1) is not written at all when BOTH its
// readers do: the forward and the weight-gradient of layer l.  That is a(0) and a(2) in all three graphs (conv_1 and conv_3, the
// 32 -> 64 channel 3x3 layers); no skip, route or head reads those two.  Decided from the launchers' own predicates under the
// context's options, the same way in the forward and the backward pass of one call.
struct EarlyIn {
    bool fwd = false, wgrad = false;   // layer l's forward / weight-gradient reads z(l - 1)
    bool virt() const { return fwd && wgrad; }
};
EarlyIn early_in(const Train& t, int l, const float* in) {
    EarlyIn e;
    if (l < 1 || l >= (int)t.L.size() || !t.ctx->early_bn) return e;
    const auto &d = t.L[l], &dp = t.L[l - 1];
    // the input is a(l - 1) of a BN layer without a residual add, and not the skip kept for a residual block
    if (!d.has_bn || !dp.has_bn || dp.role == 2 || d.role == 1 || in != t.k.a[l - 1]) return e;
    const int H = t.S / d.in_div;
    e.fwd = (t.ctx->early_bn & FV_EARLY_FWD) && fv_op_conv_forward_takes_bn_in(t.ctx, t.B, H, H, d.cin, d.cout, d.ksize, d.stride);
    e.wgrad = (t.ctx->early_bn & FV_EARLY_WGRAD) && fv_op_conv_wgrad_takes_bn_in(t.ctx, t.B, H, H, d.cin, d.cout, d.cout, d.ksize, d.stride);
    return e;
}

// Option "bn_in_1x1" (DESIGN.md 4.3): the first 1x1 conv of a residual block (role 1, C -> C/2, stride 1) reads every element of
// its input once, and that input a(l) is what layer l's normalise pass has just written.  Where the persistent 1x1 kernel takes
// the launch (and its shape class measured faster) the pass of layer l runs inside the forward of layer l + 1: the kernel sums
// layer l's slots, publishes its vectors, forms a(l) while staging z(l) and writes it once (a(l) is the block's skip and the input of
// the weight-gradient; nothing in the backward pass changes).  Decided from the layer table and the launcher's predicate alone:
// a consumer that is 3x3, strided, fed by a route / concatenation or a head (none of them has role 1) keeps the pass in front.
bool bn_in_next(const Layers& L, int l, int option, bool persist_on, int B, int S, bool with_skip) {
    if (option <= 0 || l < 0 || l + 1 >= (int)L.size()) return false;
    const auto &d = L[l], &dn = L[l + 1];
    if (!d.has_bn || !dn.has_bn || dn.role != 1 || dn.cin != d.cout || dn.in_div != d.out_div) return false;
    const int H = S / dn.in_div;
    return fv_op_conv_forward_takes_bn_stats_in(option, persist_on, B, H, H, dn.cin, dn.cout, dn.ksize, dn.stride, with_skip);
}
// the listing behind fv_train_bn_in_1x1_plan / fv_yolov3_train_bn_in_1x1_plan
void bn_in_plan(const Layers& L, int option, int B, int S, int32_t* folded) {
    for (int l = 0; l < (int)L.size(); ++l) folded[l] = bn_in_next(L, l, option, true, B, S, L[l].role == 2) ? 1 : 0;
}

// Training forward of BN layer l: the conv adds its column sums to the fp64 accumulator slots and the normalise pass reduces
// them itself -- two launches per layer (the per-operator API keeps the partial-row form + fv_bn_finalize).  `in` is a(l - 1) as
// the caller's graph names it; a(l) stays unwritten when layer l + 1 reads z(l) in both passes (the caller hands a(l) on as ever).
// (The pass of layer l: train_bn_pass; where bn_in_next says so it waits and runs inside the forward of layer l + 1.)
int train_bn_pass(const Train& t, int l, const float* skip) {
    const auto& d = t.L[l];
    const int Ho = t.S / d.out_div;
    const long long rows = (long long)t.B * Ho * Ho;
    return fv_ew_bn_act_stats(t.ctx, t.k.z[l], t.k.slots[l], fv_ew_bn_stat_slots(d.cout), (double)rows, t.params + d.gamma_off,
                              t.params + d.beta_off, BN_EPS, BN_MOMENTUM, t.k.mean[l], t.k.invstd[l], t.k.scale[l], t.k.shift[l],
                              t.bn_state + d.mean_off, t.bn_state + d.var_off, skip, t.k.a[l], rows, d.cout, LEAKY);
}
int train_bn_forward(const Train& t, int l, const float* in, const float* w, const float* skip) {
    const auto& d = t.L[l];
    const int H = t.S / d.in_div, Ho = t.S / d.out_div;
    const long long rows = (long long)t.B * Ho * Ho;
    const int ns = fv_ew_bn_stat_slots(d.cout);
    if (t.deferred >= 0) {   // the pass of layer l - 1 runs inside this conv: x is z(l - 1), and the kernel writes a(l - 1)
        const int lp = t.deferred;
        const auto& dp = t.L[lp];
        FV_REQUIRE(t.ctx, lp == l - 1 && in == t.k.a[lp], "train_bn_forward: layer %d does not read the layer whose normalise pass waits for it", l);
        const FvBnStatsIn bi{t.k.slots[lp], fv_ew_bn_stat_slots(dp.cout), (double)t.B * H * H, t.params + dp.gamma_off, t.params + dp.beta_off,
                             BN_EPS, BN_MOMENTUM, t.k.mean[lp], t.k.invstd[lp], t.k.scale[lp], t.k.shift[lp], t.bn_state + dp.mean_off,
                             t.bn_state + dp.var_off, t.deferred_skip, t.k.a[lp], LEAKY};
        t.deferred = -1; t.deferred_skip = nullptr;
        if (int rc = fv_op_conv_forward(t.ctx, t.k.z[lp], w, t.B, H, H, d.cin, d.cout, d.ksize, d.stride, FV_EPI_STATS, nullptr, nullptr, 0.f,
                                        nullptr, t.k.z[l], nullptr, nullptr, 1, t.k.slots[l], ns, nullptr, &bi)) return rc;
    } else {
        const bool from_z = early_in(t, l, in).fwd;
        const FvBnIn bi{from_z ? t.k.scale[l - 1] : nullptr, from_z ? t.k.shift[l - 1] : nullptr, LEAKY};
        if (int rc = fv_op_conv_forward(t.ctx, from_z ? t.k.z[l - 1] : in, w, t.B, H, H, d.cin, d.cout, d.ksize, d.stride, FV_EPI_STATS, nullptr,
                                        nullptr, 0.f, nullptr, t.k.z[l], nullptr, nullptr, 1, t.k.slots[l], ns, from_z ? &bi : nullptr)) return rc;
    }
    if (!skip && early_in(t, l + 1, t.k.a[l]).virt())
        return fv_ew_bn_stats_publish(t.ctx, t.k.slots[l], ns, (double)rows, t.params + d.gamma_off, t.params + d.beta_off, BN_EPS,
                                      BN_MOMENTUM, t.k.mean[l], t.k.invstd[l], t.k.scale[l], t.k.shift[l], t.bn_state + d.mean_off,
                                      t.bn_state + d.var_off, d.cout);
    if (bn_in_next(t.L, l, t.ctx->bn_in_1x1, t.ctx->conv1x1_persist, t.B, t.S, skip != nullptr)) {
        t.deferred = l; t.deferred_skip = skip;
        return FV_OK;
    }
    return train_bn_pass(t, l, skip);
}
// After the last train_bn_forward of a pass: a pass still waiting (the caller stopped in front of its reader) runs on its own.
int train_bn_forward_end(const Train& t) {
    if (t.deferred < 0) return FV_OK;
    const int l = t.deferred;
    const float* skip = t.deferred_skip;
    t.deferred = -1; t.deferred_skip = nullptr;
    return train_bn_pass(t, l, skip);
}

// What every training step enqueues first: the gradient vector and the accumulator slots (forward and backward) of each plan's
// kept tensors zeroed, then the weight images of this step -- the first layer's kernel packed into w0p and the transposed kernels
// for the data-gradients in kept[0]'s wt -- made once, whichever plans share them.
int train_step_begin(fv_ctx* ctx, const Layers& L, const float* params, float* grads, int64_t nparam,
                     const std::vector<const Kept*>& kept, float* w0p, int cpad) {
    FV_HIP(ctx, hipMemsetAsync(grads, 0, (size_t)nparam * sizeof(float), ctx->stream));
    for (const Kept* k : kept) FV_HIP(ctx, hipMemsetAsync(k->slots[0], 0, k->slots_bytes, ctx->stream));
    if (int rc = fv_ew_pad_rows(ctx, params + L[0].w_off, w0p, 32, 27, 32)) return rc;
    return transpose_weights(ctx, L, params, kept[0]->wt, cpad);
}

// Training forward of the Darknet-53 base L[0, nb) from x into t.k.a[nb - 1]; the caller ends the pass (train_bn_forward_end)
// where its own forward stops.
int base_train_forward(const Train& t, int nb, const float* x, const float* w0p) {
    const float* cur = x;
    const float* skip = nullptr;
    for (int l = 0; l < nb; ++l) {
        const auto& d = t.L[l];
        if (d.role == 1) skip = cur;
        if (int rc = train_bn_forward(t, l, cur, l == 0 ? w0p : t.params + d.w_off, d.role == 2 ? skip : nullptr)) return rc;
        cur = t.k.a[l];
    }
    return FV_OK;
}

// Every data-gradient also reduces d-beta / d-gamma of the BN layer whose output gradient it produces (conv.h FV_EPI_BNRED):
// that layer's BN-backward then is the apply pass alone (measured for every layer, also the 32/64-channel ones: fusing all of
// them 59.4 ms per step, none 61.0).  l < 0: no reduction (that gradient is not complete yet, or it is a concatenation's).
const FvBnRed* bn_red(const Train& t, int l, FvBnRed& b) {
    if (l < 0) return nullptr;
    b = FvBnRed{t.k.z[l], t.k.scale[l], t.k.shift[l], t.k.mean[l], t.k.invstd[l], t.k.bslots[l], fv_ew_bn_stat_slots(t.L[l].cout), LEAKY};
    return &b;
}

// The weight-gradients of the backward pass.  With the overlap on they run on the low-priority side stream: wgrad(l) needs only
// dz(l) and a saved forward activation, so the context's stream goes on with dgrad(l) and the next layer's BN-backward.  dz
// alternates between two buffers (slot = submission count & 1); a buffer is rewritten only after the weight-gradient that read
// it has signalled ev_wg[slot], which join() makes the context's stream wait for.
//
// A layer's gradient range [w_off, + kernel + (gamma, beta | bias)) is handed to the bucket callback once ev_wg[slot] of its
// weight-gradient has been waited for -- or, with fv_set_bucket_on_side, as soon as that weight-gradient is in the side stream's
// queue (the callback then works on the side stream).  The slots alternate strictly, so ranges are reported in submission
// order = reverse execution order = descending offsets.  EVERY weight-gradient, the heads' included, runs on the side stream: a
// range is never reported from a stream other than the one its gradient was made on (round 3 ran the head's on the compute
// stream and reported it at once: with a bucket smaller than the head's 221 KB a side-stream collective could have overtaken it).
struct WgradPipe {
    const Train& t;
    fv_bucket_fn on_bucket; void* user;
    float* dz[2];
    hipStream_t main_stream;
    bool ov, early;   // early: the callback fires at enqueue time and works on the side stream
    int slot = 0;
    struct Pending { bool on; int64_t off, cnt; } pend[2] = {{false, 0, 0}, {false, 0, 0}};

    WgradPipe(const Train& tr, fv_bucket_fn cb, void* u, float* dz0, float* dz1)
        : t(tr), on_bucket(cb), user(u), dz{dz0, dz1}, main_stream(tr.ctx->stream), ov(tr.ctx->overlap && tr.ctx->side),
          early(ov && tr.ctx->bucket_on_side) {}

    int join(int s) {
        if (!pend[s].on) return FV_OK;
        FV_HIP(t.ctx, hipStreamWaitEvent(main_stream, t.ctx->ev_wg[s], 0));
        if (on_bucket && !early) on_bucket(user, pend[s].off, pend[s].cnt);
        pend[s].on = false;
        return FV_OK;
    }
    // weight-gradient of layer l from its input xin and its output gradient dy (rows of ndy floats), in the current slot
    // (bn_in: xin is z(l - 1), normalised on load; bn_dy: dy is g(l) and the kernel forms dz(l) on load and writes d-beta / d-gamma)
    int submit(int l, const float* xin, const float* dy, int ndy, const FvBnIn* bn_in = nullptr, const FvBnDy* bn_dy = nullptr) {
        fv_ctx* ctx = t.ctx;
        const auto& d = t.L[l];
        const int H = t.S / d.in_div, s = slot;
        const int64_t cnt = (int64_t)d.cout * d.ksize * d.ksize * d.cin + (d.has_bn ? 2 : 1) * d.cout;
        slot ^= 1;
        if (!ov) {
            if (int rc = fv_op_conv_wgrad(ctx, xin, dy, t.B, H, H, d.cin, d.cout, ndy, d.ksize, d.stride, t.grads + d.w_off, bn_in, bn_dy)) return rc;
            if (on_bucket) on_bucket(user, d.w_off, cnt);
            return FV_OK;
        }
        FV_HIP(ctx, hipEventRecord(ctx->ev_dz[s], main_stream));
        FV_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_dz[s], 0));
        ctx->stream = ctx->side;
        const int rc = fv_op_conv_wgrad(ctx, xin, dy, t.B, H, H, d.cin, d.cout, ndy, d.ksize, d.stride, t.grads + d.w_off, bn_in, bn_dy);
        ctx->stream = main_stream;
        if (rc) return rc;
        // ev_wg is recorded BEFORE an early callback: it guards the reuse of the dz buffer, which needs the weight-gradient alone --
        // recorded after the callback it would make the compute stream wait for the collective the callback enqueued (the host
        // joins the side stream once, before Adam)
        FV_HIP(ctx, hipEventRecord(ctx->ev_wg[s], ctx->side));
        if (early && on_bucket) on_bucket(user, d.w_off, cnt);      // may enqueue a collective on the side stream
        pend[s] = Pending{true, d.w_off, cnt};
        return FV_OK;
    }
    int finish() {   // `slot` names the older of the two outstanding weight-gradients: ranges stay in descending order
        if (int rc = join(slot)) return rc;
        return join(slot ^ 1);
    }
};

// A layer without BN (a detection conv): its output gradient dy (padded to cpad channels; the bias gradient is already in
// grads) -> dW, and the gradient of its input a(lin) into g_out, reducing layer lin's d-beta/d-gamma.
int linear_layer_backward(WgradPipe& pipe, int l, int lin, const float* dy, int cpad, float* g_out) {
    const Train& t = pipe.t;
    const auto& d = t.L[l];
    const int H = t.S / d.in_div;
    if (int rc = pipe.join(pipe.slot)) return rc;
    if (int rc = pipe.submit(l, t.k.a[lin], dy, cpad)) return rc;
    FvBnRed b;
    return fv_op_conv_dgrad(t.ctx, dy, t.k.wt[l], t.B, H, H, d.cin, cpad, d.ksize, 1, nullptr, g_out, bn_red(t, lin, b));
}

// BN layer l: its output gradient g (d-beta/d-gamma already reduced into its slots unless !reduced) -> dz -> dW (side stream);
// then, unless g_out is NULL, the data-gradient into g_out (+ addend), reducing for layer lred.  xin is a(l - 1) as the graph names
// it (the weight-gradient reads z(l - 1) instead where early_in says so).
//
// A layer without a data-gradient whose reduction is done (the first layer) needs dz for its weight-gradient alone: with option
// "early_bn_fused" wgrad0_mfma.hip forms it on load from g and z, and no dz is written.  That launch reads g -- one of the
// caller's gradient buffers -- and z(l) on the SIDE stream, so the compute stream waits for it here, before anything after this
// layer can rewrite either (both outstanding weight-gradients are joined, the older first: ranges stay in descending order).
// d-beta / d-gamma then come from the side stream together with dW; the layer's range is reported after ev_wg as ever.
int bn_layer_backward(WgradPipe& pipe, int l, const float* g, bool reduced, const float* xin, float* g_out, const float* addend,
                      int lred) {
    const Train& t = pipe.t;
    const auto& d = t.L[l];
    const int H = t.S / d.in_div, Ho = t.S / d.out_div;
    const long long rows = (long long)t.B * Ho * Ho;
    if (int rc = pipe.join(pipe.slot)) return rc;
    const bool from_z = early_in(t, l, xin).wgrad;
    const FvBnIn bi{from_z ? t.k.scale[l - 1] : nullptr, from_z ? t.k.shift[l - 1] : nullptr, LEAKY};
    if (from_z) xin = t.k.z[l - 1];
    if (!g_out && reduced && (t.ctx->early_bn & FV_EARLY_DZ0) &&
        fv_op_conv_wgrad_takes_bn_dy(t.ctx, t.B, H, H, d.cin, d.cout, d.cout, d.ksize, d.stride)) {
        const FvBnDy bd{t.k.z[l], t.k.scale[l], t.k.shift[l], t.k.mean[l], t.k.invstd[l], t.k.bslots[l], fv_ew_bn_stat_slots(d.cout), LEAKY,
                        t.grads + d.beta_off, t.grads + d.gamma_off, t.accumulate_bn};
        if (int rc = pipe.submit(l, xin, g, d.cout, from_z ? &bi : nullptr, &bd)) return rc;
        return pipe.finish();
    }
    float* dz = pipe.dz[pipe.slot];
    if (int rc = fv_ew_bn_bwd(t.ctx, g, t.k.z[l], t.k.scale[l], t.k.shift[l], t.k.mean[l], t.k.invstd[l], rows, d.cout, LEAKY, nullptr,
                              nullptr, t.grads + d.beta_off, t.grads + d.gamma_off, dz, t.k.bslots[l], fv_ew_bn_stat_slots(d.cout),
                              reduced, t.accumulate_bn)) return rc;
    if (int rc = pipe.submit(l, xin, dz, d.cout, from_z ? &bi : nullptr)) return rc;
    if (!g_out) return FV_OK;
    FvBnRed b;
    return fv_op_conv_dgrad(t.ctx, dz, t.k.wt[l], t.B, H, H, d.cin, d.cout, d.ksize, d.stride, addend, g_out, bn_red(t, lred, b));
}

// Backward through the Darknet-53 base L[0, nb) from the gradient of its output in g[0]; g[1] holds the kept block gradient of a
// residual pair.  addend_at[l] (when given): a gradient of a(l) that arrived by another route, added where dgrad(l + 1) forms
// the gradient of a(l).  top_reduced: the top layer's d-beta / d-gamma were reduced by the launch that formed g[0] (a conv
// data-gradient with FV_EPI_BNRED); false: its BN-backward reduces them itself (g[0] came from elsewhere, net_fid.hip's dense layer).
int base_backward(WgradPipe& pipe, int nb, const float* x, float* const g[2], const std::vector<const float*>& addend_at,
                  bool top_reduced = true) {
    const Train& t = pipe.t;
    int ig = 0, ires = -1;
    for (int l = nb - 1; l > 0; --l) {
        const auto& d = t.L[l];
        if (d.role == 2) ires = ig;   // add(skip, x): the same gradient also reaches the skip input
        // dgrad overwrites the consumed gradient buffer g[ig] unless that is the kept block gradient
        const int iout = (ig == ires) ? 1 - ig : ig;
        const float* addend = d.role == 1 ? g[ires] : nullptr;
        if (!addend_at.empty() && addend_at[l - 1]) addend = addend_at[l - 1];
        if (int rc = bn_layer_backward(pipe, l, g[ig], l < nb - 1 || top_reduced, t.k.a[l - 1], g[iout], addend, l - 1)) return rc;
        ig = iout;
        if (d.role == 1) ires = -1;
    }
    return bn_layer_backward(pipe, 0, g[ig], true, x, nullptr, nullptr, -1);
}

}  // namespace
