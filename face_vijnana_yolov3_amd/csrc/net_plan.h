// The FaceDetector network and the carving of its workspace, shared by the schedules that run its Darknet-53 base: net.hip
// (the detector: fv_forward_infer, fv_train_step) and net_fid.hip (the FaceIdentifier: three towers of the same base).
#pragma once
#include "schedule.h"

namespace {

constexpr int HEAD_C = 6;             // nn_arch.bb_info_c_size
constexpr int HEAD_PAD = 32;

struct Net {
    std::vector<fv_layer_desc> L;
    int64_t nparam = 0, nstate = 0;
    Net() {
        auto add = [&](int idx, int k, int s, int cin, int cout, int role, int in_div) {
            fv_layer_desc d{};
            d.darknet_index = idx; d.ksize = k; d.stride = s; d.cin = cin; d.cout = cout; d.has_bn = 1; d.role = role;
            d.in_div = in_div; d.out_div = in_div * s;
            d.w_off = nparam; nparam += (int64_t)cout * k * k * cin;
            d.gamma_off = nparam; nparam += cout;
            d.beta_off = nparam; nparam += cout;
            d.mean_off = nstate; nstate += cout;
            d.var_off = nstate; nstate += cout;
            L.push_back(d);
        };
        int idx = 0, div = 1, cin = 32;
        add(idx++, 3, 1, 3, 32, 0, div);
        const int stages[5][2] = {{64, 1}, {128, 2}, {256, 8}, {512, 8}, {1024, 4}};
        for (auto& st : stages) {
            const int cout = st[0];
            add(idx++, 3, 2, cin, cout, 0, div);
            div *= 2;
            for (int b = 0; b < st[1]; ++b) {
                add(idx++, 1, 1, cout, cout / 2, 1, div);
                add(idx++, 3, 1, cout / 2, cout, 2, div);
                ++idx;  // the Darknet shortcut layer owns an index
            }
            cin = cout;
        }
        fv_layer_desc h{};
        h.darknet_index = -1; h.ksize = 3; h.stride = 1; h.cin = 1024; h.cout = HEAD_C; h.has_bn = 0; h.role = 3;
        h.in_div = div; h.out_div = div;
        h.w_off = nparam; nparam += (int64_t)HEAD_C * 9 * 1024;
        h.gamma_off = -1; h.beta_off = nparam; nparam += HEAD_C;
        h.mean_off = h.var_off = -1;
        L.push_back(h);
    }
};
const Net& net() { static Net n; return n; }

struct Plan {
    int B, S, nl;
    Kept k;
    float *w0p, *yhat, *dyp, *G[4], *loss, *slab, *tail, *mse_part, *head_slab;
    size_t tail_floats;
    size_t bytes;
};

// Carve the workspace (base == NULL: size query only).  weight_images = false (training only): no packed first-layer kernel and
// no transposed kernels are carved -- the caller points w0p / k.wt at those of another plan of the same step.
Plan make_plan(void* base, int B, int S, bool training, bool weight_images = true) {
    const Net& N = net();
    Plan p{};
    p.B = B; p.S = S; p.nl = (int)N.L.size();
    Carver c(base);
    const int nb = p.nl - 1;
    p.k.resize(p.nl);
    size_t max_act = 0;
    for (int l = 0; l < nb; ++l) max_act = std::max(max_act, (size_t)B * (S / N.L[l].out_div) * (S / N.L[l].out_div) * N.L[l].cout);
    {   // per-channel BN vectors of all layers are contiguous (channel offset = mean_off / 2)
        float* sc_all = c.take((size_t)N.nstate / 2);
        float* sh_all = c.take((size_t)N.nstate / 2);
        for (int l = 0; l < nb; ++l) {
            const auto& d = N.L[l];
            p.k.scale[l] = sc_all ? sc_all + d.mean_off / 2 : nullptr;
            p.k.shift[l] = sh_all ? sh_all + d.mean_off / 2 : nullptr;
            if (training) { p.k.mean[l] = c.take(d.cout); p.k.invstd[l] = c.take(d.cout); }
        }
    }
    p.w0p = weight_images ? c.take(32 * 32) : nullptr;
    const int G = S / 32;
    p.yhat = c.take((size_t)B * G * G * HEAD_C);
    if (training) {
        for (int l = 0; l < nb; ++l) {
            const auto& d = N.L[l];
            size_t elems = (size_t)B * (S / d.out_div) * (S / d.out_div) * d.cout;
            p.k.z[l] = c.take(elems); p.k.a[l] = c.take(elems);
        }
        for (int l = 1; l < p.nl && weight_images; ++l) {
            const auto& d = N.L[l];
            int cp = d.has_bn ? d.cout : HEAD_PAD;
            p.k.wt[l] = c.take((size_t)d.cin * d.ksize * d.ksize * cp);
        }
        p.k.carve_slots(c, N.L);
        p.dyp = c.take((size_t)B * G * G * HEAD_PAD);
        // G[0], G[1]: activation gradients g(l) = dL/d a(l) (the one being consumed / produced and the kept block gradient of a
        // residual pair); G[2], G[3]: dz of the even / odd layers (a weight-gradient on the side stream may still read one)
        for (int i = 0; i < 4; ++i) p.G[i] = c.take(max_act);
        p.loss = c.take(64);
        p.mse_part = c.take(fv_ew_mse_scratch_floats());
        // the head conv has 6 output channels: 53 tiles of 288 K steps -- K-split it like the batch-1 inference path
        const int head_ks = fv_conv_choose_ksplit(B * G * G, HEAD_C, 9 * 1024 / 32);
        p.head_slab = c.take_some(head_ks > 1 ? (size_t)head_ks * B * G * G * HEAD_C : 0);
    } else {
        for (int i = 0; i < 3; ++i) p.G[i] = c.take(max_act);
        p.slab = c.take_some(ksplit_slab_floats(N.L, B, S));
    }
    p.tail_floats = tail_split_floats(N.L, B, S, training, HEAD_PAD);
    p.tail = c.take_some(p.tail_floats);
    p.bytes = c.off;
    return p;
}

}  // namespace
