"""FaceIdentifier on the GPU against a float64 restatement of the reference's model (face_identification.py:318-345, 72-76):
Dense(64, relu) + K.l2_normalize + triplet loss written out here in torch, the Darknet-53 base from oracle.net_oracle.forward.

Tolerances follow test_net_gpu.py: forward values within 4x of the error the same oracle makes in fp32 on the CPU; gradients in
relative L2 per tensor with the 2e-2 floor that LeakyReLU's kink needs (see that file's docstring)."""
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import face_identification as fi

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(S):
    if S not in _MODELS:
        _MODELS[S] = fi.FidModel(S, 0)
    m = _MODELS[S]
    m.grads = m.m = m.v = None
    m.iterations, m.bn_updates, m.bn_zero_debias = 0, 0, True
    return m


def _within(got, ref64, ref32, what, factor=4.0, floor=1e-6):
    e_gpu = (got.double() - ref64).abs().max().item()
    e_cpu = (ref32.double() - ref64).abs().max().item()
    lim = factor * e_cpu + floor * max(ref64.abs().max().item(), 1.0)
    assert e_gpu <= lim, '%s: gpu err %.3e > limit %.3e (cpu fp32 err %.3e)' % (what, e_gpu, lim, e_cpu)


def _grad_close(got, ref64, ref32, what, factor=6.0, floor=2e-2):
    n64 = ref64.double().norm().item()
    rel = (got.double() - ref64).norm().item() / max(n64, 1e-30)
    rel32 = (ref32.double() - ref64).norm().item() / max(n64, 1e-30)
    assert rel <= max(factor * rel32, floor), '%s: rel L2 err %.3e (cpu fp32 %.3e)' % (what, rel, rel32)


# ----------------------------------------------------------------------------- float64 restatement of the model
def dense_l2(feat, K, b):
    """Flatten -> Dense(relu) -> l2_normalize (TF 1.13: x * rsqrt(max(sum x^2, 1e-12)))."""
    pre = feat.reshape(feat.shape[0], -1) @ K + b
    r = torch.relu(pre)
    return pre, r * torch.rsqrt(torch.clamp((r * r).sum(-1, keepdim=True), min=1e-12))


def triplet_loss(ua, up, un, per_row=False):
    h = torch.sqrt(((ua - up) ** 2).sum(-1)) - torch.sqrt(((ua - un) ** 2).sum(-1)) + fi.ALPHA
    return h if per_row else torch.clamp(h, min=0.0).mean()


def towers(params, state, xs, S, training, ema_step=0):
    """The shared base over each input (BN moving-statistics updates chained a -> p -> n), dense + l2 -> ([u], [feat], new state)."""
    from oracle import net_oracle as no
    top = no.param_layout()[0][fi.NUM_BASE_LAYERS - 1]['name']
    k, b = fi.dense_offsets(S)
    K, bias = params[k:b].view(-1, 64), params[b:b + 64]
    us, feats = [], []
    for i, x in enumerate(xs):
        _, state, inter = no.forward(params, state, x, training=training, return_intermediates=True,
                                     ema_step=ema_step + i if ema_step else 0)
        feat = inter[top][1]
        feats.append(feat)
        us.append(dense_l2(feat, K, bias)[1])
    return us, feats, state


def fid_params(S, seed, dtype=torch.float64):
    """Detector base weights of the oracle with non-trivial BN parameters / moving statistics, a glorot dense kernel, a small
    random bias -- in the fv_fid_param_count layout."""
    from oracle import net_oracle as no
    p, s = no.init_params(seed, torch.float64)
    g = torch.Generator().manual_seed(seed + 100)
    for e in no.param_layout()[0]:
        if e['has_bn']:
            c = e['cout']
            p[e['gamma_off']:e['gamma_off'] + c] = 0.8 + 0.4 * torch.rand(c, generator=g, dtype=torch.float64)
            p[e['beta_off']:e['beta_off'] + c] = 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
            s[e['mean_off']:e['mean_off'] + c] = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
            s[e['var_off']:e['var_off'] + c] = 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
    k, b = fi.dense_offsets(S)
    F = fi.feature_size(S)
    out = torch.zeros(b + 64, dtype=torch.float64)
    out[:k] = p[:k]
    lim = np.sqrt(6.0 / (F + 64))
    out[k:b] = (torch.rand(F * 64, generator=g, dtype=torch.float64) * 2 - 1) * lim
    out[b:] = 0.05 * torch.randn(64, generator=g, dtype=torch.float64)
    return out, s


def _images(B, S, seed):
    return torch.rand((B, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _active_triplet(B, S, seed):
    """Negative = the anchor plus a little noise, positive = another image: the hinge is active for every triplet."""
    xa, xp = _images(B, S, seed), _images(B, S, seed + 1)
    xn = torch.clamp(xa + 0.02 * torch.randn(xa.shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64), 0, 1)
    return xa, xp, xn


# ----------------------------------------------------------------------------- 1. dense forward + finish
@pytest.mark.parametrize('F,M', [(173056, 5), (2048, 40)])
def test_dense_forward_and_finish(F, M):
    from face_vijnana_yolov3_amd._lib import lib, ptr
    m = _model(64)
    g = torch.Generator().manual_seed(F + M)
    X = torch.randn((M, F), generator=g)
    X[3] = 0                                                   # pre-activation = bias <= 0 everywhere: the row stays exactly 0
    W = (torch.rand((F, 64), generator=g) * 2 - 1) * float(np.sqrt(6.0 / (F + 64)))
    bias = -0.01 * torch.rand(64, generator=g)
    dev = m.dev
    Xd, Wd, bd = X.to(dev), W.to(dev), bias.to(dev)
    part = torch.empty(int(lib().fv_fid_dense_partial_floats(M, F)), device=dev)

    def run(rows):
        pre = torch.empty((rows.shape[0], 64), device=dev)
        out = torch.empty((rows.shape[0], 64), device=dev)
        rows = rows.contiguous()
        m.ctx.check(lib().fv_fid_dense_l2(m.ctx.handle, ptr(rows), rows.shape[0], F, ptr(Wd), ptr(bd), ptr(part), ptr(pre), ptr(out)),
                    'fv_fid_dense_l2')
        return pre.cpu(), out.cpu()

    pre, out = run(Xd)
    pre64, out64 = dense_l2(X.double(), W.double(), bias.double())
    absdot = X.double().abs() @ W.double().abs() + bias.double().abs()
    assert ((pre.double() - pre64).abs() <= 1e-5 * absdot + 1e-7).all()
    torch.testing.assert_close(out.double(), out64, rtol=0, atol=1e-5)
    norms = out.double().norm(dim=1)
    assert torch.equal(out[3], torch.zeros(64))
    keep = [i for i in range(M) if i != 3]
    assert ((norms[keep] - 1).abs() < 1e-5).all()
    pre2, out2 = run(Xd)
    assert torch.equal(out, out2) and torch.equal(pre, pre2)
    _, a = run(Xd[:2])
    _, b = run(Xd[2:])
    assert torch.equal(torch.cat([a, b]), out)


# ----------------------------------------------------------------------------- 2. extraction
@pytest.mark.parametrize('S,B', [(64, 1), (64, 3), (96, 1), (96, 3)])
def test_fid_extract_matches_oracle(S, B):
    m = _model(S)
    p64, s64 = fid_params(S, 11)
    x = _images(B, S, 12)
    (u64,), _, _ = towers(p64, s64, [x], S, training=False)
    (u32,), _, _ = towers(p64.float(), s64.float(), [x.float()], S, training=False)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    got = fi.FidExtractor(m).predict_device(x.float()).cpu()
    _within(got, u64, u32, 'fid S=%d B=%d' % (S, B))
    assert ((got.double().norm(dim=1) - 1).abs() < 1e-5).all()
    assert torch.equal(fi.FidExtractor(m).predict_device(x.float()).cpu(), got)           # bit-reproducible
    u8 = (x * 255).round().to(torch.uint8).numpy()
    np.testing.assert_array_equal(fi.FidExtractor(m).predict(u8), m.extract_device(torch.from_numpy(u8).float() / 255).cpu().numpy())


# ----------------------------------------------------------------------------- 3. training step
class _SlicedParams(object):
    """The flat parameter vector as the oracle reads it (slices only), each distinct slice a leaf of its own: autograd then keeps
    one small gradient per slice instead of summing a full-length gradient per use (~500 uses of 40.8M floats for three towers)."""

    def __init__(self, flat):
        self.flat, self.leaves = flat, {}

    def __getitem__(self, sl):
        key = (sl.start, sl.stop)
        if key not in self.leaves:
            self.leaves[key] = self.flat[sl].clone().requires_grad_(True)
        return self.leaves[key]

    def grad(self, loss):
        keys = list(self.leaves)
        gs = torch.autograd.grad(loss, [self.leaves[k] for k in keys], allow_unused=True)
        g = torch.zeros_like(self.flat)
        for (a, b), gk in zip(keys, gs):
            if gk is not None:
                g[a:b] += gk.reshape(-1)
        return g


def _oracle_step(p, s, xs, S, ema_step):
    sp = _SlicedParams(p)
    (ua, up, un), _, ns = towers(sp, s, xs, S, training=True, ema_step=ema_step)
    loss = triplet_loss(ua, up, un)
    return loss.detach(), sp.grad(loss), ns.detach(), triplet_loss(ua, up, un, per_row=True).detach()


@pytest.mark.parametrize('B', [1, 2])
def test_fid_train_step_matches_oracle(B):
    from oracle import net_oracle as no
    S = 64
    m = _model(S)
    p64, s64 = fid_params(S, 21 + B)
    xs = _active_triplet(B, S, 30 + B)
    l64, g64, ns64, h = _oracle_step(p64, s64, xs, S, ema_step=1)
    assert (h > 0.02).all(), h                                   # the hinge is active: every gradient is exercised
    l32, g32, ns32, _ = _oracle_step(p64.float(), s64.float(), [x.float() for x in xs], S, ema_step=1)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    loss = m.forward_backward(*[x.float() for x in xs]).item()
    assert m.bn_updates == 3
    assert abs(loss - l64.item()) <= 4 * abs(l32.item() - l64.item()) + 1e-5 * abs(l64.item())
    _within(m.state.cpu(), ns64, ns32, 'bn moving state after a -> p -> n')
    g = m.grads.cpu()
    for e in no.param_layout()[0][:fi.NUM_BASE_LAYERS]:
        sl = slice(e['w_off'], e['w_off'] + e['cout'] * e['k'] * e['k'] * e['cin'])
        _grad_close(g[sl], g64[sl], g32[sl], 'dW ' + e['name'])
        for nm in ('gamma_off', 'beta_off'):
            sl = slice(e[nm], e[nm] + e['cout'])
            _grad_close(g[sl], g64[sl], g32[sl], nm + ' ' + e['name'])
    k, b = fi.dense_offsets(S)
    _grad_close(g[k:b], g64[k:b], g32[k:b], 'dense kernel')
    _grad_close(g[b:b + 64], g64[b:b + 64], g32[b:b + 64], 'dense bias')
    assert len(g) == b + 64 and torch.isfinite(g).all()


# ----------------------------------------------------------------------------- 4. inactive hinge
def test_inactive_hinge_gives_zero_loss_and_gradients():
    """Dense layer built so that the anchor's ReLU units and the negative's are disjoint (distance sqrt 2), positive = anchor.
    Each batch repeats one image, so that every row of a tower has the same features."""
    S, B = 64, 2
    m = _model(S)
    p64, s64 = fid_params(S, 41)
    xa = _images(1, S, 42).expand(B, -1, -1, -1).contiguous()
    xn = _images(1, S, 43).expand(B, -1, -1, -1).contiguous()
    _, (fa, fn), _ = towers(p64, s64, [xa, xn], S, training=True)
    fa, fn = fa.reshape(B, -1).mean(0), fn.reshape(B, -1).mean(0)
    d, mid = fa - fn, (fa + fn) / 2
    c = 1.0 / (d @ d)
    k, b = fi.dense_offsets(S)
    K = torch.cat([d[:, None].expand(-1, 32), -d[:, None].expand(-1, 32)], dim=1) * c
    p64[k:b] = K.reshape(-1)
    p64[b:b + 32] = -c * (mid @ d)
    p64[b + 32:b + 64] = c * (mid @ d)
    (ua, up, un), _, _ = towers(p64, s64, [xa, xa, xn], S, training=True)
    assert (triplet_loss(ua, up, un, per_row=True) < -0.5).all()
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    st0 = m.state.clone()
    loss = m.forward_backward(xa.float(), xa.float(), xn.float()).item()
    assert loss == 0.0
    assert torch.count_nonzero(m.grads).item() == 0
    assert not torch.equal(m.state, st0)


# ----------------------------------------------------------------------------- 5. progress
def test_training_makes_progress_on_a_fixed_batch():
    S, B = 64, 2
    m = _model(S)
    p64, s64 = fid_params(S, 51)
    xs = [x.float() for x in _active_triplet(B, S, 52)]
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    losses = [m.train_on_batch(*xs, 1e-5, 0.99, 0.99).item() for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert losses[-1] < losses[0], losses


# ----------------------------------------------------------------------------- 6. end to end
def test_face_identifier_train_end_to_end(tmp_path, monkeypatch):
    import pandas as pd
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    S = 64
    rng = np.random.RandomState(1)
    os.makedirs(tmp_path / 'subject_faces')
    rows, crops = [], []
    for sid in range(3):
        base = rng.randint(0, 256, (S, S, 3))
        for j in range(2):
            img = np.clip(base + rng.randint(-20, 21, (S, S, 3)), 0, 255).astype(np.uint8)
            name = 'f%d_%d.png' % (sid, j)
            Image.fromarray(img).save(tmp_path / 'subject_faces' / name)
            rows.append(dict(subject_id=sid, face_file=name)); crops.append(img)
    pd.DataFrame(rows).to_csv(tmp_path / 'subject_image_db.csv')
    conf = {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(tmp_path), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64),
                            hps=dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2)),
            'fd_conf': {}}
    ident = fi.FaceIdentifier(conf)
    assert ident._fd is None                                    # the detector is made on first use only
    ident.train()
    assert conf['fi_conf']['hps']['step'] == 2 and ident.model.iterations == 2     # 3 triplets: a batch of 2 and a short one
    assert os.path.exists('face_identifier.h5') and os.path.exists('img_triplet_pairs.pickle')
    crops = np.asarray(crops)
    want = ident.fid_extractor.predict(crops)
    conf['fi_conf']['model_loading'] = True
    again = fi.FaceIdentifier(conf)
    np.testing.assert_array_equal(again.fid_extractor.predict(crops), want)
    assert want.shape == (6, 64) and np.isfinite(want).all()

