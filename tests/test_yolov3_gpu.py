"""Secondary path on the GPU: the full three-scale YOLOv3 forward against the
torch-CPU oracle, and decode_netout + correct_yolo_boxes + do_nms against the golden vectors minted
from the reference's own functions (tests/golden/decode_netout.npz)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model():
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    return Yolov3(0, out_channels=255)


def test_layout_matches_oracle(model):
    from oracle import net_oracle as no
    ents, n, ns = no.yolov3_layout(255)
    assert model.n_params == n == 61949149 and model.n_state == ns == 52608 and len(model.layers) == len(ents) == 75
    for d, e in zip(model.layers, ents):
        assert (d['darknet_index'], d['ksize'], d['cin'], d['cout'], d['w_off']) == (e['idx'], e['k'], e['cin'], e['cout'], e['w_off'])
        if e['has_bn']:
            assert (d['gamma_off'], d['beta_off'], d['mean_off'], d['var_off']) == (e['gamma_off'], e['beta_off'], e['mean_off'], e['var_off'])
        else:
            assert d['beta_off'] == e['bias_off'] and d['role'] == 5


@pytest.mark.parametrize('B,S', [(1, 96), (2, 64)])
def test_three_scale_forward_matches_oracle(model, B, S):
    from oracle import net_oracle as no
    p64, s64 = no.yolov3_init(11, 255, torch.float64)
    x = torch.rand((B, S, S, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    r64 = no.yolov3_forward(p64, s64, x)
    r32 = no.yolov3_forward(p64.float(), s64.float(), x.float())
    model.set_params(p64.float(), s64.float())
    ys = model.predict_device(x.float())
    torch.cuda.synchronize()
    for y, a, b, name in zip(ys, r64, r32, ('yolo_82', 'yolo_94', 'yolo_106')):
        assert tuple(y.shape) == tuple(a.shape)
        e_gpu = (y.cpu().double() - a).abs().max().item()
        e_cpu = (b.double() - a).abs().max().item()
        assert e_gpu <= 4 * e_cpu + 1e-6 * max(1.0, a.abs().max().item()), (name, e_gpu, e_cpu)


def test_darknet_full_weights_roundtrip(model, tmp_path):
    """Full-model .weights ordering (conv 0..105, yd.py:90-121): write a synthetic file in that
    order from the oracle layout and read it back through Yolov3.load_darknet."""
    import struct
    from oracle import net_oracle as no
    ents, n, ns = no.yolov3_layout(255)
    p, s = no.yolov3_init(5, 255, torch.float32)
    p, s = p.numpy(), s.numpy()
    path = str(tmp_path / 'y.weights')
    with open(path, 'wb') as f:
        f.write(struct.pack('iii', 0, 2, 0) + struct.pack('q', 0))
        for e in sorted(ents, key=lambda e: e['idx']):
            k, cin, cout = e['k'], e['cin'], e['cout']
            if e['has_bn']:
                for arr, o in ((p, e['beta_off']), (p, e['gamma_off']), (s, e['mean_off']), (s, e['var_off'])):
                    f.write(arr[o:o + cout].tobytes())
            else:
                f.write(p[e['bias_off']:e['bias_off'] + cout].tobytes())
            f.write(p[e['w_off']:e['w_off'] + cout * k * k * cin].reshape(cout, k, k, cin).transpose(0, 3, 1, 2).tobytes())
    used = model.load_darknet(path)
    assert used == n + ns
    assert np.array_equal(model.params.cpu().numpy(), p) and np.array_equal(model.state.cpu().numpy(), s)


@pytest.mark.parametrize('fixture', ['decode_netout.npz', 'decode_netout_coco80.npz', 'decode_netout_else.npz:portrait',
                                     'decode_netout_else.npz:square'])
def test_decode_nms_matches_reference_golden(model, golden_dir, fixture):
    """fv_yolo_decode_nms against vectors minted by the reference's decode_netout / correct_yolo_boxes /
    do_nms (4 classes on a 1440x1920 image; 80 classes on a 375x500 image; 20 classes on a 1920x1440 and a
    416x416 image with NMS at 0.45: the `else` branch of correct_yolo_boxes).  Candidate set, order and
    objectness: exact.  Integer corners: exact, except where the reference's own pre-truncation value --
    recomputed here from the golden's float corners -- sits within a few float32 ulps of an integer: the
    kernel's exp is the correctly rounded one, NumPy's SIMD float32 exp may differ by 1 ulp, and int()
    turns that into a whole pixel exactly there and nowhere else.  Suppression pattern: exactly what the
    reference's greedy per-class NMS (restated in oracle/host_oracle.py and pinned by the same golden)
    gives on the DEVICE's integer boxes -- so a corner that moved is the only way it can differ."""
    from face_vijnana_yolov3_amd.yolov3 import decode_nms
    from oracle import host_oracle
    from test_oracle_golden import load_decode_case
    netouts, g, ih, iw, post, nms_thresh = load_decode_case(golden_dir, fixture)
    ys = [torch.from_numpy(a).cuda() for a in netouts]
    res = decode_nms(model.ctx, ys[0], ys[1], ys[2], (ih, iw), (416, 416), g['anchors'].tolist(), 0.5, nms_thresh)
    pre = g['pre']
    n = post.shape[0]
    assert res['boxes'].shape[0] == n                                   # same candidates, same order
    np.testing.assert_allclose(res['objness'].cpu().numpy(), post[:, 4], rtol=3e-7, atol=0)
    got = res['boxes'].cpu().numpy().astype(np.int64)
    want = post[:, :4].astype(np.int64)
    # the reference's pre-truncation values (yd.py:389-404), float32 like its np.float32 corners
    if (416.0 / iw) < (416.0 / ih):
        new_w, new_h = 416.0, (ih * 416.0) / iw
    else:
        new_h, new_w = 416.0, (iw * 416.0) / ih
    x_off, x_sc = (416 - new_w) / 2. / 416, new_w / 416
    y_off, y_sc = (416 - new_h) / 2. / 416, new_h / 416
    f = pre[:, :4].astype(np.float32)
    v = np.stack([(f[:, 0] - np.float32(x_off)) / np.float32(x_sc) * np.float32(iw), (f[:, 1] - np.float32(y_off)) / np.float32(y_sc) * np.float32(ih),
                  (f[:, 2] - np.float32(x_off)) / np.float32(x_sc) * np.float32(iw), (f[:, 3] - np.float32(y_off)) / np.float32(y_sc) * np.float32(ih)], 1)
    assert np.array_equal(v.astype(np.float64).astype(np.int64), want)   # the restated chain reproduces the golden ints
    d = got - want
    bad = np.argwhere(d != 0)
    span = np.maximum(np.abs(v).max(1), 1.0)                             # ulp scale: the box's largest coordinate in pixels
    for (i, k) in bad:
        assert abs(d[i, k]) == 1, (i, k, d[i, k])
        dist = abs(v[i, k] - np.round(v[i, k]))
        assert dist <= 8 * np.spacing(np.float32(span[i])), 'corner %d of box %d moved a pixel away from any integer boundary (v=%r)' % (k, i, v[i, k])
    assert len(bad) <= max(2, 0.005 * 4 * n)
    # suppression pattern == the reference's NMS run on the device's integer boxes and the reference's probabilities
    rows = [list(got[i]) + [float(pre[i, 4])] + [float(c) for c in pre[i, 5:]] for i in range(n)]
    host_oracle.do_nms(rows, nms_thresh)
    exp_zero = np.array([r[5:] for r in rows]) == 0
    cls = res['classes'].cpu().numpy()
    assert np.array_equal(cls == 0, exp_zero)
    if len(bad) == 0:
        assert np.array_equal(cls == 0, post[:, 5:] == 0)
    nz = (cls != 0) & (post[:, 5:] != 0)
    np.testing.assert_allclose(cls[nz], post[:, 5:][nz], rtol=3e-7, atol=0)
    # do_nms really suppressed something in this fixture
    assert ((pre[:, 5:] != 0) & (post[:, 5:] == 0)).sum() > 10


def test_decode_nms_properties_at_full_size(model):
    """416 input, COCO shape (80 classes): size-independent properties of the per-class NMS."""
    from face_vijnana_yolov3_amd.yolov3 import decode_nms
    from oracle import postproc as opp
    rng = np.random.default_rng(1)
    ys = []
    for gsz in (13, 26, 52):
        a = rng.normal(0, 1.0, (gsz, gsz, 255)).astype(np.float32)
        a.reshape(gsz, gsz, 3, 85)[..., 4] -= 1.5
        a.reshape(gsz, gsz, 3, 85)[..., 2:4] *= 0.3
        ys.append(torch.from_numpy(a).cuda())
    r1 = decode_nms(model.ctx, *ys, (1440, 1920), (416, 416), obj_thresh=0.5, nms_thresh=0.5)
    r2 = decode_nms(model.ctx, *ys, (1440, 1920), (416, 416), obj_thresh=0.5, nms_thresh=0.5)
    for k in r1:
        assert torch.equal(r1[k], r2[k])                                 # idempotent / deterministic
    n = r1['boxes'].shape[0]
    assert 100 < n <= 13 * 13 + 2 * 26 * 26 + 52 * 52
    b = r1['boxes'].cpu().numpy(); c = r1['classes'].cpu().numpy()
    for cl in (0, 17, 79):                                               # survivors of a class never overlap >= th
        idx = np.nonzero(c[:, cl] > 0)[0][:400]
        ii, jj = np.triu_indices(len(idx), 1)
        iou = opp.bbox_iou(b[idx][ii], b[idx][jj])
        assert not np.any(iou >= 0.5)


@pytest.mark.parametrize('nclass,gsz', [(1, 13), (4, 13), (80, 13), (1, 3)])
def test_batched_decode_nms_equals_the_per_image_calls(model, nclass, gsz):
    """fv_yolo_decode_nms_batch (one launch pair per batch; yd.py:596-604 loops over the images) returns, image by image, exactly
    what the per-image call -- the one pinned by the reference goldens above -- returns: boxes, objectness, class probabilities
    after NMS and the count, bit for bit; images with no candidate included."""
    from face_vijnana_yolov3_amd.yolov3 import decode_nms, decode_nms_batch
    rng = np.random.default_rng(nclass * 100 + gsz)
    B, C = 5, 3 * (5 + nclass)
    ys = []
    for g in (gsz, 2 * gsz, 4 * gsz):
        a = rng.normal(0, 1.0, (B, g, g, C)).astype(np.float32)
        a5 = a.reshape(B, g, g, 3, 5 + nclass)
        a5[..., 4] -= 1.0
        a5[..., 2:4] *= 0.3
        a5[3, ..., 4] = -20.0                                    # image 3: nothing passes the objectness threshold
        ys.append(torch.from_numpy(a).cuda())
    S = 32 * gsz
    rb = decode_nms_batch(model.ctx, ys[0], ys[1], ys[2], (S, S), (S, S), obj_thresh=0.5, nms_thresh=0.45)
    cnt = rb['count'].cpu().numpy()
    assert cnt[3] == 0 and cnt.max() > 10
    for b in range(B):
        r1 = decode_nms(model.ctx, ys[0][b], ys[1][b], ys[2][b], (S, S), (S, S), obj_thresh=0.5, nms_thresh=0.45)
        n = int(cnt[b])
        assert r1['boxes'].shape[0] == n
        assert torch.equal(rb['boxes'][b, :n], r1['boxes']) and torch.equal(rb['objness'][b, :n], r1['objness'])
        assert torch.equal(rb['classes'][b, :n], r1['classes'])


# ------------------------------------------------------------------------------------------ training
def _train_setup(out_ch, B, S, seed):
    from oracle import net_oracle as no
    p64, s64 = no.yolov3_init(seed, out_ch, torch.float64)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((B, S, S, 3), dtype=torch.float64, generator=g)
    tg = []
    for d in (32, 16, 8):
        t = torch.rand((B, S // d, S // d, out_ch), dtype=torch.float64, generator=g)
        t4 = t.view(B, S // d, S // d, 3, out_ch // 3)
        t4[..., 4] = (t4[..., 4] > 0.8).double(); t4[..., 5:] = (t4[..., 5:] > 0.7).double()     # objectness / class targets in {0, 1}
        tg.append(t)
    return p64, s64, x, tg


@pytest.mark.parametrize('out_ch,B,S', [(27, 2, 64), (255, 1, 64), (27, 2, 96), (27, 3, 128), (255, 1, 96)])
def test_three_scale_train_step_matches_oracle(out_ch, B, S):
    """fv_yolov3_train_step: forward with training-mode BN in all 72 BN layers, the three-scale loss, backward through
    the heads, both upsample+concat routes and the base -- against the float64 oracle evaluated on the device's side of
    every LeakyReLU kink (tests/test_net_gpu.py explains the method): loss, BN moving state and EVERY gradient tensor
    (relative L2 <= max(6 x the float32 oracle's own error, 4e-5)).  The 64x64 cases are the smallest grids the graph
    admits (2x2 cells per image at the coarsest scale: 8- and 4-row BatchNorm reductions); round 2 saw ONE run of
    [27-2-64] with dW conv_0 at 2.6e-2 on a work-tree that held the first draft of the direct first-layer kernel -- the
    committed kernels measure 9.7e-5 there against 1.1e-4 for float32 on the CPU (tools/diag_small.py prints every
    layer's forward statistics and gradient errors; gpurun_out/r3_diag1.txt), with every schedule switch toggled."""
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    from oracle import net_oracle as no
    model = Yolov3(0, out_channels=out_ch)
    p64, s64, x, tg = _train_setup(out_ch, B, S, 21)
    model.set_params(p64.float(), s64.float())
    loss = model.forward_backward(x.float(), [t.float() for t in tg])
    torch.cuda.synchronize()
    pos = [m.cpu() for m in model.leaky_slopes_taken(B, S)]
    l64, g64, ns64 = no.yolov3_train_step_grads(p64, s64, x, tg, out_ch, positive=pos)
    l32, g32, ns32 = no.yolov3_train_step_grads(p64.float(), s64.float(), x.float(), [t.float() for t in tg], out_ch, positive=pos)
    assert abs(loss.item() - l64.item()) <= 4 * abs(l32.item() - l64.item()) + 2e-6 * abs(l64.item())
    e_gpu = (model.state.cpu().double() - ns64).abs().max().item(); e_cpu = (ns32.double() - ns64).abs().max().item()
    assert e_gpu <= 4 * e_cpu + 1e-6 * max(1.0, ns64.abs().max().item())
    ents, n, _ = no.yolov3_layout(out_ch)
    g = model.grads.cpu().double()
    worst = 0.0
    bad = []
    for e in ents:
        k, cin, cout = e['k'], e['cin'], e['cout']
        parts = [('dW', slice(e['w_off'], e['w_off'] + cout * k * k * cin))]
        parts += [('dgamma', slice(e['gamma_off'], e['gamma_off'] + cout)), ('dbeta', slice(e['beta_off'], e['beta_off'] + cout))] if e['has_bn'] \
            else [('dbias', slice(e['bias_off'], e['bias_off'] + cout))]
        for nm, sl in parts:
            n64 = g64[sl].norm().item()
            rel = (g[sl] - g64[sl]).norm().item() / max(n64, 1e-30)
            rel32 = (g32[sl].double() - g64[sl]).norm().item() / max(n64, 1e-30)
            if rel > max(6 * rel32, 4e-5):
                bad.append('%s %s: rel L2 err %.3e (cpu fp32 %.3e)' % (nm, e['name'], rel, rel32))
            worst = max(worst, rel)
    print('three-scale step out_ch=%d B=%d S=%d: worst rel-L2 %.2e' % (out_ch, B, S, worst))
    assert not bad, '%d tensors off: %s' % (len(bad), '; '.join(bad[:6]))


def test_three_scale_side_stream_overlap_equals_serial():
    """fv_set_option("overlap") in fv_yolov3_train_step: the weight-gradients on the side stream vs everything on one stream --
    the same bucket protocol (contiguous ranges in descending offset order that cover the gradient vector exactly), the same loss
    and the same gradients up to the float-atomic summation order inside dW (tests/test_net_gpu.py has the FaceDetector's)."""
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    out_ch, B, S = 18, 2, 64
    model = Yolov3(0, out_channels=out_ch)
    p64, s64, x, tg = _train_setup(out_ch, B, S, 31)
    res = []
    try:
        for on in (True, False):
            model.ctx.set_overlap(on)
            model.set_params(p64.float(), s64.float())
            buckets = []
            loss = model.forward_backward(x.float(), [t.float() for t in tg], on_bucket=lambda o, c: buckets.append((o, c)))
            torch.cuda.synchronize()
            res.append((loss.item(), model.grads.clone(), list(buckets)))
    finally:
        model.ctx.set_overlap(True)
    n = model.grads.numel()
    assert res[0][2] == res[1][2]
    ranges = res[0][2]
    assert ranges[0][0] + ranges[0][1] == n and ranges[-1][0] == 0
    assert all(hi[0] == lo[0] + lo[1] for hi, lo in zip(ranges, ranges[1:]))
    assert abs(res[0][0] - res[1][0]) <= 1e-6 * abs(res[1][0])
    d = (res[0][1] - res[1][1]).abs().max().item()
    assert d <= 1e-5 * res[1][1].abs().max().item() + 1e-9, d


def test_three_scale_training_reduces_the_loss():
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    model = Yolov3(0, out_channels=27)
    p64, s64, x, tg = _train_setup(27, 4, 96, 5)
    model.set_params(p64.float(), s64.float())
    xs, ts = x.float().cuda(), [t.float().cuda() for t in tg]
    losses = [model.train_on_batch(xs, ts, 1e-4, 0.9, 0.999).item() for _ in range(40)]
    assert all(np.isfinite(losses)) and bool(torch.isfinite(model.params).all())
    assert losses[-1] < 0.8 * losses[0], (losses[0], losses[-1])
