"""fv_yolo_det_loss_grad and fv_yolov3_train_step_det (the YOLOv3 detection loss of the three-scale head)
against tests/yolo_det_loss_ref.py (torch-CPU float64, gradient by autograd) on planted inputs: images with 0, 1, exactly
max_boxes = 4 and 5 boxes (one dropped by the cap), positives on every scale and two in one cell, predictions on both sides of
the ignore threshold, saturated logits, tw / th = +-30 at the clamp."""
import numpy as np
import pytest
import torch

import yolo_det_loss_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
GIOU_FACTOR = 1.0       # the kernel is fp64 inside and rounds once: it may not be worse than the all-float32 evaluation


def _conf(box_loss, **over):
    from face_vijnana_yolov3_amd import data
    return data.det_loss_conf({'yolo': dict(dict(box_loss=box_loss, max_boxes=4), **over)})


# image_size, boxes per image, classes, c_pad, box loss, seed of the planted inputs (chosen so that check_conditions holds)
CASES = [
    (64, (5,), 1, 32, 'giou', 1),
    (64, (0, 4), 4, 32, 'l2', 2),
    (96, (1, 5, 4), 1, 32, 'l2', 3),
    (96, (4, 1, 0), 80, 256, 'giou', 4),
    (64, (1, 4), 80, 256, 'l2', 5),
    (96, (4, 5, 1), 4, 32, 'giou', 6),
]
_cache = {}


def check_conditions(conf, detail, giou):
    """What the comparison needs of the inputs: no slot's best IoU within 1e-6 of the ignore threshold, no positive's IoU within
    1e-9 of the recall thresholds, no GIoU min / max tie within 1e-9, and at least 5 % of the unassigned slots on either side of
    the threshold.  -> a list of violations."""
    thr = ref.f32(conf['ignore_thresh'])
    bad = []
    best = torch.cat([b[~p] for b, p in zip(detail['best'], detail['pos'])])
    if float((best - thr).abs().min()) <= 1e-6:
        bad.append('best IoU at the ignore threshold')
    share = float((best > thr).double().mean())
    if not 0.05 <= share <= 0.95:
        bad.append('ignored share %.3f' % share)
    pio = torch.cat(detail['pos_iou'])
    if pio.numel() and float(torch.minimum((pio - 0.5).abs(), (pio - 0.75).abs()).min()) <= 1e-9:
        bad.append('positive IoU at a recall threshold')
    if giou and pio.numel() and float(torch.cat(detail['margin']).min()) <= 1e-9:
        bad.append('GIoU tie')
    return bad


def _reference(case):
    """The planted inputs of a case and their float64 reference (and float32 evaluation), computed once."""
    if case not in _cache:
        from face_vijnana_yolov3_amd import data
        S, counts, ncls, cpad, box_loss, seed = case
        conf = _conf(box_loss)
        ys, ts = ref.planted_case(S, counts, ncls, seed, data.YOLO_ANCHORS)
        loss, dys, stats, detail = ref.det_loss_grad(ys, ts, S, ncls, conf, detail=True)
        _, dys32, _ = ref.det_loss_grad(ys, ts, S, ncls, conf, dtype=torch.float32)
        _cache[case] = dict(conf=conf, ys=ys, ts=ts, loss=loss, dys=dys, dys32=dys32, stats=stats, detail=detail)
    return _cache[case]


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _run(ctx, r, case, loss_weight=1.0):
    from face_vijnana_yolov3_amd import ops
    S, counts, ncls, cpad, _, _ = case
    B = len(counts)
    yd = [torch.from_numpy(y).cuda().reshape(-1, y.shape[-1]) for y in r['ys']]
    td = [torch.from_numpy(t).cuda().reshape(-1, t.shape[-1]) for t in r['ts']]
    dy3 = [torch.full((y.shape[0], cpad), float('nan'), device='cuda') for y in yd]
    loss, dys, stats = ops.yolo_det_loss_grad(ctx, yd, td, B, S, ncls, cpad, r['conf'], loss_weight, dy3=dy3)
    torch.cuda.synchronize()
    return loss.cpu(), [d.cpu() for d in dys], stats.cpu()


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%s-%d-%d-%s' % (c[0], 'x'.join(map(str, c[1])), c[2], c[3], c[4]))
def test_loss_grad_and_stats_match_the_float64_reference(ctx, case):
    S, counts, ncls, cpad, box_loss, _ = case
    r = _reference(case)
    assert not check_conditions(r['conf'], r['detail'], box_loss == 'giou')
    assert r['stats'][9] == max(counts) and r['stats'][10] == sum(max(0, c - 4) for c in counts) and r['stats'][4] == sum(counts)
    loss, dys, stats = _run(ctx, r, case)
    E3 = 3 * (5 + ncls)
    print('case %r: loss %.9g (ref %.9g), stats %s' % (case, loss.item(), r['loss'], [float(v) for v in stats]))
    assert abs(loss.item() - r['loss']) <= EPS * abs(r['loss'])
    for k, (got, want) in enumerate(zip(stats.tolist(), r['stats'])):
        if k >= 4 and k != 6:
            assert got == want, (ref.STATS[k], got, want)              # counts: exact
        else:
            assert abs(got - want) <= EPS * abs(want), (ref.STATS[k], got, want)
    for s, (got, want, want32) in enumerate(zip(dys, r['dys'], r['dys32'])):
        want = want.reshape(-1, E3)
        assert torch.all(got[:, E3:] == 0), 'padding columns of scale %d' % s
        got = got[:, :E3].double()
        assert torch.isfinite(got).all()
        err = (got - want).abs()
        tol = EPS * want.abs() + 1e-30
        if box_loss == 'giou':
            # the box entries of the assigned slots pass through the GIoU: against the float32 evaluation of the reference
            pos = r['detail']['pos'][s].reshape(-1)                    # (rows * 3,)
            e5 = err.reshape(-1, 5 + ncls); w5 = want.reshape(-1, 5 + ncls); w32 = want32.double().reshape(-1, 5 + ncls)
            if pos.any():
                e_gpu = float(e5[pos][:, :4].max()); e_32 = float((w32[pos][:, :4] - w5[pos][:, :4]).abs().max())
                print('  scale %d GIoU box gradient: max abs error %.3e, float32 evaluation %.3e' % (s, e_gpu, e_32))
                assert e_gpu <= GIOU_FACTOR * e_32, (s, e_gpu, e_32)
            assert torch.all(got.reshape(-1, 5 + ncls)[~pos][:, :4] == 0)
            t5 = tol.reshape(-1, 5 + ncls)
            assert torch.all(e5[:, 4:] <= t5[:, 4:]), (s, float((e5[:, 4:] - t5[:, 4:]).max()))
        else:
            assert torch.all(err <= tol), (s, float((err / (want.abs() + 1e-300)).max()))


def test_two_runs_are_bit_identical_and_loss_weight_scales_the_gradient(ctx):
    case = CASES[3]
    r = _reference(case)
    a = _run(ctx, r, case)
    b = _run(ctx, r, case)
    q = _run(ctx, r, case, loss_weight=0.25)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[0], q[0]) and torch.equal(a[2], q[2])          # the reported loss and the stats are unweighted
    for full, quarter in zip(a[1], q[1]):
        normal = full.abs() >= 2.0 ** -120
        assert normal.any() and torch.equal(quarter[normal], full[normal] * 0.25)


def test_an_all_empty_batch_has_only_noobj_terms(ctx):
    """No box anywhere: nothing is listed, nothing ignored (so the 5 % condition of the other cases cannot hold here)."""
    case = (96, (0,), 4, 32, 'giou', 7)
    r = _reference(case)
    loss, dys, stats = _run(ctx, r, case)
    assert abs(loss.item() - r['loss']) <= EPS * abs(r['loss'])
    st = stats.tolist()
    assert st[0] == 0 and st[1] == 0 and st[3] == 0 and st[4:] == [0.0] * 8 and abs(st[2] - r['stats'][2]) <= EPS * r['stats'][2]
    for got, want in zip(dys, r['dys']):
        want = want.reshape(-1, 27)
        assert torch.all((got[:, :27].double() - want).abs() <= EPS * want.abs() + 1e-30) and torch.all(got[:, 27:] == 0)
        assert torch.all(got[:, :27].reshape(-1, 9)[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0)


@pytest.mark.parametrize('bad', [dict(ignore_thresh=0.0), dict(ignore_thresh=1.5), dict(box_weight=0.0), dict(box_weight=float('inf')),
                                 dict(noobj_weight=-1.0), dict(noobj_weight=float('nan')), dict(max_boxes=0), dict(max_boxes=1025),
                                 dict(box_loss=7), dict(c_pad=17), dict(loss_weight=0.0), dict(scratch=8)])
def test_bad_arguments_are_refused_before_any_launch(ctx, bad):
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import FvError
    S, B, ncls = 64, 1, 1
    conf = dict(_conf('giou'))
    over = dict(bad)
    cpad, lw, scratch = over.pop('c_pad', 32), over.pop('loss_weight', 1.0), over.pop('scratch', None)
    conf.update(over)
    yd = [torch.zeros((B * (2 << s) ** 2, 18), device='cuda') for s in range(3)]
    dy3 = [torch.full((y.shape[0], cpad), float('nan'), device='cuda') for y in yd]
    if scratch is not None:
        scratch = torch.zeros(scratch, dtype=torch.float64, device='cuda')
    elif not 1 <= conf['max_boxes'] <= 1024:
        scratch = torch.zeros(1 << 14, dtype=torch.float64, device='cuda')
    with pytest.raises(FvError):
        ops.yolo_det_loss_grad(ctx, yd, yd, B, S, ncls, cpad, conf, lw, dy3=dy3, scratch=scratch)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(d).all()) for d in dy3)


def test_train_step_det_is_the_step_with_the_operator_as_its_loss_stage(ctx):
    """fv_yolov3_train_step_det at 64x64, batch 2, 27 channels: activations and BN state bit-equal to fv_yolov3_train_step's; its
    loss and dy are the operator's on the head outputs the step left in its workspace; the detection convs' bias gradients are
    the column sums of dy."""
    from face_vijnana_yolov3_amd import data, ops
    from face_vijnana_yolov3_amd._lib import FvError
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    from oracle import net_oracle as no
    out_ch, B, S, ncls = 27, 2, 64, 4
    p64, s64 = no.yolov3_init(21, out_ch, torch.float64)
    x = torch.rand((B, S, S, 3), generator=torch.Generator().manual_seed(3))
    _, ts = ref.planted_case(S, (4, 1), ncls, 8, data.YOLO_ANCHORS)
    ts = [torch.from_numpy(t) for t in ts]
    conf = _conf('giou')
    kept = {}
    for name, det in (('fd', None), ('det', conf)):
        m = Yolov3(0, out_channels=out_ch)
        m.set_params(p64.float(), s64.float())
        m.det_loss = det
        loss = m.forward_backward(x, ts, loss_weight=0.5).clone()
        torch.cuda.synchronize()
        # per BN layer the pre-BN output z and the batch statistics / scale / shift that turn it into the activation (the
        # activation itself is not materialised for every layer: the halo kernels of the first layers form it on load)
        acts = [m._train_tensor(B, S, l, code).clone() for l, d in enumerate(m.layers) if d['has_bn'] for code in (0, 2, 3, 4, 5)]
        kept[name] = dict(model=m, loss=loss, state=m.state.clone(), acts=acts, ys=[m.head_tensor(B, S, s).clone() for s in range(3)])
    a, b = kept['fd'], kept['det']
    assert torch.equal(a['state'], b['state']) and all(torch.equal(u, v) for u, v in zip(a['ys'], b['ys']))
    assert len(a['acts']) == 5 * 72 and all(torch.equal(u, v) for u, v in zip(a['acts'], b['acts']))
    m = b['model']
    td = [t.cuda().reshape(-1, out_ch) for t in ts]
    loss, dys, stats = ops.yolo_det_loss_grad(ctx, b['ys'], td, B, S, ncls, 32, conf, 0.5)
    assert torch.equal(loss, b['loss']) and torch.equal(stats, m.det_stats) and float(stats[4]) == 5.0
    assert a['loss'].item() != b['loss'].item()
    det_convs = [d for d in m.layers if not d['has_bn']]
    assert [d['darknet_index'] for d in det_convs] == [81, 93, 105]
    for s, d in enumerate(det_convs):
        assert torch.equal(m.head_tensor(B, S, s, grad=True), dys[s])
        assert torch.equal(m.grads[d['beta_off']:d['beta_off'] + out_ch], ops.colsum(ctx, dys[s], out_ch))
    # and the totals the epoch line is made of
    sums, steps, slots = m.take_det_epoch()
    assert steps == 1 and slots == B * 63 * 4 and np.array_equal(sums, stats.cpu().numpy()) and m.take_det_epoch() is None
