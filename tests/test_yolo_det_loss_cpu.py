"""hps['loss'] = 'yolo' without a GPU: data.det_loss_conf, header / binding / export of the new entry points, facts about the
float64 reference the GPU tests compare against (tests/yolo_det_loss_ref.py), and train()'s epoch line over recorders."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yolo_det_loss_ref as ref
from face_vijnana_yolov3_amd import data, face_detection, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- 1. data.det_loss_conf
def test_absent_or_fd_keeps_todays_loss():
    assert data.det_loss_conf(None) is None and data.det_loss_conf('fd') is None
    assert data.det_loss_conf(None, 'single') is None and data.det_loss_conf('fd', 'single') is None


def test_yolo_defaults_and_overrides():
    c = data.det_loss_conf('yolo')
    assert c == dict(box_loss='giou', ignore_thresh=0.5, box_weight=1.0, noobj_weight=1.0, max_boxes=256,
                     anchors=[[float(v) for v in row] for row in data.YOLO_ANCHORS])
    assert data.det_loss_conf({'yolo': {}}) == c
    d = data.det_loss_conf({'yolo': {'box_loss': 'l2', 'ignore_thresh': 1, 'box_weight': 2, 'noobj_weight': 0.5, 'max_boxes': 1024}})
    assert (d['box_loss'], d['ignore_thresh'], d['box_weight'], d['noobj_weight'], d['max_boxes']) == ('l2', 1.0, 2.0, 0.5, 1024)
    assert all(isinstance(d[k], float) for k in ('ignore_thresh', 'box_weight', 'noobj_weight'))


@pytest.mark.parametrize('value', ['mse', 'YOLO', True, 1, {'yolo': 'giou'}, {'yolo': {}, 'fd': {}}, {'fd': {}}, ['yolo'],
                                   {'yolo': {'iou': 'giou'}}, {'yolo': {'box_loss': 'ciou'}}, {'yolo': {'box_loss': 1}},
                                   {'yolo': {'ignore_thresh': 0}}, {'yolo': {'ignore_thresh': 1.01}}, {'yolo': {'ignore_thresh': '0.5'}},
                                   {'yolo': {'box_weight': 0}}, {'yolo': {'box_weight': float('inf')}}, {'yolo': {'noobj_weight': -1}},
                                   {'yolo': {'noobj_weight': float('nan')}}, {'yolo': {'noobj_weight': True}}, {'yolo': {'max_boxes': 0}},
                                   {'yolo': {'max_boxes': 1025}}, {'yolo': {'max_boxes': 16.0}}, {'yolo': {'max_boxes': True}}])
def test_every_refusal(value):
    with pytest.raises(ValueError, match='fd_conf.hps.loss'):
        data.det_loss_conf(value)


@pytest.mark.parametrize('value', ['yolo', {'yolo': {'box_loss': 'l2'}}])
def test_yolo_with_the_single_scale_head_is_refused_before_a_device_is_touched(value, monkeypatch):
    with pytest.raises(ValueError, match='three_scale'):
        data.det_loss_conf(value, 'single')
    from face_vijnana_yolov3_amd import engine
    monkeypatch.setattr(engine, 'Engine', lambda *a, **k: pytest.fail('a device was touched'))
    conf = dict(raw_data_path='.', hps=dict(loss=value), nn_arch=dict(image_size=416), model_loading=False)
    with pytest.raises(ValueError, match='three_scale'):
        face_detection.FaceDetector(conf)


# ----------------------------------------------------------------------------- 2. header, binding, export
NEW = ('fv_yolo_det_scratch_bytes', 'fv_yolo_det_loss_grad', 'fv_yolov3_train_step_det', 'fv_yolov3_train_workspace_head')


def test_header_binding_and_export_agree():
    from face_vijnana_yolov3_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fv_hotpath.h')).read(), flags=re.S)
    L = _lib.lib()
    assert L.fv_abi_version() == 4
    for name in NEW:
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, header, flags=re.S)
        assert m, name
        assert len(getattr(L, name).argtypes) == len([a for a in m.group(1).split(',') if a.strip()]), name
    # the struct: field for field
    m = re.search(r'typedef struct \{([^}]*)\}\s*fv_yolo_det_conf;', header, flags=re.S)
    fields = [re.sub(r'\[\d+\]', '', f.split()[-1]) for f in m.group(1).split(';') if f.strip()]
    assert fields == [f[0] for f in _lib.YoloDetConf._fields_] == ['box_loss', 'ignore_thresh', 'box_weight', 'noobj_weight', 'max_boxes', 'anchors']
    assert ctypes.sizeof(_lib.YoloDetConf) == 4 * 5 + 4 * 18
    assert re.search(r'#define FV_DET_BOX_L2 0', header) and re.search(r'#define FV_DET_BOX_GIOU 1', header)
    assert data.DET_BOX_LOSSES == ('l2', 'giou')
    # fv_yolov3_train_step keeps its signature; the new scratch is sized on its own
    assert len(L.fv_yolov3_train_step.argtypes) == 17 and len(L.fv_yolov3_train_step_det.argtypes) == 21
    assert L.fv_yolo_det_scratch_bytes(16, 416, 256) > 16 * 256 * 32
    for bad in ((0, 416, 256), (1, 400, 256), (1, 416, 0), (1, 416, 1025)):
        assert L.fv_yolo_det_scratch_bytes(*bad) == 0


def test_argument_checks_need_no_device():
    """FV_ERR_INVALID comes back before anything is launched: a NULL context is refused outright."""
    from face_vijnana_yolov3_amd import _lib
    L = _lib.lib()
    c = _lib.YoloDetConf()
    assert L.fv_yolo_det_loss_grad(None, None, None, 1, 64, 1, 32, ctypes.byref(c), 1.0, None, 0, None, None, None) == -1


# ----------------------------------------------------------------------------- 3. facts about the reference
@pytest.mark.parametrize('S', [96, 416])
def test_gather_returns_the_boxes_the_encoder_placed(S):
    """Random faces through data.encode_gt_three_scale; the list gathered from the float64 targets is, up to order, the set of
    letterboxed boxes the encoder was given (centre clamped as the encoder clamps it), within 1e-9 px."""
    rng = np.random.default_rng(S)
    h, w = 480, 640
    for trial in range(5):
        faces = [[float(rng.integers(0, w - 200)), float(rng.integers(0, h - 200)), float(rng.integers(8, 200)), float(rng.integers(8, 200))]
                 for _ in range(int(rng.integers(1, 12)))]
        ts = data.encode_gt_three_scale(faces, h, w, S)
        want = {}
        for x1, y1, x2, y2, xc, yc, m, T in data._placed_centres(faces, h, w, S, None):
            bw, bh = (x2 - x1 + 1) / m * T, (y2 - y1 + 1) / m * T
            best, best_iou = None, -1.0
            for (s, b) in data.YOLO_ANCHORS_DECODED:
                aw, ah = data.YOLO_ANCHORS[s][2 * b], data.YOLO_ANCHORS[s][2 * b + 1]
                inter = min(bw, aw) * min(bh, ah)
                if inter / (bw * bh + aw * ah - inter) > best_iou:
                    best, best_iou = (s, b), inter / (bw * bh + aw * ah - inter)
            s, b = best
            cell = 32 >> s
            cx, cy = xc // cell, yc // cell
            px = min(max((xc - cx * cell) / cell, 0.5 / cell), 1 - 0.5 / cell); py = min(max((yc - cy * cell) / cell, 0.5 / cell), 1 - 0.5 / cell)
            want[(s, cy, cx, b)] = ((cx + px) * cell, (cy + py) * cell, bw, bh)       # later rows overwrite, as in the encoder
        lists, counts = ref.gather([torch.from_numpy(t)[None] for t in ts], S, 1, data.YOLO_ANCHORS)
        assert counts == [len(want)]
        got = lists[0].numpy()
        assert np.abs(got - np.asarray([want[k] for k in sorted(want)])).max() <= 1e-9


@pytest.mark.parametrize('box_loss', ['l2', 'giou'])
def test_the_gradient_passes_gradcheck(box_loss):
    """A 32 x 32 image (grids 1 / 2 / 4, 63 slots, two classes) with three planted boxes; predictions near the targets so
    that ignored and penalised slots both occur."""
    conf = data.det_loss_conf({'yolo': {'box_loss': box_loss, 'max_boxes': 4, 'box_weight': 2.0, 'noobj_weight': 0.5}})
    S, ncls, B = 32, 2, 1
    g = torch.Generator().manual_seed(5)
    ts = [torch.zeros((B, 1 << s, 1 << s, 3, 7), dtype=torch.float64) for s in range(3)]
    ys = [torch.randn((B, 1 << s, 1 << s, 3, 7), dtype=torch.float64, generator=g) * 0.5 for s in range(3)]
    for (b, s, r, c, a, tw, th) in ((0, 0, 0, 0, 1, -2.5, -2.6), (0, 2, 2, 3, 0, 0.2, -0.1), (0, 1, 1, 0, 2, -1.5, -2.0)):
        ts[s][b, r, c, a] = torch.tensor([0.3, -0.4, tw, th, 1.0, 0.0, 1.0], dtype=torch.float64)
        ys[s][b, r, c, :, :4] = ts[s][b, r, c, a, :4] + torch.randn((3, 4), dtype=torch.float64, generator=g) * 0.2
        ys[s][b, r, c, :, 2] += torch.log(torch.tensor([data.YOLO_ANCHORS[s][2 * a] / data.YOLO_ANCHORS[s][2 * k] for k in range(3)]))
        ys[s][b, r, c, :, 3] += torch.log(torch.tensor([data.YOLO_ANCHORS[s][2 * a + 1] / data.YOLO_ANCHORS[s][2 * k + 1] for k in range(3)]))
    ys = [y.reshape(B, y.shape[1], y.shape[2], 21) for y in ys]
    ts = [t.reshape(B, t.shape[1], t.shape[2], 21) for t in ts]
    _, stats, detail = ref.det_loss(ys, ts, S, ncls, conf, detail=True)
    best = torch.cat([b[~p] for b, p in zip(detail['best'], detail['pos'])])
    assert stats[4] == 3 and stats[5] >= 2 and int((best <= 0.5).sum()) >= 2
    # nothing flips inside the 1e-6 probe step
    assert float((best - 0.5).abs().min()) > 1e-4 and float(torch.cat(detail['margin']).min()) > 1e-4
    ys = [y.requires_grad_(True) for y in ys]
    assert torch.autograd.gradcheck(lambda a, b, c: ref.det_loss([a, b, c], ts, S, ncls, conf)[0], ys, eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=True)


def test_an_all_empty_batch_gives_only_noobj_terms():
    conf = data.det_loss_conf('yolo')
    ys, ts = ref.planted_case(64, (0, 0), 1, 1, data.YOLO_ANCHORS)
    loss, dys, stats = ref.det_loss_grad(ys, ts, 64, 1, conf)
    want = sum(float(ref.bce(torch.from_numpy(y).double().reshape(-1, 6)[:, 4], torch.zeros(())).sum()) for y in ys) / 2
    assert abs(loss - want) <= 1e-12 * want and stats[0] == stats[1] == stats[3] == 0 and stats[4:] == [0, 0, 0.0, 0, 0, 0, 0, 0.0]
    for g, y in zip(dys, ys):
        assert float(g.reshape(-1, 6)[:, [0, 1, 2, 3, 5]].abs().max()) == 0
        assert float((g.reshape(-1, 6)[:, 4] - torch.sigmoid(torch.from_numpy(y).double().reshape(-1, 6)[:, 4]) / 2).abs().max()) <= 1e-15


def test_the_cap_cuts_the_list_in_slot_order_and_counts_what_it_drops():
    conf = data.det_loss_conf({'yolo': {'max_boxes': 4}})
    _, ts = ref.planted_case(64, (5, 4), 1, 1, data.YOLO_ANCHORS)
    full, counts = ref.gather([torch.from_numpy(t) for t in ts], 64, 1, conf['anchors'])
    cut, _ = ref.gather([torch.from_numpy(t) for t in ts], 64, 1, conf['anchors'], 4)
    assert counts == [5, 4] and [len(l) for l in cut] == [4, 4] and torch.equal(cut[0], full[0][:4])
    ys, _ = ref.planted_case(64, (5, 4), 1, 1, data.YOLO_ANCHORS)
    assert ref.det_loss(ys=[torch.from_numpy(y) for y in ys], ts=ts, image_size=64, ncls=1, conf=conf)[1][9:11] == [5, 1]


# ----------------------------------------------------------------------------- 4. train()'s epoch line over recorders
class _Sequence(object):
    def __init__(self, raw_data_path, hps, nn_arch, grid, cell_image_size):
        self.hps = hps

    def __len__(self):
        return 3


class _Feeder(object):
    def __init__(self, seq, world, rank, threads):
        pass

    def set_epoch(self, epoch):
        pass

    def close(self):
        pass


class _Trainer(object):
    def __init__(self, model, world_size=1, rank=0):
        pass

    def merged_loss(self, loss, weight=None):
        return loss

    def max_over_ranks(self, value):
        return value

    def shutdown(self):
        pass


class _Model(object):
    def __init__(self, epochs):
        self.epochs, self.saved, self.det_loss = list(epochs), [], None

    def take_det_epoch(self):
        return self.epochs.pop(0)

    def save(self, path):
        self.saved.append(path)


def _detector(monkeypatch, loss, epochs):
    monkeypatch.setattr(parallel, 'DataParallelTrainer', _Trainer)
    monkeypatch.setattr(face_detection, 'BatchFeeder', _Feeder)

    def run(engine, trainer, feeder, indices, image_size, hp, after_step=None):
        for k in range(len(indices)):
            after_step(k, 0.5, (None, None, 1.0, None))
    monkeypatch.setattr(face_detection, 'run_pipelined', run)
    fd = object.__new__(face_detection.FaceDetector)
    fd.hps = dict(epochs=len(epochs), lr=1e-3, beta_1=0.9, beta_2=0.999, loader_threads=1, loss=loss)
    fd.raw_data_path, fd.nn_arch, fd.grid, fd.cell_image_size, fd.image_size = '.', dict(head='three_scale'), 3, 32, 96
    fd.world = 1; fd.rank = 0
    fd.det_loss = data.det_loss_conf(loss, 'three_scale')
    fd.model = _Model(epochs)
    fd.TrainingSequence = _Sequence
    return fd


def _sums(**kw):
    return np.asarray([kw.get(k, 0.0) for k in data.DET_STATS], np.float64)


def test_train_prints_one_line_per_epoch(monkeypatch, capsys):
    e0 = (_sums(box=3.0, obj=1.5, noobj=6.0, cls=0.75, positives=8, ignored=100, iou_sum=2.0, iou_gt_50=2, iou_gt_75=1, max_count=3), 3, 1008)
    e1 = (_sums(box=1.5, obj=0.75, noobj=3.0, cls=0.3, positives=8, ignored=250, iou_sum=6.0, iou_gt_50=6, iou_gt_75=4, max_count=3), 3, 1008)
    fd = _detector(monkeypatch, 'yolo', [e0, e1])
    fd.train()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('yolo loss')]
    assert lines == ['yolo loss - box: 1.0000 - obj: 0.5000 - noobj: 2.0000 - cls: 0.2500 - mean IoU: 0.2500 - recall@0.5: 0.2500 - '
                     'recall@0.75: 0.1250 - ignored: 0.1000',
                     'yolo loss - box: 0.5000 - obj: 0.2500 - noobj: 1.0000 - cls: 0.1000 - mean IoU: 0.7500 - recall@0.5: 0.7500 - '
                     'recall@0.75: 0.5000 - ignored: 0.2500']
    assert fd.model.saved == [face_detection.FaceDetector.MODEL_PATH]


def test_train_without_the_key_prints_no_such_line_and_never_asks_for_stats(monkeypatch, capsys):
    fd = _detector(monkeypatch, None, [None])
    monkeypatch.setattr(_Model, 'take_det_epoch', lambda self: pytest.fail('stats were read'))
    fd.train()
    out = capsys.readouterr().out
    assert 'yolo loss' not in out and out.count('Epoch') == 1


def test_train_raises_when_the_cap_dropped_a_box(monkeypatch):
    fd = _detector(monkeypatch, {'yolo': {'max_boxes': 2}}, [(_sums(positives=9, max_count=5, dropped=3), 3, 1008)])
    with pytest.raises(ValueError, match=r'max_boxes = 2 .*5 assigned boxes'):
        fd.train()
    assert fd.model.saved == []
