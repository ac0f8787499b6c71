"""The detection metric on the GPU (csrc/det_metric.hip) against its numpy restatement (tests/det_metric_ref.py) -- rows, assigned
IoUs, ranking and running counts for equality, AP within the rounding of an N-term sum -- cal_mAP_sweep_device against the golden
minted from the reference's cal_mAP_fd, and FaceDetector.train() with hps['validate'] end to end."""
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import det_metric as dm
from face_vijnana_yolov3_amd._lib import Context, FvError
import det_metric_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', ctx.device))


# ----------------------------------------------------------------------------- fv_det_rows_from_nms
def test_rows_from_nms_bit_for_bit(ctx):
    """Counts 0, 1 and 61 (cut to 60) at K = 64; a w > h, an h > w and a square geometry; a box that clips at every border."""
    from face_vijnana_yolov3_amd.data import letterbox_geometry
    S, K = 96, 64
    rng = np.random.default_rng(0)
    hw = [(480, 640), (640, 480), (416, 416)]
    geom = np.array([(h, w) + tuple(letterbox_geometry(h, w, S)[2:]) for h, w in hw], np.int32)
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1]):                       # every geometry meets every count
        g = geom[perm]
        count = np.array([0, 1, 61], np.int32)
        lo = rng.integers(0, S - 1, (3, K, 2)); hi = lo + rng.integers(0, S, (3, K, 2))
        boxes = np.concatenate([lo, np.minimum(hi, S - 1)], axis=2).astype(np.int32)
        boxes[:, 0] = (0, 0, S - 1, S - 1)                                # over the padding on both sides: every clamp acts
        boxes[2, 1] = (S - 1, S - 1, S - 1, S - 1)
        score = rng.uniform(0.01, 1.0, (3, K)).astype(np.float32)
        score[2, 2] = np.float32(1.0)
        res = dict(boxes=_dev(boxes, ctx), score=_dev(score, ctx), count=_dev(count, ctx))
        rows, nrows = dm.rows_from_nms(ctx, res, _dev(g, ctx), S)
        want_rows, want_nrows = ref.rows_from_nms(boxes, score, count, g, S)
        assert list(want_nrows) == [0, 1, 60]
        assert np.array_equal(nrows.cpu().numpy(), want_nrows)
        assert rows.cpu().numpy().tobytes() == want_rows.tobytes()


# ----------------------------------------------------------------------------- fv_det_match_rows
def _match_cases():
    rng = np.random.default_rng(1)

    def boxes(n, span):
        return np.concatenate([np.round(rng.uniform(0, span, (n, 2)), 1), np.round(rng.uniform(5, 60, (n, 2)), 1)], axis=1)
    cases = [(boxes(g, 300 if g < 1000 else 500), boxes(d, 300 if g < 1000 else 500))
             for g, d in ((0, 3), (3, 0), (1, 1), (5, 60), (300, 7), (4096, 60))]
    cases.append((boxes(4, 100), boxes(5, 100) + np.array([1000, 1000, 0, 0])))          # nothing overlaps: flag clear
    dup_g = boxes(3, 50)
    cases.append((np.concatenate([dup_g, dup_g, dup_g[:1]]), np.concatenate([dup_g[::-1], dup_g, boxes(4, 50)])))   # IoU ties
    cases.append((np.array([[0., 0, 10, 10], [20, 20, 10, 10]]),
                  np.array([[10., 0, 10, 10], [10, 10, 10, 10], [0, 10, 10, 10], [30, 30, 5, 5], [20, 30, 10, 10],
                            [5, 5, -3, 10], [5, 5, -3, -3]])))      # touching: zero extents; inverted boxes: negative extents and their product
    cases.append((np.array([[5., 5, 0, 0], [5, 5, 10, 10], [50, 50, 0, 10]]),
                  np.array([[5., 5, 0, 0], [50, 50, 0, 10], [5, 5, 10, 10], [5, 5, 0, 0]])))                            # zero area: nan
    return cases


def test_match_rows_exact(ctx):
    cases = _match_cases()
    n = len(cases)
    rows = np.zeros((n, ref.ROWS, 5)); nrows = np.zeros(n, np.int32)
    offs = [0]
    for i, (g, d) in enumerate(cases):
        nrows[i] = len(d)
        rows[i, :len(d), :4] = d
        offs.append(offs[-1] + len(g))
    gt = np.concatenate([g for g, _ in cases]).reshape(-1, 4)
    offs = np.asarray(offs, np.int64)
    want_iou, want_flag = ref.match_rows(rows, nrows, gt, offs)
    assert list(want_flag[[0, 1, 3, 4, 5, 6, 7]]) == [0, 0, 1, 1, 1, 0, 1]
    assert list(want_iou[8, :7]) == [-1.0] * 6 + [0.09] and np.isnan(ref.iou_matrix(*cases[9])[0, 0])
    iou, flag = dm.match_rows(ctx, _dev(rows, ctx), _dev(nrows, ctx), _dev(gt, ctx), _dev(offs, ctx), 4096)
    assert np.array_equal(flag.cpu().numpy(), want_flag)
    got = iou.cpu().numpy()
    for i in range(n):
        assert got[i].tobytes() == want_iou[i].tobytes(), i
    assert (want_iou[5, :60] > 0).sum() > 30                              # the 4096 x 60 image really assigns


def test_match_rows_refuses_4097_boxes(ctx, tmp_path):
    rows = _dev(np.zeros((1, ref.ROWS, 5)), ctx); nrows = _dev(np.array([1], np.int32), ctx)
    gt = _dev(np.ones((4097, 4)), ctx); off = _dev(np.array([0, 4097], np.int64), ctx)
    with pytest.raises(FvError, match=r'\(-1\).*ground-truth'):           # FV_ERR_INVALID
        dm.match_rows(ctx, rows, nrows, gt, off, 4097)
    import pandas as pd
    df = pd.DataFrame({'FACE_ID': range(4097), 'FILE': 'a.jpg', 'SUBJECT_ID': 1, 'FACE_X': 1.0, 'FACE_Y': 1.0, 'FACE_WIDTH': 2.0,
                       'FACE_HEIGHT': 2.0})
    with pytest.raises(ValueError, match='validation.csv'):
        dm.group_ground_truth(df, ['a.jpg'], str(tmp_path / 'validation.csv'))


# ----------------------------------------------------------------------------- fv_det_ap_sweep
def _sweep_case(N, ties, seed):
    """N counted detections in images of up to 60 rows, with two images whose flag is clear (their rows count nowhere) between."""
    rng = np.random.default_rng(seed)
    sizes = [60] * (N // 60) + ([N % 60] if N % 60 else [])
    p = len(sizes) // 2
    sizes.insert(p, 17); sizes.append(60)                                 # the two dropped images
    dropped = (p, len(sizes) - 1)
    n = len(sizes)
    rows = np.zeros((n, ref.ROWS, 5)); nrows = np.asarray(sizes, np.int32)
    iou = np.full((n, ref.ROWS), -1.0); flag = np.ones(n, np.int32)
    for i in dropped:
        flag[i] = 0
    if ties:
        values = rng.uniform(0.01, 1, 50).astype(np.float32)
        conf = values[rng.integers(0, 50, (n, ref.ROWS))]
    else:
        conf = (rng.permutation(n * ref.ROWS).astype(np.float32) + 1).reshape(n, ref.ROWS) / np.float32(n * ref.ROWS + 1)
        assert len(np.unique(conf)) == conf.size
    rows[:, :, 4] = conf.astype(np.float64)
    v = rng.uniform(0, 1, (n, ref.ROWS))
    iou[:] = np.where(rng.random((n, ref.ROWS)) < 0.3, -1.0, v)
    return rows, nrows, iou, flag


@pytest.mark.parametrize('ties', [True, False])
@pytest.mark.parametrize('N', [0, 1, 2, 1023, 1024, 1025, 70001])
def test_ap_sweep_against_numpy(ctx, N, ties):
    rows, nrows, iou, flag = _sweep_case(N, ties, N + int(ties))
    conf, ious = ref.compact(rows, nrows, iou, flag)
    assert len(conf) == N
    gt_count = N // 2 + 3
    d = [_dev(a, ctx) for a in (rows, nrows, iou, flag)]
    for T in (1, 10, 16):
        ths = [float(t) for t in (np.arange(0.5, 1.0, 0.05) if T == 10 else np.linspace(0.05, 1.0, T) if T == 16 else [0.5])]
        out = dm.ap_sweep(ctx, d[0], d[1], d[2], d[3], ths, gt_count, want_curve=True)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        again = {k: v.cpu().numpy() for k, v in dm.ap_sweep(ctx, d[0], d[1], d[2], d[3], ths, gt_count, want_curve=True).items()}
        order, counts, ap, prec, rec = ref.ap_sweep(conf, ious, ths, gt_count)
        assert int(got['n_det'][0]) == N
        assert np.array_equal(got['order'][:N], order)
        assert np.array_equal(got['counts'][:, :N], counts)
        assert np.array_equal(got['result'][1], prec) and np.array_equal(got['result'][2], rec)
        err = np.abs(got['result'][0] - ap)
        print('N %d T %d ties %s: largest |AP - trapezoid| %.3e (bound %.3e)' % (N, T, ties, err.max(), N * 2.0 ** -53 * 4))
        assert (err <= N * 2.0 ** -53 * 4).all()
        assert got['result'].tobytes() == again['result'].tobytes() and got['n_det'].tobytes() == again['n_det'].tobytes()
        assert got['order'][:N].tobytes() == again['order'][:N].tobytes()
        assert got['counts'][:, :N].tobytes() == again['counts'][:, :N].tobytes()


def test_ap_sweep_ignores_what_its_workspace_held(ctx):
    """the same bytes out of a zero-filled, a 0xFF-filled and a used workspace."""
    from face_vijnana_yolov3_amd._lib import lib
    rows, nrows, iou, flag = _sweep_case(2500, True, 5)
    d = [_dev(a, ctx) for a in (rows, nrows, iou, flag)]
    ths = [float(t) for t in np.arange(0.5, 1.0, 0.05)]
    need = int(lib().fv_det_ap_sweep_workspace_bytes(len(nrows)))
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device=d[0].device)
    guard = lambda: bool((ws[need:] == 0xA5).all())
    outs = []
    for fill in (0x00, 0xFF, None):                                       # None: what the previous call left behind
        if fill is not None:
            ws[:need] = fill
        ws[need:] = 0xA5
        out = dm.ap_sweep(ctx, d[0], d[1], d[2], d[3], ths, 1300, want_curve=True, workspace=ws)
        outs.append(b''.join(out[k].cpu().numpy()[..., :2500].tobytes() for k in ('result', 'n_det', 'order', 'counts')))
        assert guard()
    assert outs[0] == outs[1] == outs[2]


# ----------------------------------------------------------------------------- cal_mAP_sweep_device
def test_cal_map_sweep_device_on_the_golden_pairs(ctx, tmp_path):
    from face_vijnana_yolov3_amd import evaluate as ev
    cases = list(ref.golden_cases(tmp_path))
    assert len(cases) == 4
    for _ci, gt, sol, ths, want in cases:
        assert len(ths) == 5
        r = ev.sweep_device(gt, sol, ths, ctx, want_curve=True)
        for t, th in enumerate(ths):
            ps, rs, m = want[th]
            assert r['ps'][t].tobytes() == np.asarray(ps, np.float64).tobytes()
            assert r['rs'][t].tobytes() == np.asarray(rs, np.float64).tobytes()
            _q, err = ref.quad_with_error(ps, rs)
            print('case %d th %.2f: AP %.12f golden %.12f (quad error estimate %.3e)' % (_ci, th, r['ap'][t], m, err))
            assert abs(r['ap'][t] - m) <= err + 1e-9
        res, mean = ev.cal_mAP_sweep_device(gt, sol, ths, ctx)
        assert [a for _, a in res] == r['ap'] and mean == r['mean_ap'] and [t for t, _ in res] == ths


# ----------------------------------------------------------------------------- train() with hps['validate'], end to end
def _conf(root, val, mode, head, validate=None):
    hps = {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 2, 'step': 1, 'batch_size': 2, 'face_conf_th': 0.0,
           'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8}
    arch = {'image_size': 96, 'bb_info_c_size': 6}
    if head == 'three_scale':
        arch.update(head='three_scale', num_classes=1)
    if validate is not None:
        hps['validate'] = validate
    return {'mode': mode, 'raw_data_path': root, 'test_path': val, 'output_file_path': os.path.join(val, 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False, 'hps': hps, 'nn_arch': arch}


def _held_out_set(val):
    """Six JPEGs of different aspect ratios and a validation.csv whose one box per image covers most of it."""
    from PIL import Image
    os.makedirs(val)
    rng = np.random.default_rng(11)
    lines = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    for k, (h, w) in enumerate([(120, 160), (160, 120), (128, 128), (100, 200), (200, 100), (150, 180)]):
        name = 'held_%02d.jpg' % k
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(val, name), quality=90)
        lines.append('%d,%s,%d,%.1f,%.1f,%.1f,%.1f' % (k, name, k + 1, 0.1 * w, 0.1 * h, 0.8 * w, 0.8 * h))
    open(os.path.join(val, 'validation.csv'), 'w').write('\n'.join(lines) + '\n')


def _training_state(model):
    """Everything the next training step reads: parameters, BN moving statistics, Adam moments, gradients buffer, the step and
    BN-update counters, and every random generator a process has."""
    import random
    torch.cuda.synchronize()
    return dict(params=model.params.clone(), state=model.state.clone(), m=model.m.clone(), v=model.v.clone(), grads=model.grads.clone(),
                iterations=model.iterations, bn_updates=model.bn_updates, torch_cpu=torch.get_rng_state(),
                torch_cuda=torch.cuda.get_rng_state(), numpy=np.random.get_state()[1].copy(), python=random.getstate())


def _same_training_state(a, b):
    return all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray)
               else a[k] == b[k] for k in a)


@pytest.mark.parametrize('head', ['single', 'three_scale'])
def test_train_validates_each_epoch(tmp_path, monkeypatch, capsys, head):
    """train() with validate {"every": 1, "save_best": true}: two history entries, the last equal to the evaluate() +
    cal_mAP_sweep round trip on the saved model, the same for eval_batch_size 1 and 4, a best checkpoint that loads.

    Validation must not perturb training.  Two training runs cannot be compared for that: the weight-gradient kernels sum their K
    splits with float atomics, so two runs of the SAME configuration end on different bits -- measured at this
    shape: without validate twice, 40.63 of 40.64 million parameters differ, max 3.8e-4 (three-scale 4.8e-4); with against without
    validate 3.8e-4 (4.9e-4), the same spread.  What can be held to the bit is held: around every validate() call inside train()
    the parameters, BN statistics, Adam moments, gradient buffer, step counters and all random generators are unchanged."""
    import pandas as pd
    from face_vijnana_yolov3_amd import data, evaluate as ev, face_detection
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(face_detection, 'DEBUG', False)
    root, val = str(tmp_path / 'train'), str(tmp_path / 'val')
    os.makedirs(root)
    data.make_synthetic_uccs(root, n_images=5, seed=1, csv_name='training.csv')
    _held_out_set(val)
    fd = FaceDetector(_conf(root, val, 'train', head, {'every': 1, 'save_best': True}))
    snaps, inner = [], fd.validate

    def spied(**kw):
        before = _training_state(fd.model)
        res = inner(**kw)
        snaps.append((before, _training_state(fd.model)))
        return res
    monkeypatch.setattr(fd, 'validate', spied)
    fd.train()
    hist = fd.validation_history
    assert len(hist) == 2 and [h['epoch'] for h in hist] == [1, 2]
    last = hist[-1]
    assert last['n_images'] == 6 and last['n_gt'] == 6 and len(last['ap']) == 10 and last['n_det'] > 0
    printed = capsys.readouterr().out
    assert printed.count('val - AP50 ') == 2 and '(%d detections on 6 images, 6 faces)' % last['n_det'] in printed
    # the round trip the reference uses, on the saved model: evaluate() writes the csv, cal_mAP_sweep reads it
    conf2 = _conf(root, val, 'evaluate', head); conf2['model_loading'] = True
    fd2 = FaceDetector(conf2)
    fd2.evaluate()
    gt_csv = os.path.join(val, 'validation.csv')
    conf_h, ious_h = ev.detection_ious(pd.read_csv(gt_csv), pd.read_csv(conf2['output_file_path'], header=None))
    assert last['n_det'] == len(conf_h) and (ious_h > 0).sum() >= 1      # not vacuous: detections exist and one is matched
    res, mean = ev.cal_mAP_sweep(gt_csv, conf2['output_file_path'])
    for t, (th, m) in enumerate(res):
        ps, rs = ev.pr_curve(conf_h, ious_h, 6, th)
        assert last['precision'][t] == ps[-1] and last['recall'][t] == rs[-1]
        _q, err = ref.quad_with_error(ps, rs)
        assert abs(last['ap'][t] - m) <= err + 1e-9, (th, last['ap'][t], m, err)
    assert abs(last['mean_ap'] - mean) <= 1e-9 + max(ref.quad_with_error(*ev.pr_curve(conf_h, ious_h, 6, th))[1] for th, _ in res)
    # validate() on the loaded model, outside train(): the same numbers, whatever the batch size
    for bs in (1, 4):
        fd2.hps['eval_batch_size'] = bs
        again = fd2.validate()
        assert again['epoch'] is None
        assert {k: v for k, v in again.items() if k != 'epoch'} == {k: v for k, v in last.items() if k != 'epoch'}, bs
    # keep-the-best: the file exists and loads
    assert os.path.exists(FaceDetector.BEST_MODEL_PATH)
    best_epoch = int(np.argmax([h['mean_ap'] for h in hist]))          # the first of equals: only a strictly greater mean replaces it
    fd2.model.load(FaceDetector.BEST_MODEL_PATH)
    assert torch.isfinite(fd2.model.params).all() and fd2.model.iterations == 3 * (best_epoch + 1)
    # validation does not perturb training: everything a later step reads is the same bits after validate() as before it
    assert len(snaps) == 2 and all(_same_training_state(a, b) for a, b in snaps)
    # the same run without the key takes the same steps (two runs never end on the same bits: see the docstring)
    plain = FaceDetector(_conf(root, val, 'train', head))
    plain.train()
    assert plain.validation_history == [] and plain.model.iterations == fd.model.iterations == 6
    assert plain.model.bn_updates == fd.model.bn_updates
    d = (plain.model.params - fd.model.params).abs().max().item()
    print('%s: max |parameter difference| to the run without validate %.3e' % (head, d))
