"""Face identification host logic against goldens minted by running the reference (tests/golden/make_fi_golden.py): the crop
rectangles and csv rows of FaceIdentifier.test(), cal_acc_fi, and the facial-ID database writers.  No GPU."""
import os
import pickle
import types

import numpy as np
import pytest

from face_vijnana_yolov3_amd import evaluate as ev
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd.face_detection import FaceDetector
from face_vijnana_yolov3_amd.postproc import BoundBox


def _geom(h, w, S):
    if w >= h:
        h_p = int(h / w * S); pad = S - h_p
        return (h, w, pad // 2, pad - pad // 2, 0, 0)
    w_p = int(w / h * S); pad = S - w_p
    return (h, w, 0, 0, pad // 2, pad - pad // 2)


def test_identification_rows_match_reference_test(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fi_test.npz'))
    S, sim_th = int(g['image_size']), float(g['sim_th'])
    reg = g['registry'].astype(np.float64)
    subjects = [int(s) for s in g['subjects']]
    names = [str(n) for n in g['frame_names']]
    crops, ids = g['crops'], g['crop_ids']
    det = types.SimpleNamespace(image_size=S)
    text, used = [], 0
    for name in [str(n) for n in g['order']]:
        fidx = names.index(name)
        h, w = (int(v) for v in g['frame_hw'][fidx])
        b, sc = g['boxes_' + name], g['scores_' + name]
        boxes = [BoundBox(b[k, 0], b[k, 1], b[k, 2], b[k, 3], objness=sc[k], classes=[np.float32(sc[k])]) for k in range(len(b))]
        FaceDetector._project_back(det, boxes, _geom(h, w, S))
        rects = fi.crop_rects(boxes, h, w, S)
        idx = np.full(len(boxes), -1); dist = np.full(len(boxes), np.nan)
        seen = crops[crops[:, 0] == fidx]
        have = [k for k, r in enumerate(rects) if r is not None]
        # the reference cut exactly these crops, in this order (a prefix: it stops after 60 written rows)
        assert len(seen) <= len(have)
        for c, k in zip(seen, have):
            assert tuple(int(v) for v in c[1:]) == rects[k], (name, k)
            q = ids[used].astype(np.float64); used += 1
            d = np.sqrt(((q[None] - reg) ** 2).sum(-1))
            idx[k], dist[k] = int(np.argmin(d)), d.min()
        if len(seen) < len(have):
            assert fi.identification_rows(name, boxes, rects, idx, dist, subjects, sim_th).count('\n') == fi.MAX_ROWS_PER_IMAGE
        text.append(fi.identification_rows(os.path.join('/some/dir', name), boxes, rects, idx, dist, subjects, sim_th))
    assert used == len(crops)
    assert ''.join(text) == g['csv'].tobytes().decode()


def test_crop_rect_slice_semantics():
    # a box on the top or left edge: int(0) - 1 = -1 starts the slice at the LAST row / column -> empty
    assert fi.crop_rect(BoundBox(0.0, 5.0, 10.0, 20.0), 50, 60) is None
    assert fi.crop_rect(BoundBox(5.0, 0.0, 10.0, 20.0), 50, 60) is None
    assert fi.crop_rect(BoundBox(1.0, 1.0, 60.0, 50.0), 50, 60) == (0, 0, 49, 59)
    assert fi.crop_rect(BoundBox(3.9, 2.2, 3.95, 9.0), 50, 60) is None         # int(3.95) - 1 == int(3.9) - 1
    assert fi.crop_rect(BoundBox(3.9, 2.2, 4.5, 9.0), 50, 60) == (1, 2, 7, 1)
    assert fi.crop_rect(BoundBox(3.9, 2.2, 5.0, 9.0), 50, 60) == (1, 2, 7, 2)
    assert not fi.lb_side_ok(1, 500, 416) and fi.lb_side_ok(2, 400, 416)


def test_cal_acc_fi_matches_reference(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, 'cal_acc_fi.npz'))
    for ci in range(int(g['ncases'])):
        gp, sp = tmp_path / 'gt.csv', tmp_path / 'sol.csv'
        gp.write_bytes(g['case%d_gt' % ci].tobytes()); sp.write_bytes(g['case%d_sol' % ci].tobytes())
        res = ev.cal_acc_fi_sweep(str(gp), str(sp))
        assert len(res) == len(g['thresholds'])
        for k, r in enumerate(res):
            assert r[0] == pytest.approx(float(g['thresholds'][k]))
            assert tuple(r[1:5]) == tuple(int(v) for v in g['case%d_counts' % ci][k]), (ci, k)
            assert r[5] == float(g['case%d_acc' % ci][k])


def test_evaluate_main_cal_acc_fi_writes_h5(golden_dir, tmp_path, monkeypatch):
    from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5
    g = np.load(os.path.join(golden_dir, 'cal_acc_fi.npz'))
    gp, sp = tmp_path / 'gt.csv', tmp_path / 'sol.csv'
    gp.write_bytes(g['case1_gt'].tobytes()); sp.write_bytes(g['case1_sol'].tobytes())
    monkeypatch.chdir(tmp_path)
    ev.main(['--mode', 'cal_acc_fi', '--gt_path', str(gp), '--sol_path', str(sp)])
    d, _ = read_hdf5(str(tmp_path / 'fi_acc.h5'))
    assert np.array_equal(d['/tp_ls'], g['case1_counts'][:, 0]) and np.array_equal(d['/fn_ls'], g['case1_counts'][:, 3])
    assert np.array_equal(d['/acc_ls'], g['case1_acc'])


def test_facial_id_db_writers_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    names = ['s%d_%d.jpg' % (s, k) for s in (2, 5, 9) for k in range(3)]
    sids = [s for s in (2, 5, 9) for _ in range(3)]
    ids = rng.normal(size=(len(names), 64)).astype(np.float32)
    p = str(tmp_path / 'subject_facial_ids.h5')
    fi.write_facial_ids_h5(p, names, ids, sids)
    back = fi.read_facial_ids_h5(p)
    assert sorted(back) == sorted(names)
    for k, n in enumerate(names):
        v, s = back[n]
        assert v.dtype == np.float32 and v.shape == (64,) and np.array_equal(v, ids[k]) and s == sids[k]
    import pandas as pd
    db = {s: fi.subject_mean(ids[k * 3:k * 3 + 3]) for k, s in enumerate((2, 5, 9))}
    with open(tmp_path / 'reg.pickle', 'wb') as f:
        pickle.dump(db, f)
    with open(tmp_path / 'reg.pickle', 'rb') as f:
        got = pickle.load(f)
    assert list(got) == [2, 5, 9]
    for k, s in enumerate((2, 5, 9)):
        assert np.array_equal(got[s], np.asarray(pd.DataFrame(ids[k * 3:k * 3 + 3]).mean()))


def test_main_dispatches_identification_modes(tmp_path, monkeypatch):
    """fid_db and test are modes now; evaluate and data are still refused."""
    import json
    monkeypatch.chdir(tmp_path)
    calls = []

    class Fake:
        def __init__(self, conf):
            pass

        def train(self):
            calls.append('train')

        def make_facial_ids_db(self):
            calls.append('db')

        def register_facial_ids(self):
            calls.append('reg')

        def test(self):
            calls.append('test')

    monkeypatch.setattr(fi, 'FaceIdentifier', Fake)
    for mode, want in (('fid_db', ['db', 'reg']), ('test', ['test']), ('train', ['train', 'db', 'reg'])):
        (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps({'fi_conf': {'mode': mode}}))
        del calls[:]
        fi.main()
        assert calls == want, mode
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps({'fi_conf': {'mode': 'data'}}))
    with pytest.raises(NotImplementedError, match='data'):
        fi.main()
