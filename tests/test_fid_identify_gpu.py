"""Face identification on the GPU: fv_letterbox_crops against fv_letterbox of host-cut copies (bit for bit), fv_fid_match
against float64 numpy, the facial-ID database and FaceIdentifier.test() against a plain per-crop restatement of the reference's
loop (fi.py:994-1153), and main()'s identification modes."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError
from face_vijnana_yolov3_amd.postproc import letterbox_batch_device, letterbox_device

pytestmark = pytest.mark.gpu

_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


# ----------------------------------------------------------------------------- 1. fv_letterbox_crops
def _crop_list(shapes, rng):
    crops = []
    for i, (H, W) in enumerate(shapes):
        crops += [(i, 0, 0, 1, 1), (i, H - 1, W - 1, 1, 1), (i, 0, 0, H, W),                 # 1 pixel, full image
                  (i, 0, 3, 10, 7), (i, H - 9, 2, 9, 12), (i, 4, 0, 11, 6), (i, 5, W - 8, 13, 8),  # each edge
                  (i, 1, 1, 2, min(W - 2, 90)), (i, 1, 1, min(H - 2, 90), 2)]                   # elongated (side rounds to 2 / 1)
        for _ in range(20):
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            if not fi.lb_side_ok(h, w, 96):
                continue
            crops.append((i, int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    return [c for c in crops if fi.lb_side_ok(c[3], c[4], 96)]


def _check_crops(images, host, crops, S):
    got = fi.letterbox_crops(_ctx(), images, crops, S)
    for k, (i, y0, x0, h, w) in enumerate(crops):
        want, _ = letterbox_device(_ctx(), np.ascontiguousarray(host[i][y0:y0 + h, x0:x0 + w]), S)
        assert torch.equal(got[k], want), (k, (i, y0, x0, h, w))


@pytest.mark.parametrize('source', ['pil', 'jpeg'])
def test_letterbox_crops_bit_identical_to_letterbox_of_host_copies(tmp_path, source):
    from PIL import Image
    from face_vijnana_yolov3_amd import jpeg
    rng = np.random.default_rng(0)
    S = 96
    shapes = [(37, 150), (120, 45), (64, 64)]
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    keep = []
    dev = torch.device('cuda', 0)
    if source == 'pil':
        letterbox_batch_device(_ctx(), raws, S, dev, keep=keep)
    else:
        datas = []
        for k, r in enumerate(raws):
            p = str(tmp_path / ('%d.jpg' % k))
            Image.fromarray(r).save(p, quality=90)
            datas.append(open(p, 'rb').read())
        infos = [jpeg.parse(d) for d in datas]
        plan = jpeg.BatchPlan(infos)
        coefs = torch.empty(int(plan.total_coefs), dtype=torch.int16)
        view = coefs.numpy()
        for i in range(len(datas)):
            jpeg.entropy_decode(datas[i], infos[i], view[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
        letterbox_batch_device(_ctx(), None, S, dev, packed=('jpeg', coefs, plan), keep=keep)
    torch.cuda.synchronize()
    images = keep[0]
    buf = images[0].cpu().numpy()
    host = [buf[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(images[1], zip(images[2][0::2], images[2][1::2]))]
    if source == 'pil':
        assert all(np.array_equal(a, b) for a, b in zip(host, raws))
    crops = _crop_list(shapes, rng)
    assert len(crops) > 64                               # more than one launch's table
    _check_crops(images, host, crops, S)
    _check_crops(images, host, crops[5:7], 128)          # another size, a short list


def test_letterbox_crops_rejects_bad_records():
    rng = np.random.default_rng(1)
    keep = []
    raws = [rng.integers(0, 256, (20, 300, 3)).astype(np.uint8)]
    letterbox_batch_device(_ctx(), raws, 96, torch.device('cuda', 0), keep=keep)
    for bad in [(0, 0, 0, 21, 5), (0, 0, 296, 3, 5), (1, 0, 0, 1, 1), (0, -1, 0, 2, 2), (0, 0, 0, 1, 299), (0, 0, 0, 0, 4)]:
        with pytest.raises(FvError):
            fi.letterbox_crops(_ctx(), keep[0], [bad], 96)


# ----------------------------------------------------------------------------- 2. fv_fid_match
def _reference(q, r):
    d = torch.cdist(torch.from_numpy(q).double(), torch.from_numpy(r).double(), compute_mode='donot_use_mm_for_euclid_dist').numpy()
    return d


def _match(q, r):
    bi, bd = fi.fid_match(_ctx(), torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda())
    return bi.cpu().numpy(), bd.cpu().numpy()


@pytest.mark.parametrize('m', [1, 1085, 8631])
def test_fid_match_against_float64(m):
    rng = np.random.default_rng(m)
    r = rng.normal(size=(m, 64)).astype(np.float32)
    q = rng.normal(size=(3000, 64)).astype(np.float32)
    d = _reference(q, r)
    want_i = np.argmin(d, axis=1)
    want_d = d[np.arange(len(q)), want_i]
    if m > 1:
        part = np.partition(d, 1, axis=1)
        assert (part[:, 1] - part[:, 0]).min() > 1e-9               # the data leave no near-ties
    bi, bd = _match(q, r)
    assert np.array_equal(bi, want_i)
    np.testing.assert_allclose(bd, want_d, rtol=1e-12, atol=0)
    # any split of the queries gives the same bits (one, a few hundred, the rest: three different kernel variants)
    parts = [_match(q[a:b], r) for a, b in ((0, 1), (1, 700), (700, 3000))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), bi)
    assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.int64), bd.view(np.int64))


def test_fid_match_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(3)
    r = rng.normal(size=(1000, 64)).astype(np.float32)
    dup = [5, 300, 777, 999]
    r[dup] = r[17]
    q = np.concatenate([r[[17, 300, 999]], r[[17, 17]] + np.float32(1e-3), r[[42]]]).astype(np.float32)
    for n in (1, 600, 3000):                                        # every kernel variant
        qq = np.tile(q, (n // len(q) + 1, 1))[:n]
        bi, bd = _match(qq, r)
        want = np.argmin(_reference(qq, r), axis=1)
        assert np.array_equal(bi, want)
        assert set(bi[:min(n, 5)].tolist()) <= {5, 42}
        if n >= 3:
            assert bi[0] == 5 and bd[0] == 0.0 and bi[1] == 5 and bi[2] == 5


def test_fid_match_rejects_an_empty_registry():
    q = torch.zeros((2, 64), dtype=torch.float32, device='cuda')
    with pytest.raises(FvError):
        fi.fid_match(_ctx(), q, torch.zeros((0, 64), dtype=torch.float32, device='cuda'))


# ----------------------------------------------------------------------------- 3. facial-ID database
def _fi_conf(tmp_path, S, mode='fid_db', model_loading=False):
    return dict(mode=mode, resource_type='uccs', raw_data_path=str(tmp_path), test_path=str(tmp_path / 'frames'),
                output_file_path=str(tmp_path / 'solution_fi.csv'), multi_gpu=False, num_gpus=1, yolov3_base_model_load=False,
                model_loading=model_loading, nn_arch=dict(image_size=S, dense1_dim=64),
                hps=dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2, sim_th=0.2))


def _fd_conf(tmp_path, S, eval_batch=8):
    return {'mode': 'test', 'raw_data_path': str(tmp_path), 'test_path': str(tmp_path / 'frames'),
            'output_file_path': str(tmp_path / 'solution_fd.csv'), 'multi_gpu': False, 'num_gpus': 1,
            'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2,
                    'face_conf_th': 0.05, 'nms_iou_th': 0.5, 'num_cands': 60, 'eval_batch_size': eval_batch},
            'nn_arch': {'image_size': S, 'bb_info_c_size': 6}}


def _subject_faces(tmp_path, S, rng):
    import pandas as pd
    from PIL import Image
    os.makedirs(tmp_path / 'subject_faces', exist_ok=True)
    rows = []
    for sid in (4, -1, 2, 9):
        for j in range(3 if sid != 9 else 1):
            img = rng.integers(0, 256, (S, S, 3)).astype(np.uint8)
            name = 's%d_%d.png' % (sid, j)
            Image.fromarray(img).save(tmp_path / 'subject_faces' / name)
            rows.append(dict(subject_id=sid, face_file=name))
    pd.DataFrame(rows).to_csv(tmp_path / 'subject_image_db.csv')


def test_facial_id_db_and_registry(tmp_path, monkeypatch):
    import pandas as pd
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    S = 64
    _subject_faces(tmp_path, S, np.random.default_rng(2))
    ident = fi.FaceIdentifier({'fi_conf': _fi_conf(tmp_path, S), 'fd_conf': {}})
    ident.make_facial_ids_db()
    ident.register_facial_ids()
    got = fi.read_facial_ids_h5('subject_facial_ids.h5')
    db = pd.read_csv('subject_image_db.csv').iloc[:, 1:]
    assert sorted(got) == sorted(db[db.subject_id != -1].face_file)
    with open('ref_facial_id_db.pickle', 'rb') as f:
        reg = pickle.load(f)
    assert list(reg) == [2, 4, 9]
    for sid, df in db.groupby('subject_id'):
        if sid == -1:
            continue
        x = np.asarray([np.asarray(Image.open(tmp_path / 'subject_faces' / ff).convert('RGB')) for ff in df.face_file])
        want = ident.fid_extractor.predict(x)                     # the reference's one predict per subject
        for k, ff in enumerate(df.face_file):
            assert np.array_equal(got[ff][0], want[k]) and got[ff][1] == sid
        assert np.array_equal(reg[sid], np.asarray(pd.DataFrame(want).mean()))


# ----------------------------------------------------------------------------- 4. test() end to end
def _frames(tmp_path, rng):
    from PIL import Image
    os.makedirs(tmp_path / 'frames', exist_ok=True)
    shapes = [(120, 200), (150, 90), (96, 96), (70, 180), (200, 120), (100, 160), (64, 64), (130, 130), (90, 210), (160, 100)]
    for k, (h, w) in enumerate(shapes):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]          # blocky: real structure for the network
        Image.fromarray(img).save(tmp_path / 'frames' / ('frame_%02d.jpg' % k), quality=92)


def _tune_head(fd, S):
    d = fd.model.layers[-1]
    y0 = fd.model.predict(np.random.default_rng(0).uniform(0, 1, (1, S, S, 3)).astype(np.float32))
    fd.model.params[d['w_off']:d['beta_off']] /= float(y0.std())
    fd.model.params[d['beta_off']] = 1.0; fd.model.params[d['beta_off'] + 5] = 1.0


def _restated(ident, files, reg_ids, subject_ids, sim_th, batch):
    """The reference's per-crop loop: detection per frame batch (the detector's own batching: its fp32 sums depend on the batch
    size), a host crop, fv_letterbox, fid_extractor.predict at batch 1, np.argmin over float64 distances."""
    from PIL import Image
    fd, S = ident.fd, ident.image_size
    out, dists = [], []
    for c0 in range(0, len(files), batch):
        chunk = files[c0:c0 + batch]
        raws = [np.asarray(Image.open(f).convert('RGB')) for f in chunk]
        xs = [letterbox_device(fd.model.ctx, r, S) for r in raws]
        all_boxes = fd.detect_batch(torch.stack([x for x, _ in xs]))
        for f, raw, (_x, geom), boxes in zip(chunk, raws, xs, all_boxes):
            fd._project_back(boxes, geom)
            h, w = raw.shape[:2]
            count = 1
            for box in boxes:
                if count > 60:
                    break
                l, t, r, b = int(box.xmin), int(box.ymin), int(box.xmax), int(box.ymax)
                crop = raw[(t - 1):(b - 1), (l - 1):(r - 1), :]
                if crop.shape[0] == 0 or crop.shape[1] == 0 or not fi.lb_side_ok(crop.shape[0], crop.shape[1], S):
                    continue
                xc, _ = letterbox_device(ident.model.ctx, np.ascontiguousarray(crop), S)
                q = ident.fid_extractor.predict(xc[None])[0].astype(np.float64)
                d = np.sqrt(((q[None] - reg_ids.astype(np.float64)) ** 2).sum(-1))
                cand = int(np.argmin(d))
                dists.append(d[cand])
                if sim_th is None or d[cand] > sim_th:
                    continue
                out.append(os.path.basename(f) + ',' + str(subject_ids[cand]) + ',' + str(box.xmin) + ',' + str(box.ymin) + ','
                           + str(box.xmax - box.xmin) + ',' + str(box.ymax - box.ymin) + ',' + str(box.get_score()) + '\n')
                count += 1
    return ''.join(out), dists


def test_identify_end_to_end_matches_per_crop_restatement(tmp_path, monkeypatch):
    import glob
    monkeypatch.chdir(tmp_path)
    S = 96
    rng = np.random.default_rng(7)
    _frames(tmp_path, rng)
    files = sorted(glob.glob(str(tmp_path / 'frames' / '*.jpg')))
    subject_ids = [11, 3, 25, 8, 40]
    reg = rng.normal(size=(5, 64)).astype(np.float32)
    reg /= np.linalg.norm(reg, axis=1, keepdims=True)
    with open('ref_facial_id_db.pickle', 'wb') as f:
        pickle.dump({s: reg[k] for k, s in enumerate(subject_ids)}, f)
    conf = {'fi_conf': _fi_conf(tmp_path, S, mode='test'), 'fd_conf': _fd_conf(tmp_path, S)}
    ident = fi.FaceIdentifier(conf)
    _tune_head(ident.fd, S)
    texts = {}
    for bs in (1, 8):
        ident.fd.hps['eval_batch_size'] = bs
        _, dists = _restated(ident, files, reg, subject_ids, None, bs)
        assert len(dists) >= 2 * len(files)                      # several boxes per frame
        ds = np.sort(np.asarray(dists))
        k = len(ds) // 2
        sim_th = float((ds[k - 1] + ds[k]) / 2)                  # the median, away from every distance
        ident.hps['sim_th'] = sim_th
        want, _ = _restated(ident, files, reg, subject_ids, sim_th, bs)
        ident.test()
        got = open(conf['fi_conf']['output_file_path']).read()
        assert got == want, bs
        assert 0 < got.count('\n') < len(dists)                   # rows both kept and rejected
        texts[bs] = got
    assert len(texts[1].splitlines()) > 0 and len(texts[8].splitlines()) > 0
    conf['fd_conf']['nn_arch']['image_size'] = 128
    with pytest.raises(ValueError, match='image_size'):
        ident.test()


# ----------------------------------------------------------------------------- 5. main()
def test_main_train_fid_db_and_test_modes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    S = 64
    rng = np.random.default_rng(9)
    _subject_faces(tmp_path, S, rng)
    _frames(tmp_path, rng)

    def run(mode, model_loading):
        conf = {'fi_conf': _fi_conf(tmp_path, S, mode=mode, model_loading=model_loading), 'fd_conf': _fd_conf(tmp_path, S)}
        (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
        fi.main()

    run('train', False)
    assert os.path.exists('face_identifier.h5') and os.path.exists('ref_facial_id_db.pickle')
    assert os.path.exists('subject_facial_ids.h5')
    for p in ('ref_facial_id_db.pickle', 'subject_facial_ids.h5'):
        os.remove(p)
    run('fid_db', True)
    with open('ref_facial_id_db.pickle', 'rb') as f:
        assert list(pickle.load(f)) == [2, 4, 9]
    assert len(fi.read_facial_ids_h5('subject_facial_ids.h5')) == 7
    run('test', True)
    assert os.path.exists(tmp_path / 'solution_fi.csv')
