"""The FaceIdentifier data mode on the GPU: fv_crop_nearest_u8 against the numpy restatement of its contract
(tests/nearest_letterbox_ref.py; uint8, exact equality), its refusals, create_db_fi end to end on synthetic UCCS and VGGFace2
trees, the device-JPEG path against the Pillow fallback, and the db it writes feeding train / fid_db."""
import io
import json
import os
import pickle

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import data
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError
from nearest_letterbox_ref import nearest_letterbox

pytestmark = pytest.mark.gpu

_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


# ----------------------------------------------------------------------------- 1. fv_crop_nearest_u8
def _upload(raws):
    """-> (device uint8 buffer, offsets, hw): the images packed back to back, as letterbox_batch_device's `keep` hands them out."""
    offs, hw, o = [], [], 0
    for r in raws:
        offs.append(o); hw += [r.shape[0], r.shape[1]]; o += r.size
    buf = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws])).cuda()
    return buf, offs, hw


def _check(raws, images, crops, S):
    got = fi.crop_nearest_u8(_ctx(), images, crops, S).cpu().numpy()
    assert got.shape == (len(crops), S, S, 3) and got.dtype == np.uint8
    for k, (i, y0, x0, h, w) in enumerate(crops):
        assert np.array_equal(got[k], nearest_letterbox(raws[i][y0:y0 + h, x0:x0 + w], S)), (k, (i, y0, x0, h, w), S)


SHAPES = [(37, 150), (120, 45), (64, 64), (3000, 3100), (20, 20)]


@pytest.fixture(scope='module')
def batch():
    rng = np.random.default_rng(0)
    raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    return raws, _upload(raws)


def _shaped_crops(S):
    """1 x 1, 1 x N, N x 1, whole images, every corner, up- and downscaling; only crops image_size S can letterbox."""
    crops = []
    for i, (H, W) in enumerate(SHAPES):
        crops += [(i, 0, 0, H, W),                                                            # the whole image
                  (i, 0, 0, 1, 1), (i, H - 1, W - 1, 1, 1),                                   # 1 x 1
                  (i, 3, 2, 1, min(W - 2, S)), (i, 2, 3, min(H - 2, S), 1),                   # 1 x N, N x 1 (the thin side rounds to >= 1)
                  (i, 0, 0, 9, 13), (i, 0, W - 13, 9, 13), (i, H - 9, 0, 9, 13), (i, H - 9, W - 13, 9, 13),   # every corner
                  (i, 0, 0, 13, 9), (i, 0, W - 9, 13, 9), (i, H - 13, 0, 13, 9), (i, H - 13, W - 9, 13, 9)]
    crops += [(4, 0, 0, 20, 20), (4, 1, 2, 17, 11),                                           # 20 px up to S
              (3, 0, 50, 3000, 3000), (3, 7, 11, 2990, 1700), (3, 100, 0, 800, 3100)]         # 3 000 px down to S
    return [c for c in crops if fi.lb_side_ok(c[3], c[4], S)]


@pytest.mark.parametrize('S', [32, 416, 608])
def test_crop_nearest_equals_the_numpy_restatement(batch, S):
    raws, images = batch
    crops = _shaped_crops(S)
    assert {c[0] for c in crops} == set(range(len(SHAPES)))
    assert any(c[3] == 1 and c[4] == 1 for c in crops) and any(c[3] == 1 and c[4] > 1 for c in crops)
    assert any(c[4] == 1 and c[3] > 1 for c in crops)
    _check(raws, images, crops, S)
    _check(raws, images, crops[::-1][::3], S)          # another order, images interleaved


def _random_crops(n, rng, S):
    crops = []
    while len(crops) < n:
        i = int(rng.integers(0, len(SHAPES)))
        H, W = SHAPES[i]
        h, w = int(rng.integers(1, min(H, 400) + 1)), int(rng.integers(1, min(W, 400) + 1))
        if fi.lb_side_ok(h, w, S):
            crops.append((i, int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    return crops


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 1000])
def test_crop_nearest_any_number_of_crops_in_one_call(batch, n):
    raws, images = batch
    S = 416
    crops = _random_crops(n, np.random.default_rng(n), S)      # arbitrary image order
    _check(raws, images, crops, S)


def test_crop_nearest_refusals_leave_dst_untouched(batch):
    raws, images = batch
    S = 96
    good = (0, 1, 1, 20, 30)
    H, W = SHAPES[0]
    bad = [(0, 0, 0, H + 1, 5), (0, 0, W - 4, 3, 5), (0, H - 2, 0, 3, 5), (0, -1, 0, 2, 2), (0, 0, -1, 2, 2),   # outside its image
           (len(SHAPES), 0, 0, 1, 1), (-1, 0, 0, 1, 1),                                                         # no such image
           (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (0, 0, 0, -3, 4),                                                  # h or w below 1
           (0, 0, 0, 1, 97), (3, 0, 0, 97, 1)]                                                                  # a side rounds to 0
    for b in bad:
        for crops in ([b], [good, b], [good] * 70 + [b]):        # the bad record alone, behind a good one, in the second chunk
            out = torch.full((len(crops), S, S, 3), 0xAB, dtype=torch.uint8, device='cuda')
            with pytest.raises(FvError):
                fi.crop_nearest_u8(_ctx(), images, crops, S, out=out)
            torch.cuda.synchronize()
            assert bool((out == 0xAB).all()), b
    out = torch.full((1, S, S, 3), 0xAB, dtype=torch.uint8, device='cuda')
    fi.crop_nearest_u8(_ctx(), images, [], S, out=out)            # n == 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    with pytest.raises(FvError):
        fi.crop_nearest_u8(_ctx(), images, [good], 100)           # rows of 300 bytes are no whole 16-byte stores
    _check(raws, images, [good], S)


# ----------------------------------------------------------------------------- 2. create_db_fi end to end
def _conf(raw, S, resource_type='uccs', mode='data', **hps):
    h = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2, sim_th=0.2)
    h.update(hps)
    return {'fi_conf': dict(mode=mode, resource_type=resource_type, raw_data_path=str(raw), test_path=str(raw / 'frames'),
                            output_file_path=str(raw / 'solution_fi.csv'), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64), hps=h),
            'fd_conf': {}}


def _roundtrip(pixels):
    """What Pillow reads back from its own default-quality JPEG of `pixels` (the same library and input: the same bytes)."""
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(pixels).save(f, format='JPEG')
    return np.asarray(Image.open(io.BytesIO(f.getvalue())).convert('RGB'))


def _check_written(records, out_dir, S):
    assert sorted(os.listdir(out_dir)) == sorted(r.name for r in records)
    sources = {}
    for r in records:
        if r.source not in sources:
            sources[r.source] = fi._imread(r.source)
        y0, x0, h, w = r.rect
        want = _roundtrip(nearest_letterbox(sources[r.source][y0:y0 + h, x0:x0 + w], S))
        assert np.array_equal(fi._imread(os.path.join(out_dir, r.name)), want), r.name
        assert r.row[2:] == (w, h)


def test_create_db_fi_uccs_end_to_end(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    S = 96
    data.make_synthetic_uccs(str(tmp_path / 'training'), n_images=6, seed=3)
    os.makedirs(tmp_path / 'subject_faces' / 'stale_dir')
    (tmp_path / 'subject_faces' / 'stale.jpg').write_bytes(b'old')
    res = fi.create_db_fi(_conf(tmp_path, S))
    records, skipped = fi.uccs_records(str(tmp_path), S)
    assert len(records) >= 6 and res == dict(skipped, written=len(records))
    _check_written(records, str(tmp_path / 'subject_faces'), S)            # the stale entries are gone
    assert open('subject_image_db.csv').read() == fi.db_csv_text(records)
    first = {r.name: open(tmp_path / 'subject_faces' / r.name, 'rb').read() for r in records}
    (tmp_path / 'subject_faces' / 'stale2.jpg').write_bytes(b'old')
    fi.create_db_fi(_conf(tmp_path, S))                                    # a second run re-creates the directory
    assert {n: open(tmp_path / 'subject_faces' / n, 'rb').read() for n in os.listdir(tmp_path / 'subject_faces')} == first


def _vgg_tree(root, rng):
    """train/<identity>/<file>.jpg of several sizes -- one grayscale, one CMYK (the device decoder refuses it: Pillow decodes
    that batch) -- and loose_bb_train.csv with skipped, clipped, wide, tall and square rows."""
    from PIL import Image
    rows = ['NAME_ID,X,Y,W,H']
    spec = [('n000001', '0001_01', (90, 120), 'RGB', (10, 5, 60, 70)), ('n000001', '0002_01', (130, 80), 'RGB', (-2, 5, 60, 70)),
            ('n000001', '0003_02', (64, 64), 'L', (0, 0, 64, 64)), ('n000007', '0001_01', (200, 150), 'RGB', (100, 150, 90, 90)),
            ('n000007', '0004_01', (75, 210), 'CMYK', (20, 10, 150, 40)), ('n000007', '0005_01', (100, 100), 'RGB', (10, 10, 0, 40)),
            ('n000007', '0006_01', (100, 100), 'RGB', (30, 100, 20, 20)), ('n000009', '0001_01', (300, 40), 'RGB', (5, 20, 30, 260))]
    for identity, name, (h, w), mode, box in spec:
        os.makedirs(os.path.join(root, 'train', identity), exist_ok=True)
        a = rng.integers(0, 256, (h, w, {'RGB': 3, 'L': 1, 'CMYK': 4}[mode]), dtype=np.uint8)
        Image.frombytes(mode, (w, h), a.tobytes()).save(os.path.join(root, 'train', identity, name + '.jpg'), quality=92)
        rows.append('%s/%s,%d,%d,%d,%d' % ((identity, name) + box))
    open(os.path.join(root, 'loose_bb_train.csv'), 'w').write('\n'.join(rows) + '\n')


def test_create_db_fi_vggface2_end_to_end(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    S = 64
    _vgg_tree(str(tmp_path), np.random.default_rng(5))
    res = fi.create_db_fi(_conf(tmp_path, S, 'vggface2'))
    records, skipped = fi.vggface2_records(str(tmp_path), S)
    assert skipped == {'empty': 1, 'side_rounds_to_0': 0} and res['written'] == len(records) == 5
    assert [r.row[0] for r in records] == ['n000001', 'n000001', 'n000007', 'n000007', 'n000009']
    _check_written(records, str(tmp_path / 'subject_faces_vggface2'), S)
    assert open('subject_image_vggface2_db.csv').read() == fi.db_csv_text(records)


def test_many_small_batches_write_the_same_files(tmp_path):
    """Batches of at most two crops: the loader thread, the pinned ring and the two output slots all come round several times."""
    S = 64
    data.make_synthetic_uccs(str(tmp_path / 'training'), n_images=9, seed=11)
    records, _ = fi.uccs_records(str(tmp_path), S)
    assert len(fi.source_batches(records, fi.image_hw, batch_crops=2)) >= 5
    os.makedirs(tmp_path / 'out')
    fi.cut_and_write(_ctx(), records, S, str(tmp_path / 'out'), 4, batch_crops=2)
    _check_written(records, str(tmp_path / 'out'), S)


def test_device_jpeg_and_pillow_fallback_cut_identical_crops(tmp_path):
    from PIL import Image
    S = 96
    data.make_synthetic_uccs(str(tmp_path / 'training'), n_images=4, seed=7)
    records, _ = fi.uccs_records(str(tmp_path), S)
    for name, device_jpeg in (('dev', True), ('pil', False)):
        os.makedirs(tmp_path / name)
        fi.cut_and_write(_ctx(), records, S, str(tmp_path / name), 4, device_jpeg=device_jpeg)
    for r in records:
        assert open(tmp_path / 'dev' / r.name, 'rb').read() == open(tmp_path / 'pil' / r.name, 'rb').read(), r.name
    # a progressive file in the batch: the parser refuses it, so the whole batch takes the fallback -- same crops again
    src = records[0].source
    Image.fromarray(fi._imread(src)).save(str(tmp_path / 'training' / 'progressive.jpg'), quality=90, progressive=True)
    from face_vijnana_yolov3_amd import jpeg
    assert jpeg.parse(open(tmp_path / 'training' / 'progressive.jpg', 'rb').read()) is None
    extra = fi.CropRecord(str(tmp_path / 'training' / 'progressive.jpg'), (2, 3, 40, 50), 'progressive_cut.jpg', (1, 'progressive_cut.jpg', 50, 40))
    os.makedirs(tmp_path / 'mixed')
    fi.cut_and_write(_ctx(), records + [extra], S, str(tmp_path / 'mixed'), 4)
    _check_written(records + [extra], str(tmp_path / 'mixed'), S)
    for r in records:
        assert open(tmp_path / 'mixed' / r.name, 'rb').read() == open(tmp_path / 'dev' / r.name, 'rb').read(), r.name


# ----------------------------------------------------------------------------- 3. the rest of the package reads what it wrote
def test_data_then_train_then_fid_db(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    S = 64
    rng = np.random.default_rng(9)
    os.makedirs(tmp_path / 'training')
    rows = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    k = 0
    for f in range(3):
        Image.fromarray(rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)).save(tmp_path / 'training' / ('frame%d.jpg' % f), quality=90)
        for sid in (5, -1, 2, 8):
            rows.append('%d,frame%d.jpg,%d,%.1f,%.1f,%.1f,%.1f' % (k, f, sid, 10 + 60 * (k % 4), 20 + 7 * f, 40 + 5 * f, 50 + 3 * (k % 4)))
            k += 1
    (tmp_path / 'training' / 'training.csv').write_text('\n'.join(rows) + '\n')
    conf = _conf(tmp_path, S)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    fi.main()                                                          # mode 'data'
    names = sorted(os.listdir(tmp_path / 'subject_faces'))
    assert len(names) == 9                                             # three subjects, three faces each
    seq = fi.TrainingSequence(str(tmp_path), conf['fi_conf']['hps'], conf['fi_conf']['nn_arch'], load_flag=False)
    assert len(seq.img_triplet_pairs) == 9 and len(seq) == 5           # 3 pairs per subject, batches of 2
    x, _ = seq[0]
    assert x['input_a'].shape == (2, S, S, 3)
    ident = fi.FaceIdentifier(conf)
    loss = ident.train_on_batch(x['input_a'], x['input_p'], x['input_n'])
    assert np.isfinite(loss)
    ident.make_facial_ids_db()
    ident.register_facial_ids()
    assert sorted(fi.read_facial_ids_h5('subject_facial_ids.h5')) == names
    with open('ref_facial_id_db.pickle', 'rb') as f:
        assert list(pickle.load(f)) == [2, 5, 8]
