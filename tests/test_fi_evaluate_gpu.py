"""FaceIdentifier.evaluate on the GPU: fv_draw_prims_u8 against Pillow drawing the same boxes (whole buffer, exact), its
refusals, and evaluate() end to end -- the csv of test(), and every annotated frame byte-identical to the file Pillow makes
from the decoded frame."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from draw_prims_ref import _box, box_cases, draw_prims_ref, pillow_boxes
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError
from face_vijnana_yolov3_amd.postproc import letterbox_batch_device, letterbox_device

pytestmark = pytest.mark.gpu

RED, GREEN = (255, 0, 0), (0, 255, 0)
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _packed(shapes, seed):
    rng = np.random.default_rng(seed)
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    keep = []
    letterbox_batch_device(_ctx(), raws, 96, torch.device('cuda', 0), keep=keep)
    torch.cuda.synchronize()
    return raws, keep[0], rng


# ----------------------------------------------------------------------------- 1. fv_draw_prims_u8 against Pillow
def test_draw_prims_u8_equals_pillow_on_the_whole_buffer():
    shapes = [(37, 150), (120, 45), (64, 64), (300, 517), (40, 50)]          # the last one gets no primitive
    raws, images, rng = _packed(shapes, 0)
    dbuf, offs, hw = images
    before = dbuf.cpu().numpy().copy()
    assert all(np.array_equal(before[o:o + r.size], r.reshape(-1)) for o, r in zip(offs, raws))
    font = fi._font()
    layers = []
    for i, (H, W) in enumerate(shapes[:4]):
        boxes = box_cases(H, W, rng)
        boxes.append(_box(0, 0, W - 1, H - 1, 0.31, 9))                       # the full image
        boxes.append(_box(W // 2 + 0.4, H // 2 + 0.9, W // 2 + 3.6, H // 2 + 3.95, 0.77, 4))   # 4 x 4 pixels
        if i == 3:                                                           # order: the second box's label lies over the first's outline
            first, second = _box(40.0, 100.0, 120.0, 160.0, 0.2, 1), _box(60.5, 112.3, 140.0, 150.0, 0.9, 2)
            boxes += [first, second]
        half = len(boxes) // 2
        layers.append((boxes[:half], boxes[half:]))
    prims = []
    for i, (gt, det) in enumerate(layers):
        prims += fi.annotation_prims(i, gt, RED, font) + fi.annotation_prims(i, det, GREEN, font)
    prims, masks = fi.pack_masks(prims)
    assert len(prims) > 3 * 32                                               # several launches, chunks that straddle images
    fi.draw_prims_u8(_ctx(), images, prims, torch.from_numpy(masks).cuda())
    torch.cuda.synchronize()
    got = dbuf.cpu().numpy()
    want = before.copy()
    for i, (gt, det) in enumerate(layers):
        img = pillow_boxes(pillow_boxes(raws[i], gt, RED, font), det, GREEN, font)
        want[offs[i]:offs[i] + img.size] = img.reshape(-1)
    assert np.array_equal(got, want)
    assert np.array_equal(got[offs[4]:], before[offs[4]:])                   # the image without primitives
    # the order check bites: swapping the two overlapping boxes changes the picture
    a = pillow_boxes(raws[3], [first, second], GREEN, font)
    b = pillow_boxes(raws[3], [second, first], GREEN, font)
    assert not np.array_equal(a, b)
    # the contract's numpy restatement says the same
    ref = draw_prims_ref(before.copy(), offs, hw, prims, masks)
    assert np.array_equal(got, ref)


def test_draw_prims_u8_mask_origin_and_colour_channels():
    """A hand-made mask at a negative origin, an ink with three different channels, an outline wider than its box."""
    raws, images, rng = _packed([(33, 70), (9, 200)], 5)
    dbuf, offs, hw = images
    before = dbuf.cpu().numpy().copy()
    m0 = rng.integers(0, 256, (20, 90)).astype(np.uint8)                     # hangs off the left, top and right of image 0
    m1 = rng.integers(0, 256, (40, 13)).astype(np.uint8)                     # taller than image 1
    m0[3, :] = 255; m0[4, :] = 0
    prims = [fi.MaskBlend(0, -11, -6, 90, 20, None, (200, 17, 99), m0), fi.Outline(0, 5, 5, 60, 30, 2, (1, 2, 3)),
             fi.MaskBlend(1, 150, -20, 13, 40, None, (0, 255, 128), m1), fi.Outline(1, -5, 2, 400, 6, 50, (9, 8, 7)),
             fi.MaskBlend(0, 40, 20, 0, 0, None, RED, np.zeros((0, 0), np.uint8)), fi.Outline(1, 30, 8, 20, 2, 3, RED)]
    prims, masks = fi.pack_masks(prims)
    fi.draw_prims_u8(_ctx(), images, prims, torch.from_numpy(masks).cuda())
    torch.cuda.synchronize()
    want = draw_prims_ref(before.copy(), offs, hw, prims, masks)
    assert np.array_equal(dbuf.cpu().numpy(), want) and not np.array_equal(want, before)


# ----------------------------------------------------------------------------- 2. rejected tables
def test_draw_prims_u8_rejects_bad_tables_and_draws_nothing():
    raws, images, rng = _packed([(37, 150), (64, 64)], 1)
    dbuf = images[0]
    before = dbuf.clone()
    mask = rng.integers(1, 256, (10, 12)).astype(np.uint8)
    good = [fi.Outline(0, 2, 2, 30, 30, 3, RED), fi.MaskBlend(1, 5, 5, 12, 10, 0, GREEN, None)]
    masks = torch.from_numpy(mask.reshape(-1).copy()).cuda()
    bad = [fi.Outline(2, 2, 2, 30, 30, 3, RED),                              # image index out of range
           fi.Outline(-1, 2, 2, 30, 30, 3, RED),
           fi.Outline(0, 2, 2, 30, 30, 0, RED),                              # width 0
           fi.MaskBlend(1, 5, 5, 12, 10, 1, GREEN, None),                    # one byte past the end of the mask buffer
           fi.MaskBlend(1, 5, 5, 12, 11, 0, GREEN, None),
           fi.MaskBlend(1, 5, 5, 12, 10, -1, GREEN, None),
           fi.MaskBlend(1, 5, 5, -12, 10, 0, GREEN, None)]                   # negative mask size
    for b in bad:
        for table in ([b], good + [b], [b] + good, good * 20 + [b]):         # also behind more than one launch's worth of good ones
            with pytest.raises(FvError):
                fi.draw_prims_u8(_ctx(), images, table, masks)
    torch.cuda.synchronize()
    assert torch.equal(dbuf, before)
    fi.draw_prims_u8(_ctx(), images, good, masks)                            # and the good table does draw
    torch.cuda.synchronize()
    assert not torch.equal(dbuf, before)


# ----------------------------------------------------------------------------- 3. evaluate() end to end
# the frames, tuned head and registry recipe of test_fid_identify_gpu.test_identify_end_to_end_matches_per_crop_restatement
def _fi_conf(tmp_path, S, mode='test', model_loading=False):
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


SHAPES = [(120, 200), (150, 90), (96, 96), (70, 180), (200, 120), (100, 160), (64, 64), (130, 130), (90, 210), (160, 100)]


def _frames(tmp_path, rng):
    from PIL import Image
    os.makedirs(tmp_path / 'frames', exist_ok=True)
    for k, (h, w) in enumerate(SHAPES):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]          # blocky: real structure for the network
        Image.fromarray(img).save(tmp_path / 'frames' / ('frame_%02d.jpg' % k), quality=92)


def _tune_head(fd, S):
    d = fd.model.layers[-1]
    y0 = fd.model.predict(np.random.default_rng(0).uniform(0, 1, (1, S, S, 3)).astype(np.float32))
    fd.model.params[d['w_off']:d['beta_off']] /= float(y0.std())
    fd.model.params[d['beta_off']] = 1.0; fd.model.params[d['beta_off'] + 5] = 1.0


NO_GT = 'frame_03.jpg'


def _validation_csv(tmp_path, rng):
    """Two float rows for every frame but NO_GT, subject ids including -1, and one more row with width 0 (skipped)."""
    import pandas as pd
    rows = []
    for k, (h, w) in enumerate(SHAPES):
        name = 'frame_%02d.jpg' % k
        if name == NO_GT:
            continue
        for j in range(2):
            bw, bh = rng.uniform(8, w / 2), rng.uniform(8, h / 2)
            rows.append(dict(FACE_ID=len(rows), FILE=name, SUBJECT_ID=int(rng.choice([-1, 3, 11, 25, 1000])),
                             FACE_X=rng.uniform(1, w - bw), FACE_Y=rng.uniform(1, h - bh), FACE_WIDTH=bw, FACE_HEIGHT=bh))
    rows.insert(1, dict(FACE_ID=999, FILE='frame_00.jpg', SUBJECT_ID=8, FACE_X=20.5, FACE_Y=30.5, FACE_WIDTH=0.0, FACE_HEIGHT=25.0))
    rows[2]['SUBJECT_ID'] = -1
    df = pd.DataFrame(rows, columns=['FACE_ID', 'FILE', 'SUBJECT_ID', 'FACE_X', 'FACE_Y', 'FACE_WIDTH', 'FACE_HEIGHT'])
    df.to_csv(tmp_path / 'frames' / 'validation.csv', index=False)
    return df


def _detections(ident, files, batch):
    """{frame name: (Pillow-decoded frame, the detector's boxes)}, as the per-crop restatement of the existing test obtains them
    (the detector's own batching: its fp32 sums depend on the batch size)."""
    from PIL import Image
    fd, S = ident.fd, ident.image_size
    out = {}
    for c0 in range(0, len(files), batch):
        chunk = files[c0:c0 + batch]
        raws = [np.asarray(Image.open(f).convert('RGB')) for f in chunk]
        xs = [letterbox_device(fd.model.ctx, r, S) for r in raws]
        all_boxes = fd.detect_batch(torch.stack([x for x, _ in xs]))
        for f, raw, (_x, geom), boxes in zip(chunk, raws, xs, all_boxes):
            fd._project_back(boxes, geom)
            out[os.path.basename(f)] = (raw, boxes)
    return out


def _row_text(name, sid, box):
    return (name + ',' + str(sid) + ',' + str(box.xmin) + ',' + str(box.ymin) + ',' + str(box.xmax - box.xmin) + ','
            + str(box.ymax - box.ymin) + ',' + str(box.get_score()))


def _assign_subject_ids(name, boxes, rows):
    """evaluate()'s csv rows of one frame are in box order: the box a row describes carries the row's subject id, every other
    box keeps -1."""
    k = 0
    for box in boxes:
        box.subject_id = -1
        if k < len(rows):
            sid = rows[k].split(',')[1]
            if _row_text(name, sid, box) == rows[k]:
                box.subject_id = sid
                k += 1
    assert k == len(rows), (name, k, len(rows))


def _reference_drawing(image, boxes, color, font):
    """draw_boxes_v3 with Pillow; the two documented deviations drawn as documented: a disordered box is left out, a box with a
    truncated extent below 3 is filled between its corners (then labelled by Pillow)."""
    from PIL import Image, ImageDraw
    slivers = 0
    for b in boxes:
        x0, y0, x1, y1 = int(b.xmin), int(b.ymin), int(b.xmax), int(b.ymax)
        if x1 < x0 or y1 < y0:
            slivers += 1
            continue
        if x1 - x0 >= 3 and y1 - y0 >= 3:
            image = pillow_boxes(image, [b], color, font)
            continue
        slivers += 1
        H, W = image.shape[:2]
        image = image.copy()
        image[max(y0, 0):max(min(y1, H - 1) + 1, 0), max(x0, 0):max(min(x1, W - 1) + 1, 0)] = color
        im = Image.fromarray(image)
        ImageDraw.Draw(im).text((b.xmin, b.ymin - 20), str(b.get_score()) + ', ' + str(b.classes[0]) + ', ' + str(b.subject_id),
                                fill=color, font=font)
        image = np.asarray(im)
    return image, slivers


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp('fi_evaluate')
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        S = 96
        rng = np.random.default_rng(7)
        _frames(tmp_path, rng)
        subject_ids = [11, 3, 25, 8, 40]
        reg = rng.normal(size=(5, 64)).astype(np.float32)
        reg /= np.linalg.norm(reg, axis=1, keepdims=True)
        with open('ref_facial_id_db.pickle', 'wb') as f:
            pickle.dump({s: reg[k] for k, s in enumerate(subject_ids)}, f)
        gt = _validation_csv(tmp_path, rng)
        conf = {'fi_conf': _fi_conf(tmp_path, S), 'fd_conf': _fd_conf(tmp_path, S)}
        ident = fi.FaceIdentifier(conf)
        _tune_head(ident.fd, S)
    finally:
        os.chdir(cwd)
    return tmp_path, conf, ident, gt


@pytest.mark.parametrize('bs', [1, 8])
def test_evaluate_end_to_end(world, bs, monkeypatch):
    """The csv of evaluate() is the csv of test(); results_fi/ holds exactly the expected names; every annotated file is
    byte-identical to the Pillow-drawn, Pillow-saved frame.  The synthetic detector yields many boxes with a truncated extent
    below 3 (63 of the drawn boxes at either batch size, measured on an MI355X); _reference_drawing draws those, and only those,
    as DESIGN.md section 17 documents -- every other box is Pillow's own rectangle and text."""
    from PIL import Image
    tmp_path, conf, ident, gt = world
    monkeypatch.chdir(tmp_path)
    files = sorted(glob.glob(str(tmp_path / 'frames' / '*.jpg')))
    out_path = conf['fi_conf']['output_file_path']
    res_dir = tmp_path / 'frames' / 'results_fi'
    ident.fd.hps['eval_batch_size'] = bs
    # sim_th at the median match distance, away from every distance
    det = _detections(ident, files, bs)
    S = ident.image_size
    with open('ref_facial_id_db.pickle', 'rb') as f:
        reg = np.asarray(list(pickle.load(f).values()), np.float64)
    crops = []
    for name, (raw, boxes) in det.items():
        for r in fi.crop_rects(boxes[:60], raw.shape[0], raw.shape[1], S):
            if r is not None:
                crops.append(letterbox_device(ident.model.ctx, np.ascontiguousarray(raw[r[0]:r[0] + r[2], r[1]:r[1] + r[3]]), S)[0])
    ids = np.concatenate([ident.fid_extractor.predict(torch.stack(crops[c:c + 64])) for c in range(0, len(crops), 64)])
    dists = np.sqrt(((ids.astype(np.float64)[:, None, :] - reg[None]) ** 2).sum(-1)).min(axis=1)
    assert len(dists) >= 2 * len(files)
    ds = np.sort(np.asarray(dists))
    k = len(ds) // 2
    ident.hps['sim_th'] = float((ds[k - 1] + ds[k]) / 2)

    ident.test()
    want_csv = open(out_path, 'rb').read()
    os.makedirs(res_dir, exist_ok=True)
    (res_dir / 'stale_detected.jpg').write_bytes(b'stale')
    ident.evaluate()
    got_csv = open(out_path, 'rb').read()
    assert got_csv == want_csv
    assert 0 < got_csv.count(b'\n') < len(dists)                             # rows both kept and rejected

    rows = {}
    for line in got_csv.decode().splitlines():
        rows.setdefault(line.split(',')[0], []).append(line)
    gt_names = set(gt.FILE)
    assert NO_GT not in gt_names
    font = fi._font()
    expected, labelled, slivers, drawn = {}, set(), 0, 0
    for name, (raw, boxes) in det.items():
        _assign_subject_ids(name, boxes, rows.get(name, []))
        gt_boxes = []
        sub = gt[gt.FILE == name]
        for i in range(len(sub)):
            x, y, w, h = (float(v) for v in sub.iloc[i, 3:7])
            if x > 0 and y > 0 and w > 0 and h > 0:
                gt_boxes.append(_box(int(x), int(y), int(x + w - 1), int(y + h - 1), 1.0, sub.iloc[i, 2]))
                gt_boxes[-1].classes = [1.0]
        if not gt_boxes or not boxes:
            continue
        img, s1 = _reference_drawing(raw, gt_boxes, RED, font)
        img, s2 = _reference_drawing(img, boxes, GREEN, font)
        slivers += s1 + s2
        drawn += len(gt_boxes) + len(boxes)
        ref_file = tmp_path / ('ref_' + name)
        Image.fromarray(img).save(os.path.join(str(tmp_path), 'ref_' + name))
        expected[name[:-4] + '_detected' + name[-4:]] = ref_file.read_bytes()
        labelled |= {str(b.subject_id) != '-1' for b in boxes}
    print('frames annotated: %d, boxes: %d, of them drawn by a documented deviation: %d' % (len(expected), drawn, slivers))
    assert drawn - slivers >= 2 * len(expected)                              # Pillow's own rectangle is compared on every frame
    assert len(expected) >= 5 and NO_GT[:-4] + '_detected.jpg' not in expected
    assert sorted(os.listdir(res_dir)) == sorted(expected)                   # the stale file is gone, NO_GT has no copy
    for name, want in expected.items():
        assert (res_dir / name).read_bytes() == want, name
    assert labelled == {True, False}                                         # detections labelled with a subject id, and with -1


def test_evaluate_raises_on_mismatched_image_sizes(world, monkeypatch):
    tmp_path, conf, ident, gt = world
    monkeypatch.chdir(tmp_path)
    conf['fd_conf']['nn_arch']['image_size'] = 128
    try:
        with pytest.raises(ValueError, match='image_size'):
            ident.evaluate()
    finally:
        conf['fd_conf']['nn_arch']['image_size'] = 96
