"""hps['augment'] on the GPU: fv_letterbox_augment_batch against the existing letterbox kernels (geometry: exact), against the
float64 restatement of its colour stage (tests/letterbox_augment_ref.py), its refusals, and the training input path end to end.

Colour figures of one run on an MI355X (printed by test_colour_stage_against_the_float64_restatement; the bound of a run is
4 x its float32-restatement error + 1e-6): in all 36 runs the device's error equalled the float32 restatement's, between 6.1e-08
and 1.181e-06."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import letterbox_augment_ref as ref
from face_vijnana_yolov3_amd import data
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError, lib, packed_args, ptr
from face_vijnana_yolov3_amd.postproc import letterbox_batch_device

pytestmark = pytest.mark.gpu

_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _dev():
    return torch.device('cuda', 0)


def _upload(raws):
    """list of uint8 images -> (device uint8 buffer, offsets, hw), as letterbox_batch_device's `keep` hands them out"""
    buf = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws])).to(_dev())
    offs = np.cumsum([0] + [r.size for r in raws])[:-1].tolist()
    hw = [int(v) for r in raws for v in r.shape[:2]]
    return buf, offs, hw


def _repeat(images, idx):
    """the images idx[0], idx[1], ... of `images` as a batch of their own (offsets may repeat: nothing is copied)"""
    dbuf, offs, hw = images
    return dbuf, [offs[i] for i in idx], [v for i in idx for v in hw[2 * i:2 * i + 2]]


def _augment(images, place, colour, S, out=None):
    dbuf, offs, hw = images
    n = len(offs)
    if out is None:
        out = torch.empty((n, S, S, 3), dtype=torch.float32, device=dbuf.device)
    place = np.ascontiguousarray(np.asarray(place, np.int32).reshape(n, 8))
    cp = None
    if colour is not None:
        colour = np.ascontiguousarray(np.asarray(colour, np.float32).reshape(n, 3))
        cp = colour.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = lib().fv_letterbox_augment_batch(_ctx().handle, *packed_args(dbuf, offs, hw), S, place.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          cp, ptr(out))
    _ctx().check(rc, 'fv_letterbox_augment_batch')
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _expected_canvases(images, cases, S, flip):
    """cases: (image, cy0, cx0, ch, cw, T, oy, ox) -> what the existing kernel makes of each crop (fi.letterbox_crops at T), placed"""
    want = torch.zeros((len(cases), S, S, 3), dtype=torch.float32, device=_dev())
    for T in sorted({c[5] for c in cases}):
        sel = [k for k, c in enumerate(cases) if c[5] == T]
        boxes = fi.letterbox_crops(_ctx(), images, [cases[k][:5] for k in sel], T)
        for j, k in enumerate(sel):
            oy, ox = cases[k][6], cases[k][7]
            want[k, oy:oy + T, ox:ox + T] = boxes[j]
    return want.flip(2) if flip else want


# ----------------------------------------------------------------------------- 1. geometry: the existing kernels' bits
SHAPES = [(80, 100), (100, 80), (64, 64), (50, 71), (9, 7)]


def _geometry_cases(S):
    T17 = 17
    return [
        (0, 0, 0, 80, 100, S, 0, 0),            # the whole image, landscape
        (1, 0, 0, 100, 80, S, 0, 0),            # portrait
        (2, 0, 0, 64, 64, S, 0, 0),             # square
        (3, 0, 0, 50, 71, S, 0, 0),             # odd sizes
        (0, 0, 0, 30, 40, S, 0, 0),             # a crop touching the top and the left edge
        (0, 50, 60, 30, 40, S, 0, 0),           # the bottom and the right edge
        (1, 0, 57, 61, 23, S, 0, 0),            # top and right, portrait crop
        (1, 93, 0, 7, 19, S, 0, 0),             # bottom and left, a flat crop
        (0, 33, 47, 1, 1, S, 0, 0),             # 1 x 1 crop
        (3, 49, 70, 1, 1, S, 0, 0),             # 1 x 1 crop in the last corner
        (0, 5, 5, 30, 50, T17, 3, S - T17),     # T = 17: h_p = 10, odd padding 7 = 3 + 4; box at the right edge of the canvas
        (1, 20, 11, 50, 30, T17, S - T17, 5),   # T = 17, portrait: w_p = 10; box at the bottom edge
        (3, 0, 0, 50, 71, T17, 0, 0),
        (2, 0, 0, 64, 64, 1, S - 1, 0),         # T = 1
        (2, 7, 9, 20, 20, 1, 0, S - 1),
        (4, 0, 0, 9, 7, S - 4, 1, 3),           # a tiny image enlarged
    ]


@pytest.mark.parametrize('S', [32, 64, 96])       # 96: a second, half-filled column of 64-pixel tiles
def test_geometry_is_the_existing_kernels_bit_for_bit(S):
    rng = np.random.default_rng(S)
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    images = _upload(raws)
    cases = _geometry_cases(S)
    batch = _repeat(images, [c[0] for c in cases])
    want = _expected_canvases(images, cases, S, flip=False)
    got = _augment(batch, [c[1:] + (0,) for c in cases], None, S)
    torch.cuda.synchronize()
    for k, c in enumerate(cases):
        assert _bits_equal(got[k], want[k]), 'case %d %r' % (k, c)
        T, oy, ox = c[5:8]
        mask = torch.ones((S, S), dtype=torch.bool, device=_dev()); mask[oy:oy + T, ox:ox + T] = False
        assert (got[k][mask].view(torch.int32) == 0).all(), 'case %d: padding is not +0' % k
    flipped = _augment(batch, [c[1:] + (1,) for c in cases], None, S)
    assert _bits_equal(flipped, got.flip(2))
    mixed = _augment(batch, [c[1:] + (k & 1,) for k, c in enumerate(cases)], None, S)   # per-image flip flags in one launch
    for k in range(len(cases)):
        assert _bits_equal(mixed[k], flipped[k] if k & 1 else got[k])
    # the whole image: also fv_letterbox_batch
    whole, _ = letterbox_batch_device(_ctx(), raws[:4], S, _dev())
    assert _bits_equal(got[:4], whole)
    again = _augment(batch, [c[1:] + (0,) for c in cases], None, S)
    assert _bits_equal(again, got)


def test_sixty_five_images_run_in_two_launches():
    S = 32
    rng = np.random.default_rng(65)
    raws = [rng.integers(0, 256, (int(rng.integers(3, 10)), int(rng.integers(3, 10)), 3)).astype(np.uint8) for _ in range(65)]
    images = _upload(raws)
    cases = [(i, 0, 0, r.shape[0], r.shape[1], S - (i % 3) * 4, i % 3, (i % 3) * 3) for i, r in enumerate(raws)]
    want = _expected_canvases(images, cases, S, flip=False)
    got = _augment(images, [c[1:] + (0,) for c in cases], None, S)
    assert _bits_equal(got, want)
    col = np.tile(np.float32([0.0, 1.0, 1.0]), (65, 1)); col[64] = [0.1, 1.5, 1.5]
    got_c = _augment(images, [c[1:] + (0,) for c in cases], col, S)
    assert _bits_equal(got_c[:64], want[:64]) and not _bits_equal(got_c[64], want[64])     # image 64 = the second launch's first


# ----------------------------------------------------------------------------- 2. colour given but (0, 1, 1)
def test_identity_colour_record_gives_the_bits_of_no_colour():
    S = 64
    rng = np.random.default_rng(2)
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES[:4]]
    images = _upload(raws)
    place = [(0, 0, 80, 100, S, 0, 0, 1), (10, 5, 70, 60, 40, 8, 16, 0), (0, 0, 64, 64, S, 0, 0, 0), (5, 5, 8, 8, S, 0, 0, 1)]
    plain = _augment(images, place, None, S)
    col = np.float32([[0, 1, 1], [0.1, 1.5, 1.5], [0, 1, 1], [0, 1, 1]])
    got = _augment(images, place, col, S)
    for k in (0, 2, 3):          # image 3 is an 8 x 8 crop enlarged eight times: overshoots below 0 and above 1 stay, nothing is clamped
        assert _bits_equal(got[k], plain[k])
    assert not _bits_equal(got[1], plain[1])
    assert _bits_equal(_augment(images, place, np.tile(np.float32([0, 1, 1]), (4, 1)), S), plain)


# ----------------------------------------------------------------------------- 3. colour against the float64 restatement
def _photo_like(rng, h, w):
    """smooth colour fields plus noise: neighbouring pixels correlate, as in a photograph"""
    coarse = rng.uniform(0, 255, (h // 8 + 2, w // 8 + 2, 3))
    img = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w]
    img = (img + np.roll(img, 3, 0) + np.roll(img, 5, 1)) / 3 + rng.normal(0, 12, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _constructed():
    """64 x 64, shown at scale 1 (bicubic weights exactly (0, 1, 0, 0)): every pixel reaches the colour stage as value / 255"""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    img[0:8] = np.arange(64, dtype=np.uint8)[None, :, None] * 4                 # greys: d == 0 (black included)
    img[8:12] = 0                                                               # black
    img[12:16] = 255                                                            # white
    for k, rgb in enumerate([(200, 200, 50), (50, 200, 200), (200, 50, 200), (255, 255, 0), (0, 255, 255), (255, 0, 255),
                             (255, 0, 0), (0, 255, 0), (0, 0, 255), (1, 1, 0), (254, 255, 255), (0, 0, 1), (128, 127, 127),
                             (3, 2, 3), (255, 254, 0), (9, 9, 9)]):          # two equal maxima, primaries, nearly grey, nearly black
        img[16:24, 4 * k:4 * k + 4] = rgb
    return img


def _edge():
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, 4:] = 255                                                            # hard black / white edge: enlarged, the bicubic overshoots
    img[5:, :, 1] = img[5:, ::-1, 0]                                            # and a coloured part, so that the hue is not always 0
    return img


COLOURS = [(0.1, 1.5, 1.5), (-0.1, 1 / 1.5, 1 / 1.5), (0.1, 1 / 1.5, 1.5), (-0.1, 1.5, 1 / 1.5), (0.45, 1.5, 1.0), (-0.45, 1.0, 1.5),
           (0.0, 1.0, 1.5), (0.0, 1.5, 1.0), (0.05, 1.0, 1.0)]                   # +-0.45 wraps h through 1 (and 0) for most hues


def test_colour_stage_against_the_float64_restatement():
    S = 64
    rng = np.random.default_rng(3)
    raws = [_photo_like(rng, 80, 100), _photo_like(rng, 100, 80), _constructed(), _edge()]
    images = _upload(raws)
    placements = [(7, 16, 67, 84, S, 0, 0, 0), (0, 0, 100, 80, 48, 9, 16, 1), (0, 0, 64, 64, S, 0, 0, 0), (0, 0, 8, 8, S, 0, 0, 1)]
    col32 = np.float32(COLOURS)
    runs = [(i, c) for i in range(len(raws)) for c in range(len(COLOURS))]
    batch = _repeat(images, [i for i, _c in runs])
    got = _augment(batch, [placements[i] for i, _c in runs], col32[[c for _i, c in runs]], S).cpu().numpy()
    # the input of the restatement: the EXISTING kernel's pixels of the same crops (test 1 pins them equal to the uncoloured output)
    base = [fi.letterbox_crops(_ctx(), images, [(i,) + placements[i][:4]], placements[i][4])[0].cpu().numpy() for i in range(len(raws))]
    assert base[3].min() < -0.01 and base[3].max() > 1.01, 'the edge image must overshoot'
    assert np.array_equal(base[2], raws[2].astype(np.float32) / np.float32(255)) or np.abs(base[2] - raws[2] / 255.0).max() < 1e-6
    worst = (0.0, 0.0)
    for k, (i, c) in enumerate(runs):
        pl = placements[i]
        top, left, h_p, w_p = ref.content_rect((0, 0) + pl[2:5] + (0, 0, 0))
        dh, sat, ex = [float(v) for v in col32[c]]                           # the float32 values the device was given
        box64, box32 = base[i].astype(np.float64), base[i].copy()
        sl = (slice(top, top + h_p), slice(left, left + w_p))
        box64[sl] = ref.colour_stage(base[i][sl], dh, sat, ex, np.float64)
        box32[sl] = ref.colour_stage(base[i][sl], dh, sat, ex, np.float32)
        want64, want32 = ref.place(box64, pl, S), ref.place(box32, pl, S)
        assert want64.min() >= 0 and want64.max() <= 1
        e_gpu = np.abs(got[k].astype(np.float64) - want64).max()
        e_32 = np.abs(want32.astype(np.float64) - want64).max()
        print('colour run image %d (dh %+.2f sat %.3f exp %.3f): device err %.3e, float32 restatement err %.3e' % (i, dh, sat, ex, e_gpu, e_32))
        worst = max(worst, (e_gpu, e_32))
        assert e_gpu <= 4 * e_32 + 1e-6, 'image %d colour %r: device err %.3e > 4 x %.3e + 1e-6' % (i, COLOURS[c], e_gpu, e_32)
    print('colour worst run: device err %.3e (float32 restatement %.3e)' % worst)


# ----------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize('bad', [(0, 0, 81, 100, 64, 0, 0, 0), (0, 1, 80, 100, 64, 0, 0, 0), (-1, 0, 10, 10, 64, 0, 0, 0), (0, 0, 0, 10, 64, 0, 0, 0),
                                 (0, 0, 80, 100, 65, 0, 0, 0), (0, 0, 80, 100, 0, 0, 0, 0), (0, 0, 80, 100, 48, 0, 17, 0), (0, 0, 80, 100, 48, 17, 0, 0),
                                 (0, 0, 80, 100, 48, -1, 0, 0), (0, 0, 80, 100, 64, 0, 0, 2), (0, 0, 80, 100, 64, 0, 0, -1), (0, 0, 1, 100, 64, 0, 0, 0)],
                         ids=['crop_rows_outside', 'crop_cols_outside', 'crop_negative', 'crop_empty', 'T_above_S', 'T_zero', 'ox_above_S_minus_T',
                              'oy_above_S_minus_T', 'oy_negative', 'flip_2', 'flip_negative', 'geometry_infeasible'])
def test_bad_record_is_refused_and_dst_untouched(bad):
    S = 64
    rng = np.random.default_rng(4)
    images = _upload([rng.integers(0, 256, (80, 100, 3)).astype(np.uint8) for _ in range(3)])
    good = (0, 0, 80, 100, 64, 0, 0, 0)
    out = torch.full((3, S, S, 3), 7.0, dtype=torch.float32, device=_dev())
    with pytest.raises(FvError, match='letterbox_augment_batch'):
        _augment(images, [good, good, bad], None, S, out=out)           # the bad record is the LAST: nothing before it may have run
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(FvError, match='letterbox_augment_batch'):
        _augment(images, [good] * 3, np.float32([[0, 1, 1], [0, 1, 1], [np.nan, 1, 1]]), S, out=out)
    with pytest.raises(FvError, match='letterbox_augment_batch'):
        _augment(images, [(0, 0, 80, 100, 62, 0, 0, 0)] * 3, None, 62, out=out[:, :62, :62].contiguous())   # image_size not a multiple of 4
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    _augment(images, [good] * 3, None, S, out=out)
    assert (out != 7.0).all()


# ----------------------------------------------------------------------------- 5. the training input path end to end
E2E_SIZES = [(72, 96), (96, 72), (80, 80), (64, 88)]


@pytest.fixture(scope='module')
def uccs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('uccs_aug_gpu'))
    data.make_synthetic_uccs(root, n_images=4, seed=5, sizes=E2E_SIZES)
    return root


def _stage(root, head, augment, device_jpeg, epoch, index=1):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, DeviceStager
    hps = dict(batch_size=2, device_jpeg=device_jpeg)
    if augment is not None:
        hps['augment'] = augment
    seq = data.TrainingSequence(root, hps, {'image_size': 64, 'bb_info_c_size': 6, 'head': head}, 2)
    feeder = BatchFeeder(seq, 1, 0, threads=2)
    eng = types.SimpleNamespace(ctx=_ctx(), dev=_dev())
    try:
        feeder.set_epoch(epoch)
        x, yd, _weight, ev = DeviceStager(eng, 64).stage(feeder.load(index))
        ev.synchronize()
    finally:
        feeder.close()
    return seq, x, yd


@pytest.mark.parametrize('head', ['single', 'three_scale'])
@pytest.mark.parametrize('device_jpeg', [True, False], ids=['device_jpeg', 'pillow'])
def test_staged_batch_is_the_direct_call_with_the_drawn_parameters(uccs, head, device_jpeg):
    S, index = 64, 1
    seq, x, yd = _stage(uccs, head, True, device_jpeg, epoch=3, index=index)
    names = seq.file_names[2 * index:2 * index + 2]
    raws = [data._pil_loader(os.path.join(uccs, nm)) for nm in names]
    aug = data.augment_conf(True)
    drawn = [data.draw_augment(aug, 3, 2 * index + i, r.shape[0], r.shape[1], S) for i, r in enumerate(raws)]
    want = _augment(_upload(raws), [d[0] for d in drawn], [d[1] for d in drawn], S)
    assert _bits_equal(x, want)
    enc = [seq.encode(seq.groups[nm].iloc[:, 3:7].values, r.shape[0], r.shape[1], placement=d[0]) for nm, r, d in zip(names, raws, drawn)]
    if head == 'three_scale':
        for s in range(3):
            assert np.array_equal(yd[s].cpu().numpy(), np.asarray([e[s] for e in enc], np.float32))
        plain = [data.encode_gt_three_scale(seq.groups[nm].iloc[:, 3:7].values, r.shape[0], r.shape[1], S) for nm, r in zip(names, raws)]
        assert any(not np.array_equal(e[s], p[s]) for e, p in zip(enc, plain) for s in range(3))
    else:
        assert np.array_equal(yd.cpu().numpy(), np.asarray(enc, np.float32))
    _seq, x_other, _ = _stage(uccs, head, True, device_jpeg, epoch=4, index=index)
    assert not torch.equal(x_other, x)                                 # another epoch of the same index: another draw
    _seq, x_again, _ = _stage(uccs, head, True, device_jpeg, epoch=3, index=index)
    assert _bits_equal(x_again, x)
    _seq, x_off, y_off = _stage(uccs, head, None, device_jpeg, epoch=3, index=index)
    whole, _ = letterbox_batch_device(_ctx(), raws, S, _dev())
    assert _bits_equal(x_off, whole)                                   # augment absent: today's launch


@pytest.mark.parametrize('head', ['single', 'three_scale'])
def test_two_training_steps_with_augment_finish_with_a_finite_loss(uccs, head, tmp_path, monkeypatch, capsys):
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    monkeypatch.chdir(tmp_path)
    conf = {'mode': 'train', 'raw_data_path': uccs, 'test_path': uccs, 'output_file_path': str(tmp_path / 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.9, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2, 'face_conf_th': 0.5,
                    'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'augment': True},
            'nn_arch': {'image_size': 64, 'bb_info_c_size': 6, 'head': head, 'num_classes': 1}}
    fd = FaceDetector(conf)
    assert fd.augment == data.augment_conf(True)
    fd.train()
    losses = [float(v) for v in re.findall(r'^\d+/2 - loss: (\S+)$', capsys.readouterr().out, flags=re.M)]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), losses
    assert fd.model.iterations == 2 and torch.isfinite(fd.model.params).all()
