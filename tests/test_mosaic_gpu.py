"""hps['mosaic'] on the GPU: fv_letterbox_mosaic_batch against the existing code (fv_letterbox_augment_batch for one full-window
tile, the numpy composition of fv_letterbox_crops boxes for real mosaics: exact), against the float64 restatement of the colour
stage, its refusals, and the training input path end to end."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import letterbox_augment_ref as aref
import letterbox_mosaic_ref as mref
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


def _mosaic(images, tiles, colour, S, n_out, out=None, fill=float('nan')):
    if out is None:
        out = torch.full((n_out, S, S, 3), fill, dtype=torch.float32, device=images[0].device)     # every element must be written
    tiles = np.ascontiguousarray(np.asarray(tiles, np.int32).reshape(-1, 14))
    cp = None
    if colour is not None:
        colour = np.ascontiguousarray(np.asarray(colour, np.float32).reshape(len(tiles), 3))
        cp = colour.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = lib().fv_letterbox_mosaic_batch(_ctx().handle, *packed_args(*images), S, n_out, tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cp,
                                         len(tiles), ptr(out))
    _ctx().check(rc, 'fv_letterbox_mosaic_batch')
    return out


def _augment(images, place, colour, S):
    dbuf, offs, hw = images
    n = len(offs)
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


def _np_bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def _boxes(images, tiles):
    """{(image, cy0, cx0, ch, cw, T): the existing kernel's T x T x 3 box (fi.letterbox_crops at image size T), numpy}"""
    keys = sorted({tuple(int(v) for v in t[1:7]) for t in tiles})
    out = {}
    for T in sorted({k[5] for k in keys}):
        sel = [k for k in keys if k[5] == T]
        got = fi.letterbox_crops(_ctx(), images, [k[:5] for k in sel], T).cpu().numpy()
        out.update({k: got[j] for j, k in enumerate(sel)})
    return out


def _composed(images, tiles, S, n_out):
    """the numpy composition of the existing kernel's boxes, canvas by canvas"""
    boxes = _boxes(images, tiles)
    want = np.zeros((n_out, S, S, 3), np.float32)
    for c in range(n_out):
        mine = [t for t in tiles if int(t[0]) == c]
        want[c] = mref.compose([boxes[tuple(int(v) for v in t[1:7])] for t in mine], mine, S)
    return want


# ----------------------------------------------------------------------------- 1a. one full-window tile == the augment entry
SHAPES = [(80, 100), (100, 80), (64, 64), (50, 71), (9, 7)]


def _placements(S):
    T17 = 17
    return [
        (0, 0, 0, 80, 100, S, 0, 0), (1, 0, 0, 100, 80, S, 0, 0), (2, 0, 0, 64, 64, S, 0, 0), (3, 0, 0, 50, 71, S, 0, 0),
        (0, 50, 60, 30, 40, S, 0, 0), (1, 0, 57, 61, 23, S, 0, 0), (0, 33, 47, 1, 1, S, 0, 0),
        (0, 5, 5, 30, 50, T17, 3, S - T17),     # T = 17: h_p = 10, odd padding 7 = 3 + 4; box at the right edge of the canvas
        (1, 20, 11, 50, 30, T17, S - T17, 5),   # T = 17, portrait: w_p = 10, pad_l 3, pad_r 4: the in-box flip moves the content
        (2, 0, 0, 64, 64, 1, S - 1, 0),         # T = 1
        (4, 0, 0, 9, 7, S - 4, 1, 3),           # a tiny image enlarged
    ]


@pytest.mark.parametrize('S', [32, 64, 96])       # 96: a second, half-filled column of 64-pixel workgroup tiles
def test_one_full_window_tile_is_the_augment_entry_bit_for_bit(S):
    rng = np.random.default_rng(S)
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    images = _upload(raws)
    cases = _placements(S)
    dbuf, offs, hw = images
    batch = (dbuf, [offs[c[0]] for c in cases], [v for c in cases for v in hw[2 * c[0]:2 * c[0] + 2]])
    col = np.float32([[0.1, 1.5, 1 / 1.5], [0, 1, 1], [-0.3, 1.2, 1.4]])[np.arange(len(cases)) % 3]
    for flips in ([0] * len(cases), [1] * len(cases), [k & 1 for k in range(len(cases))]):
        for colour in (None, col):
            want = _augment(batch, [c[1:] + (f,) for c, f in zip(cases, flips)], colour, S)
            tiles = [(k, k) + c[1:6] + (c[6], S - c[5] - c[7] if f else c[7], f, 0, 0, S, S) for k, (c, f) in enumerate(zip(cases, flips))]
            got = _mosaic(batch, tiles, colour, S, len(cases))
            torch.cuda.synchronize()
            for k in range(len(cases)):
                assert _bits_equal(got[k], want[k]), 'case %d %r flip %d colour %s' % (k, cases[k], flips[k], colour is not None)
    whole, _ = letterbox_batch_device(_ctx(), raws[:4], S, _dev())     # the whole image, no flip: also fv_letterbox_batch
    ident = [(k, k) + data.identity_placement(h, w, S)[:7] + (0, 0, 0, S, S) for k, (h, w) in enumerate(SHAPES[:4])]
    assert _bits_equal(_mosaic(_upload(raws[:4]), ident, None, S, 4), whole)


# ----------------------------------------------------------------------------- 1b. mosaics == the composition of fv_letterbox_crops boxes
def _canvases(S):
    """canvases as lists of tile records without the canvas number"""
    def Q(py, px, spec, keep=(0, 1, 2, 3)):
        return [mref.quadrant_tile(0, im, SHAPES[im][0], SHAPES[im][1], q, py, px, T, f, S)[1:] for q, (im, T, f) in enumerate(spec) if q in keep]
    xm = 32 if S >= 64 else 16                     # the middle of a 64-wide workgroup tile (S = 32: of the canvas)
    xb = 64 if S > 64 else S // 2                  # S = 96: exactly on the boundary of the two workgroup columns
    mixed = [(0, S // 2 + 5, 0), (1, 21, 1), (2, S // 2, 0), (3, 21, 1)]        # portrait and landscape; T = 21: odd with odd padding
    big = [(0, S + 20, 1), (1, 2 * S, 0), (2, 1, 0), (3, 4 * S, 0)]            # T > S (boxes reach beyond the canvas), T = 1, T = 4 S
    same = [(0, S - 4, 1), (0, S // 2, 0), (0, 21, 0), (4, S - 4, 1)]          # one source in three tiles; a tiny image enlarged
    out = [Q(24 if S > 32 else 8, xm, mixed), Q(16, xb, mixed), Q(16, xb, big), Q(S - 1, 1, mixed), Q(1, S - 1, same),
           Q(1, 1, big), Q(S - 1, S - 1, same), Q(S // 2 + 3, S // 2 - 5, big), Q(16, xm, same),
           Q(20, xb, mixed, keep=(0, 1, 3)),                                   # three tiles: the bottom-left quadrant stays +0
           Q(20, 9, same, keep=(1, 2))]                                        # two tiles
    # a window that holds only a tile's letterbox padding (the rows above the content of a landscape image), and the rest
    T = S // 2 + 8
    pad_t = data.letterbox_geometry(80, 100, T)[2]
    assert pad_t >= 2
    out.append([(0, 0, 0, 80, 100, T, 0, 0, 0, 0, 0, pad_t, S), (1, 0, 0, 100, 80, S - 3, pad_t, 3, 1, pad_t, 0, S, S)])
    # crops (not whole images) in boxes that reach beyond the canvas on every side, mirrored and not; a column window of one pixel
    out.append([(0, 5, 5, 30, 50, S + 9, -4, -7, 1, 0, 0, S, S - 1), (3, 10, 20, 40, 40, 2 * S, -S // 2, -S, 0, 0, S - 1, S, S)])
    return out


@pytest.mark.parametrize('S', [32, 64, 96])
def test_mosaics_are_the_composition_of_the_existing_kernels_boxes(S):
    rng = np.random.default_rng(100 + S)
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    images = _upload(raws)
    canvases = _canvases(S)
    tiles = [(c,) + tuple(t) for c, cv in enumerate(canvases) for t in cv]
    want = _composed(images, tiles, S, len(canvases))
    got = _mosaic(images, tiles, None, S, len(canvases))
    torch.cuda.synchronize()
    got_np = got.cpu().numpy()
    for c in range(len(canvases)):
        assert _np_bits_equal(got_np[c], want[c]), 'canvas %d %r' % (c, canvases[c])
        assert np.abs(want[c]).sum() > 0
    # the uncovered quadrant and the padding-only window are +0 (bit pattern 0), not merely equal to zero
    assert (got_np[9][20:, :(64 if S > 64 else S // 2)].view(np.int32) == 0).all()
    pad_t = canvases[11][0][11]
    assert (got_np[11][:pad_t].view(np.int32) == 0).all()
    again = _mosaic(images, tiles, None, S, len(canvases))
    assert _bits_equal(again, got)                                     # determinism: two calls, the same bits
    # every tile mirrored the other way: still the composition
    flipped = [t[:9] + (1 - t[9],) + t[10:] for t in tiles]
    got_f = _mosaic(images, flipped, None, S, len(canvases)).cpu().numpy()
    assert _np_bits_equal(got_f, _composed(images, flipped, S, len(canvases)))


def test_twenty_four_tile_canvases_run_in_two_launches():
    S, n = 32, 20                                                      # 80 tiles: 12 canvases in the first launch, 8 in the second
    rng = np.random.default_rng(7)
    shapes = [(int(rng.integers(20, 100)), int(rng.integers(20, 100))) for _ in range(n)]
    raws = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    images = _upload(raws)
    tiles, colour = data.draw_mosaic(data.mosaic_conf({'prob': 1}), data.augment_conf(True), 0, list(range(n)), shapes, S)
    assert len(tiles) == 4 * n and tiles[:, 9].any() and not tiles[:, 9].all()
    got = _mosaic(images, tiles, None, S, n).cpu().numpy()
    want = _composed(images, tiles.tolist(), S, n)
    for c in range(n):
        assert _np_bits_equal(got[c], want[c]), 'canvas %d' % c
    ident = np.tile(np.float32([0, 1, 1]), (4 * n, 1)); ident[4 * 12] = [0.1, 1.5, 1.5]   # the second launch's first tile
    got_c = _mosaic(images, tiles, ident, S, n).cpu().numpy()
    assert _np_bits_equal(got_c[:12], want[:12]) and _np_bits_equal(got_c[13:], want[13:]) and not _np_bits_equal(got_c[12], want[12])


# ----------------------------------------------------------------------------- 2. colour against the float64 restatement
def _photo_like(rng, h, w):
    """smooth colour fields plus noise: neighbouring pixels correlate, as in a photograph"""
    coarse = rng.uniform(0, 255, (h // 8 + 2, w // 8 + 2, 3))
    img = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w]
    img = (img + np.roll(img, 3, 0) + np.roll(img, 5, 1)) / 3 + rng.normal(0, 12, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_colour_stage_against_the_float64_restatement():
    S = 64
    rng = np.random.default_rng(3)
    edge = np.zeros((8, 8, 3), np.uint8); edge[:, 4:] = 255; edge[5:, :, 1] = edge[5:, ::-1, 0]   # enlarged, the bicubic overshoots
    raws = [_photo_like(rng, 80, 100), _photo_like(rng, 100, 80), _photo_like(rng, 64, 64), edge]
    shapes = [r.shape[:2] for r in raws]
    images = _upload(raws)
    records = np.float32([[0.1, 1.5, 1.5], [0.0, 1.0, 1.0], [-0.45, 1 / 1.5, 1.5], [0.05, 1.5, 1 / 1.5]])   # one exactly (0, 1, 1)
    canvases = []
    for (py, px), flips, order in (((24, 32), (0, 1, 0, 1), (0, 1, 2, 3)), ((16, 40), (1, 0, 1, 0), (3, 2, 1, 0)), ((40, 20), (0, 0, 1, 1), (1, 3, 0, 2))):
        canvases.append([mref.quadrant_tile(len(canvases), im, shapes[im][0], shapes[im][1], q, py, px, (40, 56, 64, 72)[q], flips[q], S)
                         for q, im in enumerate(order)])
    tiles = [t for cv in canvases for t in cv]
    colour = np.float32([records[(q + c) % 4] for c, cv in enumerate(canvases) for q in range(4)])
    got = _mosaic(images, tiles, colour, S, len(canvases)).cpu().numpy()
    boxes = _boxes(images, tiles)                                      # the restatement's input: the EXISTING kernel's pixels
    assert min(b.min() for b in boxes.values()) < -0.01 and max(b.max() for b in boxes.values()) > 1.01, 'the edge image must overshoot'
    worst = (0.0, 0.0)
    for c, cv in enumerate(canvases):
        cols = colour[4 * c:4 * c + 4]
        assert sum(tuple(r) == (0.0, 1.0, 1.0) for r in cols.tolist()) == 1
        base = [boxes[tuple(int(v) for v in t[1:7])] for t in cv]
        want64 = mref.compose([mref.colour_box(b, t, r, np.float64) for b, t, r in zip(base, cv, cols)], cv, S, np.float64)
        want32 = mref.compose([mref.colour_box(b, t, r, np.float32) for b, t, r in zip(base, cv, cols)], cv, S, np.float32)
        e_gpu = np.abs(got[c].astype(np.float64) - want64).max()
        e_32 = np.abs(want32.astype(np.float64) - want64).max()
        print('colour run canvas %d: device err %.3e, float32 restatement err %.3e' % (c, e_gpu, e_32))
        worst = max(worst, (e_gpu, e_32))
        assert e_gpu <= 4 * e_32 + 1e-6, 'canvas %d: device err %.3e > 4 x %.3e + 1e-6' % (c, e_gpu, e_32)
        # the tile with the record (0, 1, 1) holds the resampled bits, overshoots included; the others differ from them
        plain = mref.compose(base, cv, S)
        for t, r in zip(cv, cols.tolist()):
            win = (slice(t[10], t[12]), slice(t[11], t[13]))
            assert _np_bits_equal(got[c][win], plain[win]) == (tuple(r) == (0.0, 1.0, 1.0))
    print('colour worst run: device err %.3e (float32 restatement %.3e)' % worst)


# ----------------------------------------------------------------------------- 4. refusals
G = (0, 0, 80, 100, 64, 0, 0, 0, 0, 0, 64, 64)                         # crop, T, oy, ox, flip, window: the whole image in the whole canvas


def _t(canvas, image=0, **kw):
    rec = dict(zip(mref.FIELDS, (canvas, image) + G))
    rec.update(kw)
    return tuple(rec[f] for f in mref.FIELDS)


REFUSED = {
    'canvas_above_range': ([_t(0), _t(1), _t(3)], 3, None),
    'canvas_negative': ([_t(0), _t(1), _t(-1)], 3, None),
    'canvas_decreasing': ([_t(0), _t(1), _t(0)], 2, None),
    'canvas_without_tile': ([_t(0), _t(1, wx1=32), _t(1, wx0=32)], 3, None),
    'canvas_skipped': ([_t(0, wx1=32), _t(0, wx0=32), _t(2)], 3, None),
    'five_tiles': ([_t(0, wx0=0, wx1=8), _t(0, wx0=8, wx1=16), _t(0, wx0=16, wx1=24), _t(0, wx0=24, wx1=32), _t(0, wx0=32, wx1=64)], 2, None),
    'image_above_range': ([_t(0), _t(1), _t(2, image=3)], 3, None),
    'image_negative': ([_t(0), _t(1), _t(2, image=-1)], 3, None),
    'crop_rows_outside': ([_t(0), _t(1), _t(2, ch=81)], 3, None),
    'crop_cols_outside': ([_t(0), _t(1), _t(2, cx0=1)], 3, None),
    'crop_negative': ([_t(0), _t(1), _t(2, cy0=-1, ch=10, cw=10)], 3, None),
    'crop_empty': ([_t(0), _t(1), _t(2, ch=0)], 3, None),
    'T_zero': ([_t(0), _t(1), _t(2, T=0)], 3, None),
    'T_above_4S': ([_t(0), _t(1), _t(2, T=257)], 3, None),
    'oy_below_minus_T': ([_t(0), _t(1), _t(2, oy=-65)], 3, None),
    'ox_below_minus_T': ([_t(0), _t(1), _t(2, ox=-65)], 3, None),
    'oy_above_S': ([_t(0), _t(1), _t(2, oy=65)], 3, None),
    'ox_above_S': ([_t(0), _t(1), _t(2, ox=65)], 3, None),
    'geometry_infeasible': ([_t(0), _t(1), _t(2, ch=1)], 3, None),
    'flip_2': ([_t(0), _t(1), _t(2, flip=2)], 3, None),
    'flip_negative': ([_t(0), _t(1), _t(2, flip=-1)], 3, None),
    'window_empty_rows': ([_t(0), _t(1), _t(2, wy0=10, wy1=10)], 3, None),
    'window_empty_cols': ([_t(0), _t(1), _t(2, wx0=40, wx1=30)], 3, None),
    'window_negative': ([_t(0), _t(1), _t(2, wy0=-1)], 3, None),
    'window_beyond_canvas': ([_t(0), _t(1), _t(2, wx1=65)], 3, None),
    'windows_overlap': ([_t(0), _t(1, wx1=33), _t(1, wx0=32)], 2, None),
    'colour_nan': ([_t(0), _t(1), _t(2)], 3, [[0, 1, 1], [0, 1, 1], [np.nan, 1, 1]]),
    'colour_inf': ([_t(0), _t(1), _t(2)], 3, [[0, 1, 1], [0, 1, 1], [0, np.inf, 1]]),
}


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_bad_record_is_refused_and_dst_untouched(name):
    S = 64
    tiles, n_out, colour = REFUSED[name]
    rng = np.random.default_rng(4)
    images = _upload([rng.integers(0, 256, (80, 100, 3)).astype(np.uint8) for _ in range(3)])
    out = torch.full((3, S, S, 3), 7.0, dtype=torch.float32, device=_dev())
    with pytest.raises(FvError, match='letterbox_mosaic_batch'):
        _mosaic(images, tiles, colour, S, n_out, out=out)              # the bad record is the LAST: nothing before it may have run
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_bad_image_size_is_refused_and_good_records_run():
    S = 64
    rng = np.random.default_rng(4)
    images = _upload([rng.integers(0, 256, (80, 100, 3)).astype(np.uint8) for _ in range(3)])
    out = torch.full((3, S, S, 3), 7.0, dtype=torch.float32, device=_dev())
    with pytest.raises(FvError, match='letterbox_mosaic_batch'):
        _mosaic(images, [_t(c, T=62, wy1=62, wx1=62) for c in range(3)], None, 62, 3, out=out[:, :62, :62].contiguous())
    with pytest.raises(FvError, match='letterbox_mosaic_batch'):
        _mosaic(images, [_t(0), _t(1)], None, S, 3, out=out)           # fewer tiles than canvases
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    _mosaic(images, [_t(0), _t(1), _t(2)], None, S, 3, out=out)
    assert (out != 7.0).all()
    with pytest.raises(ValueError, match='mosaic'):
        letterbox_batch_device(_ctx(), None, S, _dev(), packed=(images[0].cpu(), images[1], images[2]), aug=([G[:8]] * 3, None),
                               mosaic=([_t(0), _t(1), _t(2)], None, 3))


# ----------------------------------------------------------------------------- 5. the training input path end to end
E2E_SIZES = [(72, 96), (96, 72), (80, 80), (64, 88)]


@pytest.fixture(scope='module')
def uccs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('uccs_mosaic_gpu'))
    data.make_synthetic_uccs(root, n_images=4, seed=5, sizes=E2E_SIZES)
    return root


def _stage(root, head, mosaic, augment, device_jpeg, epoch):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, DeviceStager
    hps = dict(batch_size=4, device_jpeg=device_jpeg)
    if mosaic is not None:
        hps['mosaic'] = mosaic
    if augment is not None:
        hps['augment'] = augment
    seq = data.TrainingSequence(root, hps, {'image_size': 64, 'bb_info_c_size': 6, 'head': head}, 2)
    feeder = BatchFeeder(seq, 1, 0, threads=2)
    eng = types.SimpleNamespace(ctx=_ctx(), dev=_dev())
    try:
        feeder.set_epoch(epoch)
        x, yd, _weight, ev = DeviceStager(eng, 64).stage(feeder.load(0))
        ev.synchronize()
    finally:
        feeder.close()
    return seq, x, yd


@pytest.mark.parametrize('head', ['single', 'three_scale'])
@pytest.mark.parametrize('device_jpeg', [True, False], ids=['device_jpeg', 'pillow'])
@pytest.mark.parametrize('augment', [None, True], ids=['mosaic_only', 'with_augment'])
def test_staged_batch_is_the_direct_call_with_the_drawn_tables(uccs, head, device_jpeg, augment):
    S = 64
    seq, x, yd = _stage(uccs, head, {'prob': 1}, augment, device_jpeg, epoch=3)
    names = seq.file_names[:4]
    raws = [data._pil_loader(os.path.join(uccs, nm)) for nm in names]
    shapes = [r.shape[:2] for r in raws]
    aug = data.augment_conf(augment)
    tiles, colour = data.draw_mosaic(data.mosaic_conf({'prob': 1}), aug, 3, range(4), shapes, S)
    assert len(tiles) == 16 and (colour is None) == (augment is None)
    want = _mosaic(_upload(raws), tiles, colour, S, 4)
    assert x.shape == (4, S, S, 3) and _bits_equal(x, want)
    rows = [seq.groups[nm].iloc[:, 3:7].values for nm in names]
    enc = [seq.encode(None, 0, 0, tiles=[(rows[t[1]], t) for t in tiles if t[0] == i]) for i in range(4)]
    if head == 'three_scale':
        for s in range(3):
            assert np.array_equal(yd[s].cpu().numpy(), np.asarray([e[s] for e in enc], np.float32))
        assert sum(float(np.abs(e[s]).sum()) for e in enc for s in range(3)) > 0
    else:
        assert np.array_equal(yd.cpu().numpy(), np.asarray(enc, np.float32)) and np.asarray(enc).sum() > 0
    _seq, x_other, _ = _stage(uccs, head, {'prob': 1}, augment, device_jpeg, epoch=4)
    assert not torch.equal(x_other, x)                                 # another epoch: another draw
    _seq, x_again, _ = _stage(uccs, head, {'prob': 1}, augment, device_jpeg, epoch=3)
    assert _bits_equal(x_again, x)
    # mosaic absent: what is staged without this key -- fv_letterbox_batch, or the augment launch
    _seq, x_off, _ = _stage(uccs, head, None, augment, device_jpeg, epoch=3)
    if augment is None:
        parent, _ = letterbox_batch_device(_ctx(), raws, S, _dev())
    else:
        drawn = [data.draw_augment(aug, 3, i, h, w, S) for i, (h, w) in enumerate(shapes)]
        parent = _augment(_upload(raws), [d[0] for d in drawn], [d[1] for d in drawn], S)
    assert _bits_equal(x_off, parent)


@pytest.mark.parametrize('head', ['single', 'three_scale'])
def test_two_training_steps_with_mosaic_finish_with_a_finite_loss(uccs, head, tmp_path, monkeypatch, capsys):
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    monkeypatch.chdir(tmp_path)
    conf = {'mode': 'train', 'raw_data_path': uccs, 'test_path': uccs, 'output_file_path': str(tmp_path / 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.9, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 2, 'step': 1, 'batch_size': 4, 'face_conf_th': 0.5,
                    'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'augment': True, 'mosaic': {'prob': 1}},
            'nn_arch': {'image_size': 64, 'bb_info_c_size': 6, 'head': head, 'num_classes': 1}}
    fd = FaceDetector(conf)
    assert fd.mosaic == data.mosaic_conf({'prob': 1}) and fd.augment == data.augment_conf(True)
    fd.train()
    losses = [float(v) for v in re.findall(r'^1/1 - loss: (\S+)$', capsys.readouterr().out, flags=re.M)]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), losses
    assert fd.model.iterations == 2 and torch.isfinite(fd.model.params).all()
