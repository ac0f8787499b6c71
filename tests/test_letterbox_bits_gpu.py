"""The bicubic letterbox entry points (fv_letterbox, fv_letterbox_batch, fv_letterbox_crops, fv_letterbox_augment_batch,
fv_letterbox_mosaic_batch) against tests/letterbox_bits_ref.py -- the float32 restatement of the resampling in the kernel's
order, which is NOT derived from the code under test -- bit for bit (int32 views), dst pre-filled with NaN.  No colour stage: it
keeps its own tolerance tests (test_augment_gpu.py, test_mosaic_gpu.py)."""
import numpy as np
import pytest
import torch

import letterbox_bits_ref as bref
import letterbox_mosaic_ref as mref
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context
from face_vijnana_yolov3_amd.postproc import letterbox_batch_device, letterbox_device

pytestmark = pytest.mark.gpu

SHAPES = [(80, 100), (100, 80), (64, 64), (50, 71), (9, 7)]
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _dev():
    return torch.device('cuda', 0)


def _raws(S, shapes=SHAPES):
    rng = np.random.default_rng(1000 + S)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


def _upload(raws):
    """list of uint8 images -> (device uint8 buffer, offsets, hw), as letterbox_batch_device's `keep` hands them out"""
    buf = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws])).to(_dev())
    offs = np.cumsum([0] + [r.size for r in raws])[:-1].tolist()
    hw = [int(v) for r in raws for v in r.shape[:2]]
    return buf, offs, hw


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=_dev())


def _assert_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert len(bad) == 0, '%s: %d of %d values differ, the first at %r: %r != %r' % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _crops(S):
    """(image, y0, x0, h, w): whole images, crops touching each edge pair, 1 x 1 crops, the tiny image (enlarged)"""
    return [(0, 0, 0, 80, 100), (1, 0, 0, 100, 80), (2, 0, 0, 64, 64), (3, 0, 0, 50, 71), (4, 0, 0, 9, 7),
            (0, 0, 0, 30, 40), (0, 50, 60, 30, 40), (1, 0, 57, 61, 23), (1, 93, 0, 7, 19),
            (0, 33, 47, 1, 1), (3, 49, 70, 1, 1), (4, 2, 1, 5, 6)]


def _placements(S):
    """(image, cy0, cx0, ch, cw, T, oy, ox): every crop of _crops in the whole canvas, then boxes of side 17, 1 and S - 4"""
    T17 = 17
    return [c + (S, 0, 0) for c in _crops(S)] + [
        (0, 5, 5, 30, 50, T17, 3, S - T17),     # T = 17: h_p = 10, odd padding 7 = 3 + 4; box at the right edge of the canvas
        (1, 20, 11, 50, 30, T17, S - T17, 5),   # T = 17, portrait: w_p = 10; box at the bottom edge
        (3, 0, 0, 50, 71, T17, 0, 0),
        (2, 0, 0, 64, 64, 1, S - 1, 0),         # T = 1
        (2, 7, 9, 20, 20, 1, 0, S - 1),
        (4, 0, 0, 9, 7, S - 4, 1, 3),           # a tiny image enlarged
    ]


@pytest.mark.parametrize('S', [32, 64, 96, 17, 30])
def test_whole_images_and_crops(S):
    raws = _raws(S)
    want = np.stack([bref.box(r, S) for r in raws])
    for k, r in enumerate(raws):
        out, _ = letterbox_device(_ctx(), r, S, out=_nan(S, S, 3))
        _assert_bits(out, want[k], 'fv_letterbox of image %d at %d' % (k, S))
    out, _ = letterbox_batch_device(_ctx(), raws, S, _dev(), out=_nan(len(raws), S, S, 3))
    _assert_bits(out, want, 'fv_letterbox_batch at %d' % S)
    crops = _crops(S)
    out = fi.letterbox_crops(_ctx(), _upload(raws), crops, S, out=_nan(len(crops), S, S, 3))
    _assert_bits(out, np.stack([bref.crop_box(raws[c[0]], c[1:], S) for c in crops]), 'fv_letterbox_crops at %d' % S)


@pytest.mark.parametrize('S', [32, 64, 96])       # 96: a second, half-filled column of 64-pixel workgroup tiles
def test_augment_and_mosaic(S):
    raws = _raws(S)
    dbuf, offs, hw = _upload(raws)
    cases = _placements(S)
    batch = (dbuf, [offs[c[0]] for c in cases], [v for c in cases for v in hw[2 * c[0]:2 * c[0] + 2]])
    for flips in ([0] * len(cases), [1] * len(cases), [k & 1 for k in range(len(cases))]):
        place = [c[1:] + (f,) for c, f in zip(cases, flips)]
        want = np.stack([bref.augment(raws[c[0]], p, S) for c, p in zip(cases, place)])
        out, _ = letterbox_batch_device(_ctx(), None, S, _dev(), out=_nan(len(cases), S, S, 3), packed=batch, aug=(place, None))
        _assert_bits(out, want, 'fv_letterbox_augment_batch at %d, flips %r' % (S, flips[:2]))
        # mosaic: every placement as a one-tile canvas with a full window (the flip is in the box), then four-tile canvases
        tiles = [(k, c[0]) + tuple(p) + (0, 0, S, S) for k, (c, p) in enumerate(zip(cases, place))]
        for py, px, spec in ((S // 2 + 3, S // 2 - 5, ((0, S // 2 + 5), (1, 17), (2, S // 2), (3, 21))),
                             (16, 64 if S > 64 else S // 2, ((3, S + 20), (4, S - 4), (2, 1), (1, 2 * S))),
                             (1, S - 1, ((0, 17), (0, S), (4, 17), (2, 1)))):
            cv = tiles[-1][0] + 1
            tiles += [mref.quadrant_tile(cv, im, SHAPES[im][0], SHAPES[im][1], q, py, px, T, (q + flips[1]) & 1, S)
                      for q, (im, T) in enumerate(spec)]
        n_out = tiles[-1][0] + 1
        want = np.stack([bref.mosaic(raws, [t for t in tiles if t[0] == c], S) for c in range(n_out)])
        out, _ = letterbox_batch_device(_ctx(), None, S, _dev(), out=_nan(n_out, S, S, 3), packed=(dbuf, offs, hw), mosaic=(tiles, None, n_out))
        _assert_bits(out, want, 'fv_letterbox_mosaic_batch at %d, flips %r' % (S, flips[:2]))


def test_lists_longer_than_one_launches_table():
    """65 images or crops (64 per launch) and 13 four-tile canvases (48 tiles per launch) at S = 16"""
    S, n = 16, 65
    rng = np.random.default_rng(65)
    shapes = [(int(rng.integers(3, 12)), int(rng.integers(3, 12))) for _ in range(n)]
    raws = _raws(S, shapes)
    images = _upload(raws)
    want = np.stack([bref.box(r, S) for r in raws])
    out, _ = letterbox_batch_device(_ctx(), raws, S, _dev(), out=_nan(n, S, S, 3))
    _assert_bits(out, want, 'fv_letterbox_batch, 65 images')
    crops = [(k, 1, 0, h - 1, w) for k, (h, w) in enumerate(shapes)]
    out = fi.letterbox_crops(_ctx(), images, crops, S, out=_nan(n, S, S, 3))
    _assert_bits(out, np.stack([bref.crop_box(raws[c[0]], c[1:], S) for c in crops]), 'fv_letterbox_crops, 65 crops')
    place = [(0, 1, h, w - 1, 12, k % 5, (3 * k) % 5, k & 1) for k, (h, w) in enumerate(shapes)]
    out, _ = letterbox_batch_device(_ctx(), None, S, _dev(), out=_nan(n, S, S, 3), packed=images, aug=(place, None))
    _assert_bits(out, np.stack([bref.augment(r, p, S) for r, p in zip(raws, place)]), 'fv_letterbox_augment_batch, 65 images')
    tiles = [mref.quadrant_tile(c, 4 * c + q, shapes[4 * c + q][0], shapes[4 * c + q][1], q, 3 + c % 11, 12 - c % 10, 8 + (c + q) % 9,
                                (c + q) & 1, S) for c in range(13) for q in range(4)]
    out, _ = letterbox_batch_device(_ctx(), None, S, _dev(), out=_nan(13, S, S, 3), packed=images, mosaic=(tiles, None, 13))
    _assert_bits(out, np.stack([bref.mosaic(raws, tiles[4 * c:4 * c + 4], S) for c in range(13)]), 'fv_letterbox_mosaic_batch, 13 canvases')
