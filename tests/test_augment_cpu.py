"""hps['augment'] on the host (no GPU): ground truth under a placement, data.draw_augment, the validation of the configuration,
BatchFeeder's tables, and the sanity of the numpy restatement the GPU tests judge the kernel's colour stage by."""
import math
import os

import numpy as np
import pytest

import letterbox_augment_ref as ref
from face_vijnana_yolov3_amd import data

SIZES = [(72, 96), (96, 72), (80, 80)]           # landscape, portrait, square


@pytest.fixture(scope='module')
def uccs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('uccs_aug'))
    df = data.make_synthetic_uccs(root, n_images=6, seed=3, sizes=SIZES)
    return root, df


# ----------------------------------------------------------------------------- 1. identity placement == placement None
def _rows_per_image(df):
    out = []
    for k, (name, g) in enumerate(sorted(df.groupby('FILE'), key=lambda kv: kv[0])):
        h, w = SIZES[k % len(SIZES)]
        rows = g.iloc[:, 3:7].values.tolist()
        rows.append([w - 20, h - 10, 20, 10])      # touches the right and the bottom edge: x2 = w - 1, y2 = h - 1
        rows.append([1, 1, 9, 7])                  # and the top-left corner
        out.append((h, w, rows))
    return out


@pytest.mark.parametrize('S,grid', [(64, 2), (416, 13)])
def test_identity_placement_is_placement_none_bit_for_bit(uccs, S, grid):
    for h, w, rows in _rows_per_image(uccs[1]):
        ident = data.identity_placement(h, w, S)
        assert ident == (0, 0, h, w, S, 0, 0, 0)
        a = data.encode_gt(rows, h, w, S, grid)
        b = data.encode_gt(rows, h, w, S, grid, placement=ident)
        assert a.sum() > 0 and a.tobytes() == b.tobytes()
        a3 = data.encode_gt_three_scale(rows, h, w, S)
        b3 = data.encode_gt_three_scale(rows, h, w, S, placement=ident)
        assert sum(t.sum() for t in a3) != 0
        for s in range(3):
            assert a3[s].tobytes() == b3[s].tobytes()


# ----------------------------------------------------------------------------- 2. a placement worked out by hand
# S = 64; image 80 x 100 (h x w); crop rows 10..49, columns 20..69 (40 x 50); box T = 48 at (oy, ox) = (8, 16).
# Crop letterbox in 48: w_p = 48, h_p = int(40 / 50 * 48) = 38, pad = 10 -> pad_t = 5; m = 50.  Content: columns 16..63, rows 13..50.
# Face A (X 40, Y 30, W 11, H 13): x1, x2 = 40, 50; y1, y2 = 30, 42.
#   x1p = int(20 / 50 * 48) + 16 = 19 + 16 = 35;  x2p = int(30 / 50 * 48) + 16 = 28 + 16 = 44;  xc = 79 // 2 = 39
#   y1p = int(20 / 50 * 48) + 13 = 32;            y2p = int(32 / 50 * 48) + 13 = 30 + 13 = 43;  yc = 75 // 2 = 37
#   single head, grid 2, cell 32: cell (1, 1), offsets 7 / 32 and 5 / 32; bw = 11 / 50 * 0.75 = 0.165, bh = 13 / 50 * 0.75 = 0.195
#   flipped: xc = 63 - 39 = 24 -> cell column 0, offset 24 / 32
# Face B (X 5, Y 5, W 10, H 10): x1p = int(-14.4) + 16 = 2, x2p = int(-5.76) + 16 = 11, xc = 6 < 16: outside, dropped.
HAND = dict(S=64, h=80, w=100, place=(10, 20, 40, 50, 48, 8, 16, 0), A=[40, 30, 11, 13], B=[5, 5, 10, 10])


def test_hand_placement_single_head():
    S, h, w, pl = HAND['S'], HAND['h'], HAND['w'], HAND['place']
    gt = data.encode_gt([HAND['A'], HAND['B']], h, w, S, 2, placement=pl)
    assert gt[..., 0].sum() == 1.0                                     # B is dropped
    assert gt[1, 1].tolist() == pytest.approx([1.0, 7 / 32, 5 / 32, 0.165, 0.195, 1.0], rel=1e-12)
    assert gt[1, 1, 1] == 7 / 32 and gt[1, 1, 2] == 5 / 32
    flipped = data.encode_gt([HAND['A'], HAND['B']], h, w, S, 2, placement=pl[:7] + (1,))
    assert flipped[..., 0].sum() == 1.0
    assert flipped[1, 0].tolist() == pytest.approx([1.0, 24 / 32, 5 / 32, 0.165, 0.195, 1.0], rel=1e-12)
    assert data.encode_gt([HAND['B']], h, w, S, 2, placement=pl).sum() == 0


def test_hand_placement_three_scale_head():
    # box in network pixels 11 / 50 * 48 = 10.56 by 13 / 50 * 48 = 12.48: best IoU with the anchor (16, 30) = scale 2, anchor 1;
    # grid 8, cell 8: cell (4, 4), offsets 7 / 8 and 5 / 8; flipped: xc = 24 -> column 3, offset 0 -> clamped to 0.5 / 8
    S, h, w, pl = HAND['S'], HAND['h'], HAND['w'], HAND['place']
    t = data.encode_gt_three_scale([HAND['A'], HAND['B']], h, w, S, placement=pl)
    assert t[0].sum() == 0 and t[1].sum() == 0 and np.count_nonzero(t[2][..., 4::6]) == 1
    want = [math.log(0.875 / 0.125), math.log(0.625 / 0.375), math.log(10.56 / 16), math.log(12.48 / 30), 1.0, 1.0]
    assert t[2][4, 4, 6:12].tolist() == pytest.approx(want, rel=1e-12)
    f = data.encode_gt_three_scale([HAND['A'], HAND['B']], h, w, S, placement=pl[:7] + (1,))
    want[0] = math.log(0.0625 / 0.9375)
    assert np.count_nonzero(f[2][..., 4::6]) == 1
    assert f[2][4, 3, 6:12].tolist() == pytest.approx(want, rel=1e-12)


# ----------------------------------------------------------------------------- 3. draw_augment
IDENTITY_CONF = {"zoom": [1, 1], "flip": 0, "hue": 0, "saturation": 1, "exposure": 1}


def test_draw_augment_is_a_pure_function_of_its_arguments():
    c = data.augment_conf(True)
    assert c == dict(data.AUGMENT_DEFAULTS, zoom=[0.75, 1.25])
    keys = [(e, f) for e in range(3) for f in range(5)]
    first = {k: data.draw_augment(c, k[0], k[1], 80, 100, 64) for k in keys}
    again = {k: data.draw_augment(c, k[0], k[1], 80, 100, 64) for k in reversed(keys)}      # another call order
    assert first == again
    assert len(set(first.values())) == len(keys)                       # every epoch and every file index its own draw
    assert data.draw_augment(dict(c, seed=1), 0, 0, 80, 100, 64) != first[(0, 0)]


def test_draw_augment_stays_inside_image_and_canvas():
    c = data.augment_conf({'zoom': [0.3, 3.0], 'flip': 0.5})
    seen_in = seen_out = flips = 0
    for f, (h, w) in enumerate([(80, 100), (100, 80), (64, 64), (7, 5), (1, 1), (33, 500)] * 40):
        S = (64, 32, 416)[f % 3]
        (cy0, cx0, ch, cw, T, oy, ox, flip), (dh, sat, ex) = data.draw_augment(c, f // 7, f, h, w, S)
        assert 1 <= ch <= h and 1 <= cw <= w and 0 <= cy0 <= h - ch and 0 <= cx0 <= w - cw
        assert 1 <= T <= S and 0 <= ox <= S - T and 0 <= oy <= S - T and flip in (0, 1)
        assert (T == S and ox == 0 and oy == 0) or (ch, cw) == (h, w)  # zoom in crops, zoom out shrinks; never both
        w_p, h_p = data.letterbox_geometry(ch, cw, T)[:2]
        assert (w_p >= 1 and h_p >= 1) or (cy0, cx0, ch, cw, T, oy, ox, flip) == data.identity_placement(h, w, S)
        assert -0.1 <= dh <= 0.1 and 1 / 1.5 <= sat <= 1.5 and 1 / 1.5 <= ex <= 1.5
        seen_in += T == S and (ch, cw) != (h, w); seen_out += T < S; flips += flip
    assert seen_in > 20 and seen_out > 20 and 60 < flips < 180


def test_identity_configuration_draws_the_identity():
    c = data.augment_conf(IDENTITY_CONF)
    for e in range(3):
        for f, (h, w) in enumerate([(80, 100), (100, 80), (64, 64), (1, 1)]):
            assert data.draw_augment(c, e, f, h, w, 64) == (data.identity_placement(h, w, 64), (0.0, 1.0, 1.0))


def test_infeasible_geometry_falls_back_to_the_identity_placement():
    c = data.augment_conf({'zoom': [0.5, 2.0], 'flip': 1.0})
    for f in range(8):
        assert data.draw_augment(c, 0, f, 1, 500, 64)[0] == data.identity_placement(1, 500, 64)


# ----------------------------------------------------------------------------- 4. validation
BAD = ['yes', 1, 0, [0.75, 1.25], {'zoon': [1, 1]}, {'zoom': 1.0}, {'zoom': [0, 1]}, {'zoom': [0.5, 0.9]}, {'zoom': [1.1, 1.2]},
       {'zoom': [0.5, 1, 2]}, {'zoom': ['a', 2]}, {'flip': -0.1}, {'flip': 1.5}, {'flip': True}, {'hue': 0.6}, {'hue': -0.1},
       {'saturation': 0.9}, {'exposure': 0.5}, {'exposure': float('nan')}, {'saturation': float('inf')}, {'seed': -1}, {'seed': 1.5},
       {'seed': '0'}]


@pytest.mark.parametrize('bad', BAD, ids=[repr(b).replace(' ', '') for b in BAD])
def test_bad_augment_value_raises_before_a_context_exists(monkeypatch, bad):
    from face_vijnana_yolov3_amd import _lib, face_detection

    def boom(*a, **k):
        raise AssertionError('a context was created')
    monkeypatch.setattr(_lib.Context, '__init__', boom)
    with pytest.raises(ValueError, match='augment'):
        data.augment_conf(bad)
    for head in ('single', 'three_scale'):
        conf = dict(raw_data_path='.', hps=dict(augment=bad), nn_arch=dict(image_size=64, bb_info_c_size=6, head=head), model_loading=False)
        with pytest.raises(ValueError, match='augment'):
            face_detection.FaceDetector(conf)


def test_augment_off_and_defaults():
    assert data.augment_conf(None) is None and data.augment_conf(False) is None
    assert data.augment_conf({}) == data.augment_conf(True)
    c = data.augment_conf({'zoom': [1, 2], 'seed': 7})
    assert c['zoom'] == [1.0, 2.0] and c['seed'] == 7 and c['flip'] == 0.5 and c['hue'] == 0.1


# ----------------------------------------------------------------------------- BatchFeeder carries the tables
@pytest.mark.parametrize('head', ['single', 'three_scale'])
def test_batch_feeder_draws_per_file_whatever_the_batching(uccs, head):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, split_augment
    root, _df = uccs
    arch = {'image_size': 64, 'bb_info_c_size': 6, 'head': head}
    aug = data.augment_conf(True)

    def per_file(batch_size, world, rank, epoch):
        seq = data.TrainingSequence(root, dict(batch_size=batch_size, augment=True), dict(arch), 2)
        f = BatchFeeder(seq, world, rank, threads=2)
        f.set_epoch(epoch)
        got = {}
        try:
            for index in range(len(seq)):
                item = f.load(index)
                names = seq.file_names[index * batch_size:(index + 1) * batch_size]
                from face_vijnana_yolov3_amd.parallel import slice_batch
                lo, hi, _w = slice_batch(len(names), world, rank) if world > 1 else (0, len(names), 1.0)
                packed, tables = split_augment(item[0])
                assert tables is not None and item[0][0] == 'augment'
                place, colour = tables
                assert place.dtype == np.int32 and place.shape == (hi - lo, 8) and colour.dtype == np.float32 and colour.shape == (hi - lo, 3)
                ys = item[1] if isinstance(item[1], tuple) else (item[1],)
                for i, nm in enumerate(names[lo:hi]):
                    got[nm] = (tuple(place[i].tolist()), tuple(colour[i].tolist()), [y[i].numpy().copy() for y in ys], seq)
        finally:
            f.close()
        return got

    a = per_file(2, 1, 0, 1)
    assert len(a) == 6
    for nm, (pl, col, ys, seq) in a.items():
        fi = seq.file_names.index(nm)
        h, w = SIZES[fi % len(SIZES)]
        want_pl, want_col = data.draw_augment(aug, 1, fi, h, w, 64)
        assert pl == want_pl and col == tuple(np.asarray(want_col, np.float32).tolist())
        enc = seq.encode(seq.groups[nm].iloc[:, 3:7].values, h, w, placement=want_pl)
        enc = enc if isinstance(enc, list) else [enc]
        for y, e in zip(ys, enc):
            assert np.array_equal(y, e.astype(np.float32))
    for other in (per_file(3, 1, 0, 1), {**per_file(2, 2, 0, 1), **per_file(2, 2, 1, 1)}):
        assert sorted(other) == sorted(a)
        for nm in a:
            assert other[nm][:2] == a[nm][:2] and all(np.array_equal(p, q) for p, q in zip(other[nm][2], a[nm][2]))
    b = per_file(2, 1, 0, 2)                                           # another epoch: another draw
    assert all(b[nm][:2] != a[nm][:2] for nm in a)


def test_batch_feeder_without_augment_is_todays_item(uccs):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, split_augment
    root, _df = uccs
    seq = data.TrainingSequence(root, dict(batch_size=2), {'image_size': 64, 'bb_info_c_size': 6}, 2)
    f = BatchFeeder(seq, 1, 0, threads=2)
    try:
        packed, yt, weight, _ = f.load(0)
    finally:
        f.close()
    assert packed[0] != 'augment' and split_augment(packed) == (packed, None)
    want = np.asarray([seq.encode(seq.groups[nm].iloc[:, 3:7].values, *SIZES[i]) for i, nm in enumerate(seq.file_names[:2])], np.float32)
    assert np.array_equal(yt.numpy(), want)


# ----------------------------------------------------------------------------- 5. the restatement itself
def test_restatement_hand_checked_two_by_two():
    # a 2 x 2 image shrunk to one pixel: source coordinate 0.5 on both axes, bicubic weights (-3/32, 19/32, 19/32, -3/32) with the
    # border replicated -> 1/2, 1/2 per axis: the mean of the four pixels.  Placed at (oy, ox) = (1, 0) of a 2 x 2 canvas.
    img = np.array([[[255, 0, 0], [0, 0, 0]], [[0, 0, 0], [255, 0, 0]]], np.uint8)
    pl = (0, 0, 2, 2, 1, 1, 0, 0)
    want = np.zeros((2, 2, 3)); want[1, 0] = [0.5, 0, 0]
    assert np.allclose(ref.augment(img, pl, None, 2), want, rtol=0, atol=1e-15)
    want_f = np.zeros((2, 2, 3)); want_f[1, 1] = [0.5, 0, 0]
    assert np.allclose(ref.augment(img, pl[:7] + (1,), None, 2), want_f, rtol=0, atol=1e-15)
    # exposure 1.5 on (0.5, 0, 0): v = 0.75, s = 1, h = 0 -> (0.75, 0, 0); a hue shift of 1/3 then makes it green
    assert np.allclose(ref.augment(img, pl, (0.0, 1.0, 1.5), 2)[1, 0], [0.75, 0, 0], rtol=0, atol=1e-15)
    assert np.allclose(ref.augment(img, pl, (1 / 3, 1.0, 1.5), 2)[1, 0], [0, 0.75, 0], rtol=0, atol=1e-15)
    # T = 2 in a 2 x 2 canvas: scale 1, weights (0, 1, 0, 0): the image itself over 255
    assert np.allclose(ref.augment(img, (0, 0, 2, 2, 2, 0, 0, 0), None, 2), img / 255.0, rtol=0, atol=1e-15)


@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-15), (np.float32, 1e-6)])
def test_restatement_colour_identity_and_hue_third(dtype, tol):
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.2, 1.2, (50, 3))
    assert np.array_equal(ref.colour_stage(x, 0.0, 1.0, 1.0, dtype), x.astype(dtype))          # skipped: not even clamped
    y = ref.colour_stage(x, 0.0, 1.0, 1.0, dtype, skip_identity=False)                        # the arithmetic is the identity on [0, 1]
    assert y.dtype == np.dtype(dtype) and np.abs(y - np.clip(x, 0, 1)).max() <= 4 * tol
    red = np.array([[1.0, 0.0, 0.0]])
    assert np.abs(ref.colour_stage(red, 1 / 3, 1.0, 1.0, dtype) - [[0, 1, 0]]).max() <= 4 * tol
    assert np.abs(ref.colour_stage(red, 2 / 3, 1.0, 1.0, dtype) - [[0, 0, 1]]).max() <= 4 * tol
    assert np.abs(ref.colour_stage(red, -1 / 3, 1.0, 1.0, dtype) - [[0, 0, 1]]).max() <= 4 * tol
    grey = np.array([[0.4, 0.4, 0.4], [0.0, 0.0, 0.0]])
    assert np.abs(ref.colour_stage(grey, 0.1, 1.5, 1.5, dtype) - [[0.6] * 3, [0.0] * 3]).max() <= 4 * tol
    two_max = np.array([[0.8, 0.8, 0.2]])                                                      # h = 1/6 whichever maximum is chosen
    assert np.abs(ref.colour_stage(two_max, 1 / 6, 1.0, 1.0, dtype) - [[0.2, 0.8, 0.2]]).max() <= 4 * tol
