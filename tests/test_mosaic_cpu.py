"""hps['mosaic'] on the host (no GPU): the validation of the configuration, data.draw_mosaic, ground truth under tiles, and
BatchFeeder's tables."""
import math

import numpy as np
import pytest

import letterbox_mosaic_ref as mref
from face_vijnana_yolov3_amd import data

SIZES = [(72, 96), (96, 72), (80, 80)]           # landscape, portrait, square


@pytest.fixture(scope='module')
def uccs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('uccs_mosaic'))
    df = data.make_synthetic_uccs(root, n_images=6, seed=3, sizes=SIZES)
    return root, df


# ----------------------------------------------------------------------------- 1. configuration
def test_mosaic_off_and_defaults():
    assert data.mosaic_conf(None) is None and data.mosaic_conf(False) is None
    assert data.mosaic_conf(True) == {'prob': 0.5, 'scale': [0.4, 1.0], 'centre': [0.25, 0.75], 'seed': 0}
    assert data.mosaic_conf({}) == data.mosaic_conf(True)
    c = data.mosaic_conf({'prob': 1, 'scale': [1, 2], 'seed': 7})
    assert c == {'prob': 1.0, 'scale': [1.0, 2.0], 'centre': [0.25, 0.75], 'seed': 7} and isinstance(c['prob'], float)
    assert data.augment_conf(True) == dict(data.AUGMENT_DEFAULTS, zoom=[0.75, 1.25])      # untouched by the new key


BAD = ['yes', 1, 0, [0.4, 1.0], {'prop': 1}, {'prob': -0.1}, {'prob': 1.5}, {'prob': True}, {'prob': '1'}, {'prob': float('nan')},
       {'scale': 1.0}, {'scale': [0, 1]}, {'scale': [0.5, 0.4]}, {'scale': [0.5, 2.5]}, {'scale': [0.5, 1, 2]}, {'scale': ['a', 1]},
       {'scale': [0.5, float('inf')]}, {'scale': [True, 1]}, {'centre': 0.5}, {'centre': [0, 0.5]}, {'centre': [0.6, 0.4]},
       {'centre': [0.5, 1.0]}, {'centre': [float('nan'), 0.5]}, {'seed': -1}, {'seed': 1.5}, {'seed': '0'}, {'seed': True}]


@pytest.mark.parametrize('bad', BAD, ids=[repr(b).replace(' ', '') for b in BAD])
def test_bad_mosaic_value_raises_before_a_context_exists(monkeypatch, bad):
    from face_vijnana_yolov3_amd import _lib, face_detection

    def boom(*a, **k):
        raise AssertionError('a context was created')
    monkeypatch.setattr(_lib.Context, '__init__', boom)
    with pytest.raises(ValueError, match='mosaic'):
        data.mosaic_conf(bad)
    for head in ('single', 'three_scale'):
        conf = dict(raw_data_path='.', hps=dict(mosaic=bad), nn_arch=dict(image_size=64, bb_info_c_size=6, head=head), model_loading=False)
        with pytest.raises(ValueError, match='mosaic'):
            face_detection.FaceDetector(conf)


# ----------------------------------------------------------------------------- 2. draw_mosaic
SHAPES = [(80, 100), (100, 80), (64, 64), (7, 5), (33, 500), (1, 1)]


def _draw(mos, aug, epoch, files, S=64, shapes=None):
    shapes = shapes or [SHAPES[f % len(SHAPES)] for f in files]
    tiles, colour = data.draw_mosaic(mos, aug, epoch, files, shapes, S)
    assert tiles.dtype == np.int32 and tiles.ndim == 2 and tiles.shape[1] == 14
    assert (colour is None) == (aug is None)
    if colour is not None:
        assert colour.dtype == np.float32 and colour.shape == (len(tiles), 3)
    return tiles, colour


def test_draw_mosaic_is_deterministic_and_independent_of_the_call_order():
    mos, aug = data.mosaic_conf(True), data.augment_conf(True)
    keys = [(e, f0) for e in range(3) for f0 in range(0, 12, 4)]
    first = {k: _draw(mos, aug, k[0], list(range(k[1], k[1] + 4))) for k in keys}
    again = {k: _draw(mos, aug, k[0], list(range(k[1], k[1] + 4))) for k in reversed(keys)}
    for k in keys:
        assert first[k][0].tobytes() == again[k][0].tobytes() and first[k][1].tobytes() == again[k][1].tobytes()
    blobs = {first[k][0].tobytes() + first[k][1].tobytes() for k in keys}
    assert len(blobs) == len(keys)                                     # every epoch and every set of file indices its own draw
    other = _draw(dict(mos, seed=1), aug, 0, [0, 1, 2, 3])
    assert other[0].tobytes() != first[(0, 0)][0].tobytes()
    # the canvas's own stream: file index f draws the same centre and sides wherever it sits, as long as the slice is as long
    mos1 = data.mosaic_conf({'prob': 1})
    a, _ = _draw(mos1, None, 2, [5, 6, 7, 8], shapes=[(80, 100)] * 4)
    b, _ = _draw(mos1, None, 2, [9, 5, 3, 1], shapes=[(80, 100)] * 4)
    assert np.array_equal(a[0:4, 6:], b[4:8, 6:])                       # T, oy, ox, flip and the window of canvas "file 5"


@pytest.mark.parametrize('augment', [False, True])
def test_windows_partition_the_canvas_and_every_tile_is_feasible(augment):
    mos = data.mosaic_conf({'prob': 0.7, 'scale': [0.05, 2.0], 'centre': [0.01, 0.99]})
    aug = data.augment_conf({'zoom': [0.3, 3.0]}) if augment else None
    mosaics = singles = flips = 0
    for S in (32, 64, 416):
        for e in range(4):
            files = list(range(6 * e, 6 * e + 6))
            tiles, colour = _draw(mos, aug, e, files, S)
            assert (np.diff(tiles[:, 0]) >= 0).all() and sorted(set(tiles[:, 0].tolist())) == list(range(6))
            for i in range(6):
                mine = tiles[tiles[:, 0] == i]
                assert len(mine) in (1, 4) and mine[0, 1] == i          # tile 0 is the canvas's own image
                cover = np.zeros((S, S), np.int32)
                for k, (_c, im, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1) in enumerate(mine.tolist()):
                    h, w = SHAPES[files[im] % len(SHAPES)]
                    assert 0 <= im < 6 and 0 <= cy0 <= h - ch and 0 <= cx0 <= w - cw and ch >= 1 and cw >= 1
                    assert 0 <= wy0 < wy1 <= S and 0 <= wx0 < wx1 <= S and flip in (0, 1)
                    assert 1 <= T <= 4 * S and -T <= oy <= S and -T <= ox <= S
                    cover[wy0:wy1, wx0:wx1] += 1
                    w_p, h_p = data.letterbox_geometry(ch, cw, T)[:2]
                    assert (w_p >= 1 and h_p >= 1) or T == S           # infeasible: the fallback to T = S, as draw_augment's identity
                    flips += flip
                    if len(mine) == 4:
                        assert (cy0, cx0, ch, cw) == (0, 0, h, w)
                        py, px = mine[0, 12], mine[0, 13]                # tile 0's window ends at the centre
                        assert tuple(mine[k]) == mref.quadrant_tile(i, im, h, w, k, py, px, T, flip, S)
                assert (cover == 1).all()
                mosaics += len(mine) == 4; singles += len(mine) == 1
            if not augment:
                assert not tiles[:, 9].any()
    assert mosaics > 20 and singles > 10 and (flips > 20) == augment


def test_prob_0_gives_todays_placements_and_prob_1_only_mosaics():
    S, files = 64, list(range(6))
    shapes = [SHAPES[f] for f in files]
    aug = data.augment_conf(True)
    for a in (None, aug):
        tiles, colour = _draw(data.mosaic_conf({'prob': 0}), a, 3, files, S)
        assert len(tiles) == 6
        for i, (h, w) in enumerate(shapes):
            pl, col = data.draw_augment(a, 3, i, h, w, S) if a else (data.identity_placement(h, w, S), None)
            cy0, cx0, ch, cw, T, oy, ox, flip = pl
            assert tuple(tiles[i]) == (i, i, cy0, cx0, ch, cw, T, oy, S - T - ox if flip else ox, flip, 0, 0, S, S)
            if a:
                assert colour[i].tolist() == np.asarray(col, np.float32).tolist()
        tiles, colour = _draw(data.mosaic_conf({'prob': 1}), a, 3, files, S)
        assert len(tiles) == 24 and tiles[:, 0].tolist() == [i for i in range(6) for _ in range(4)]
        if a:                                                          # a tile carries ITS source image's flip and colour
            for t, c in zip(tiles, colour):
                h, w = shapes[t[1]]
                pl, col = data.draw_augment(a, 3, files[t[1]], h, w, S)
                assert t[9] == pl[7] and c.tolist() == np.asarray(col, np.float32).tolist()
        else:
            assert colour is None and not tiles[:, 9].any()


def test_centre_is_clamped_so_that_no_window_is_empty():
    mos = data.mosaic_conf({'prob': 1, 'centre': [0.001, 0.002]})
    tiles, _ = _draw(mos, None, 0, [0, 1, 2, 3], 32)
    assert (tiles[:, 12] > tiles[:, 10]).all() and (tiles[:, 13] > tiles[:, 11]).all() and tiles[0, 12] == 1 and tiles[0, 13] == 1


# ----------------------------------------------------------------------------- 3. one tile worked out by hand
# S = 64; image 80 x 100 (h x w) whole; T = 48; centre (py, px) = (40, 24); quadrant 1 (top right): window rows 0..39, columns 24..63.
# Letterbox in 48: w_p = 48, h_p = int(80 / 100 * 48) = 38, pad = 10 -> pad_t = 5, pad_l = 0; m = 100.
# The content's bottom-left corner lies at the centre: ox = 24 - 0 = 24, oy = 40 - (5 + 38) = -3.  Content: columns 24..71, rows 2..39.
# Face A (X 40, Y 30, W 11, H 13): x1, x2 = 40, 50; y1, y2 = 30, 42.
#   x1p = int(19.2) + 24 = 43;  x2p = int(24.0) + 24 = 48;  xc = 91 // 2 = 45
#   y1p = int(14.4) + 2 = 16;   y2p = int(20.16) + 2 = 22;  yc = 38 // 2 = 19
#   single head, grid 2, cell 32: cell (0, 1), offsets 13 / 32 and 19 / 32; bw = 11 / 100 * 0.75 = 0.0825, bh = 13 / 100 * 0.75 = 0.0975
#   flipped in the box (pad_l = pad_r = 0, so ox stays 24): xc = 2 * 24 + 47 - 45 = 50 -> cell column 1, offset 18 / 32
# Face B (X 90, Y 30, W 8, H 8): x1p = int(43.2) + 24 = 67, x2p = int(46.56) + 24 = 70, xc = 68: inside the content (24..71) but
#   outside the window (..63): dropped.  Flipped: xc = 95 - 68 = 27, y1p = 16, y2p = int(17.76) + 2 = 19, yc = 17: kept, cell (0, 0),
#   offsets 27 / 32 and 17 / 32, bw = bh = 8 / 100 * 0.75 = 0.06.
HAND = dict(S=64, tile=(0, 0, 0, 0, 80, 100, 48, -3, 24, 0, 0, 24, 40, 64), A=[40, 30, 11, 13], B=[90, 30, 8, 8])


def test_hand_tile_is_what_the_quadrant_rule_gives():
    assert mref.quadrant_tile(0, 0, 80, 100, 1, 40, 24, 48, 0, 64) == HAND['tile']
    assert mref.quadrant_tile(0, 0, 80, 100, 1, 40, 24, 48, 1, 64) == HAND['tile'][:9] + (1,) + HAND['tile'][10:]


def test_hand_tile_single_head():
    S, tile = HAND['S'], HAND['tile']
    faces = [HAND['A'], HAND['B']]
    gt = data.encode_gt(None, 0, 0, S, 2, tiles=[(faces, tile)])
    assert gt[..., 0].sum() == 1.0                                     # B is dropped: its centre lies outside the window
    assert gt[0, 1].tolist() == pytest.approx([1.0, 13 / 32, 19 / 32, 0.0825, 0.0975, 1.0], rel=1e-12)
    assert gt[0, 1, 1] == 13 / 32 and gt[0, 1, 2] == 19 / 32
    flipped = data.encode_gt(None, 0, 0, S, 2, tiles=[(faces, tile[:9] + (1,) + tile[10:])])
    assert flipped[..., 0].sum() == 2.0                                # the mirror brings B into the window
    assert flipped[0, 1].tolist() == pytest.approx([1.0, 18 / 32, 19 / 32, 0.0825, 0.0975, 1.0], rel=1e-12)
    assert flipped[0, 0].tolist() == pytest.approx([1.0, 27 / 32, 17 / 32, 0.06, 0.06, 1.0], rel=1e-12)
    assert data.encode_gt(None, 0, 0, S, 2, tiles=[([HAND['B']], tile)]).sum() == 0


def test_hand_tile_three_scale_head():
    # A in network pixels: 11 / 100 * 48 = 5.28 by 13 / 100 * 48 = 6.24, inside every kept anchor: the smallest, (16, 30) = scale 2
    # anchor 1, has the best IoU; grid 8, cell 8: xc 45 -> column 5, offset 5 / 8; yc 19 -> row 2, offset 3 / 8
    S, tile = HAND['S'], HAND['tile']
    faces = [HAND['A'], HAND['B']]
    t = data.encode_gt_three_scale(None, 0, 0, S, tiles=[(faces, tile)])
    assert t[0].sum() == 0 and t[1].sum() == 0 and np.count_nonzero(t[2][..., 4::6]) == 1
    want = [math.log(0.625 / 0.375), math.log(0.375 / 0.625), math.log(5.28 / 16), math.log(6.24 / 30), 1.0, 1.0]
    assert t[2][2, 5, 6:12].tolist() == pytest.approx(want, rel=1e-12)
    f = data.encode_gt_three_scale(None, 0, 0, S, tiles=[(faces, tile[:9] + (1,) + tile[10:])])
    assert np.count_nonzero(f[2][..., 4::6]) == 2
    want[0] = math.log(0.25 / 0.75)                                    # xc = 50 -> column 6, offset 2 / 8
    assert f[2][2, 6, 6:12].tolist() == pytest.approx(want, rel=1e-12)
    want_b = [math.log(0.375 / 0.625), math.log(0.125 / 0.875), math.log(3.84 / 16), math.log(3.84 / 30), 1.0, 1.0]   # xc 27, yc 17
    assert f[2][2, 3, 6:12].tolist() == pytest.approx(want_b, rel=1e-12)


def test_tiles_are_written_in_order_and_a_later_row_overwrites():
    S = 64
    t0 = (0, 0, 0, 0, 64, 64, 64, 0, 0, 0, 0, 0, 64, 32)               # the left half shows image 0 at scale 1
    t1 = (0, 1, 0, 0, 64, 64, 64, 0, 0, 0, 0, 32, 64, 64)              # the right half image 1
    a, b = [10, 10, 9, 9], [40, 10, 5, 5]                              # centres (14, 14) and (42, 12)
    gt = data.encode_gt(None, 0, 0, S, 1, tiles=[([a, b], t0), ([a, b], t1)])   # grid 1: one cell, the last kept face stays
    assert gt[0, 0].tolist() == pytest.approx([1.0, 42 / 64, 12 / 64, 5 / 64, 5 / 64, 1.0])   # tile 1's b (a lies outside its window)
    gt = data.encode_gt(None, 0, 0, S, 1, tiles=[([a, b], t1), ([a, b], t0)])
    assert gt[0, 0].tolist() == pytest.approx([1.0, 14 / 64, 14 / 64, 9 / 64, 9 / 64, 1.0])   # now tile 0's a is written last


# ----------------------------------------------------------------------------- 4. one full-window tile == placement=
def _rows_per_image(df):
    out = []
    for k, (name, g) in enumerate(sorted(df.groupby('FILE'), key=lambda kv: kv[0])):
        h, w = SIZES[k % len(SIZES)]
        rows = g.iloc[:, 3:7].values.tolist()
        rows.append([w - 20, h - 10, 20, 10])      # touches the right and the bottom edge
        rows.append([1, 1, 9, 7])                  # and the top-left corner
        out.append((h, w, rows))
    return out


@pytest.mark.parametrize('S,grid', [(64, 2), (416, 13)])
def test_one_full_window_tile_is_the_placement_bit_for_bit(uccs, S, grid):
    aug = data.augment_conf({'zoom': [0.4, 2.0], 'flip': 0.5})
    seen_flip = seen_plain = 0
    for k, (h, w, rows) in enumerate(_rows_per_image(uccs[1])):       # landscape, portrait and square, twice
        places = [data.identity_placement(h, w, S)] + [data.draw_augment(aug, e, k, h, w, S)[0] for e in range(6)]
        for pl in places:
            cy0, cx0, ch, cw, T, oy, ox, flip = pl
            tile = (0, 0, cy0, cx0, ch, cw, T, oy, S - T - ox if flip else ox, flip, 0, 0, S, S)
            a = data.encode_gt(rows, h, w, S, grid, placement=pl)
            b = data.encode_gt(None, 0, 0, S, grid, tiles=[(rows, tile)])
            assert a.tobytes() == b.tobytes()
            a3 = data.encode_gt_three_scale(rows, h, w, S, placement=pl)
            b3 = data.encode_gt_three_scale(None, 0, 0, S, tiles=[(rows, tile)])
            for s in range(3):
                assert a3[s].tobytes() == b3[s].tobytes()
            seen_flip += flip and a.sum() > 0; seen_plain += (not flip) and a.sum() > 0
    assert seen_flip > 5 and seen_plain > 5


# ----------------------------------------------------------------------------- 5. BatchFeeder carries the tables
@pytest.mark.parametrize('head', ['single', 'three_scale'])
@pytest.mark.parametrize('augment', [False, True])
def test_batch_feeder_hands_out_draw_mosaics_tables_and_targets(uccs, head, augment):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, split_augment, split_mosaic
    from face_vijnana_yolov3_amd.parallel import slice_batch
    root, _df = uccs
    arch = {'image_size': 64, 'bb_info_c_size': 6, 'head': head}
    mos, aug = data.mosaic_conf({'prob': 0.75}), (data.augment_conf(True) if augment else None)

    def load(world, rank, epoch, index=0, batch_size=6):
        hps = dict(batch_size=batch_size, mosaic={'prob': 0.75})
        if augment:
            hps['augment'] = True
        seq = data.TrainingSequence(root, hps, dict(arch), 2)
        f = BatchFeeder(seq, world, rank, threads=2)
        f.set_epoch(epoch)
        try:
            item = f.load(index)
        finally:
            f.close()
        assert item[0][0] == 'mosaic'
        packed, tables = split_mosaic(item[0])
        assert split_augment(packed) == (packed, None)                 # what is left is the plain packed batch
        names = seq.file_names[index * batch_size:(index + 1) * batch_size]
        lo, hi, _w = slice_batch(len(names), world, rank) if world > 1 else (0, len(names), 1.0)
        tiles, colour, n_out = tables
        assert n_out == hi - lo
        first = index * batch_size + lo
        shapes = [SIZES[(first + i) % len(SIZES)] for i in range(hi - lo)]
        want_t, want_c = data.draw_mosaic(mos, aug, epoch, range(first, first + hi - lo), shapes, 64)
        assert tiles.dtype == np.int32 and np.array_equal(tiles, want_t) and 0 <= tiles[:, 1].min() and tiles[:, 1].max() < hi - lo
        assert (colour is None and want_c is None) or (colour.dtype == np.float32 and np.array_equal(colour, want_c))
        rows = [seq.groups[nm].iloc[:, 3:7].values for nm in names[lo:hi]]
        ys = item[1] if isinstance(item[1], tuple) else (item[1],)
        for i in range(hi - lo):
            enc = seq.encode(None, 0, 0, tiles=[(rows[t[1]], t) for t in want_t if t[0] == i])
            for y, e in zip(ys, enc if isinstance(enc, list) else [enc]):
                assert np.array_equal(y[i].numpy(), e.astype(np.float32))
        return tiles, colour, [y.numpy().copy() for y in ys]

    a, again = load(1, 0, 1), load(1, 0, 1)
    assert np.array_equal(a[0], again[0]) and all(np.array_equal(p, q) for p, q in zip(a[2], again[2]))
    assert 6 < len(a[0]) < 24 and sum(float(np.abs(y).sum()) for y in a[2]) > 0
    other = load(1, 0, 2)
    assert not np.array_equal(a[0], other[0])                          # another epoch: another draw
    # two ranks: each draws its own slice of three -- partners only from that slice, so not the one-rank run's canvases
    r0, r1 = load(2, 0, 1), load(2, 1, 1)
    assert set(r0[0][:, 0].tolist()) == {0, 1, 2} and set(r1[0][:, 0].tolist()) == {0, 1, 2}
    assert not np.array_equal(np.concatenate([r0[0], r1[0]])[:, 1:], a[0][:, 1:])


def test_batch_feeder_without_mosaic_is_todays_item(uccs):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, split_augment, split_mosaic
    root, _df = uccs
    for hps in (dict(batch_size=2), dict(batch_size=2, mosaic=None), dict(batch_size=2, mosaic=False), dict(batch_size=2, augment=True)):
        seq = data.TrainingSequence(root, dict(hps), {'image_size': 64, 'bb_info_c_size': 6}, 2)
        f = BatchFeeder(seq, 1, 0, threads=2)
        try:
            packed, yt, weight, _ = f.load(0)
        finally:
            f.close()
        assert f.mosaic is None and packed[0] != 'mosaic' and split_mosaic(packed) == (packed, None)
        assert (packed[0] == 'augment') == ('augment' in hps)
        if 'augment' not in hps:
            want = np.asarray([seq.encode(seq.groups[nm].iloc[:, 3:7].values, *SIZES[i]) for i, nm in enumerate(seq.file_names[:2])], np.float32)
            assert np.array_equal(yt.numpy(), want)
