"""hps['tiles'] without a GPU: data.tiles_conf / data.tile_grid, and the float64 restatement of the projection and the greedy
cross-tile merge (tests/tile_merge_ref.py) on a synthetic round trip and on hand-built cases."""
import ctypes

import numpy as np
import pytest

from face_vijnana_yolov3_amd import data
import tile_merge_ref as ref


# ----------------------------------------------------------------------------- tiles_conf
def test_conf_off_and_defaults():
    assert data.tiles_conf(None) is None and data.tiles_conf(False) is None
    c = data.tiles_conf(True)
    assert c == {'size': 1024, 'overlap': 0.2, 'full': True, 'metric': 'ios', 'merge_th': 0.5, 'max_tiles': 64}
    assert data.tiles_conf({}) == c
    c = data.tiles_conf({'size': 32, 'overlap': 0, 'full': False, 'metric': 'iou', 'merge_th': 1, 'max_tiles': 1})
    assert c == {'size': 32, 'overlap': 0.0, 'full': False, 'metric': 'iou', 'merge_th': 1.0, 'max_tiles': 1}
    assert type(c['overlap']) is float and type(c['merge_th']) is float
    assert data.tiles_conf({'overlap': 0.5, 'max_tiles': 64})['overlap'] == 0.5


@pytest.mark.parametrize('bad', [
    {'sise': 512}, {'size': 31}, {'size': 512.0}, {'size': True}, {'size': '512'},
    {'overlap': -0.01}, {'overlap': 0.51}, {'overlap': True}, {'overlap': float('nan')}, {'overlap': '0.2'},
    {'full': 1}, {'full': None}, {'metric': 'giou'}, {'metric': 0},
    {'merge_th': 0}, {'merge_th': 1.01}, {'merge_th': True}, {'merge_th': float('inf')},
    {'max_tiles': 0}, {'max_tiles': 65}, {'max_tiles': 8.0}, {'max_tiles': False},
    'yes', 1, [512],
])
def test_conf_rejects_and_names_the_key(bad):
    with pytest.raises(ValueError, match='tiles'):
        data.tiles_conf(bad)
    if isinstance(bad, dict):
        with pytest.raises(ValueError, match='tiles.*%s' % list(bad)[0]):
            data.tiles_conf(bad)


def test_conf_refuses_the_three_scale_head_only_when_on():
    assert data.tiles_conf(None, 'three_scale') is None and data.tiles_conf(False, 'three_scale') is None
    for v in (True, {'size': 256}):
        with pytest.raises(NotImplementedError, match='tiles'):
            data.tiles_conf(v, 'three_scale')
    assert data.tiles_conf(True, 'single') is not None


def test_face_detector_checks_tiles_before_a_device_is_touched(monkeypatch):
    """FaceDetector.__init__ raises on a bad `tiles` (and on the three-scale head) before it builds an engine."""
    from face_vijnana_yolov3_amd import engine, face_detection

    def no_device(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(engine, 'Engine', no_device)
    conf = {'raw_data_path': '.', 'test_path': '.', 'model_loading': False, 'nn_arch': {'image_size': 96, 'bb_info_c_size': 6},
            'hps': {'num_cands': 60, 'tiles': {'size': 8}}}
    with pytest.raises(ValueError, match='tiles.size'):
        face_detection.FaceDetector(conf)
    conf['hps']['tiles'] = True
    conf['nn_arch']['head'] = 'three_scale'
    with pytest.raises(NotImplementedError, match='tiles'):
        face_detection.FaceDetector(conf)


# ----------------------------------------------------------------------------- tile_grid
def _frames():
    rng = np.random.default_rng(5)
    return [(1, 1), (31, 2000), (1024, 1024), (1025, 1024), (3456, 5184)] + [tuple(int(v) for v in rng.integers(1, 4000, 2)) for _ in range(6)]


@pytest.mark.parametrize('hw', _frames(), ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('size,overlap', [(1024, 0.2), (640, 0.5), (777, 0.0), (1500, 0.33)])
@pytest.mark.parametrize('full', [True, False])
def test_grid_properties(hw, size, overlap, full):
    h, w = hw
    conf = data.tiles_conf({'size': size, 'overlap': overlap, 'full': full})
    want = ref.tile_grid(h, w, size, overlap, full, max_tiles=10 ** 9)
    if len(want) > 64:                                     # never a silently thinner grid
        with pytest.raises(ValueError, match=r'tiles\.max_tiles.*%d x %d' % (w, h)):
            data.tile_grid(h, w, conf)
        return
    grid = data.tile_grid(h, w, conf)
    assert grid == want
    assert all(type(v) is int for g in grid for v in g) and len(set(grid)) == len(grid)
    stride = max(1, int(size * (1 - overlap)))
    tiles = grid
    if full and grid != [(0, 0, h, w)]:
        assert grid[-1] == (0, 0, h, w) and grid.count((0, 0, h, w)) == 1          # last, once
        tiles = grid[:-1]
    elif not full:
        assert (0, 0, h, w) not in grid or grid == [(0, 0, h, w)]
    cover_y, cover_x = np.zeros(h, bool), np.zeros(w, bool)
    for y0, x0, th, tw in tiles:
        assert 0 <= y0 and 0 <= x0 and th >= 1 and tw >= 1 and y0 + th <= h and x0 + tw <= w   # inside the frame
        assert th == min(size, h) and tw == min(size, w)                                       # `size` long wherever the frame is
        cover_y[y0:y0 + th] = True; cover_x[x0:x0 + tw] = True
    assert cover_y.all() and cover_x.all()                 # the tiles are a product of spans: every pixel is covered
    ys = sorted({g[0] for g in tiles}); xs = sorted({g[1] for g in tiles})
    assert tiles == [(y, x, min(size, h), min(size, w)) for y in ys for x in xs]                # row-major product
    for starts in (ys, xs):
        assert starts[0] == 0 and all(0 < b - a <= stride for a, b in zip(starts, starts[1:]))


def test_grid_known_counts_and_max_tiles():
    conf = data.tiles_conf(True)
    assert data.tile_grid(1, 1, conf) == [(0, 0, 1, 1)]
    assert data.tile_grid(1024, 1024, conf) == [(0, 0, 1024, 1024)]                 # exactly the frame: no second copy
    assert data.tile_grid(1025, 1024, conf) == [(0, 0, 1024, 1024), (1, 0, 1024, 1024), (0, 0, 1025, 1024)]
    assert data.tile_grid(31, 2000, conf) == [(0, 0, 31, 1024), (0, 819, 31, 1024), (0, 976, 31, 1024), (0, 0, 31, 2000)]
    assert len(data.tile_grid(3456, 5184, conf)) == 4 * 7 + 1
    small = data.tiles_conf({'max_tiles': 28})
    with pytest.raises(ValueError, match=r'tiles\.max_tiles.*5184 x 3456'):
        data.tile_grid(3456, 5184, small)
    assert len(data.tile_grid(3456, 5184, data.tiles_conf({'max_tiles': 28, 'full': False}))) == 28
    # the kernel's candidate cap: views x num_cands, checked on the host
    assert len(data.tile_views(3456, 5184, conf, 60)) == 29
    with pytest.raises(ValueError, match=r'tiles.*5184 x 3456'):
        data.tile_views(3456, 5184, conf, 142)                                       # 29 x 142 = 4118 > 4096
    assert len(data.tile_views(3456, 5184, conf, 141)) == 29


# ----------------------------------------------------------------------------- round trip on the reference
def _to_view(face, tile, S):
    """A face's frame box clipped to the tile, mapped to the tile's network pixels as the letterbox places it, truncated to int;
    None when less than half of the face's area is inside the tile."""
    y0, x0, th, tw = tile
    fx0, fy0, fx1, fy1 = face
    cx0, cy0, cx1, cy1 = max(fx0, x0), max(fy0, y0), min(fx1, x0 + tw), min(fy1, y0 + th)
    if cx1 <= cx0 or cy1 <= cy0 or (cx1 - cx0) * (cy1 - cy0) < 0.5 * (fx1 - fx0) * (fy1 - fy0):
        return None
    pad_t, pad_l = ref.letterbox_pads(th, tw, S)
    m = max(th, tw)
    return (int((cx0 - x0) * S / m) + pad_l, int((cy0 - y0) * S / m) + pad_t, int((cx1 - x0) * S / m) + pad_l, int((cy1 - y0) * S / m) + pad_t)


def _round_trip_views(seed):
    """25 faces of 8 .. 200 px in a 2000 x 3000 frame, seen by the 3 x 4 tiles of 1024 and the whole frame.  Scores are distinct and
    ordered by the visible share first (a detector scores a cut face below a whole one), random within a share.  The network size
    is 2208 so that the claim below is a theorem and not luck: two truncated whole-face boxes of side s whose corners are off by
    less than E each overlap by at least (s - E)^2 / (s + E)^2 of the smaller, which is >= 0.5 for E <= 0.1716 s; for the
    smallest face (8 px) that asks for a step of at most 1.37 source pixels in the coarsest view, the whole frame: 3000 / 2208 =
    1.36.  At 416 the whole-frame view (7.2 pixels per network pixel) cannot place an 8-pixel face, with or without tiles."""
    H, W, S, K = 2000, 3000, 2208, 60
    rng = np.random.default_rng(seed)
    grid = ref.tile_grid(H, W, 1024, 0.2, True, 64)
    faces = []
    while len(faces) < 25:                       # seeded faces of 8 .. 200 px that keep clear of one another
        s = int(rng.integers(8, 201))
        x, y = int(rng.integers(0, W - s)), int(rng.integers(0, H - s))
        if all(x + s + 40 < f[0] or f[2] + 40 < x or y + s + 40 < f[1] or f[3] + 40 < y for f in faces):
            faces.append((x, y, x + s, y + s))
    T = len(grid)
    boxes = np.full((T, K, 4), -1, np.int32); score = np.zeros((T, K), np.float32); count = np.zeros(T, np.int32)
    seen = []                                    # (visible share, tie-breaker, view, box)
    for t, tile in enumerate(grid):
        for f in faces:
            b = _to_view(f, tile, S)
            if b is not None:
                y0, x0, th, tw = tile
                vis = (min(f[2], x0 + tw) - max(f[0], x0)) * (min(f[3], y0 + th) - max(f[1], y0)) / ((f[2] - f[0]) * (f[3] - f[1]))
                seen.append((vis, rng.random(), t, b))
    for rank, (_vis, _r, t, b) in enumerate(sorted(seen)):
        boxes[t, count[t]] = b; score[t, count[t]] = np.float32(rank + 1) / np.float32(len(seen) + 1); count[t] += 1
    return H, W, S, grid, faces, dict(boxes=boxes, score=score, count=count)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_round_trip_one_box_per_face(seed):
    H, W, S, grid, faces, views = _round_trip_views(seed)
    assert len(np.unique(views['score'][views['score'] > 0])) == int(views['count'].sum()) > len(faces)        # distinct scores
    out = ref.merge_views(views, grid, S, 'ios', 0.5)
    n = int(out['nrows'][0])
    assert n == len(faces)                                     # exactly one box per face
    K = views['score'].shape[1]
    left = list(faces)
    for r in range(n):
        t = int(out['src'][0, r]) // K
        step = max(grid[t][2], grid[t][3]) / S                 # source pixels per network pixel of the view the box came from
        c = out['corners'][0, r]
        hit = [f for f in left if max(abs(c[0] - f[0]), abs(c[1] - f[1]), abs(c[2] - f[2]), abs(c[3] - f[3])) <= step]
        assert len(hit) == 1, (r, c, step)
        left.remove(hit[0])
    assert not left
    assert (np.diff(out['rows'][0, :n, 4]) < 0).all()          # descending score
    assert np.array_equal(out['rows'][0, :n, 2], out['corners'][0, :n, 2] - out['corners'][0, :n, 0])
    assert (out['src'][0, n:] == -1).all() and not out['corners'][0, n:].any() and not out['rows'][0, n:].any()


def test_round_trip_iou_at_one_merges_identical_boxes_only():
    H, W, S, grid, faces, views = _round_trip_views(3)
    # every view's candidates, projected: at merge_th 1.0 with 'iou' a candidate dies only to an identical box
    boxes, score, count = views['boxes'].copy(), views['score'].copy(), views['count'].copy()
    t_full = len(grid) - 1
    k = int(count[t_full])
    boxes[t_full, k] = boxes[t_full, 0]; score[t_full, k] = np.float32(0.5) * score[t_full, 0]; count[t_full] += 1   # one exact duplicate
    out = ref.merge(boxes, score, count, np.array([(0,) + g for g in grid], np.int32), [0, len(grid)], S, 'iou', 1.0)
    cand = [ref.project(boxes[t, :count[t]], grid[t], S) for t in range(len(grid))]
    distinct = {tuple(b) for c in cand for b in c}
    total = int(count.sum())
    assert len(distinct) < total                                # there IS something identical to merge
    assert int(out['nrows'][0]) == min(len(distinct), 60)
    got = [tuple(out['corners'][0, r]) for r in range(int(out['nrows'][0]))]
    assert len(set(got)) == len(got)


# ----------------------------------------------------------------------------- hand-built cases
SQUARE = [(0, 0, 0, 96, 96)]          # one 96 x 96 view at image size 96: the projection is the identity


def _one_view(boxes, score, metric, th, tiles=None, off=None, K=None):
    boxes = np.asarray(boxes, np.int32); score = np.asarray(score, np.float32)
    if boxes.ndim == 2:
        boxes, score = boxes[None], score[None]
    count = np.full(boxes.shape[0], boxes.shape[1], np.int32)
    tiles = np.array(tiles if tiles is not None else SQUARE * boxes.shape[0], np.int32)
    return ref.merge(boxes, score, count, tiles, off if off is not None else [0, boxes.shape[0]], 96, metric, th)


def test_identity_projection_of_the_square_view():
    b = np.array([[3, 5, 40, 95]], np.int32)
    assert ref.project(b, (0, 0, 96, 96), 96).tolist() == [[3.0, 5.0, 40.0, 95.0]]
    assert ref.project(b, (7, 9, 96, 96), 96).tolist() == [[12.0, 12.0, 49.0, 102.0]]
    # 48 x 96 (w >= h): pad_t = 24, scale 1; 96 x 48: pad_l = 24
    assert ref.project([[10, 30, 20, 50]], (0, 0, 48, 96), 96).tolist() == [[10.0, 6.0, 20.0, 26.0]]
    assert ref.project([[30, 10, 50, 20]], (0, 0, 96, 48), 96).tolist() == [[6.0, 10.0, 26.0, 20.0]]
    assert ref.project([[0, 0, 95, 95]], (100, 200, 48, 96), 96).tolist() == [[200.0, 100.0, 295.0, 148.0]]   # clamped to the tile, then moved


def test_iou_exactly_at_the_threshold():
    a, b = (0, 0, 10, 10), (0, 0, 10, 5)                      # inter 50, union 100: IoU exactly 0.5
    assert ref.overlaps(np.array(a, float), np.array([b], float), 'iou')[0] == 0.5
    assert int(_one_view([a, b], [0.9, 0.8], 'iou', 0.5)['nrows'][0]) == 1                       # merged at 0.5
    assert int(_one_view([a, b], [0.9, 0.8], 'iou', float(np.nextafter(0.5, 1.0)))['nrows'][0]) == 2   # kept at the next double
    assert ref.overlaps(np.array(a, float), np.array([b], float), 'ios')[0] == 1.0               # the part inside the whole


def test_equal_scores_resolve_by_view_then_slot():
    # three disjoint boxes and one that overlaps all of them... all with the same score: the order is view, then slot
    boxes = np.array([[[50, 50, 60, 60], [0, 0, 10, 10]], [[20, 20, 30, 30], [70, 70, 80, 80]]], np.int32)
    out = _one_view(boxes, np.full((2, 2), 0.5, np.float32), 'ios', 0.5)
    assert out['src'][0, :4].tolist() == [0, 1, 2, 3] and int(out['nrows'][0]) == 4
    # the same box in both views, same score: view 0's copy survives; a higher score in view 1 wins over the order
    same = np.array([[[0, 0, 10, 10]], [[0, 0, 10, 10]]], np.int32)
    assert _one_view(same, [[0.5], [0.5]], 'iou', 0.5)['src'][0, :2].tolist() == [0, -1]
    assert _one_view(same, [[0.5], [0.6]], 'iou', 0.5)['src'][0, :2].tolist() == [1, -1]


def test_zero_area_boxes():
    # identical zero-area boxes: inter 0, union 0 -> 0 / 0 = nan: never >= th, both kept
    out = _one_view([(5, 5, 5, 5), (5, 5, 5, 5)], [0.9, 0.8], 'iou', 0.5)
    assert int(out['nrows'][0]) == 2
    assert np.isnan(ref.overlaps(np.array([5., 5, 5, 5]), np.array([[5., 5, 5, 5]]), 'iou')[0])
    assert np.isnan(ref.overlaps(np.array([5., 5, 5, 5]), np.array([[5., 5, 5, 5]]), 'ios')[0])
    # an inverted thin box (xmax < xmin by one) inside a real one: width -1, area -6, inter (3 - 4) * 6 = -6: -6 / fmin(100, -6) = 1
    a, b = np.array([0., 0, 10, 10]), np.array([[4., 2, 3, 8]])
    assert ref.overlaps(a, b, 'ios')[0] == 1.0
    c = np.array([[2., 2, 8, 2]])                                        # zero height inside a: iw 6, ih 0 -> inter 0, min area 0: nan
    assert np.isnan(ref.overlaps(a, c, 'ios')[0])
    # a point against a box inverted on both axes from that point: iw = -2, ih = -3 -> inter 6 = the inverted box's area, the
    # point's area 0: 'ios' 6 / fmin(0, 6) and 'iou' 6 / (0 + 6 - 6) are both x / 0 = +inf: merged, even at merge_th 1.0
    d, e = np.array([5., 5, 5, 5]), np.array([[5., 5, 3, 2]])
    assert ref.overlaps(d, e, 'ios')[0] == np.inf and ref.overlaps(d, e, 'iou')[0] == np.inf
    for metric in ('ios', 'iou'):
        out = _one_view([(5, 5, 5, 5), (5, 5, 3, 2)], [0.9, 0.8], metric, 1.0)
        assert int(out['nrows'][0]) == 1 and out['src'][0, 0] == 0


def test_sixty_one_disjoint_candidates_give_sixty_rows():
    boxes = np.array([(8 * (i % 10), 8 * (i // 10), 8 * (i % 10) + 5, 8 * (i // 10) + 5) for i in range(61)], np.int32)
    score = (np.arange(61, 0, -1) / 100).astype(np.float32)
    out = _one_view(boxes, score, 'ios', 0.5)
    assert int(out['nrows'][0]) == 60 and out['src'][0].tolist() == list(range(60))


def test_a_survivor_ranked_after_the_sixtieth_never_appears():
    # 60 disjoint boxes, then a duplicate of the first (suppressed), then a 62nd disjoint box nobody suppresses
    boxes = [(8 * (i % 10), 8 * (i // 10), 8 * (i % 10) + 5, 8 * (i // 10) + 5) for i in range(60)]
    boxes += [boxes[0], (88, 88, 93, 93)]
    score = (np.arange(62, 0, -1) / 100).astype(np.float32)
    out = _one_view(np.array(boxes, np.int32), score, 'ios', 0.5)
    assert int(out['nrows'][0]) == 60 and out['src'][0].tolist() == list(range(60))
    # the duplicate one rank earlier: it is decided (suppressed) before the 60th row, the next survivor takes that row, and the
    # one after it -- suppressed by nobody -- never appears
    boxes = boxes[:59] + [boxes[0], boxes[59], (88, 88, 93, 93)]
    out = _one_view(np.array(boxes, np.int32), score, 'ios', 0.5)
    assert int(out['nrows'][0]) == 60 and out['src'][0].tolist() == list(range(59)) + [60]


def test_counts_scores_and_bad_ranges():
    boxes = np.array([[[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]]], np.int32)
    score = np.array([[0.5, np.nan, 0.0]], np.float32)
    tiles = np.array(SQUARE, np.int32)
    for count, want in ((3, 1), (99, 1), (-4, 0), (0, 0)):                # above K: clamped; nan and 0 are no candidates
        out = ref.merge(boxes, score, [count], tiles, [0, 1], 96, 'ios', 0.5)
        assert int(out['nrows'][0]) == want
    out = ref.merge(boxes, score, [3], tiles, [0, 2, 1, 1], 96, 'ios', 0.5)  # a range beyond the views, a reversed one, an empty one
    assert out['nrows'].tolist() == [-1, -1, 0]
    assert float(ref.merge(boxes, np.array([[2.5, 0, 0]], np.float32), [1], tiles, [0, 1], 96, 'ios', 0.5)['rows'][0, 0, 4]) == 1.0


# ----------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points():
    from face_vijnana_yolov3_amd.build import build_library
    L = ctypes.CDLL(build_library())
    assert hasattr(L, 'fv_tile_merge') and hasattr(L, 'fv_tile_merge_workspace_bytes')
    L.fv_tile_merge_workspace_bytes.restype = ctypes.c_size_t
    L.fv_tile_merge_workspace_bytes.argtypes = [ctypes.c_int]
    assert L.fv_tile_merge_workspace_bytes(0) == 0 and L.fv_tile_merge_workspace_bytes(-3) == 0
    assert L.fv_tile_merge_workspace_bytes(3) == 3 * 4096 * 32
    # a NULL context is refused without touching anything
    L.fv_tile_merge.restype = ctypes.c_int
    assert L.fv_tile_merge(*([None] * 6), 1, 1, 1, 96, 0, ctypes.c_double(0.5), None, ctypes.c_size_t(0), None, None, None, None) == -1
