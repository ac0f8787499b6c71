"""Tiled inference restated in NumPy / Python float64, from the definitions, not from the kernel:
tile_grid, the projection of a view's network-pixel boxes into frame coordinates, and the greedy cross-tile merge.  Every
operation on a coordinate is one IEEE double operation in the order FaceDetector._project_back and bbox_iou perform it, so the
device result must equal this one bit for bit."""
import numpy as np

ROWS = 60
MAX_CANDS = 4096


# ----------------------------------------------------------------------------- grid
def axis_spans(length, size, stride):
    if length <= size:
        return [(0, length)]
    starts = []
    s = 0
    while s + size < length:
        starts.append(s)
        s += stride
    starts.append(length - size)
    out = []
    for s in starts:
        if (s, size) not in out:
            out.append((s, size))
    return out


def tile_grid(h, w, size=1024, overlap=0.2, full=True, max_tiles=64):
    stride = max(1, int(size * (1 - overlap)))
    grid = [(y0, x0, th, tw) for (y0, th) in axis_spans(h, size, stride) for (x0, tw) in axis_spans(w, size, stride)]
    if full and grid != [(0, 0, h, w)]:
        grid.append((0, 0, h, w))
    if len(grid) > max_tiles:
        raise ValueError('tiles.max_tiles')
    return grid


# ----------------------------------------------------------------------------- projection
def letterbox_pads(h, w, S):
    """(pad_t, pad_l) of the reference's letterbox (face_detection.py:120-147)."""
    if w >= h:
        return (S - int(h / w * S)) // 2, 0
    return 0, (S - int(w / h * S)) // 2


def project(boxes, tile, S):
    """boxes (n, 4) ints xmin, ymin, xmax, ymax in network pixels of a view whose source is tile = (y0, x0, th, tw) -> (n, 4)
    float64 in frame pixels: the reference's projection (fd.py:700-710) for an image of th x tw, then the tile's origin added."""
    y0, x0, h, w = [int(v) for v in tile]
    c = np.asarray(boxes, dtype=np.int64).reshape(-1, 4).astype(np.float64)
    pad_t, pad_l = letterbox_pads(h, w, S)
    out = np.empty_like(c)
    if w >= h:
        out[:, (0, 2)] = np.minimum(c[:, (0, 2)] * w / S, w)
        out[:, (1, 3)] = np.minimum(np.maximum(c[:, (1, 3)] - pad_t, 0) * w / S, h)
    else:
        out[:, (0, 2)] = np.minimum(np.maximum(c[:, (0, 2)] - pad_l, 0) * h / S, w)
        out[:, (1, 3)] = np.minimum(c[:, (1, 3)] * h / S, h)
    out[:, (0, 2)] = out[:, (0, 2)] + float(x0)
    out[:, (1, 3)] = out[:, (1, 3)] + float(y0)
    return out


# ----------------------------------------------------------------------------- overlap
def _interval_overlap(x1, x2, x3, x4):
    """interval_overlap of yolov3_detect.py:165-181 for the scalar interval [x1, x2] against arrays [x3, x4]."""
    left = np.where(x4 < x1, 0.0, np.minimum(x2, x4) - x1)
    right = np.where(x2 < x3, 0.0, np.minimum(x2, x4) - x3)
    return np.where(x3 < x1, left, right)


def overlaps(a, b, metric):
    """Overlap of the kept box a (4,) with every box of b (n, 4): bbox_iou (yd.py:183-194) for 'iou'; for 'ios' the same
    intersection over the smaller of the two areas.  0 / 0 is nan, x / 0 is inf, as NumPy divides."""
    b = np.asarray(b, np.float64).reshape(-1, 4)
    iw = _interval_overlap(a[0], a[2], b[:, 0], b[:, 2])
    ih = _interval_overlap(a[1], a[3], b[:, 1], b[:, 3])
    inter = iw * ih
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        if metric == 'iou':
            return inter / (area_a + area_b - inter)
        assert metric == 'ios'
        return inter / np.fmin(area_a, area_b)


# ----------------------------------------------------------------------------- merge
def merge(boxes, score, count, tiles, frame_off, S, metric='ios', merge_th=0.5, stats=None):
    """boxes (T, K, 4) int, score (T, K) float32, count (T,), tiles (T, 5) (frame, y0, x0, th, tw), frame_off (F + 1,) ->
    dict corners (F, 60, 4) f64, rows (F, 60, 5) f64, nrows (F,) i32, src (F, 60) i32.  stats: a dict that collects 'ties' (pairs of
    neighbouring ranks with equal scores), 'at_threshold' (overlaps exactly equal to merge_th that were evaluated) and
    'late_kills_early' / 'early_kills_late' (a kept candidate of a later / earlier view suppressing one of an earlier / later)."""
    boxes = np.asarray(boxes)
    score = np.asarray(score, np.float32)
    count = np.asarray(count)
    tiles = np.asarray(tiles)
    T, K = score.shape
    F = len(frame_off) - 1
    th = np.float64(merge_th)
    corners = np.zeros((F, ROWS, 4), np.float64)
    rows = np.zeros((F, ROWS, 5), np.float64)
    nrows = np.zeros(F, np.int32)
    src = np.full((F, ROWS), -1, np.int32)
    if stats is not None:
        for k in ('ties', 'at_threshold', 'late_kills_early', 'early_kills_late'):
            stats.setdefault(k, 0)
    for f in range(F):
        v0, v1 = int(frame_off[f]), int(frame_off[f + 1])
        if v0 < 0 or v1 < v0 or v1 > T:
            nrows[f] = -1
            continue
        cand = []                                      # (view, slot)
        for t in range(v0, v1):
            c = min(max(int(count[t]), 0), K)
            cand += [(t, k) for k in range(c) if score[t, k] > 0]           # a nan is never > 0
        if len(cand) > MAX_CANDS:
            nrows[f] = -1
            continue
        if not cand:
            continue
        view = np.array([c[0] for c in cand]); slot = np.array([c[1] for c in cand])
        sc = score[view, slot]
        order = np.lexsort((slot, view, -sc.astype(np.float64)))             # descending score, then view, then slot
        view, slot, sc = view[order], slot[order], sc[order]
        if stats is not None:
            stats['ties'] += int((sc[1:] == sc[:-1]).sum())
        fb = np.empty((len(view), 4), np.float64)
        for t in np.unique(view):
            m = view == t
            fb[m] = project(boxes[t, slot[m]], tiles[t, 1:5], S)
        alive = np.ones(len(view), bool)
        kept = []
        for i in range(len(view)):
            if not alive[i]:
                continue
            kept.append(i)
            if len(kept) == ROWS:
                break
            later = np.nonzero(alive[i + 1:])[0] + i + 1
            if len(later) == 0:
                continue
            ov = overlaps(fb[i], fb[later], metric)
            kill = ov >= th                                                  # nan never, +inf always
            if stats is not None:
                stats['at_threshold'] += int((ov == th).sum())
                stats['late_kills_early'] += int((kill & (view[later] < view[i])).sum())
                stats['early_kills_late'] += int((kill & (view[later] > view[i])).sum())
            alive[later[kill]] = False
        nrows[f] = len(kept)
        for r, i in enumerate(kept):
            corners[f, r] = fb[i]
            rows[f, r] = (fb[i, 0], fb[i, 1], fb[i, 2] - fb[i, 0], fb[i, 3] - fb[i, 1], np.float64(min(sc[i], np.float32(1.0))))
            src[f, r] = view[i] * K + slot[i]
    return dict(corners=corners, rows=rows, nrows=nrows, src=src)


def merge_views(view_results, grid, S, metric='ios', merge_th=0.5):
    """One frame: view_results = decode_nms-style host arrays (boxes (T, K, 4), score (T, K), count (T,)) for the T views of
    `grid` ([(y0, x0, th, tw)]) -> merge()'s dict for that one frame."""
    tiles = np.array([(0,) + tuple(g) for g in grid], np.int32)
    return merge(view_results['boxes'], view_results['score'], view_results['count'], tiles, [0, len(grid)], S, metric, merge_th)
