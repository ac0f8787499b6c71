"""Host-side data path of FaceDetector: letterbox geometry, ground-truth tensor encoding and the
UCCS-format training sequence (reference face_detection.py:75-310), plus a synthetic UCCS-shaped
dataset generator (the real UCCS set is download-only and unavailable offline).

This is CPU code in the reference too (Keras `Sequence` workers); it is not part of the device
hot path.  FaceDetector itself letterboxes on the device (`fv_letterbox` via
`TrainingSequence.get_raw` / `postproc.letterbox_device`); `letterbox()` / `__getitem__` below
keep the reference's `Sequence[i] -> ({'input1': ...}, {'output': ...})` contract for callers
that want host arrays.  Pixel resampling uses a bicubic (a = -0.75, OpenCV INTER_CUBIC's kernel)
restatement; its pixel values are "parity unpinned" against cv2 (absent here) -- geometry is
pinned exactly."""
import os

import numpy as np

CSV_COLUMNS = ['FACE_ID', 'FILE', 'SUBJECT_ID', 'FACE_X', 'FACE_Y', 'FACE_WIDTH', 'FACE_HEIGHT']


def letterbox_geometry(h, w, image_size):
    """-> (w_p, h_p, pad_t, pad_b, pad_l, pad_r); odd padding puts the extra row/col at the
    bottom/right (face_detection.py:120-147)."""
    pad_t = pad_b = pad_l = pad_r = 0
    if w >= h:
        w_p, h_p = image_size, int(h / w * image_size)
        pad = image_size - h_p
        pad_t, pad_b = pad // 2, pad - pad // 2
    else:
        h_p, w_p = image_size, int(w / h * image_size)
        pad = image_size - w_p
        pad_l, pad_r = pad // 2, pad - pad // 2
    return w_p, h_p, pad_t, pad_b, pad_l, pad_r


def identity_placement(h, w, image_size):
    """The placement of today's letterbox: the whole image in the whole canvas, not mirrored."""
    return (0, 0, int(h), int(w), int(image_size), 0, 0, 0)


def _placed_centres(faces, h, w, image_size, placement):
    """The corner / centre arithmetic both encoders share (face_detection.py:150-202), under a placement
    (cy0, cx0, ch, cw, T, oy, ox, flip) -- the ch x cw crop at (cy0, cx0) letterboxed into the T x T box at (oy, ox) of the S x S
    canvas, the canvas then mirrored when flip -- or under None, today's letterbox of the whole image.  Yields
    (x1, y1, x2, y2, xc, yc, m, T) per kept face.  With m = max(cw, ch) and (pad_t, pad_l) the crop's letterbox padding in T:
        x1p = int((x1 - cx0) / m * T) + ox + pad_l,  x2p, y1p, y2p likewise,  xc = (x1p + x2p) // 2,  yc = (y1p + y2p) // 2.
    Under a placement a face is kept only when (xc, yc) lies inside the placed content rectangle (its box is NOT clipped to the
    crop); a flip then maps xc to S - 1 - xc and changes nothing else.  With identity_placement(h, w, S) every expression
    reduces to the one of placement None, bit for bit: x1 - 0 is x1, the single non-zero pad is the old offset and T is S."""
    S = image_size
    placed = placement is not None
    cy0, cx0, ch, cw, T, oy, ox, flip = placement if placed else identity_placement(h, w, S)
    w_p, h_p, pad_t, _, pad_l, _ = letterbox_geometry(ch, cw, T)
    m = cw if cw >= ch else ch
    left, top = ox + pad_l, oy + pad_t
    for fx, fy, fw, fh in np.asarray(faces, dtype=np.float64).reshape(-1, 4):
        if not (fx > 0 and fy > 0 and fw > 0 and fh > 0):
            continue
        x1, y1 = int(fx), int(fy)
        x2, y2 = x1 + int(fw) - 1, y1 + int(fh) - 1
        x1p, x2p = int((x1 - cx0) / m * T) + left, int((x2 - cx0) / m * T) + left
        y1p, y2p = int((y1 - cy0) / m * T) + top, int((y2 - cy0) / m * T) + top
        xc, yc = (x1p + x2p) // 2, (y1p + y2p) // 2
        if placed:
            if not (left <= xc < left + w_p and top <= yc < top + h_p):
                continue
            if flip:
                xc = S - 1 - xc
        yield x1, y1, x2, y2, xc, yc, m, T


def _tile_centres(tiles, image_size):
    """_placed_centres for a canvas made of tiles (hps['mosaic'], draw_mosaic).  tiles: [(faces of the tile's source image, the
    tile's record (canvas, image, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1))], in the table's order; the faces of
    tile 0 come first, then tile 1's, ...  Per tile _placed_centres' expressions with the tile's numbers,
        x1p = int((x1 - cx0) / m * T) + ox + pad_l,  ...,  xc = (x1p + x2p) // 2,  yc = (y1p + y2p) // 2,
    ox and oy possibly negative; a tile's flip mirrors its box in place, xc = 2 * ox + T - 1 - xc.  A face is kept only when its
    centre, after the flip, lies inside both the tile's placed content rectangle and its window rows [wy0, wy1) x columns
    [wx0, wx1); its box is NOT clipped, neither to the crop nor to the window.  One tile whose window is the whole canvas yields
    what the equivalent placement yields (the canvas flip of a placement with box column ox is the in-box flip with S - T - ox)."""
    for faces, rec in tiles:
        _canvas, _image, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1 = (int(v) for v in rec)
        w_p, h_p, pad_t, _, pad_l, _ = letterbox_geometry(ch, cw, T)
        m = cw if cw >= ch else ch
        left, top = ox + pad_l, oy + pad_t
        for fx, fy, fw, fh in np.asarray(faces, dtype=np.float64).reshape(-1, 4):
            if not (fx > 0 and fy > 0 and fw > 0 and fh > 0):
                continue
            x1, y1 = int(fx), int(fy)
            x2, y2 = x1 + int(fw) - 1, y1 + int(fh) - 1
            x1p, x2p = int((x1 - cx0) / m * T) + left, int((x2 - cx0) / m * T) + left
            y1p, y2p = int((y1 - cy0) / m * T) + top, int((y2 - cy0) / m * T) + top
            xc, yc = (x1p + x2p) // 2, (y1p + y2p) // 2
            if not (left <= xc < left + w_p and top <= yc < top + h_p):
                continue
            if flip:
                xc = 2 * ox + T - 1 - xc
            if not (wx0 <= xc < wx1 and wy0 <= yc < wy1):
                continue
            yield x1, y1, x2, y2, xc, yc, m, T


def encode_gt(faces, h, w, image_size=416, grid=13, channels=6, placement=None, tiles=None):
    """Ground-truth tensor of one image (face_detection.py:150-202).

    faces: array-like (n,4) of FACE_X, FACE_Y, FACE_WIDTH, FACE_HEIGHT in csv order; rows with
    any value <= 0 are skipped; later rows overwrite earlier ones in the same cell.
    placement: None (the reference's letterbox) or (cy0, cx0, ch, cw, T, oy, ox, flip) as draw_augment returns it
    (_placed_centres states the arithmetic); the box sizes are then fractions of the canvas, (x2 - x1 + 1) / m * (T / S).
    tiles: a mosaic canvas, [(faces, tile record)] as _tile_centres takes it (faces, h, w and placement are then not read):
    the tiles are written in their order, sizes with each tile's own m and T."""
    cell = image_size // grid
    gt = np.zeros((grid, grid, channels), np.float64)
    centres = _tile_centres(tiles, image_size) if tiles is not None else _placed_centres(faces, h, w, image_size, placement)
    for x1, y1, x2, y2, xc, yc, m, T in centres:
        cx, cy = xc // cell, yc // cell
        k = T / image_size
        gt[cy, cx, :6] = [1.0, (xc - cx * cell) / cell, (yc - cy * cell) / cell,
                          (x2 - x1 + 1) / m * k, (y2 - y1 + 1) / m * k, 1.0]
    return gt


# ----------------------------------------------------------------------------- three-scale targets
YOLO_ANCHORS = [[116, 90, 156, 198, 373, 326], [30, 61, 62, 45, 59, 119], [10, 13, 16, 30, 33, 23]]   # yolov3_detect.py:560
# The reference's decode_netout (yolov3_detect.py:354-362) SKIPS (116,90), (373,326), (62,45), (10,13), (33,23): only these
# (scale, anchor) pairs ever reach its box list, so they are the ones a face may be assigned to by default.
YOLO_ANCHORS_DECODED = ((0, 1), (1, 0), (1, 2), (2, 1))


def encode_gt_three_scale(faces, h, w, image_size=416, nclass=1, anchors=YOLO_ANCHORS, anchor_keep=YOLO_ANCHORS_DECODED,
                          placement=None, tiles=None):
    """Ground truth of one image for the three-scale head: [t13, t26, t52], t_s of shape (g_s, g_s, 3*(5+nclass)) float64 with
    g_s = image_size/32 * 2^s, laid out [cell][anchor][tx, ty, tw, th, objectness, classes...] like the network output.

    The single-scale encoder (face_detection.py:150-202) generalised: the same skip rule (all of X, Y, W, H > 0), the same
    integer letterbox arithmetic for the corners and the centre (`int()` truncation, `//2`), cell = centre // cell_size and
    offset = remainder / cell_size per scale.  New here (the reference never trains this head): the face goes to the ONE
    (scale, anchor) whose anchor box has the best IoU with the face box (sizes only, network pixels; ties -> the first in
    `anchor_keep` order) among the anchors the reference's decode keeps, and the box is stored in the parametrisation that
    decode_netout (yolov3_detect.py:335-387) inverts: sigma(tx) = offset, anchor_w * exp(tw) = box width in network pixels.
    Offsets are clamped to [0.5/cell, 1 - 0.5/cell] (logit of 0 is -inf; half a pixel is below the decode's int() grain).
    Objectness 1 and class 0 = 1 at the assigned slot; later rows overwrite earlier ones in the same slot.
    placement: as for encode_gt; the box in network pixels is then (x2 - x1 + 1) / m * T.
    tiles: as for encode_gt (a mosaic canvas; every tile's faces with that tile's m and T)."""
    S = int(image_size)
    C = 5 + nclass
    out = [np.zeros((S // 32 << s, S // 32 << s, 3 * C), np.float64) for s in range(3)]
    centres = _tile_centres(tiles, S) if tiles is not None else _placed_centres(faces, h, w, S, placement)
    for x1, y1, x2, y2, xc, yc, m, T in centres:
        bw, bh = (x2 - x1 + 1) / m * T, (y2 - y1 + 1) / m * T          # the single-scale targets bw, bh times the network size
        best, best_iou = None, -1.0
        for (s, b) in anchor_keep:
            aw, ah = anchors[s][2 * b], anchors[s][2 * b + 1]
            inter = min(bw, aw) * min(bh, ah)
            iou = inter / (bw * bh + aw * ah - inter)
            if iou > best_iou:
                best, best_iou = (s, b), iou
        s, b = best
        g = S // 32 << s
        cell = S // g
        cx, cy = xc // cell, yc // cell
        lo, hi = 0.5 / cell, 1.0 - 0.5 / cell
        px = min(max((xc - cx * cell) / cell, lo), hi); py = min(max((yc - cy * cell) / cell, lo), hi)
        t = np.zeros(C, np.float64)
        t[0] = np.log(px / (1.0 - px)); t[1] = np.log(py / (1.0 - py))
        t[2] = np.log(bw / anchors[s][2 * b]); t[3] = np.log(bh / anchors[s][2 * b + 1])
        t[4] = 1.0; t[5] = 1.0
        out[s][cy, cx, b * C:(b + 1) * C] = t
    return out


# ----------------------------------------------------------------------------- detection loss of the three-scale head (hps['loss'])
DET_LOSS_DEFAULTS = {'box_loss': 'giou', 'ignore_thresh': 0.5, 'box_weight': 1.0, 'noobj_weight': 1.0, 'max_boxes': 256}
DET_BOX_LOSSES = ('l2', 'giou')        # FV_DET_BOX_L2, FV_DET_BOX_GIOU of include/fv_hotpath.h, in this order


def det_loss_conf(value, head='three_scale'):
    """fd_conf.hps['loss'] -> None (absent, None or "fd": the fd_loss generalisation every head trains with today) or the complete
    parameter dict of the YOLOv3 detection loss (fv_yolo_det_loss_grad) -- "yolo": DET_LOSS_DEFAULTS; an
    object {"yolo": {...}}: its keys over the defaults; either way plus 'anchors' = YOLO_ANCHORS.  ValueError for an
    unknown name or key, a value outside its range (box_loss 'l2' / 'giou', ignore_thresh in (0, 1], box_weight and noobj_weight
    finite and > 0, max_boxes an int in [1, 1024]) and for "yolo" with the single-scale head.  Not in the reference; pure host
    code."""
    if value is None or value == 'fd':
        return None
    opts = {}
    if isinstance(value, dict) and set(value) == {'yolo'} and isinstance(value['yolo'], dict):
        opts = dict(value['yolo'])
    elif not (isinstance(value, str) and value == 'yolo'):
        raise ValueError('fd_conf.hps.loss %r is not valid ("fd", "yolo" or {"yolo": {%s}})' % (value, ', '.join(sorted(DET_LOSS_DEFAULTS))))
    if head != 'three_scale':
        raise ValueError("fd_conf.hps.loss 'yolo' needs nn_arch.head = 'three_scale' (the single-scale head trains with 'fd')")
    unknown = sorted(set(opts) - set(DET_LOSS_DEFAULTS))
    if unknown:
        raise ValueError('fd_conf.hps.loss has unknown key(s) %s (available: %s)' % (', '.join(map(repr, unknown)),
                                                                                  ', '.join(sorted(DET_LOSS_DEFAULTS))))
    c = dict(DET_LOSS_DEFAULTS)
    c.update(opts)
    if c['box_loss'] not in DET_BOX_LOSSES:
        raise ValueError('fd_conf.hps.loss.box_loss %r is not valid (%s)' % (c['box_loss'], ' or '.join(map(repr, DET_BOX_LOSSES))))
    if not (_is_number(c['ignore_thresh']) and 0 < c['ignore_thresh'] <= 1):
        raise ValueError('fd_conf.hps.loss.ignore_thresh %r is not valid (an IoU in (0, 1])' % (c['ignore_thresh'],))
    for k in ('box_weight', 'noobj_weight'):
        if not (_is_number(c[k]) and c[k] > 0):
            raise ValueError('fd_conf.hps.loss.%s %r is not valid (a finite number > 0)' % (k, c[k]))
    if not (isinstance(c['max_boxes'], int) and not isinstance(c['max_boxes'], bool) and 1 <= c['max_boxes'] <= 1024):
        raise ValueError('fd_conf.hps.loss.max_boxes %r is not valid (an int in [1, 1024])' % (c['max_boxes'],))
    for k in ('ignore_thresh', 'box_weight', 'noobj_weight'):
        c[k] = float(c[k])
    c['anchors'] = [list(map(float, row)) for row in YOLO_ANCHORS]
    return c


DET_STATS = ('box', 'obj', 'noobj', 'cls', 'positives', 'ignored', 'iou_sum', 'iou_gt_50', 'iou_gt_75', 'max_count', 'dropped', 'spare')


def det_stats_line(sums, steps, slots):
    """The epoch line of hps['loss'] = 'yolo': `sums` = the 12 stats of fv_yolo_det_loss_grad added up over the `steps` steps of
    the epoch (entry 9: their maximum), `slots` = (cell, anchor) slots the steps held in all.  Loss parts are means per step;
    mean IoU and recall over the assigned slots; the ignored share over the unassigned ones."""
    s = dict(zip(DET_STATS, (float(v) for v in sums)))
    pos = max(s['positives'], 1.0)
    neg = max(float(slots) - s['positives'], 1.0)
    n = max(int(steps), 1)
    return ('yolo loss - box: %.4f - obj: %.4f - noobj: %.4f - cls: %.4f - mean IoU: %.4f - recall@0.5: %.4f - recall@0.75: %.4f - '
            'ignored: %.4f' % (s['box'] / n, s['obj'] / n, s['noobj'] / n, s['cls'] / n, s['iou_sum'] / pos, s['iou_gt_50'] / pos,
                               s['iou_gt_75'] / pos, s['ignored'] / neg))


def check_det_dropped(dropped, max_count, max_boxes):
    """A box beyond the cap is missing from the ignore mask of its image: an error, never a quietly weaker loss."""
    if dropped > 0:
        raise ValueError('fd_conf.hps.loss.max_boxes = %d is too small: an image holds %d assigned boxes (%d dropped this epoch); '
                         'raise max_boxes (at most 1024)' % (max_boxes, int(max_count), int(dropped)))


# ----------------------------------------------------------------------------- per-epoch validation (hps['validate'])
VALIDATE_DEFAULTS = {'path': None, 'every': 1, 'iou_ths': None, 'save_best': False}
VALIDATE_MAX_THS = 16                  # FV_DET_MAX_TH of include/fv_hotpath.h


def validate_conf(value, test_path=None):
    """fd_conf.hps['validate'] -> None (absent, None or false: train() looks at no held-out image, as without the key) or the complete
    parameter dict (true: VALIDATE_DEFAULTS; an object: its keys over the defaults) with 'path' resolved (default: `test_path`, the
    configuration's test_path) and 'iou_ths' a list of floats (default: np.arange(0.5, 1.0, 0.05), cal_mAP_sweep's).  ValueError for
    another type, an unknown key or a value outside its range: path a string, every an int >= 1, iou_ths 1 to 16 numbers in (0, 1]
    in ascending order, save_best a bool.  Not in the reference; pure host code."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError('fd_conf.hps.validate %r is not valid (false, true or an object with the keys %s)'
                         % (value, ', '.join(sorted(VALIDATE_DEFAULTS))))
    unknown = sorted(set(value) - set(VALIDATE_DEFAULTS))
    if unknown:
        raise ValueError('fd_conf.hps.validate has unknown key(s) %s (available: %s)' % (', '.join(map(repr, unknown)),
                                                                                      ', '.join(sorted(VALIDATE_DEFAULTS))))
    c = dict(VALIDATE_DEFAULTS)
    c.update(value)
    if c['path'] is None:
        c['path'] = test_path
    if not (isinstance(c['path'], str) and c['path']):
        raise ValueError('fd_conf.hps.validate.path %r is not valid (a directory with validation.csv and the *.jpg files; default: '
                         'fd_conf.test_path)' % (c['path'],))
    if not (isinstance(c['every'], int) and not isinstance(c['every'], bool) and c['every'] >= 1):
        raise ValueError('fd_conf.hps.validate.every %r is not valid (an int >= 1)' % (c['every'],))
    ths = c['iou_ths']
    if ths is None:
        ths = [float(t) for t in np.arange(0.5, 1.0, 0.05)]
    if not (isinstance(ths, (list, tuple)) and 1 <= len(ths) <= VALIDATE_MAX_THS and all(_is_number(t) and 0 < t <= 1 for t in ths)
            and all(a < b for a, b in zip(ths, ths[1:]))):
        raise ValueError('fd_conf.hps.validate.iou_ths %r is not valid (1 to %d numbers in (0, 1], ascending)' % (ths, VALIDATE_MAX_THS))
    c['iou_ths'] = [float(t) for t in ths]
    if not isinstance(c['save_best'], bool):
        raise ValueError('fd_conf.hps.validate.save_best %r is not valid (true or false)' % (c['save_best'],))
    return c


def refuse_validate_on_ranks(hps, ranks):
    """Validation on more than one rank is not served: the ranking needs every rank's detections in one list, which needs a gather
    and a run on two GPUs to prove."""
    if int(ranks) > 1 and hps.get('validate') not in (None, False):
        raise NotImplementedError('fd_conf.hps.validate with multi_gpu and %d ranks is not implemented: train on one GPU, or '
                                  'without validate' % int(ranks))


def validate_line(res):
    """The line train() prints after a validation: AP50, AP75 (where those thresholds are in the sweep), the mean over the sweep,
    and what it was computed from."""
    parts = ['val -']
    for name, th in (('AP50', 0.5), ('AP75', 0.75)):
        for t, ap in zip(res['iou_ths'], res['ap']):
            if abs(t - th) < 1e-9:
                parts.append('%s %.4f' % (name, ap))
    parts.append('mAP %.4f' % res['mean_ap'])
    parts.append('(%d detections on %d images, %d faces)' % (res['n_det'], res['n_images'], res['n_gt']))
    return ' '.join(parts)


# ----------------------------------------------------------------------------- tiled inference (hps['tiles'])
TILES_DEFAULTS = {'size': 1024, 'overlap': 0.2, 'full': True, 'metric': 'ios', 'merge_th': 0.5, 'max_tiles': 64}
TILE_METRICS = ('ios', 'iou')          # FV_TILE_METRIC_IOS, FV_TILE_METRIC_IOU of csrc/tile_merge.h, in this order
TILE_MAX_CANDS = 4096                  # FV_TILE_MAX_CANDS
TILE_MAX_TILES = 64


def tiles_conf(value, head='single'):
    """fd_conf.hps['tiles'] -> None (absent, None or false: every frame is letterboxed whole, as without the key) or the complete
    parameter dict (true: TILES_DEFAULTS; an object: its keys over the defaults).  ValueError for another type, an unknown key, a
    bool where a number is expected or a value outside its range: size (tile side in source pixels) an int >= 32, overlap (share
    of size neighbouring tiles have in common) in [0, 0.5], full (the whole frame as one more view) a bool, metric 'ios'
    (intersection over the smaller area) or 'iou', merge_th in (0, 1], max_tiles (per frame) an int in [1, 64].
    NotImplementedError with the three-scale head.  Not in the reference; pure host code."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError('fd_conf.hps.tiles %r is not valid (false, true or an object with the keys %s)'
                         % (value, ', '.join(sorted(TILES_DEFAULTS))))
    unknown = sorted(set(value) - set(TILES_DEFAULTS))
    if unknown:
        raise ValueError('fd_conf.hps.tiles has unknown key(s) %s (available: %s)' % (', '.join(map(repr, unknown)),
                                                                                   ', '.join(sorted(TILES_DEFAULTS))))
    c = dict(TILES_DEFAULTS)
    c.update(value)

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not (is_int(c['size']) and c['size'] >= 32):
        raise ValueError('fd_conf.hps.tiles.size %r is not valid (source pixels, an int >= 32)' % (c['size'],))
    if not (_is_number(c['overlap']) and 0 <= c['overlap'] <= 0.5):
        raise ValueError('fd_conf.hps.tiles.overlap %r is not valid (a share of size in [0, 0.5])' % (c['overlap'],))
    if not isinstance(c['full'], bool):
        raise ValueError('fd_conf.hps.tiles.full %r is not valid (true or false)' % (c['full'],))
    if not (isinstance(c['metric'], str) and c['metric'] in TILE_METRICS):
        raise ValueError('fd_conf.hps.tiles.metric %r is not valid (%s)' % (c['metric'], ' or '.join(map(repr, TILE_METRICS))))
    if not (_is_number(c['merge_th']) and 0 < c['merge_th'] <= 1):
        raise ValueError('fd_conf.hps.tiles.merge_th %r is not valid (an overlap in (0, 1])' % (c['merge_th'],))
    if not (is_int(c['max_tiles']) and 1 <= c['max_tiles'] <= TILE_MAX_TILES):
        raise ValueError('fd_conf.hps.tiles.max_tiles %r is not valid (an int in [1, %d])' % (c['max_tiles'], TILE_MAX_TILES))
    if head == 'three_scale':
        raise NotImplementedError("fd_conf.hps.tiles with nn_arch.head = 'three_scale' is not implemented: the merge kernel takes "
                                  "the single-scale head's decode/NMS result")
    c['overlap'], c['merge_th'] = float(c['overlap']), float(c['merge_th'])
    return c


def _tile_spans(length, size, stride):
    if length <= size:
        return [(0, length)]
    starts, s = [], 0
    while s + size < length:
        starts.append(s)
        s += stride
    if not starts or starts[-1] != length - size:
        starts.append(length - size)
    return [(s, size) for s in starts]


def tile_grid(h, w, conf):
    """The views of an h x w frame under tiles_conf()'s dict -> [(y0, x0, th, tw)] ints.  Per axis of length L, with
    stride = max(1, int(size * (1 - overlap))): one span [0, L) when L <= size; else the starts 0, stride, 2 * stride, ... while
    start + size < L, then L - size (duplicates dropped), every span `size` long.  The tiles are the row-major product of the two
    axes; with `full` the whole frame (0, 0, h, w) comes last, unless the grid is exactly that one tile.  More than max_tiles
    views is a ValueError: the grid is never changed silently.  Pure host code."""
    h, w, size = int(h), int(w), int(conf['size'])
    if h < 1 or w < 1:
        raise ValueError('fd_conf.hps.tiles: a frame of %d x %d pixels has no tile' % (w, h))
    stride = max(1, int(size * (1 - conf['overlap'])))
    grid = [(y0, x0, th, tw) for y0, th in _tile_spans(h, size, stride) for x0, tw in _tile_spans(w, size, stride)]
    if conf['full'] and grid != [(0, 0, h, w)]:
        grid.append((0, 0, h, w))
    if len(grid) > conf['max_tiles']:
        raise ValueError('fd_conf.hps.tiles.max_tiles = %d is too small: a frame of %d x %d pixels (width x height) makes %d views at '
                         'size %d, overlap %g; raise size or max_tiles (at most %d)'
                         % (conf['max_tiles'], w, h, len(grid), size, conf['overlap'], TILE_MAX_TILES))
    return grid


def tile_views(h, w, conf, num_cands):
    """tile_grid for a frame whose views each hand fv_tile_merge up to num_cands candidates: ValueError when they could exceed
    the kernel's cap (FV_TILE_MAX_CANDS per frame)."""
    grid = tile_grid(h, w, conf)
    if len(grid) * int(num_cands) > TILE_MAX_CANDS:
        raise ValueError('fd_conf.hps.tiles.max_tiles: a frame of %d x %d pixels (width x height) makes %d views of up to %d '
                         'candidates (hps.num_cands) each, more than the %d per frame the merge takes; raise tiles.size or lower '
                         'num_cands' % (w, h, len(grid), int(num_cands), TILE_MAX_CANDS))
    return grid


# ----------------------------------------------------------------------------- training augmentation (hps['augment'])
AUGMENT_DEFAULTS ={'zoom': [0.75, 1.25], 'flip': 0.5, 'hue': 0.1, 'saturation': 1.5, 'exposure': 1.5, 'seed': 0}


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)


def augment_conf(value):
    """fd_conf.hps['augment'] -> None (absent, None or false: the reference's fixed letterbox) or the complete parameter dict
    (true: AUGMENT_DEFAULTS; an object: its keys over the defaults).  ValueError for an unknown key or a value outside its
    range: zoom [lo, hi] with 0 < lo <= 1 <= hi, flip in [0, 1], hue in [0, 0.5], saturation >= 1, exposure >= 1, seed an
    int >= 0.  Not in the reference (Darknet's detector recipe); pure host code."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError('fd_conf.hps.augment %r is not valid (false, true or an object with the keys %s)'
                         % (value, ', '.join(sorted(AUGMENT_DEFAULTS))))
    unknown = sorted(set(value) - set(AUGMENT_DEFAULTS))
    if unknown:
        raise ValueError('fd_conf.hps.augment has unknown key(s) %s (available: %s)' % (', '.join(map(repr, unknown)),
                                                                                     ', '.join(sorted(AUGMENT_DEFAULTS))))
    c = dict(AUGMENT_DEFAULTS)
    c.update(value)
    z = c['zoom']
    if not (isinstance(z, (list, tuple)) and len(z) == 2 and all(_is_number(v) for v in z) and 0 < z[0] <= 1 <= z[1]):
        raise ValueError('fd_conf.hps.augment.zoom %r is not valid ([lo, hi] with 0 < lo <= 1 <= hi)' % (z,))
    if not (_is_number(c['flip']) and 0 <= c['flip'] <= 1):
        raise ValueError('fd_conf.hps.augment.flip %r is not valid (a probability in [0, 1])' % (c['flip'],))
    if not (_is_number(c['hue']) and 0 <= c['hue'] <= 0.5):
        raise ValueError('fd_conf.hps.augment.hue %r is not valid (turns, in [0, 0.5])' % (c['hue'],))
    for k in ('saturation', 'exposure'):
        if not (_is_number(c[k]) and c[k] >= 1):
            raise ValueError('fd_conf.hps.augment.%s %r is not valid (a number >= 1)' % (k, c[k]))
    if not (isinstance(c['seed'], int) and not isinstance(c['seed'], bool) and c['seed'] >= 0):
        raise ValueError('fd_conf.hps.augment.seed %r is not valid (an int >= 0)' % (c['seed'],))
    c['zoom'] = [float(z[0]), float(z[1])]
    for k in ('flip', 'hue', 'saturation', 'exposure'):
        c[k] = float(c[k])
    return c


def draw_augment(aug_conf, epoch, file_index, h, w, S):
    """The augmentation of image `file_index` (its index in TrainingSequence.file_names; h x w pixels) in epoch `epoch` at network
    size S -> (placement, colour) = ((cy0, cx0, ch, cw, T, oy, ox, flip), (dh, sat, exp)): what fv_letterbox_augment_batch and
    encode_gt(..., placement=) take.  aug_conf: augment_conf()'s dict.  A pure function of its arguments -- the batch size, the
    position in the batch, the rank and the world size do not enter, so every rank and every rerun sees the same augmented
    dataset.  Draws from rng = np.random.default_rng([seed, epoch, file_index]) in this fixed order (round = Python's round):
      1. z = rng.uniform(lo, hi)
      2. z >= 1 (zoom in): cw = max(1, round(w / z)), ch = max(1, round(h / z)); cx0 = rng.integers(0, w - cw + 1), then
         cy0 = rng.integers(0, h - ch + 1); T = S, ox = oy = 0
         z < 1 (zoom out): the whole image; T = max(1, round(S * z)); ox = rng.integers(0, S - T + 1), then
         oy = rng.integers(0, S - T + 1)
      3. flip = rng.random() < flip probability
      4. dh = rng.uniform(-hue, hue)
      5. sat: s = rng.uniform(1, saturation), then 1 / s if rng.random() < 0.5 (Darknet's rand_scale)
      6. exp: likewise from exposure
    The crop is letterboxed by letterbox_geometry(ch, cw, T) into the T x T box at (oy, ox) of the zero S x S canvas (aspect
    preserved), the finished canvas mirrored when flip.  Where that geometry is not feasible (w_p < 1 or h_p < 1) the placement
    falls back to identity_placement(h, w, S); the colour draw stays."""
    h, w, S = int(h), int(w), int(S)
    rng = np.random.default_rng([int(aug_conf['seed']), int(epoch), int(file_index)])
    lo, hi = aug_conf['zoom']
    z = float(rng.uniform(lo, hi))
    if z >= 1:
        cw, ch = max(1, round(w / z)), max(1, round(h / z))
        cx0 = int(rng.integers(0, w - cw + 1)); cy0 = int(rng.integers(0, h - ch + 1))
        T, ox, oy = S, 0, 0
    else:
        cy0, cx0, ch, cw = 0, 0, h, w
        T = max(1, round(S * z))
        ox = int(rng.integers(0, S - T + 1)); oy = int(rng.integers(0, S - T + 1))
    flip = int(rng.random() < aug_conf['flip'])
    dh = float(rng.uniform(-aug_conf['hue'], aug_conf['hue']))
    scale = []
    for k in ('saturation', 'exposure'):
        s = float(rng.uniform(1.0, aug_conf[k]))
        scale.append(1.0 / s if rng.random() < 0.5 else s)
    w_p, h_p = letterbox_geometry(ch, cw, T)[:2]
    placement = (cy0, cx0, ch, cw, T, oy, ox, flip)
    if w_p < 1 or h_p < 1:
        placement = identity_placement(h, w, S)
    return placement, (dh + 0.0, scale[0], scale[1])


# ----------------------------------------------------------------------------- mosaic (hps['mosaic'])
MOSAIC_DEFAULTS = {'prob': 0.5, 'scale': [0.4, 1.0], 'centre': [0.25, 0.75], 'seed': 0}


def mosaic_conf(value):
    """fd_conf.hps['mosaic'] -> None (absent, None or false: every canvas holds one image, as without the key) or the complete
    parameter dict (true: MOSAIC_DEFAULTS; an object: its keys over the defaults).  ValueError for another type, an unknown key
    or a value outside its range: prob in [0, 1] (the share of canvases that are mosaics), scale [lo, hi] with
    0 < lo <= hi <= 2 (a tile's box side as a fraction of the network size), centre [lo, hi] with 0 < lo <= hi < 1 (the mosaic
    centre as a fraction of the network size, per axis), seed an int >= 0.  Not in the reference; pure host code."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError('fd_conf.hps.mosaic %r is not valid (false, true or an object with the keys %s)'
                         % (value, ', '.join(sorted(MOSAIC_DEFAULTS))))
    unknown = sorted(set(value) - set(MOSAIC_DEFAULTS))
    if unknown:
        raise ValueError('fd_conf.hps.mosaic has unknown key(s) %s (available: %s)' % (', '.join(map(repr, unknown)),
                                                                                    ', '.join(sorted(MOSAIC_DEFAULTS))))
    c = dict(MOSAIC_DEFAULTS)
    c.update(value)
    if not (_is_number(c['prob']) and 0 <= c['prob'] <= 1):
        raise ValueError('fd_conf.hps.mosaic.prob %r is not valid (a share in [0, 1])' % (c['prob'],))
    for k, ok, rule in (('scale', lambda lo, hi: 0 < lo <= hi <= 2, '0 < lo <= hi <= 2'),
                        ('centre', lambda lo, hi: 0 < lo <= hi < 1, '0 < lo <= hi < 1')):
        v = c[k]
        if not (isinstance(v, (list, tuple)) and len(v) == 2 and all(_is_number(x) for x in v) and ok(v[0], v[1])):
            raise ValueError('fd_conf.hps.mosaic.%s %r is not valid ([lo, hi] with %s)' % (k, v, rule))
        c[k] = [float(v[0]), float(v[1])]
    if not (isinstance(c['seed'], int) and not isinstance(c['seed'], bool) and c['seed'] >= 0):
        raise ValueError('fd_conf.hps.mosaic.seed %r is not valid (an int >= 0)' % (c['seed'],))
    c['prob'] = float(c['prob'])
    return c


def draw_mosaic(mos_conf, aug_conf, epoch, file_indices, shapes, S):
    """The canvases of one rank's slice of a batch in epoch `epoch` at network size S -> (tiles, colour): what
    fv_letterbox_mosaic_batch and the encoders' `tiles=` take.  file_indices[i] / shapes[i]: the index in
    TrainingSequence.file_names and the (h, w) of the slice's image i, in order; canvas i is built around image i.  tiles: int32
    [n_tiles][14] records (canvas, image, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1), `image` a position in the
    slice, sorted by canvas; colour: float32 [n_tiles][3] records (dh, sat, exp), or None when aug_conf is None.  Pure host
    code.  mos_conf: mosaic_conf()'s dict; aug_conf: augment_conf()'s dict or None.

    Canvas i draws from rng = np.random.default_rng([seed, epoch, file_indices[i], 1]) (the trailing 1 keeps the stream apart
    from draw_augment's) in this fixed order (round = Python's round):
      1. mosaic = rng.random() < prob
      2. a mosaic: px = rng.integers(round(lo * S), round(hi * S) + 1), then py likewise, (lo, hi) = centre, each then clamped
         to [1, S - 1] (no window is empty)
      3. a mosaic: three partner positions rng.integers(0, n) in the slice of n images, for tiles 1, 2, 3; repeats and i itself
         are allowed; tile 0 is image i
      4. a mosaic: four u = rng.uniform(lo, hi), (lo, hi) = scale: tile q's box side is T = max(1, round(S * u))
    Tile q = 0, 1, 2, 3 is the top-left, top-right, bottom-left, bottom-right quadrant around the centre (py, px): its window is
    rows [0, py) or [py, S) x columns [0, px) or [px, S); the four windows partition the canvas.  The tile's WHOLE image is
    letterboxed by letterbox_geometry(h, w, T) into a T x T box, and the box is placed so that the corner of its CONTENT
    rectangle that faces the centre lies at (py, px): for q = 0, ox = px - (pad_l + w_p) and oy = py - (pad_t + h_p); for q = 1,
    ox = px - pad_l; for q = 2 and 3, oy = py - pad_t.  ox and oy may be negative and the box may reach beyond the canvas: the
    window cuts.  Where that geometry is not feasible (w_p < 1 or h_p < 1) the tile falls back to T = S, as draw_augment falls
    back to the identity.
    With aug_conf, tile q takes the flip and the colour record of ITS source image from
    draw_augment(aug_conf, epoch, that image's file index, ...); the zoom of that draw is not used for a tile.  A tile's flip
    mirrors the T x T box in place (local column c -> T - 1 - c, padding included) and the content corner is aligned AFTER the
    flip (pad_l above is then the mirrored box's, T - pad_l - w_p).  Without aug_conf a tile has no flip and no colour.
    A canvas that is not a mosaic is ONE tile whose window is the whole canvas, with the parameters it has without mosaic:
    draw_augment's placement and colour -- a canvas flip restated as the in-box flip, ox' = S - T - ox -- or, without
    aug_conf, identity_placement.

    The partners are positions in the slice, so the result is determined by (seed, epoch, the slice's composition): the batch
    size, the world size and the rank all enter.  Unlike draw_augment, two ranks do NOT see the one-GPU run's dataset."""
    S, epoch, n = int(S), int(epoch), len(shapes)
    lo_c, hi_c = mos_conf['centre']
    lo_s, hi_s = mos_conf['scale']
    aug = {}

    def augmented(i):                      # draw_augment of the slice's image i, once
        if i not in aug:
            aug[i] = draw_augment(aug_conf, epoch, file_indices[i], shapes[i][0], shapes[i][1], S)
        return aug[i]

    tiles, colour = [], []
    for i in range(n):
        rng = np.random.default_rng([int(mos_conf['seed']), epoch, int(file_indices[i]), 1])
        if not rng.random() < mos_conf['prob']:
            h, w = int(shapes[i][0]), int(shapes[i][1])
            if aug_conf is None:
                pl = identity_placement(h, w, S)
            else:
                pl, col = augmented(i)
                colour.append(col)
            cy0, cx0, ch, cw, T, oy, ox, flip = pl
            tiles.append((i, i, cy0, cx0, ch, cw, T, oy, S - T - ox if flip else ox, flip, 0, 0, S, S))
            continue
        px = min(max(int(rng.integers(round(lo_c * S), round(hi_c * S) + 1)), 1), S - 1)
        py = min(max(int(rng.integers(round(lo_c * S), round(hi_c * S) + 1)), 1), S - 1)
        members = [i] + [int(rng.integers(0, n)) for _ in range(3)]
        sides = [max(1, round(S * float(rng.uniform(lo_s, hi_s)))) for _ in range(4)]
        for q, (j, T) in enumerate(zip(members, sides)):
            h, w = int(shapes[j][0]), int(shapes[j][1])
            flip = 0
            if aug_conf is not None:
                pl, col = augmented(j)
                flip = pl[7]
                colour.append(col)
            w_p, h_p, pad_t, _, pad_l, _ = letterbox_geometry(h, w, T)
            if w_p < 1 or h_p < 1:
                T = S
                w_p, h_p, pad_t, _, pad_l, _ = letterbox_geometry(h, w, T)
            if flip:
                pad_l = T - pad_l - w_p
            ox = px - pad_l if q & 1 else px - (pad_l + w_p)
            oy = py - pad_t if q & 2 else py - (pad_t + h_p)
            wy0, wy1 = (py, S) if q & 2 else (0, py)
            wx0, wx1 = (px, S) if q & 1 else (0, px)
            tiles.append((i, j, 0, 0, h, w, T, oy, ox, flip, wy0, wx0, wy1, wx1))
    tiles = np.asarray(tiles, np.int32).reshape(-1, 14)
    return tiles, (None if aug_conf is None else np.asarray(colour, np.float32).reshape(-1, 3))


# ----------------------------------------------------------------------------- bicubic letterbox
def _cubic_weights(t, a=-0.75):
    t = np.asarray(t, np.float64)
    w = np.empty(t.shape + (4,), np.float64)
    w[..., 0] = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w[..., 1] = ((a + 2) * t - (a + 3)) * t * t + 1
    w[..., 2] = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    w[..., 3] = 1.0 - w[..., 0] - w[..., 1] - w[..., 2]
    return w


def _resize_axis(img, n_out, axis):
    n_in = img.shape[axis]
    scale = n_in / n_out
    src = (np.arange(n_out) + 0.5) * scale - 0.5
    i0 = np.floor(src).astype(np.int64)
    wts = _cubic_weights(src - i0)
    out = 0
    for k in range(4):
        idx = np.clip(i0 - 1 + k, 0, n_in - 1)  # replicate border
        shape = [1] * img.ndim
        shape[axis] = n_out
        out = out + np.take(img, idx, axis=axis) * wts[:, k].reshape(shape)
    return out


def letterbox(image, image_size):
    """uint8/float HxWx3 -> (S,S,3) float64 in ~[0,1] + geometry (face_detection.py:112-147)."""
    img = np.asarray(image, np.float64) / 255
    h, w = img.shape[0], img.shape[1]
    w_p, h_p, pt, pb, pl, pr = letterbox_geometry(h, w, image_size)
    img = _resize_axis(_resize_axis(img, max(h_p, 1), 0), max(w_p, 1), 1)
    img = np.pad(img, ((pt, pb), (pl, pr), (0, 0)))
    return img, (h, w, pt, pb, pl, pr)


# ----------------------------------------------------------------------------- training sequence
class TrainingSequence(object):
    """Same batching contract as the reference's keras Sequence (face_detection.py:75-310):
    sorted unique FILE names, fixed consecutive slices, short last batch, hps['step'] overwritten.
    `loader(path) -> HxWx3 uint8` is injectable (PIL by default)."""

    def __init__(self, raw_data_path, hps, nn_arch, CELL_SIZE=None, cell_image_size=None, loader=None):
        import pandas as pd
        self.raw_data_path = raw_data_path
        self.hps = hps
        self.nn_arch = nn_arch
        self.gt_df = pd.read_csv(os.path.join(raw_data_path, 'training.csv'))
        self.groups = {k: v for k, v in self.gt_df.groupby('FILE')}
        self.file_names = sorted(self.groups.keys())
        self.batch_size = hps['batch_size']
        self.hps['step'] = len(self.file_names) // self.batch_size + (1 if len(self.file_names) % self.batch_size else 0)
        self.image_size = nn_arch['image_size']
        self.grid = CELL_SIZE if CELL_SIZE else self.image_size // 32
        self.loader = loader or _pil_loader
        # nn_arch['head'] == 'three_scale' (the build's extension): three target tensors per image
        self.three_scale = nn_arch.get('head', 'single') == 'three_scale'
        self.nclass = int(nn_arch.get('num_classes', 1))

    def encode(self, rows, h, w, placement=None, tiles=None):
        """GT of one image: (G,G,6) for the reference's single-scale head, [t13, t26, t52] for the three-scale head; placement:
        an augmented sample's placement (draw_augment), None = the reference's letterbox; tiles: a mosaic canvas as
        [(rows of the tile's image, tile record)] (draw_mosaic; rows, h, w are then not read)."""
        if self.three_scale:
            return encode_gt_three_scale(rows, h, w, self.image_size, self.nclass, placement=placement, tiles=tiles)
        return encode_gt(rows, h, w, self.image_size, self.grid, self.nn_arch['bb_info_c_size'], placement=placement, tiles=tiles)

    def __len__(self):
        return self.hps['step']

    def __getitem__(self, index):
        names = self.file_names[index * self.batch_size:(index + 1) * self.batch_size]
        images, gts = [], []
        for name in names:
            raw = self.loader(os.path.join(self.raw_data_path, name))
            img, (h, w, *_rest) = letterbox(raw, self.image_size)
            df = self.groups[name]
            gts.append(self.encode(df.iloc[:, 3:7].values, h, w))
            images.append(img)
        if self.three_scale:
            return ({'input1': np.asarray(images)}, {'output%d' % s: np.asarray([g[s] for g in gts]) for s in range(3)})
        return ({'input1': np.asarray(images)}, {'output': np.asarray(gts)})

    def get_raw(self, index):
        """Same batch, but images stay raw uint8 (decoded only): the letterbox then runs on the
        device (fv_letterbox).  -> (list of HxWx3 uint8 arrays, (b,G,G,6) float32 GT tensors)."""
        names = self.file_names[index * self.batch_size:(index + 1) * self.batch_size]
        raws, gts = [], []
        for name in names:
            raw = self.loader(os.path.join(self.raw_data_path, name))
            df = self.groups[name]
            gts.append(self.encode(df.iloc[:, 3:7].values, raw.shape[0], raw.shape[1]))
            raws.append(raw)
        if self.three_scale:
            return raws, [np.asarray([g[s] for g in gts], np.float32) for s in range(3)]
        return raws, np.asarray(gts, np.float32)


def _pil_loader(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


# ----------------------------------------------------------------------------- synthetic data
def synth_gt_batch(batch, image_size=416, faces_per_image=5, seed=1234, grid=None):
    """Synthetic GT tensors (B,G,G,6) float32 through encode_gt."""
    rng = np.random.default_rng(seed)
    grid = grid or image_size // 32
    out = np.zeros((batch, grid, grid, 6), np.float32)
    for b in range(batch):
        h, w = int(rng.integers(300, 1100)), int(rng.integers(300, 1100))
        n = max(1, int(rng.poisson(faces_per_image)))
        fw = rng.uniform(12, w / 4, n); fh = rng.uniform(12, h / 4, n)
        fx = rng.uniform(1, w - fw - 1); fy = rng.uniform(1, h - fh - 1)
        out[b] = encode_gt(np.stack([fx, fy, fw, fh], 1), h, w, image_size, grid)
    return out


def make_synthetic_uccs(root, n_images=4, seed=0, csv_name='training.csv', sizes=None):
    """Write a tiny UCCS-format dataset: JPEGs of uniform noise + csv with the reference's column
    order.  Returns the DataFrame."""
    import pandas as pd
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    sizes = sizes or [(480, 640), (640, 480), (600, 800), (416, 416)]
    rows = []
    fid = 0
    for k in range(n_images):
        h, w = sizes[k % len(sizes)]
        name = 'synth_%04d.jpg' % k
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, name), quality=90)
        for _ in range(int(rng.integers(1, 4))):
            fw = float(rng.uniform(20, w / 3)); fh = float(rng.uniform(20, h / 3))
            fx = float(rng.uniform(1, w - fw - 1)); fy = float(rng.uniform(1, h - fh - 1))
            rows.append([fid, name, int(rng.integers(1, 100)), round(fx, 1), round(fy, 1), round(fw, 1), round(fh, 1)])
            fid += 1
    df = pd.DataFrame(rows, columns=CSV_COLUMNS)
    df.to_csv(os.path.join(root, csv_name), index=False)
    return df
