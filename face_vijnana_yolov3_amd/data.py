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


def encode_gt(faces, h, w, image_size=416, grid=13, channels=6, placement=None):
    """Ground-truth tensor of one image (face_detection.py:150-202).

    faces: array-like (n,4) of FACE_X, FACE_Y, FACE_WIDTH, FACE_HEIGHT in csv order; rows with
    any value <= 0 are skipped; later rows overwrite earlier ones in the same cell.
    placement: None (the reference's letterbox) or (cy0, cx0, ch, cw, T, oy, ox, flip) as draw_augment returns it
    (_placed_centres states the arithmetic); the box sizes are then fractions of the canvas, (x2 - x1 + 1) / m * (T / S)."""
    cell = image_size // grid
    gt = np.zeros((grid, grid, channels), np.float64)
    for x1, y1, x2, y2, xc, yc, m, T in _placed_centres(faces, h, w, image_size, placement):
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
                          placement=None):
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
    placement: as for encode_gt; the box in network pixels is then (x2 - x1 + 1) / m * T."""
    S = int(image_size)
    C = 5 + nclass
    out = [np.zeros((S // 32 << s, S // 32 << s, 3 * C), np.float64) for s in range(3)]
    for x1, y1, x2, y2, xc, yc, m, T in _placed_centres(faces, h, w, S, placement):
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


# ----------------------------------------------------------------------------- training augmentation (hps['augment'])
AUGMENT_DEFAULTS = {'zoom': [0.75, 1.25], 'flip': 0.5, 'hue': 0.1, 'saturation': 1.5, 'exposure': 1.5, 'seed': 0}


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

    def encode(self, rows, h, w, placement=None):
        """GT of one image: (G,G,6) for the reference's single-scale head, [t13, t26, t52] for the three-scale head; placement:
        an augmented sample's placement (draw_augment), None = the reference's letterbox."""
        if self.three_scale:
            return encode_gt_three_scale(rows, h, w, self.image_size, self.nclass, placement=placement)
        return encode_gt(rows, h, w, self.image_size, self.grid, self.nn_arch['bb_info_c_size'], placement=placement)

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
