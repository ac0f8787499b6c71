"""numpy restatement of fv_letterbox_mosaic_batch's contract (test aid): a canvas composed from per-tile T x T boxes -- window
slicing, the in-box flip, zeros elsewhere -- and the placement rule of data.draw_mosaic's quadrants, written out once more.  The
colour stage is tests/letterbox_augment_ref.py's."""
import numpy as np

import letterbox_augment_ref as aref
from face_vijnana_yolov3_amd import data

FIELDS = ('canvas', 'image', 'cy0', 'cx0', 'ch', 'cw', 'T', 'oy', 'ox', 'flip', 'wy0', 'wx0', 'wy1', 'wx1')


def content_rect(rec):
    """-> (pad_t, pad_l, h_p, w_p): the content rectangle inside the tile's UNFLIPPED T x T box."""
    ch, cw, T = int(rec[4]), int(rec[5]), int(rec[6])
    w_p, h_p, pad_t, _, pad_l, _ = data.letterbox_geometry(ch, cw, T)
    return pad_t, pad_l, h_p, w_p


def colour_box(box, rec, colour, dtype=np.float64):
    """The unflipped box with the colour stage run on its content rectangle (padding stays 0); colour None: the box as it is."""
    out = np.asarray(box).astype(dtype)
    if colour is not None:
        t, l, h_p, w_p = content_rect(rec)
        out[t:t + h_p, l:l + w_p] = aref.colour_stage(np.asarray(box)[t:t + h_p, l:l + w_p], *[float(v) for v in colour], dtype=dtype)
    return out


def compose(boxes, recs, S, dtype=np.float32):
    """One canvas: boxes[k] is the UNFLIPPED T x T x 3 box of tile recs[k] (any tile order; the windows are disjoint)."""
    canvas = np.zeros((S, S, 3), dtype)
    for box, rec in zip(boxes, recs):
        _c, _i, _cy0, _cx0, _ch, _cw, T, oy, ox, flip, wy0, wx0, wy1, wx1 = (int(v) for v in rec)
        assert box.shape == (T, T, 3)
        placed = box[:, ::-1] if flip else box
        y_lo, y_hi, x_lo, x_hi = max(wy0, oy), min(wy1, oy + T), max(wx0, ox), min(wx1, ox + T)
        if y_lo < y_hi and x_lo < x_hi:
            canvas[y_lo:y_hi, x_lo:x_hi] = placed[y_lo - oy:y_hi - oy, x_lo - ox:x_hi - ox]
    return canvas


def quadrant_tile(canvas, image, h, w, q, py, px, T, flip, S):
    """Tile q (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) of a mosaic with centre (py, px): the whole h x w image in a
    box of side T whose content corner facing the centre lies at (py, px), the corner taken AFTER the in-box flip."""
    w_p, h_p, pad_t, _pb, pad_l, pad_r = data.letterbox_geometry(h, w, T)
    left = pad_r if flip else pad_l                                    # the content's first column in the (mirrored) box
    ox = px - left if q in (1, 3) else px - (left + w_p)
    oy = py - pad_t if q in (2, 3) else py - (pad_t + h_p)
    win = [(0, 0, py, px), (0, px, py, S), (py, 0, S, px), (py, px, S, S)][q]
    return (canvas, image, 0, 0, h, w, T, oy, ox, int(flip)) + win
