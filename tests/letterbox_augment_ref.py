"""numpy restatement of fv_letterbox_augment_batch's contract (test aid): the colour stage -- Darknet's distort_image as
include/fv_hotpath.h states it -- in float64, or with every operation in float32 (dtype=np.float32: the kernel's arithmetic in the
kernel's order, the yardstick of what float32 itself costs), and the whole canvas of one sample built on data.letterbox."""
import numpy as np

from face_vijnana_yolov3_amd import data


def colour_stage(rgb, dh, sat, ex, dtype=np.float64, skip_identity=True):
    """rgb: array [..., 3] -> [..., 3] of dtype.  (dh, sat, ex) exactly (0, 1, 1) returns the input unchanged (not even clamped),
    as the kernel skips the stage; skip_identity=False runs the arithmetic anyway."""
    F = np.dtype(dtype).type
    x = np.asarray(rgb).astype(dtype)
    dh, sat, ex = F(dh), F(sat), F(ex)
    if skip_identity and dh == 0 and sat == 1 and ex == 1:
        return x
    x = np.clip(x, F(0), F(1))
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mx = np.maximum(r, np.maximum(g, b)); mn = np.minimum(r, np.minimum(g, b))
    d = mx - mn
    s = np.where(mx == 0, F(0), d / np.where(mx == 0, F(1), mx))
    dd = np.where(d == 0, F(1), d)
    h = np.where(r == mx, (g - b) / dd, np.where(g == mx, F(2) + (b - r) / dd, F(4) + (r - g) / dd))
    h = np.where(d == 0, F(0), h)
    h = np.where(h < 0, h + F(6), h)
    h = h / F(6)
    h = h + dh
    h = h - np.floor(h)
    s = s * sat
    v = mx * ex
    h6 = F(6) * h
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int64) % 6
    p = v * (F(1) - s); q = v * (F(1) - s * f); t = v * (F(1) - s * (F(1) - f))
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty_like(x)
    for c in range(3):
        out[..., c] = np.select([i == k for k in range(6)], [table[k][c] for k in range(6)])
    assert out.dtype == np.dtype(dtype)
    return np.clip(out, F(0), F(1))


def content_rect(placement):
    """-> (top, left, h_p, w_p) of the placed content in the unflipped canvas."""
    cy0, cx0, ch, cw, T, oy, ox, flip = placement
    w_p, h_p, pad_t, _, pad_l, _ = data.letterbox_geometry(ch, cw, T)
    return oy + pad_t, ox + pad_l, h_p, w_p


def place(box, placement, S):
    """A T x T x 3 letterboxed crop -> the S x S x 3 canvas of `placement` (zeros around the box, mirrored when flip)."""
    cy0, cx0, ch, cw, T, oy, ox, flip = placement
    canvas = np.zeros((S, S, 3), box.dtype)
    canvas[oy:oy + T, ox:ox + T] = box
    return canvas[:, ::-1].copy() if flip else canvas


def augment(image, placement, colour, S, dtype=np.float64):
    """One sample from scratch: uint8 h x w x 3 image -> S x S x 3 canvas (data.letterbox's bicubic restatement for the pixels)."""
    cy0, cx0, ch, cw, T, oy, ox, flip = placement
    box, _ = data.letterbox(np.asarray(image)[cy0:cy0 + ch, cx0:cx0 + cw], T)
    box = box.astype(dtype)
    if colour is not None:
        top, left, h_p, w_p = content_rect((0, 0, ch, cw, T, 0, 0, 0))
        box[top:top + h_p, left:left + w_p] = colour_stage(box[top:top + h_p, left:left + w_p], *colour, dtype=dtype)
    return place(box, placement, S)
