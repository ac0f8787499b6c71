"""numpy restatement of the bicubic letterbox IN FLOAT32, IN THE KERNEL'S ORDER (test aid): the pin of the resampling's bits that
does not come from csrc/preproc.hip.  The library is built with -ffp-contract=off, so every float32 operation below rounds
where the kernel's does:

  * the source coordinate of output index i is float64: (i + 0.5) * (n_src / n_dst) - 0.5; s = floor, t = float32(f - s);
  * the four weights are evaluated term by term in float32 (a = -0.75);
  * a pixel is the sum over tap rows j = 0..3 of wy[j] * (the sum over i = 0..3 of wx[i] * tap), both sums starting from +0,
    the border replicated at the CROP's edges, multiplied once by float32(1) / float32(255);
  * padding is +0; the geometry is data.letterbox_geometry.

box() makes one T x T box per crop; placement, flip and window composition are tests/letterbox_augment_ref.py's place() and
tests/letterbox_mosaic_ref.py's compose()."""
import numpy as np

import letterbox_augment_ref as aref
import letterbox_mosaic_ref as mref
from face_vijnana_yolov3_amd import data

F = np.float32


def cubic_w(t):
    """float32 array t -> [..., 4] float32 weights, the kernel's expressions term by term."""
    t = np.asarray(t, F)
    a = F(-0.75)
    one = F(1)
    w = np.empty(t.shape + (4,), F)
    u = t + one
    w[..., 0] = ((a * u - F(5) * a) * u + F(8) * a) * u - F(4) * a
    w[..., 1] = ((a + F(2)) * t - (a + F(3))) * t * t + one
    v = one - t
    w[..., 2] = ((a + F(2)) * v - (a + F(3))) * v * v + one
    w[..., 3] = one - w[..., 0] - w[..., 1] - w[..., 2]
    assert w.dtype == F
    return w


def axis(n_dst, n_src):
    """-> (s int64 [n_dst], w float32 [n_dst, 4]): floor of the source coordinate and the weights of every output index."""
    f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5
    s = np.floor(f)
    return s.astype(np.int64), cubic_w((f - s).astype(F))


def resample(crop, h_p, w_p):
    """uint8 h x w x 3 -> float32 h_p x w_p x 3: the taps of one pixel in the kernel's order."""
    crop = np.asarray(crop)
    assert crop.dtype == np.uint8 and crop.ndim == 3 and crop.shape[2] == 3
    h, w = crop.shape[:2]
    sy, wy = axis(h_p, h)
    sx, wx = axis(w_p, w)
    px = crop.astype(F)
    out = np.zeros((h_p, w_p, 3), F)
    for j in range(4):
        rows = px[np.clip(sy - 1 + j, 0, h - 1)]                          # [h_p, w, 3]
        rr = np.zeros((h_p, w_p, 3), F)
        for i in range(4):
            rr = rr + wx[None, :, i, None] * rows[:, np.clip(sx - 1 + i, 0, w - 1)]
        out = out + wy[:, j, None, None] * rr
    out = out * (F(1) / F(255))
    assert out.dtype == F
    return out


def box(crop, T):
    """uint8 h x w x 3 crop -> its T x T x 3 float32 letterbox (fv_letterbox of a contiguous copy of the crop at image size T)."""
    h, w = np.asarray(crop).shape[:2]
    w_p, h_p, pad_t, _pb, pad_l, _pr = data.letterbox_geometry(h, w, T)
    out = np.zeros((T, T, 3), F)
    out[pad_t:pad_t + h_p, pad_l:pad_l + w_p] = resample(crop, h_p, w_p)
    return out


def crop_box(image, rec, T):
    """rec = (y0, x0, h, w) inside `image`"""
    y0, x0, h, w = (int(v) for v in rec)
    return box(np.asarray(image)[y0:y0 + h, x0:x0 + w], T)


def augment(image, placement, S):
    """placement = (cy0, cx0, ch, cw, T, oy, ox, flip) -> the S x S x 3 canvas of fv_letterbox_augment_batch without colour"""
    return aref.place(crop_box(image, placement[:4], placement[4]), placement, S)


def mosaic(images, recs, S):
    """recs: the 14-int tile records of ONE canvas -> the S x S x 3 canvas of fv_letterbox_mosaic_batch without colour"""
    return mref.compose([crop_box(images[int(r[1])], r[2:6], int(r[6])) for r in recs], recs, S)
