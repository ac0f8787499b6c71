"""numpy restatement of fv_crop_nearest_u8's contract (test aid): the reference's cv.resize(INTER_NEAREST) followed by
cv.copyMakeBorder(value 0) on a uint8 crop, with OpenCV's resizeNN index rule
    source column of destination column x = min(floor(x * ifx), w - 1),  ifx = 1.0 / (w_p / w)   (IEEE fp64; rows likewise)
and data.letterbox_geometry's sizes and pads.  cv2 is not installed here: this rule is the build's definition of INTER_NEAREST."""
import numpy as np

from face_vijnana_yolov3_amd.data import letterbox_geometry


def nearest_index(n_src, n_dst):
    inv = 1.0 / (n_dst / float(n_src))
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * inv).astype(np.int64), n_src - 1)


def nearest_letterbox(crop, image_size):
    """uint8 (h, w, 3) -> uint8 (S, S, 3)."""
    h, w = crop.shape[:2]
    w_p, h_p, pad_t, pad_b, pad_l, pad_r = letterbox_geometry(h, w, image_size)
    assert w_p >= 1 and h_p >= 1
    out = np.zeros((image_size, image_size, 3), np.uint8)
    out[pad_t:pad_t + h_p, pad_l:pad_l + w_p] = crop[nearest_index(h, h_p)][:, nearest_index(w, w_p)]
    assert pad_t + h_p + pad_b == image_size and pad_l + w_p + pad_r == image_size
    return out
