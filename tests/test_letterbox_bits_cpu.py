"""tests/letterbox_bits_ref.py (the float32 restatement the GPU bit tests compare against) against data.letterbox (float64): the
restatement itself stays within the bound tests/test_postproc_gpu.py sets for the device, 3e-6 (measured here: 1.2e-6 at most)."""
import numpy as np
import pytest

import letterbox_bits_ref as bref
from face_vijnana_yolov3_amd import data

CASES = [(80, 100, 32), (100, 80, 64), (64, 64, 96), (50, 71, 17), (9, 7, 60), (1, 1, 1), (33, 47, 64), (1080, 1920, 416)]


@pytest.mark.parametrize('h,w,S', CASES)
def test_float32_restatement_against_data_letterbox(h, w, S):
    raw = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = bref.box(raw, S)
    want, (_h, _w, pt, pb, pl, pr) = data.letterbox(raw, S)
    assert got.dtype == np.float32 and got.shape == (S, S, 3)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('%d x %d -> %d: max |float32 restatement - float64| = %.3g' % (h, w, S, err))
    assert err <= 3e-6
    pad = np.ones((S, S), bool); pad[pt:S - pb, pl:S - pr] = False
    assert (got[pad].view(np.int32) == 0).all()                       # padding is +0
