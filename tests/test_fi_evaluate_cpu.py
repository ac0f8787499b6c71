"""FaceIdentifier.evaluate without a GPU: annotate.annotation_prims through the numpy restatement of fv_draw_prims_u8's
contract (tests/draw_prims_ref.py) against Pillow drawing the same boxes as draw_boxes_v3 does (exact), the two documented
deviations, the ground-truth filter, and the method's presence."""
import numpy as np
import pytest

from draw_prims_ref import _box, box_cases, draw_prims_ref, pillow_boxes
from face_vijnana_yolov3_amd import face_identification as fi

RED, GREEN = (255, 0, 0), (0, 255, 0)


def _drawn(img, layers, font):
    """`layers` = [(boxes, color), ...] through annotation_prims + the contract -> a new (H, W, 3) array."""
    H, W = img.shape[:2]
    prims = []
    for boxes, color in layers:
        prims += fi.annotation_prims(0, boxes, color, font)
    prims, masks = fi.pack_masks(prims)
    buf = img.reshape(-1).copy()
    draw_prims_ref(buf, [0], [H, W], prims, masks)
    return buf.reshape(H, W, 3), prims


@pytest.mark.parametrize('shape', [(37, 150), (120, 45), (64, 64), (90, 131)])
def test_annotation_prims_equal_pillow(shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    font = fi._font()
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = box_cases(H, W, rng)
    gt, det = boxes[:len(boxes) // 2], boxes[len(boxes) // 2:]
    for layers in ([(boxes, RED)], [(boxes, GREEN)], [(gt, RED), (det, GREEN)]):
        got, prims = _drawn(img, layers, font)
        want = img
        for bs, color in layers:
            want = pillow_boxes(want, bs, color, font)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, img)
        n = sum(len(bs) for bs, _ in layers)
        assert len(prims) == 2 * n
        assert all(isinstance(p, fi.Outline) and p.width == 3 for p in prims[0::2])
        assert all(isinstance(p, fi.MaskBlend) for p in prims[1::2])


def test_label_text_and_truncation_toward_zero():
    font = fi._font()
    b = _box(-2.7, 30.9, 17.99, 44.2, 0.5, 31)
    o, m = fi.annotation_prims(3, [b], GREEN, font)
    assert (o.image, o.x0, o.y0, o.x1, o.y1, o.width, o.color) == (3, -2, 30, 17, 44, 3, GREEN)
    assert m.image == 3 and m.color == GREEN and m.mask.shape == (m.mh, m.mw) and m.mask.dtype == np.uint8
    from face_vijnana_yolov3_amd.annotate import label_text
    assert label_text(b) == '0.5, 0.5, 31'
    b.classes = [np.float32(1.5)]; b.score = -1
    assert label_text(b) == '1.0, 1.5, 31'                  # get_score() caps at 1, classes[0] does not


def test_font_is_the_reference_size():
    f = fi._font()
    assert getattr(f, 'size', 25) == 25


def test_deviation_disordered_box_is_not_drawn():
    """int(xmax) < int(xmin) or int(ymax) < int(ymin): Pillow raises ValueError; here the box leaves the frame alone."""
    from PIL import Image, ImageDraw
    font = fi._font()
    img = np.random.default_rng(1).integers(0, 256, (50, 60, 3)).astype(np.uint8)
    for b in (_box(30.2, 30.0, 20.9, 40.0, 0.5, 1), _box(10.0, 41.5, 30.0, 35.5, 0.5, 1)):
        with pytest.raises(ValueError):
            ImageDraw.Draw(Image.fromarray(img)).rectangle([b.xmin, b.ymin, b.xmax, b.ymax], outline=RED, width=3)
        assert fi.annotation_prims(0, [b], RED, font) == []
        ok = _box(5.0, 25.0, 25.0, 45.0, 0.5, 2)
        got, _ = _drawn(img, [([b, ok], RED)], font)
        assert np.array_equal(got, pillow_boxes(img, [ok], RED, font))


@pytest.mark.parametrize('ext', [(0, 9), (1, 9), (2, 9), (9, 0), (9, 2), (2, 2), (0, 0)])
def test_deviation_sliver_is_filled_inside_its_corners(ext):
    """A truncated extent below 3: the closed form paints every pixel of [x0, x1] x [y0, y1] and none outside (Pillow's
    width-3 outline of such a box spills over its corners)."""
    dx, dy = ext
    font = fi._font()
    img = np.random.default_rng(2).integers(0, 256, (40, 50, 3)).astype(np.uint8)
    b = _box(20.3, 30.6, 20.3 + dx, 30.6 + dy, 0.5, 1)
    outline = fi.annotation_prims(0, [b], GREEN, font)[0]
    buf = img.reshape(-1).copy()
    draw_prims_ref(buf, [0], [40, 50], [outline], np.zeros(0, np.uint8))
    want = img.copy()
    want[30:30 + dy + 1, 20:20 + dx + 1] = GREEN
    assert np.array_equal(buf.reshape(40, 50, 3), want)


def test_extent_three_is_where_pillow_and_the_closed_form_meet():
    font = fi._font()
    img = np.random.default_rng(3).integers(0, 256, (40, 50, 3)).astype(np.uint8)
    for dx, dy in ((3, 3), (3, 8), (8, 3), (4, 5)):
        b = _box(10.0, 25.0, 10.0 + dx, 25.0 + dy, 0.5, 1)
        got, _ = _drawn(img, [([b], RED)], font)
        assert np.array_equal(got, pillow_boxes(img, [b], RED, font))


def test_ground_truth_boxes_filter_and_corners():
    import pandas as pd
    df = pd.DataFrame({'FACE_ID': [0, 1, 2, 3, 4], 'FILE': ['a.jpg'] * 5, 'SUBJECT_ID': [7, -1, 3, 4, 5],
                       'FACE_X': [10.5, 3.0, 0.0, 5.0, 8.0], 'FACE_Y': [20.25, 4.0, 5.0, 6.0, 9.0],
                       'FACE_WIDTH': [30.5, 5.0, 5.0, 0.0, 4.0], 'FACE_HEIGHT': [12.0, 6.0, 5.0, 7.0, -1.0]})
    boxes = fi.ground_truth_boxes(df)
    assert [(b.xmin, b.ymin, b.xmax, b.ymax, b.subject_id) for b in boxes] == [(10, 20, 40, 31, 7), (3, 4, 7, 9, -1)]
    assert all(b.objness == 1. and b.classes == [1.0] for b in boxes)


def test_matched_boxes_is_the_row_rule():
    rects = [(0, 0, 1, 1), None, (0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1)]
    dist = np.array([0.1, np.inf, 0.9, 0.2, 0.3])
    assert fi.matched_boxes(rects, dist, 0.5) == [0, 3, 4]
    assert fi.matched_boxes(rects, dist, 0.5, limit=2) == [0, 3]


def test_evaluate_is_a_method():
    assert callable(getattr(fi.FaceIdentifier, 'evaluate'))
    assert 'main()' in fi.FaceIdentifier.evaluate.__doc__
