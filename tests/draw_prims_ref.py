"""numpy restatement of fv_draw_prims_u8's contract (test aid): the primitives applied one after another, in table order, to
the packed uint8 RGB images of a batch.  Written from include/fv_hotpath.h, pixel set by pixel set; no tiles, no culling."""
import numpy as np

from face_vijnana_yolov3_amd.annotate import MaskBlend, Outline


def draw_prims_ref(buf, offsets, hw, prims, masks):
    """buf: uint8 (bytes,) packed images, changed in place; offsets / hw as for fv_letterbox_batch; prims: Outline / MaskBlend
    records (MaskBlend.mask_off into `masks`, a uint8 array)."""
    for p in prims:
        H, W = int(hw[2 * p.image]), int(hw[2 * p.image + 1])
        img = buf[offsets[p.image]:offsets[p.image] + H * W * 3].reshape(H, W, 3)
        ys, xs = np.mgrid[0:H, 0:W]
        if isinstance(p, Outline):
            inside = (xs >= p.x0) & (xs <= p.x1) & (ys >= p.y0) & (ys <= p.y1)
            w = p.width
            edge = (xs - p.x0 < w) | (p.x1 - xs < w) | (ys - p.y0 < w) | (p.y1 - ys < w)
            img[inside & edge] = p.color
        else:
            assert isinstance(p, MaskBlend)
            m = np.asarray(masks[p.mask_off:p.mask_off + p.mw * p.mh], np.uint8).reshape(p.mh, p.mw)
            inside = (xs >= p.x) & (xs < p.x + p.mw) & (ys >= p.y) & (ys < p.y + p.mh)
            mm = m[(ys - p.y)[inside], (xs - p.x)[inside]].astype(np.uint32)[:, None]
            old = img[inside].astype(np.uint32)
            t = old * (255 - mm) + np.asarray(p.color, np.uint32)[None, :] * mm + 128
            img[inside] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return buf


def pillow_boxes(image, boxes, color, font):
    """draw_boxes_v3 (yolov3_detect.py:515-530) with Pillow, on a uint8 (H, W, 3) array -> a new array."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.ascontiguousarray(image))
    draw = ImageDraw.Draw(im)
    for box in boxes:
        draw.rectangle([box.xmin, box.ymin, box.xmax, box.ymax], outline=color, width=3)
        draw.text((box.xmin, box.ymin - 20), str(box.get_score()) + ', ' + str(box.classes[0]) + ', ' + str(box.subject_id),
                  fill=color, font=font)
    return np.asarray(im)


def _box(xmin, ymin, xmax, ymax, score, subject_id):
    from face_vijnana_yolov3_amd.postproc import BoundBox
    return BoundBox(xmin, ymin, xmax, ymax, objness=1., classes=[np.float32(score)], subject_id=subject_id)


def box_cases(H, W, rng, n_random=4):
    """About a dozen boxes for an H x W image, every kind the drawing has to get right: float corners, a box hanging off each of
    the four sides, one fully outside, boxes that overlap, labels that clip at the top (ymin < 20) and at the right, a negative
    fractional xmin.  Both truncated extents of every box are >= 3 and the corners ordered, where the closed form is Pillow's."""
    boxes = [
        _box(5.7, H * 0.35 + 0.3, min(W - 2.5, 40.2), H * 0.35 + 14.9, 0.9371, 12),             # float corners, inside
        _box(-7.6, H * 0.3, 9.4, H * 0.3 + 9.2, 0.25, -1),                                   # off the left; negative fractional xmin
        _box(W - 9.3, H * 0.4 + 0.5, W + 11.8, H - 3.0, 0.5, 7),                             # off the right; label clips at the right
        _box(W / 3, -6.4, W / 3 + 14.6, 8.9, 0.125, 3),                                   # off the top; label wholly above the image
        _box(W / 4, H - 7.7, W / 4 + 12.1, H + 9.2, 0.75, 1041),                          # off the bottom
        _box(W + 30.5, H + 30.5, W + 60.0, H + 70.0, 0.3, 5),                             # fully outside, label too
        _box(-90.0, -80.0, -50.5, -40.5, 0.3, 5),                                         # fully outside, above and left
        _box(3.2, 6.8, W - 4.4, 17.3, 0.6021, 44),                                        # label clips at the top (ymin < 20)
        _box(W - 30.5, H / 2, W - 3.5, H / 2 + 9.5, 0.8, 123456),                         # inside, its label runs off the right
        _box(8.9, H * 0.35 + 2.1, min(W - 1.2, 44.0), H * 0.35 + 12.5, 0.4, 2),             # overlaps the first
    ]
    for _ in range(n_random):
        x0, y0 = rng.uniform(-20, W), rng.uniform(-20, H)
        boxes.append(_box(x0, y0, x0 + rng.uniform(4.5, W), y0 + rng.uniform(4.5, H), rng.uniform(0, 1), int(rng.integers(-1, 99))))
    for b in boxes:
        assert int(b.xmax) - int(b.xmin) >= 3 and int(b.ymax) - int(b.ymin) >= 3, (H, W, b.xmin, b.ymin, b.xmax, b.ymax)
    return boxes
