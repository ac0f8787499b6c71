"""Host side of FaceIdentifier.evaluate's annotated frames: boxes -> the ordered primitives fv_draw_prims_u8 draws.

draw_boxes_v3 (yolov3_detect.py:515-530) draws, box after box, `ImageDraw.rectangle([xmin, ymin, xmax, ymax], outline=color,
width=3)` and `ImageDraw.text((xmin, ymin - 20), '<score>, <class score>, <subject id>', fill=color, font=arial 25)`; it
ignores its threshold argument.  Here a box becomes an Outline (the closed form of that rectangle) and a MaskBlend (Pillow's
own rasterisation of the label, blended on the device by Pillow's own formula), so the device draws what Pillow would have drawn
-- bit for bit, but for the two deviations at annotation_prims."""
import collections
import math

import numpy as np

# image: index into the batch; color: (r, g, b).  Outline: integer corners, inclusive.  MaskBlend: top-left (x, y) of an mh x mw
# 8-bit mask that lies mask_off bytes into the mask buffer (pack_masks sets it); mask: the host array until then.
Outline = collections.namedtuple('Outline', 'image x0 y0 x1 y1 width color')
MaskBlend = collections.namedtuple('MaskBlend', 'image x y mw mh mask_off color mask')

OUTLINE_WIDTH = 3               # yolov3_detect.py:524
FONT_SIZE = 25                  # yolov3_detect.py:525
LABEL_RISE = 20                 # the label's anchor sits 20 rows above the box (yolov3_detect.py:526)


def _font(size=FONT_SIZE):
    """The reference asks for arial.ttf, which a Linux host rarely has: the fallback chain of face_detection._font."""
    from PIL import ImageFont
    for name in ('arial.ttf', 'DejaVuSans.ttf'):
        try:
            return ImageFont.truetype(name, size)
        except OSError:
            continue
    return ImageFont.load_default()


def label_text(box):
    return str(box.get_score()) + ', ' + str(box.classes[0]) + ', ' + str(box.subject_id)


def text_mask(font, text, x, y):
    """What ImageDraw.text((x, y), text, font=font) blends into an RGB image: (mask uint8 (mh, mw), left, top).  The position is
    split as ImageDraw.text splits it -- the integer part places the mask, the fraction goes to the rasteriser."""
    from PIL import Image
    left, top = int(x), int(y)
    if hasattr(font, 'getmask2'):
        core, offset = font.getmask2(text, mode='L', anchor='la', start=(math.modf(x)[0], math.modf(y)[0]))
        left += offset[0]; top += offset[1]
    else:                                       # the bitmap font of a Pillow built without FreeType: a 0 / 255 mask, no offset
        core = font.getmask(text)
    mw, mh = core.size
    if mw == 0 or mh == 0:
        return np.zeros((0, 0), np.uint8), left, top
    return np.asarray(Image.Image()._new(core).convert('L')), left, top


def annotation_prims(image_index, boxes, color, font):
    """The primitives that draw `boxes` on image `image_index` as draw_boxes_v3 does: per box, in box order, an Outline of width 3
    with corners int() of xmin, ymin, xmax, ymax (truncation toward zero, as Pillow treats float coordinates), then the
    MaskBlend of its label at (xmin, ymin - 20).  Two deviations from Pillow:
      * a box with int(xmax) < int(xmin) or int(ymax) < int(ymin) is not drawn at all -- neither outline nor label (Pillow's
        rectangle raises ValueError for it, which would end the reference's evaluate());
      * a box with int(xmax) - int(xmin) < 3 or int(ymax) - int(ymin) < 3 is filled by the Outline's closed form; Pillow's
        width-3 outline of such a sliver spills outside the box.
    From 3 upward the closed form is Pillow's rectangle exactly."""
    color = tuple(int(c) for c in color)
    prims = []
    for box in boxes:
        x0, y0, x1, y1 = int(box.xmin), int(box.ymin), int(box.xmax), int(box.ymax)
        if x1 < x0 or y1 < y0:
            continue
        prims.append(Outline(image_index, x0, y0, x1, y1, OUTLINE_WIDTH, color))
        mask, left, top = text_mask(font, label_text(box), box.xmin, box.ymin - LABEL_RISE)
        prims.append(MaskBlend(image_index, left, top, mask.shape[1], mask.shape[0], None, color, mask))
    return prims


def pack_masks(prims):
    """-> (the primitives with every MaskBlend's mask_off set and its host mask dropped, the masks back to back as one uint8
    array): the table and the mask buffer of draw_prims_u8."""
    out, parts, off = [], [], 0
    for p in prims:
        if isinstance(p, MaskBlend):
            m = np.ascontiguousarray(p.mask, np.uint8)
            assert m.shape == (p.mh, p.mw)
            out.append(p._replace(mask_off=off, mask=None))
            parts.append(m.reshape(-1)); off += m.size
        else:
            out.append(p)
    return out, (np.concatenate(parts) if parts else np.zeros(0, np.uint8))
