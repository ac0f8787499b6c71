"""FaceIdentifier.evaluate's drawing step on one GPU: fv_draw_prims_u8 per batch of decoded frames (the device call, and the
host work in front of it: Pillow's label rasterisation + the table) against the host alternative it avoids -- decoding the
batch's JPEGs again with Pillow and drawing the same boxes with ImageDraw (draw_boxes_v3's calls), on one thread.  Two frame
sizes: 1920 x 1080 and UCCS' 5184 x 3456; `--boxes` boxes per frame, a fifth of them ground truth.  Prints one JSON line.

    python tools/fi_evaluate_bench.py [--boxes N] [--iters N]
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import face_identification as fi  # noqa: E402
from face_vijnana_yolov3_amd._lib import Context  # noqa: E402
from face_vijnana_yolov3_amd.postproc import BoundBox, letterbox_batch_device  # noqa: E402

S = 416
RED, GREEN = (255, 0, 0), (0, 255, 0)


def frame_boxes(rng, H, W, n):
    out = []
    for _ in range(n):
        w, h = int(rng.integers(40, 220)), int(rng.integers(40, 220))
        x, y = rng.uniform(2, W - w), rng.uniform(2, H - h)
        out.append(BoundBox(x, y, x + w, y + h, objness=1., classes=[np.float32(rng.uniform(0.5, 1.0))],
                            subject_id=int(rng.integers(-1, 1000))))
    return out[:max(1, n // 5)], out[max(1, n // 5):]


def one_size(ctx, H, W, frames, boxes, iters):
    from PIL import Image
    from face_vijnana_yolov3_amd.annotate import label_text
    rng = np.random.default_rng(H)
    font = fi._font()
    raws, datas = [], []
    for _ in range(frames):
        base = rng.integers(0, 256, (H // 16, W // 16, 3)).astype(np.uint8)
        raws.append(np.kron(base, np.ones((16, 16, 1), np.uint8)))
        f = io.BytesIO()
        Image.fromarray(raws[-1]).save(f, format='JPEG', quality=90)
        datas.append(f.getvalue())
    keep = []
    letterbox_batch_device(ctx, raws, S, torch.device('cuda', 0), keep=keep)
    per_frame = [frame_boxes(rng, H, W, boxes) for _ in range(frames)]

    def host_prims():
        prims = []
        for i, (gt, det) in enumerate(per_frame):
            prims += fi.annotation_prims(i, gt, RED, font) + fi.annotation_prims(i, det, GREEN, font)
        return fi.pack_masks(prims)

    t = time.perf_counter()
    for _ in range(iters):
        prims, masks = host_prims()
    t_prims = (time.perf_counter() - t) / iters
    dmasks = torch.from_numpy(masks).cuda()
    for _ in range(2):
        fi.draw_prims_u8(ctx, keep[0], prims, dmasks)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fi.draw_prims_u8(ctx, keep[0], prims, dmasks)
    torch.cuda.synchronize()
    t_draw = (time.perf_counter() - t) / iters

    def host_alternative():
        from PIL import ImageDraw
        for data, (gt, det) in zip(datas, per_frame):
            im = Image.open(io.BytesIO(data)).convert('RGB')
            draw = ImageDraw.Draw(im)
            for bs, color in ((gt, RED), (det, GREEN)):
                for b in bs:
                    draw.rectangle([b.xmin, b.ymin, b.xmax, b.ymax], outline=color, width=3)
                    draw.text((b.xmin, b.ymin - 20), label_text(b), fill=color, font=font)
    host_alternative()
    reps = max(1, iters // 5)
    t = time.perf_counter()
    for _ in range(reps):
        host_alternative()
    t_host = (time.perf_counter() - t) / reps
    tag = '%dx%d' % (W, H)
    return {tag + '_frames': frames, tag + '_prims': len(prims), tag + '_host_prims_ms': t_prims * 1e3,
            tag + '_draw_prims_u8_ms': t_draw * 1e3, tag + '_pillow_decode_and_draw_ms': t_host * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--boxes', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    ctx = Context(0)
    res = {'device': torch.cuda.get_device_name(0), 'boxes_per_frame': a.boxes}
    res.update(one_size(ctx, 1080, 1920, 8, a.boxes, a.iters))
    res.update(one_size(ctx, 3456, 5184, 3, a.boxes, a.iters))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
