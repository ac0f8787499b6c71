"""Tiled inference (hps['tiles']) on one GPU at 416 x 416: the fv_tile_merge launch with device events at 1 frame x 29 views x 60
slots and at 48 frames x 29 views x 60 slots (the views of a 5184 x 3456 frame at the default tile size), against the NumPy
reference (tests/tile_merge_ref.py) on the same inputs -- the outputs must be equal -- and FaceDetector.test() frames/s on
synthetic 2592 x 1728 JPEGs with tiles off and on.  Warm-up first, then `--reps` repetitions; the median and the range over the
repetitions are reported.  Prints one JSON line.

    python tools/tiles_bench.py [--frames N] [--reps N] [--iters N]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import data, postproc  # noqa: E402
from face_vijnana_yolov3_amd._lib import Context  # noqa: E402

S, K = 416, 60
H, W = 1728, 2592


def spread(values):
    v = sorted(values)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def merge_inputs(frames, rng):
    """What fv_decode_nms leaves for the 29 views of `frames` 5184 x 3456 frames: 5 .. 60 boxes of 8 .. 80 network pixels per view."""
    grid = data.tile_grid(3456, 5184, data.tiles_conf(True))
    T = frames * len(grid)
    lo = rng.integers(0, S - 80, (T, K, 2))
    boxes = np.concatenate([lo, lo + rng.integers(8, 80, (T, K, 2))], axis=2).astype(np.int32)
    score = rng.uniform(0.5, 1.0, (T, K)).astype(np.float32)
    count = rng.integers(5, K + 1, T).astype(np.int32)
    tiles = np.array([(f,) + g for f in range(frames) for g in grid], np.int32)
    off = (np.arange(frames + 1) * len(grid)).astype(np.int32)
    return dict(boxes=boxes, score=score, count=count, tiles=tiles, frame_off=off), len(grid)


def merge_launch(ctx, frames, iters, reps):
    import tile_merge_ref as ref
    dev = torch.device('cuda', ctx.device)
    p, views = merge_inputs(frames, np.random.default_rng(frames))
    d = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    ws = postproc.tile_merge_workspace(frames, dev)
    out = postproc.tile_merge(ctx, d, d['tiles'], d['frame_off'], S, 'ios', 0.5, workspace=ws)
    t = time.perf_counter()
    want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, 'ios', 0.5)
    t_ref = time.perf_counter() - t
    equal = all(out[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ('corners', 'rows', 'nrows', 'src'))
    for _ in range(5):                                                    # warm-up
        postproc.tile_merge(ctx, d, d['tiles'], d['frame_off'], S, 'ios', 0.5, workspace=ws, out=out)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            postproc.tile_merge(ctx, d, d['tiles'], d['frame_off'], S, 'ios', 0.5, workspace=ws, out=out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return {'frames': frames, 'views_per_frame': views, 'candidates': int(p['count'].sum()), 'kept_rows': int(want['nrows'].sum()),
            'equals_numpy_reference': equal, 'launch_ms': spread(ms), 'numpy_reference_ms': t_ref * 1e3}


def test_pass(frames, reps):
    from PIL import Image
    from face_vijnana_yolov3_amd import face_detection
    face_detection.DEBUG = False
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        rng = np.random.default_rng(1)
        os.makedirs('frames')
        for k in range(frames):
            base = rng.integers(0, 256, (H // 16, W // 16, 3)).astype(np.uint8)
            Image.fromarray(np.kron(base, np.ones((16, 16, 1), np.uint8))).save('frames/f%03d.jpg' % k, quality=90)
        res = {}
        for name, tiles in (('off', None), ('on', True)):
            hps = {'face_conf_th': 0.5, 'nms_iou_th': 0.5, 'num_cands': K, 'eval_batch_size': 48}
            if tiles is not None:
                hps['tiles'] = tiles
            conf = {'mode': 'test', 'raw_data_path': tmp, 'test_path': os.path.join(tmp, 'frames'),
                    'output_file_path': os.path.join(tmp, 'solution_%s.csv' % name), 'multi_gpu': False, 'num_gpus': 1,
                    'yolov3_base_model_load': False, 'model_loading': False, 'hps': hps, 'nn_arch': {'image_size': S, 'bb_info_c_size': 6}}
            fd = face_detection.FaceDetector(conf)
            d = fd.model.layers[-1]                                        # a head that fires on some cells
            y0 = fd.model.predict(np.random.default_rng(0).uniform(0, 1, (1, S, S, 3)).astype(np.float32))
            fd.model.params[d['w_off']:d['beta_off']] /= float(y0.std())
            fd.model.params[d['beta_off']] = 1.0; fd.model.params[d['beta_off'] + 5] = 1.0
            fd.test()                                                      # warm-up: workspaces, pinned buffers, code objects
            fps = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fd.test()
                torch.cuda.synchronize()
                fps.append(frames / (time.perf_counter() - t))
            views = len(data.tile_grid(H, W, fd.tiles)) if fd.tiles is not None else 1
            res['test_tiles_%s' % name] = {'frames': frames, 'views_per_frame': views, 'rows': open(conf['output_file_path']).read().count('\n'),
                                           'frames_per_s': spread(fps), 'views_per_s_median': spread(fps)['median'] * views}
            del fd
        return res
    finally:
        os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=48)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    ctx = Context(0)
    res = {'device': torch.cuda.get_device_name(0), 'image_size': S, 'num_cands': K, 'frame': '%dx%d' % (W, H)}
    for frames in (1, 48):
        res['merge_%d' % frames] = merge_launch(ctx, frames, a.iters, a.reps)
    res.update(test_pass(a.frames, a.reps))

    def rnd(v):
        return {k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else round(v, 4) if isinstance(v, float) else v
    print(json.dumps(rnd(res)))


if __name__ == '__main__':
    main()
