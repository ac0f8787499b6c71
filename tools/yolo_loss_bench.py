"""hps['loss'] = 'yolo'  on one GPU at the three-scale training shape, S = 416, B = 16.  Two measurements, one JSON line:

  stage    the loss stage alone on device-resident head outputs and targets (1 - 5 faces per image through
           data.encode_gt_three_scale), alternating blocks in this process of
             fd     fv_yolo_loss_grad (today's stage: the fd_loss generalisation, three part launches + finish)
             l2     fv_yolo_det_loss_grad, box_loss 'l2'    (gather + loss + finish)
             giou   fv_yolo_det_loss_grad, box_loss 'giou'
           for 1 class (18 channels, c_pad 32) and 80 classes (255 channels, c_pad 256): median ms per call (HIP events
           around a block of calls), the bytes the stage streams (y and t read, dy written) and TB/s = bytes / time
  step     Yolov3.train_on_batch (fv_yolov3_train_step / fv_yolov3_train_step_det + Adam) at 18 channels with the loss off and
           on, alternating blocks, ms per step between two events

    python tools/yolo_loss_bench.py [--rounds R] [--block N] [--steps K] [--alternations A] [--skip-step] [--skip-stage]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import data  # noqa: E402
from face_vijnana_yolov3_amd._lib import c_void_p, lib, ptr  # noqa: E402

S, B = 416, 16


def make_targets(ncls, seed=0):
    rng = np.random.default_rng(seed)
    per = []
    for _ in range(B):
        h, w = 768, 1024
        faces = []
        for _ in range(int(rng.integers(1, 6))):
            fw, fh = float(rng.uniform(20, w / 3)), float(rng.uniform(20, h / 3))
            faces.append([float(rng.uniform(1, w - fw - 1)), float(rng.uniform(1, h - fh - 1)), fw, fh])
        per.append(data.encode_gt_three_scale(faces, h, w, S, nclass=ncls))
    return [torch.from_numpy(np.stack([p[s] for p in per]).astype(np.float32)) for s in range(3)]


def stage_bench(ctx, dev, ncls, rounds, block):
    from face_vijnana_yolov3_amd import ops
    E3 = 3 * (5 + ncls)
    cpad = (E3 + 31) // 32 * 32
    ts = [t.to(dev).reshape(-1, E3) for t in make_targets(ncls)]
    g = torch.Generator().manual_seed(1)
    ys = [torch.randn(t.shape, generator=g).to(dev) for t in ts]
    dys = [torch.empty((t.shape[0], cpad), dtype=torch.float32, device=dev) for t in ts]
    cells = (ctypes.c_int64 * 3)(*[int(t.shape[0]) for t in ts])
    part = torch.empty(max(1, lib().fv_yolo_loss_partial_doubles(cells, 3)), dtype=torch.float64, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    stats = torch.zeros(12, dtype=torch.float64, device=dev)
    arr = lambda v: (c_void_p * 3)(*[t.data_ptr() for t in v])
    ya, ta, da = arr(ys), arr(ts), arr(dys)
    confs = {nm: data.det_loss_conf({'yolo': {'box_loss': nm}}) for nm in ('l2', 'giou')}
    structs = {nm: ops.yolo_det_conf(c) for nm, c in confs.items()}
    scratch = ops.yolo_det_scratch(B, S, 256, dev)

    def run(nm):
        if nm == 'fd':
            rc = lib().fv_yolo_loss_grad(ctx.handle, ya, ta, cells, ncls, 3, cpad, 1.0, ptr(part), ptr(loss), da)
        else:
            rc = lib().fv_yolo_det_loss_grad(ctx.handle, ya, ta, B, S, ncls, cpad, ctypes.byref(structs[nm]), 1.0, ptr(scratch),
                                             scratch.numel() * 8, ptr(loss), da, ptr(stats))
        ctx.check(rc, nm)

    names = ['fd', 'l2', 'giou']
    for nm in names:
        for _ in range(5):
            run(nm)
    torch.cuda.synchronize()
    seen = [float(v) for v in stats.cpu()]
    ms = {nm: [] for nm in names}
    for _ in range(rounds):
        for nm in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                run(nm)
            e1.record(); e1.synchronize()
            ms[nm].append(e0.elapsed_time(e1) / block)
    moved = sum(4 * t.shape[0] * (2 * E3 + cpad) for t in ts)
    res = dict(classes=ncls, c_pad=cpad, bytes=moved, positives=seen[4], ignored=seen[5], max_boxes_per_image=seen[9])
    for nm in names:
        med = float(np.median(ms[nm]))
        res[nm] = dict(ms_median=round(med, 4), ms_min=round(min(ms[nm]), 4), ms_max=round(max(ms[nm]), 4),
                       tb_per_s=round(moved / (med * 1e-3) / 1e12, 3))
    return res


def step_bench(steps, alternations):
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    m = Yolov3(0, out_channels=18)
    m.init_synthetic(seed=7)
    ts = [t.to(m.dev) for t in make_targets(1)]
    x = torch.rand((B, S, S, 3), generator=torch.Generator().manual_seed(2)).to(m.dev)
    modes = [('off', None), ('on', data.det_loss_conf('yolo'))]
    series = {nm: [] for nm, _ in modes}

    def one(conf, n):
        m.det_loss = conf
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.train_on_batch(x, ts, 1e-5, 0.9, 0.999)
        e0.record()
        for _ in range(n):
            m.train_on_batch(x, ts, 1e-5, 0.9, 0.999)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n

    for _, conf in modes:
        one(conf, 3)
    for _ in range(alternations):
        for nm, conf in modes:
            series[nm].append(round(one(conf, steps), 3))
    res = dict(steps=steps, batch=B, image_size=S, out_channels=18)
    for nm in series:
        res['ms_per_step_' + nm] = series[nm]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--block', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--alternations', type=int, default=4)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-stage', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('yolo_loss_bench needs the GPU: there is nothing to measure on a CPU')
    res = {}
    if not a.skip_stage:
        from face_vijnana_yolov3_amd._lib import Context
        ctx = Context(0)
        res['stage'] = [stage_bench(ctx, torch.device('cuda', 0), ncls, a.rounds, a.block) for ncls in (1, 80)]
    if not a.skip_step:
        res['step'] = step_bench(a.steps, a.alternations)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
