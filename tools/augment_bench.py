"""hps['augment'] on one GPU at the training shape, S = 416, B = 40.  Two measurements, one JSON line:

  launch   one launch over 40 synthetic 1080p-class images already on the device, alternating blocks in this process of
             plain      fv_letterbox_batch (the reference's fixed letterbox)
             identity   fv_letterbox_augment_batch with the identity placement and colour (0, 1, 1): the same pixels as plain
             augment    fv_letterbox_augment_batch with data.draw_augment's parameters (defaults): crop / shrink, flip, colour
           per variant: median ms per launch over the rounds (HIP events around a block of launches), the bytes the algorithm
           moves (source crop bytes read once + 12 S^2 written per image) and TB/s = bytes / time
  step     run_pipelined (the real input path: JPEG files, host Huffman decode, device reconstruction, staging stream) with
           augmentation off and on, alternating, ms per step between two events on the compute stream as bench.py's `loader`
           figure takes it

    python tools/augment_bench.py [--rounds R] [--block N] [--steps K] [--alternations A] [--skip-step]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import data  # noqa: E402
from face_vijnana_yolov3_amd._lib import lib, ptr  # noqa: E402

S, B = 416, 40
HPS = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=B)
SIZES_1080P = [(1080, 1920), (1080, 1920), (1920, 1080), (1080, 1440)]


def launch_bench(ctx, dev, rounds, block):
    rng = np.random.default_rng(0)
    shapes = [SIZES_1080P[k % len(SIZES_1080P)] for k in range(B)]
    offs, hw, o = [], [], 0
    for h, w in shapes:
        offs.append(o); hw += [h, w]; o += h * w * 3
    dbuf = torch.from_numpy(rng.integers(0, 256, o, dtype=np.uint8)).to(dev)
    out = torch.empty((B, S, S, 3), dtype=torch.float32, device=dev)
    c_offs, c_hw = (ctypes.c_int64 * B)(*offs), (ctypes.c_int32 * (2 * B))(*hw)
    aug = data.augment_conf(True)
    drawn = [data.draw_augment(aug, 0, i, h, w, S) for i, (h, w) in enumerate(shapes)]
    tables = {
        'identity': (np.asarray([data.identity_placement(h, w, S) for h, w in shapes], np.int32), np.tile(np.float32([0, 1, 1]), (B, 1))),
        'augment': (np.asarray([d[0] for d in drawn], np.int32), np.asarray([d[1] for d in drawn], np.float32)),
    }
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)

    def run(name):
        if name == 'plain':
            rc = lib().fv_letterbox_batch(ctx.handle, ptr(dbuf), c_offs, c_hw, B, S, ptr(out), None)
        else:
            place, colour = tables[name]
            rc = lib().fv_letterbox_augment_batch(ctx.handle, ptr(dbuf), c_offs, c_hw, B, S, place.ctypes.data_as(i32p),
                                                  colour.ctypes.data_as(f32p), ptr(out))
        ctx.check(rc, name)

    def moved(name):
        src = sum(h * w * 3 for h, w in shapes) if name != 'augment' else sum(int(p[2]) * int(p[3]) * 3 for p in tables['augment'][0])
        return src + 12 * S * S * B

    names = ['plain', 'identity', 'augment']
    run('plain'); plain = out.clone(); run('identity'); same = bool(torch.equal(out.view(torch.int32), plain.view(torch.int32)))
    for nm in names:                                                  # warm-up of every variant
        for _ in range(5):
            run(nm)
    torch.cuda.synchronize()
    ms = {nm: [] for nm in names}
    for _ in range(rounds):
        for nm in names:                                              # alternating blocks
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                run(nm)
            e1.record(); e1.synchronize()
            ms[nm].append(e0.elapsed_time(e1) / block)
    res = {'identity_equals_plain_bitwise': same, 'images': B, 'image_size': S, 'rounds': rounds, 'launches_per_block': block}
    for nm in names:
        med = float(np.median(ms[nm]))
        res[nm] = dict(ms_median=round(med, 4), ms_min=round(min(ms[nm]), 4), ms_max=round(max(ms[nm]), 4), bytes=moved(nm),
                       tb_per_s=round(moved(nm) / (med * 1e-3) / 1e12, 3))
    return res


def make_jpegs(root, n_img):
    """bench.py's loader folder: photo-like JPEGs (768 x 1024 .. 720 x 1280) with 1-5 faces each"""
    import pandas as pd
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = [(768, 1024), (1024, 768), (720, 1280), (600, 800)]
    rows, fid = [], 0
    for k in range(n_img):
        h, w = sizes[k % len(sizes)]
        lo = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        name = 'img_%04d.jpg' % k
        Image.fromarray(lo).resize((w, h), Image.BICUBIC).save(os.path.join(root, name), quality=90)
        for _ in range(int(rng.integers(1, 6))):
            fw = float(rng.uniform(20, w / 4)); fh = float(rng.uniform(20, h / 4))
            rows.append([fid, name, 1, round(float(rng.uniform(1, w - fw - 1)), 1), round(float(rng.uniform(1, h - fh - 1)), 1), round(fw, 1), round(fh, 1)])
            fid += 1
    pd.DataFrame(rows, columns=data.CSV_COLUMNS).to_csv(os.path.join(root, 'training.csv'), index=False)


def step_bench(eng, steps, alternations):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, run_pipelined
    from face_vijnana_yolov3_amd.parallel import DataParallelTrainer
    trainer = DataParallelTrainer(eng, world_size=1, rank=0)
    threads = min(16, max(2, (os.cpu_count() or 8) // 2))
    series = {'off': [], 'on': []}
    with tempfile.TemporaryDirectory() as root:
        make_jpegs(root, 2 * B)
        feeders = {}
        for nm, hps in (('off', dict(HPS)), ('on', dict(HPS, augment=True))):
            feeders[nm] = BatchFeeder(data.TrainingSequence(root, hps, {'image_size': S, 'bb_info_c_size': 6}), 1, 0, threads)

        def one(nm, epoch):
            f = feeders[nm]
            f.set_epoch(epoch)
            n = 4 + steps
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def after_step(k, loss, item):
                if k == 2:
                    ev0.record()
            torch.cuda.synchronize()
            run_pipelined(eng, trainer, f, [k % len(f.seq) for k in range(n)], S, f.seq.hps, after_step)
            ev1.record(); torch.cuda.synchronize()
            return ev0.elapsed_time(ev1) / steps

        one('off', 0); one('on', 0)                                   # warm-up of both: file cache, pinned buffers, code objects
        for a in range(alternations):
            for nm in ('off', 'on'):
                series[nm].append(round(one(nm, a + 1), 3))
        for f in feeders.values():
            f.close()
    trainer.shutdown()
    return dict(ms_per_step_off=series['off'], ms_per_step_on=series['on'], steps=steps, batch=B, image_size=S, loader_threads=threads,
                on_within_spread_of_off=bool(min(series['off']) <= float(np.median(series['on'])) <= max(series['off'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--block', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs the GPU: there is nothing to measure on a CPU')
    from face_vijnana_yolov3_amd.engine import Engine
    eng = Engine(0)
    res = {'launch': launch_bench(eng.ctx, eng.dev, a.rounds, a.block)}
    if not a.skip_step:
        res['step'] = step_bench(eng, a.steps, a.alternations)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
