"""hps['mosaic'] on one GPU at the training shape, S = 416, B = 40.  Two measurements, one JSON line:

  launch   one batch over 40 synthetic 1080p-class images already on the device, alternating blocks in this process of
             augment    fv_letterbox_augment_batch with data.draw_augment's parameters (defaults): the launch of a batch without mosaic
             prob0      fv_letterbox_mosaic_batch with data.draw_mosaic's tables at prob 0: one full-window tile per canvas, the
                        same bits as `augment` (compared here)
             default    fv_letterbox_mosaic_batch at the defaults (prob 0.5): what `"mosaic": true` launches
             prob1      fv_letterbox_mosaic_batch at prob 1 (defaults otherwise): four tiles per canvas, 160 tiles, four launches
           per variant: median ms per batch over the rounds (HIP events around a block of calls), the host's median ms per call
           to enqueue it, the bytes the algorithm moves (every tile's source crop read once + 12 S^2 written per canvas) and
           TB/s = bytes / time
  step     run_pipelined (the real input path: JPEG files, host Huffman decode, device reconstruction, staging stream) with
           augment alone ("off") and augment + mosaic ("on", defaults), alternating, ms per step between two events on the
           compute stream, and the loader thread's wall time per batch inside BatchFeeder.load (decode, draws, target encoding)

    python tools/mosaic_bench.py [--rounds R] [--block N] [--steps K] [--alternations A] [--skip-step]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import data  # noqa: E402
from face_vijnana_yolov3_amd._lib import lib, ptr  # noqa: E402

from augment_bench import B, HPS, S, SIZES_1080P, make_jpegs  # noqa: E402  (the same shapes and the same JPEG folder)


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
    place, colour = np.asarray([d[0] for d in drawn], np.int32), np.asarray([d[1] for d in drawn], np.float32)
    tables = {nm: data.draw_mosaic(data.mosaic_conf({'prob': p}), aug, 0, range(B), shapes, S) for nm, p in (('prob0', 0), ('default', 0.5), ('prob1', 1))}
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)

    def run(name):
        if name == 'augment':
            rc = lib().fv_letterbox_augment_batch(ctx.handle, ptr(dbuf), c_offs, c_hw, B, S, place.ctypes.data_as(i32p),
                                                  colour.ctypes.data_as(f32p), ptr(out))
        else:
            tiles, col = tables[name]
            rc = lib().fv_letterbox_mosaic_batch(ctx.handle, ptr(dbuf), c_offs, c_hw, B, S, B, tiles.ctypes.data_as(i32p),
                                                 col.ctypes.data_as(f32p), len(tiles), ptr(out))
        ctx.check(rc, name)

    def moved(name):
        src = sum(int(p[2]) * int(p[3]) * 3 for p in place) if name == 'augment' else sum(int(t[4]) * int(t[5]) * 3 for t in tables[name][0])
        return src + 12 * S * S * B

    names = ['augment', 'prob0', 'default', 'prob1']
    run('augment'); first = out.clone(); run('prob0'); same = bool(torch.equal(out.view(torch.int32), first.view(torch.int32)))
    for nm in names:                                                  # warm-up of every variant
        for _ in range(5):
            run(nm)
    torch.cuda.synchronize()
    ms, host = {nm: [] for nm in names}, {nm: [] for nm in names}
    for _ in range(rounds):
        for nm in names:                                              # alternating blocks
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(block):
                run(nm)
            host[nm].append(1e3 * (time.perf_counter() - t0) / block)
            e1.record(); e1.synchronize()
            ms[nm].append(e0.elapsed_time(e1) / block)
    res = {'prob0_equals_augment_bitwise': same, 'images': B, 'image_size': S, 'rounds': rounds, 'calls_per_block': block,
           'tiles': {nm: int(len(tables[nm][0])) for nm in tables}}
    for nm in names:
        med = float(np.median(ms[nm]))
        res[nm] = dict(ms_median=round(med, 4), ms_min=round(min(ms[nm]), 4), ms_max=round(max(ms[nm]), 4),
                       host_enqueue_ms_median=round(float(np.median(host[nm])), 4), bytes=moved(nm),
                       tb_per_s=round(moved(nm) / (med * 1e-3) / 1e12, 3))
    return res


def step_bench(eng, steps, alternations):
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, run_pipelined
    from face_vijnana_yolov3_amd.parallel import DataParallelTrainer
    trainer = DataParallelTrainer(eng, world_size=1, rank=0)
    threads = min(16, max(2, (os.cpu_count() or 8) // 2))
    series, loads = {'off': [], 'on': []}, {'off': [], 'on': []}
    with tempfile.TemporaryDirectory() as root:
        make_jpegs(root, 2 * B)
        feeders = {}
        for nm, hps in (('off', dict(HPS, augment=True)), ('on', dict(HPS, augment=True, mosaic=True))):
            f = feeders[nm] = BatchFeeder(data.TrainingSequence(root, hps, {'image_size': S, 'bb_info_c_size': 6}), 1, 0, threads)
            f.load_s = []

            def timed(index, f=f, load=f.load):                        # the loader thread's wall time per batch
                t0 = time.perf_counter()
                item = load(index)
                f.load_s.append(time.perf_counter() - t0)
                return item
            f.load = timed

        def one(nm, epoch):
            f = feeders[nm]
            f.set_epoch(epoch)
            f.load_s.clear()
            n = 4 + steps
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def after_step(k, loss, item):
                if k == 2:
                    ev0.record()
            torch.cuda.synchronize()
            run_pipelined(eng, trainer, f, [k % len(f.seq) for k in range(n)], S, f.seq.hps, after_step)
            ev1.record(); torch.cuda.synchronize()
            return ev0.elapsed_time(ev1) / steps, 1e3 * float(np.median(f.load_s))

        one('off', 0); one('on', 0)                                   # warm-up of both: file cache, pinned buffers, code objects
        for a in range(alternations):
            for nm in ('off', 'on'):
                step_ms, load_ms = one(nm, a + 1)
                series[nm].append(round(step_ms, 3)); loads[nm].append(round(load_ms, 3))
        for f in feeders.values():
            f.close()
    trainer.shutdown()
    return dict(ms_per_step_off=series['off'], ms_per_step_on=series['on'], loader_ms_per_batch_off=loads['off'],
                loader_ms_per_batch_on=loads['on'], steps=steps, batch=B, image_size=S, loader_threads=threads,
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
        raise SystemExit('mosaic_bench needs the GPU: there is nothing to measure on a CPU')
    from face_vijnana_yolov3_amd.engine import Engine
    eng = Engine(0)
    res = {'launch': launch_bench(eng.ctx, eng.dev, a.rounds, a.block)}
    if not a.skip_step:
        res['step'] = step_bench(eng, a.steps, a.alternations)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
