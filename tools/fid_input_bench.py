"""FaceIdentifier.train()'s input path on one GPU at 416 x 416, B = 13, on a seeded synthetic db of JPEG crops made with Pillow
(subjects of 2-6 crops).  Alternating in this process, blocks of whole training steps (inputs + fv_fid_train_step + fv_adam_step):

    (a) resident   the three input tensors already on the device (what tools/fid_bench.py times)
    (b) sequence   the sequence's own path: tr_gen.load(rows) -- 3 B Pillow decodes, float conversion on the host, pageable copy
    (c) store      crop_store.TripletInputs, resident tier: one fv_gather_u8_f32 per step
    (d) per_batch  crop_store.TripletInputs, per-batch tier (crop_store_mb 0): the next batch decodes while this one trains

and, as facts: the one-off load of the resident store (crops/s), fv_gather_u8_f32 alone at n = 39 and n = 120 against a torch
device copy of the same byte count, and FaceIdentifier._extract_db over the db with and without the store.  Prints one JSON line.

    python tools/fid_input_bench.py [--steps N] [--rounds R] [--subjects M]
"""
import argparse
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

from face_vijnana_yolov3_amd import crop_store as cs  # noqa: E402
from face_vijnana_yolov3_amd import face_identification as fi  # noqa: E402

S, B = 416, 13
HPS = dict(lr=1e-6, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=B)


def make_db(root, subjects, seed=0):
    """subjects x (2..6) crops: a smooth face-sized pattern per subject plus noise per crop, saved as Pillow saves a crop."""
    import pandas as pd
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'subject_faces'))
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    rows = []
    for sid in range(subjects):
        f = rng.uniform(0.01, 0.05, 6)
        base = np.stack([127 + 100 * np.sin(f[0] * x + f[1] * y), 127 + 100 * np.cos(f[2] * x - f[3] * y),
                         127 + 100 * np.sin(f[4] * x) * np.cos(f[5] * y)], -1)
        for j in range(rng.randint(2, 7)):
            img = np.clip(base + rng.randint(-20, 21, (S, S, 3)), 0, 255).astype(np.uint8)
            name = 's%03d_%d.jpg' % (sid, j)
            Image.fromarray(img).save(os.path.join(root, 'subject_faces', name))
            rows.append(dict(subject_id=sid, face_file=name))
    pd.DataFrame(rows).to_csv(os.path.join(root, 'subject_image_db.csv'))
    return len(rows)


def block(m, feed, steps):
    """seconds per step of `steps` steps whose inputs come from the iterator `feed`, the device drained at the end"""
    h = HPS
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _, xs in zip(range(steps), feed):
        m.train_on_batch(*xs, h['lr'], h['beta_1'], h['beta_2'], h['decay'])
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8, help='training steps per block')
    ap.add_argument('--rounds', type=int, default=3, help='alternating rounds of the four blocks')
    ap.add_argument('--subjects', type=int, default=40)
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix='fid_input_bench_')
    os.chdir(root)
    n_crops = make_db(root, args.subjects)
    conf = {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=root, multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64),
                            hps=dict(HPS)), 'fd_conf': {}}
    ident = fi.FaceIdentifier(conf)
    m = ident.model
    np.random.seed(0)
    import random
    random.seed(0)
    tr_gen = fi.TrainingSequence(root, dict(HPS), ident.nn_arch, load_flag=False)
    batches = [tr_gen.rows(k) for k in range(len(tr_gen)) if len(tr_gen.rows(k)) == B]
    batches = (batches * (args.steps // max(1, len(batches)) + 1))[:args.steps]
    out = dict(image_size=S, batch=B, crops=n_crops, triplets=len(tr_gen.img_triplet_pairs), steps_per_block=args.steps,
               distinct_crops_per_batch=round(float(np.mean([len(cs.batch_slots(r)[0]) for r in batches])), 1))

    # the stores (the training workspace first, as train() does)
    m.ensure_optimizer()
    m._workspace(B, S, True)
    from concurrent.futures import ThreadPoolExecutor
    labels = list(tr_gen.db.index)
    paths = [tr_gen.path(label) for label in labels]
    with ThreadPoolExecutor(max_workers=ident._loader_threads()) as pool:
        store = cs.CropStore(m.ctx, n_crops, S, m.dev)
        loads = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            store.load(paths, list(range(n_crops)), pool)
            torch.cuda.synchronize()
            loads.append(n_crops / (time.perf_counter() - t))
        out['store_load_crops_per_s'] = [round(v, 1) for v in loads]          # the first pass also page-locks the ring's buffers
        out['loader_threads'] = ident._loader_threads()

        # fv_gather_u8_f32 alone against a device copy of the same bytes (1 read + 4 written per element)
        elems = S * S * 3
        for n in (39, 120):
            idx = np.random.RandomState(n).randint(0, n_crops, n)
            dst = torch.empty((n, S, S, 3), dtype=torch.float32, device=m.dev)
            a = torch.empty(5 * elems * n // 8, dtype=torch.float32, device=m.dev)      # copy: 2.5 bytes/element read, 2.5 written
            b = torch.empty_like(a)
            res = {}
            for r in range(3):
                res.setdefault('gather', []).append(timed(lambda: store.gather(idx, out=dst), 200, 20))
                res.setdefault('copy', []).append(timed(lambda: b.copy_(a), 200, 20))
            nbytes = 5.0 * elems * n
            out['gather_n%d' % n] = dict(us=[round(1e6 * v, 1) for v in res['gather']], tb_s=round(nbytes / min(res['gather']) / 1e12, 3),
                                         copy_us=[round(1e6 * v, 1) for v in res['copy']],
                                         copy_tb_s=round(nbytes / min(res['copy']) / 1e12, 3))
            del a, b, dst
    del store

    # the four input paths, alternating
    ident.hps = dict(HPS)
    resident = ident._triplet_inputs(tr_gen)
    ident.hps = dict(HPS, crop_store_mb=0)
    per_batch = ident._triplet_inputs(tr_gen)
    assert (resident.tier, per_batch.tier) == (cs.RESIDENT, cs.PER_BATCH)
    fixed = next(resident.batches(batches[:1]))
    params0, state0 = m.params.clone(), m.state.clone()

    def sequence_feed():
        for rows in batches:
            x, _ = tr_gen.load(rows)
            yield x['input_a'], x['input_p'], x['input_n']
    feeds = dict(resident=lambda: (fixed for _ in batches), sequence=sequence_feed, store=lambda: resident.batches(batches),
                 per_batch=lambda: per_batch.batches(batches))
    ms = {k: [] for k in feeds}
    block(m, feeds['resident'](), 2)                                      # warm-up: code objects, workspaces
    for _ in range(args.rounds):
        for name, feed in feeds.items():
            ms[name].append(1e3 * block(m, feed(), len(batches)))
            m.params.copy_(params0); m.state.copy_(state0)
    for name, v in ms.items():
        out['step_ms_' + name] = [round(x, 2) for x in v]
        out['triplets_per_s_' + name] = round(B / (min(v) / 1e3), 1)
    resident.close(); per_batch.close()

    # the facial-ID database over the same db
    db = {}
    for _ in range(2):
        for name, hps in (('store', {}), ('per_chunk', dict(crop_store_mb=0)), ('host', dict(crop_store=False))):
            ident.hps = dict(HPS, **hps)
            torch.cuda.synchronize()
            t = time.perf_counter()
            ident._extract_db()
            db.setdefault(name, []).append(time.perf_counter() - t)
    out['extract_db_s'] = {k: [round(x, 3) for x in v] for k, v in db.items()}
    out['extract_db_crops_per_s'] = {k: round(n_crops / min(v), 1) for k, v in db.items()}
    print(json.dumps(out))
    import shutil
    shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
