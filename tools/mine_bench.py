"""Triplet mining on one GPU.  Synthetic unit-norm facial IDs, l2_normalize(relu(centre[subject] + 0.6 *
noise)), at two sizes: the db of section 19 (171 rows, 308 pairs) and a UCCS-sized one (2 000 subjects x 10 crops = 20 000 rows,
90 000 pairs).  Host clock around blocks that end in a synchronise, the best of three alternating blocks.  Prints one JSON line:

    1. fv_fid_mine_negatives with the pairs grouped by anchor (up to FV_MINE_PB positives share a scan) and with every pair a
       group of its own, on the same triplets, in both modes;
    2. the numpy oracle (tests/mine_negatives_ref.py) on a sample of the pairs, extrapolated to all of them;
    3. at 416 x 416: extraction of the db's IDs from a resident crop store (measured on --extract-crops crops, scaled by the
       crop count: crops are independent and the chunks alike) plus the operator, as a share of one epoch of training steps
       (fv_fid_train_step + Adam, B = 13, inputs gathered from the store; measured per step, times the epoch's step count).

    python tools/mine_bench.py [--iters N] [--steps N] [--extract-crops N] [--skip-model]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import face_identification as fi  # noqa: E402
import mine_negatives_ref as ref  # noqa: E402

S, B = 416, 13
# 40 subjects of 2..6 crops with section 19's totals: 171 rows, 308 pairs
SMALL = [2] * 3 + [3] * 7 + [4] * 14 + [5] * 8 + [6] * 8
LARGE = [10] * 2000


def make_ids(sizes, seed=0):
    rng = np.random.RandomState(seed)
    subjects = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    centres = rng.randn(len(sizes), 64)
    x = np.maximum(centres[subjects] + 0.6 * rng.randn(len(subjects), 64), 0.0)
    ids = (x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), 1e-12))).astype(np.float32)
    return ids, subjects, ref.same_subject_pairs(subjects)


def block(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def operator(ctx, sizes, iters, sample):
    ids, subjects, pairs = make_ids(sizes)
    assert (len(ids), len(pairs)) == (sum(sizes), sum(m * (m - 1) // 2 for m in sizes))
    x, sub = torch.from_numpy(ids).cuda(), torch.from_numpy(subjects).cuda()
    grouped = fi.triplet_groups(pairs)[:3]
    single = (np.asarray([a for a, _ in pairs], np.int32), np.arange(len(pairs) + 1, dtype=np.int32),
              np.asarray([p for _, p in pairs], np.int32))
    out = dict(rows=len(ids), pairs=len(pairs), groups=len(grouped[0]),
               scans_grouped=int(sum(-(-int(k) // fi.MINE_PB) for k in np.diff(grouped[1]))))
    for mode in ('semi_hard', 'hardest'):
        runs = dict(grouped=lambda: fi.fid_mine_negatives(ctx, x, sub, *grouped, mode=mode),
                    singleton=lambda: fi.fid_mine_negatives(ctx, x, sub, *single, mode=mode))
        a, b = runs['grouped'](), runs['singleton']()                  # warm-up, and the two must agree bit for bit
        assert all(torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v)
                   for u, v in zip(a, b))
        ms = {k: [] for k in runs}
        for _ in range(3):
            for k, fn in runs.items():
                ms[k].append(1e3 * block(fn, iters))
        out[mode] = {k + '_ms': [round(v, 3) for v in vs] for k, vs in ms.items()}
        out[mode]['singleton_over_grouped'] = round(min(ms['singleton']) / min(ms['grouped']), 2)
        out[mode]['kinds'] = np.bincount(a[1].cpu().numpy(), minlength=4).tolist()
    # the oracle on a sample of the pairs (whole anchors, so that its per-anchor distances are shared as they would be)
    take = pairs[:sample]
    t = time.perf_counter()
    want = ref.mine_negatives(ids, subjects, take, fi.TRIPLET_MARGIN, 0)
    dt = time.perf_counter() - t
    got = fi.fid_mine_negatives(ctx, x, sub, *fi.triplet_groups(take)[:3])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[3].cpu().numpy().view(np.int64), want[3].view(np.int64))
    out['oracle'] = dict(sample_pairs=len(take), sample_s=round(dt, 3), all_pairs_s=round(dt * len(pairs) / len(take), 2))
    return out


def model_share(out, iters, steps, extract_crops):
    """Mining (extraction + operator) against an epoch of training steps, in this process, alternating."""
    from face_vijnana_yolov3_amd.engine import Engine
    m = fi.FidModel(S)
    m.init_synthetic(seed=7)
    m.init_dense()
    m.ensure_optimizer()
    m._workspace(B, S, True)
    chunk = max(1, Engine.max_infer_batch(S))
    n_store = max(extract_crops, sum(SMALL))
    store = torch.randint(0, 256, (n_store, S, S, 3), dtype=torch.uint8, device=m.dev)
    rng = np.random.RandomState(0)
    idx = [rng.randint(0, n_store, 3 * B) for _ in range(steps)]

    def train_block():
        for k in range(steps):
            x = fi.gather_crops_f32(m.ctx, store, idx[k])
            m.train_on_batch(x[:B], x[B:2 * B], x[2 * B:], 1e-6, 0.99, 0.99, 0.0)

    def extract(n):
        return torch.cat([m.extract_device(fi.gather_crops_f32(m.ctx, store, range(i, min(i + chunk, n)))) for i in range(0, n, chunk)])
    params0, state0 = m.params.clone(), m.state.clone()
    train_block(); extract(sum(SMALL)); extract(extract_crops)         # warm-up: code objects, both workspaces
    step_ms, small_ms, many_ms = [], [], []
    for _ in range(3):
        step_ms.append(1e3 * block(train_block, 1) / steps)
        small_ms.append(1e3 * block(lambda: extract(sum(SMALL)), 1))
        many_ms.append(1e3 * block(lambda: extract(extract_crops), 1))
        m.params.copy_(params0); m.state.copy_(state0)
    res = dict(image_size=S, batch=B, infer_chunk=chunk, train_step_ms=[round(v, 2) for v in step_ms],
               extract_171_ms=[round(v, 2) for v in small_ms], extract_crops=extract_crops,
               extract_ms=[round(v, 1) for v in many_ms], extract_ms_per_crop=round(min(many_ms) / extract_crops, 3))
    for name, key, measured in (('small', 'small', min(small_ms)), ('large', 'large', None)):
        o = out[key]
        n_steps = fi.num_batches(o['pairs'], B)
        epoch_ms = min(step_ms) * n_steps
        extract_ms = measured if measured is not None else min(many_ms) / extract_crops * o['rows']
        op_ms = min(o['semi_hard']['grouped_ms'])
        res[name] = dict(epoch_steps=n_steps, epoch_ms=round(epoch_ms, 1), extract_ms=round(extract_ms, 1),
                         extract_extrapolated=measured is None, operator_ms=round(op_ms, 3),
                         mining_share_of_epoch=round((extract_ms + op_ms) / epoch_ms, 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='operator calls per block')
    ap.add_argument('--steps', type=int, default=8, help='training steps per block')
    ap.add_argument('--extract-crops', type=int, default=960)
    ap.add_argument('--skip-model', action='store_true', help='the operator and the oracle only')
    args = ap.parse_args()
    from face_vijnana_yolov3_amd._lib import Context
    ctx = Context(0)
    out = dict(pb=fi.MINE_PB, margin=fi.TRIPLET_MARGIN)
    out['small'] = operator(ctx, SMALL, args.iters, 308)
    out['large'] = operator(ctx, LARGE, max(2, args.iters // 5), 450)
    if not args.skip_model:
        out['model'] = model_share(out, args.iters, args.steps, args.extract_crops)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
