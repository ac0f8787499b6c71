"""Face-verification pair distances on one GPU: fv_fid_pair_dists over seeded synthetic subject databases shaped like UCCS (1 085
subjects, 1-15 faces each) and VGGFace2's training split (8 631 subjects, 364 faces each, ~1.1e9 pairs), counts only and
materialised, with 10 thresholds (cal_VAL_FAR's).  Device events bracket each call (the table upload included); the
materialised rows add the device-to-host copy of the distances, timed on its own.  The rate is set against the fp64 vector peak
(78.6 TFLOP/s spec, 3 * 64 ops per pair) and the materialised write against the measured HBM copy bandwidth (6.29 TB/s).  The
reference's per-pair loop (one scipy.linalg.norm per pair, evaluate.py:158, 187; its per-pair HDF5 reads left out) is timed on a
subsample and extrapolated -- an extrapolation, not a run.  Prints one JSON line.

    python tools/face_pairs_bench.py [--iters N] [--skip-vgg]
"""
import argparse
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

FP64_PEAK = 78.6e12
HBM_BW = 6.29e12
THS = np.arange(0.1, 1.1, 0.1).astype(np.float32)


def synthetic(n_subjects, sizes, seed):
    """Blocks as face_pairs() builds them (subjects contiguous; triangles, then S // 2 drawn rectangles) over random unit IDs."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows, off = [], 0
    for s in range(n_subjects):
        n = int(sizes[s])
        if n >= 2:
            rows.append((start[s], n, start[s], n, off, 0)); off += n * (n - 1) // 2
    n_same = off
    draw = rng.permutation(n_subjects)[:2 * (n_subjects // 2)].reshape(-1, 2)
    for k, l in draw:
        rows.append((start[k], sizes[k], start[l], sizes[l], off, 1)); off += int(sizes[k]) * int(sizes[l])
    ids = rng.normal(size=(int(start[-1]), 64)).astype(np.float32)
    ids /= np.linalg.norm(ids, axis=1, keepdims=True)
    return ids, np.asarray(rows, np.int64), n_same, off - n_same


def time_call(ctx, x, blocks, n_dists, iters):
    fi.fid_pair_dists(ctx, x, blocks, THS, n_dists=n_dists)              # warm-up (and the allocation)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, wall = [], []
    for _ in range(iters):
        t = time.perf_counter()
        e0.record()
        d, c = fi.fid_pair_dists(ctx, x, blocks, THS, n_dists=n_dists)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(e0.elapsed_time(e1))
        del d
    return float(np.median(ms)), float(np.median(wall)), c.cpu().numpy()


def d2h_ms(n):
    x = torch.empty(n, dtype=torch.float32, device='cuda')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h = x.cpu()
    e1.record()
    torch.cuda.synchronize()
    del h, x
    return e0.elapsed_time(e1)


def reference_loop_s_per_pair(ids, blocks, sample=20000, seed=0):
    from scipy.linalg import norm
    ra, rb = fi.expand_pair_blocks(blocks[:64])
    pick = np.random.default_rng(seed).integers(0, len(ra), min(sample, len(ra)))
    t = time.perf_counter()
    for p in pick:
        norm(ids[ra[p]] - ids[rb[p]])
    return (time.perf_counter() - t) / len(pick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-vgg', action='store_true')
    a = ap.parse_args()
    ctx = Context(0)
    rng = np.random.default_rng(1)
    cases = [('uccs_like', 1085, rng.integers(1, 16, 1085))]
    if not a.skip_vgg:
        cases.append(('vggface2_like', 8631, np.full(8631, 364)))
    out = {'thresholds': len(THS), 'fp64_peak_spec': FP64_PEAK, 'hbm_copy_bw_measured': HBM_BW}
    for name, S, sizes in cases:
        ids, blocks, n_same, n_diff = synthetic(S, sizes, 7)
        n = n_same + n_diff
        x = torch.from_numpy(ids).cuda()
        r = {'subjects': S, 'ids': len(ids), 'blocks': len(blocks), 'same_pairs': n_same, 'diff_pairs': n_diff}
        for mode, nd in (('counts_only', None), ('materialised', n)):
            ms, wall, c = time_call(ctx, x, blocks, nd, a.iters)
            assert int(c[0, -1]) + int(c[1, -1]) <= n
            flops = 3.0 * 64 * n
            rr = {'device_ms': round(ms, 3), 'call_wall_ms': round(wall, 3), 'pairs_per_s': n / (ms * 1e-3),
                  'fp64_op_per_s': flops / (ms * 1e-3), 'fp64_share_of_peak': flops / (ms * 1e-3) / FP64_PEAK}
            if nd is not None:
                rr['dists_bytes'] = 4 * n
                rr['write_share_of_hbm_bw'] = 4.0 * n / (ms * 1e-3) / HBM_BW
                rr['d2h_ms'] = round(d2h_ms(n), 3)
                rr['d2h_GB_per_s'] = 4.0 * n / (rr['d2h_ms'] * 1e-3) / 1e9
            r[mode] = rr
        del x
        torch.cuda.empty_cache()
        try:
            spp = reference_loop_s_per_pair(ids, blocks)
            r['reference_loop_extrapolated_s'] = spp * n
            r['reference_loop_s_per_pair'] = spp
        except ImportError:
            r['reference_loop_extrapolated_s'] = None
        out[name] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
