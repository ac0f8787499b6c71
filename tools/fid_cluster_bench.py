"""fv_fid_cluster (DBSCAN over facial IDs) on one GPU: the call between two device events at n = 1 000,
10 000 and 65 536 rows of the mixed-spread generator of tests/fid_cluster_ref.py (30 centres, a spread per row from U[0.2, 1.6],
rows normalised) at eps 0.9, min_pts 4.  5 warm-up calls, then `--reps` repetitions of `--iters` calls; the median and the range
over the repetitions.  The share of each of the four passes comes from fv_profile_collect over further calls.  For n <= 10 000
the host side is timed once for comparison: scikit-learn's DBSCAN(algorithm='brute') on float64 copies of the rows where
scikit-learn imports, the NumPy reference otherwise.  At n = 1 000 the outputs must equal the NumPy reference's.  Prints one JSON
line and writes it to profiles/fid_cluster_bench.json.

    python tools/fid_cluster_bench.py [--reps N] [--iters N] [--out FILE]
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
from face_vijnana_yolov3_amd._lib import Context, lib  # noqa: E402
import fid_cluster_ref as ref  # noqa: E402

EPS, MIN_PTS = 0.9, 4
SIZES = (1000, 10000, 65536)
PASSES = {'neighbours': ('fidc_neighbours_kernel', 'fidc_count_kernel'), 'components': ('fidc_unite_kernel', 'fidc_flatten_kernel'),
          'borders': ('fidc_border_kernel',), 'relabel': ('fidc_scan_kernel', 'fidc_label_kernel')}


def spread(values):
    v = sorted(values)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def host_side(ids):
    """(what ran, seconds): the comparison, never the code under test."""
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        t = time.perf_counter()
        ref.cluster(ids, EPS, MIN_PTS)
        return 'numpy reference', time.perf_counter() - t
    x = ids.astype(np.float64)
    t = time.perf_counter()
    DBSCAN(eps=EPS, min_samples=MIN_PTS, algorithm='brute').fit(x)
    return 'sklearn DBSCAN(brute)', time.perf_counter() - t


def measure(ctx, n, iters, reps):
    ids = ref.mixed(n, n)
    x = torch.from_numpy(ids).cuda()
    ws = torch.empty(int(lib().fv_fid_cluster_workspace_bytes(n)), dtype=torch.uint8, device=x.device)
    out = fi.fid_cluster(ctx, x, EPS, MIN_PTS, workspace=ws)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    core = host['core'].astype(bool)
    res = {'n': n, 'workspace_mib': ws.numel() / 2.0 ** 20, 'clusters': int(host['n_clusters'][0]), 'core_rows': int(core.sum()),
           'border_rows': int((~core & (host['labels'] >= 0)).sum()), 'noise_rows': int((host['labels'] < 0).sum()),
           'mean_neighbours': float(host['n_nbr'].mean())}
    if n == SIZES[0]:
        want = ref.cluster(ids, EPS, MIN_PTS)
        res['equals_numpy_reference'] = all(host[k].tobytes() == want[k].tobytes() for k in want)
        assert res['equals_numpy_reference'], 'fv_fid_cluster differs from the NumPy reference at n = %d' % n
    for _ in range(5):                                                    # warm-up
        fi.fid_cluster(ctx, x, EPS, MIN_PTS, workspace=ws)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fi.fid_cluster(ctx, x, EPS, MIN_PTS, workspace=ws)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    res['call_ms'] = spread(ms)
    ctx.profile(True)
    try:
        for _ in range(iters):
            fi.fid_cluster(ctx, x, EPS, MIN_PTS, workspace=ws)
        recs = ctx.profile_collect()
    finally:
        ctx.profile(False)
    per_pass = {name: sum(recs[k]['ms'] for k in kernels if k in recs) / iters for name, kernels in PASSES.items()}
    total = sum(per_pass.values())
    res['pass_ms'] = per_pass
    res['pass_share'] = {name: v / total for name, v in per_pass.items()}
    res['neighbours_fp64_tflops'] = 1.5 * n * n * 64 / (recs['fidc_neighbours_kernel']['ms'] / iters * 1e-3) / 1e12
    if n <= 10000:
        what, seconds = host_side(ids)
        res['host_side'] = what
        res['host_side_ms'] = seconds * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fid_cluster_bench.json'))
    a = ap.parse_args()
    ctx = Context(0)
    res = {'device': torch.cuda.get_device_name(0), 'eps': EPS, 'min_pts': MIN_PTS, 'iters': a.iters, 'reps': a.reps}
    for n in SIZES:
        res['n_%d' % n] = measure(ctx, n, a.iters, a.reps)

    def rnd(v):
        return {k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else round(v, 4) if isinstance(v, float) else v
    line = json.dumps(rnd(res))
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
