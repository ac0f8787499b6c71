"""FaceIdentifier throughput on one GPU at 416 x 416: facial-ID extraction (fv_fid_extract) at batch 1 and 48, triplet training
steps (fv_fid_train_step + fv_adam_step) at B = 1 and 13, and the per-launch time of the four dense-head kernels of a B = 13 step
against their byte floors at the measured device-to-device copy bandwidth; then, alternating in this process, the plain B = 13
step and the same step through parallel.DataParallelTrainer with the bucket path forced over a world-size-1 `nccl` group (RCCL
launches no kernel at one rank: what the callbacks and the stream traffic cost).  Prints one JSON line.

    python tools/fid_bench.py [--iters N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from face_vijnana_yolov3_amd.face_identification import FidModel  # noqa: E402

S = 416
DENSE_KERNELS = ('fid_dense_fwd_kernel', 'fid_dense_finish_kernel', 'fid_triplet_kernel', 'fid_dense_wgrad_kernel',
                 'fid_dense_dgrad_kernel')


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def copy_bandwidth():
    """Device-to-device copy of 1 GiB: bytes read + written per second."""
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
    b = torch.empty_like(a)
    dt = timed(lambda: b.copy_(a), 10, 3)
    return 2.0 * a.numel() * 4 / dt


def bucket_path_cost(m, xs, iters, params0, state0, rounds=3):
    """ms per step of the plain step and of the trainer's bucket path at one rank, `rounds` alternating blocks of `iters` steps
    each (the first block of either is preceded by a warm-up step); the model's context exists before the communicator."""
    import torch.distributed as dist
    from face_vijnana_yolov3_amd.parallel import DataParallelTrainer
    dist.init_process_group('nccl', store=dist.HashStore(), rank=0, world_size=1, device_id=m.dev)
    tr = DataParallelTrainer(m, world_size=1, rank=0, force_bucket_path=True)
    ms = dict(plain=[], bucket_path=[])
    for r in range(rounds):
        for name, step in (('plain', lambda: m.train_on_batch(*xs, 1e-6, 0.99, 0.99)),
                           ('bucket_path', lambda: tr.train_on_inputs(xs, 1e-6, 0.99, 0.99))):
            ms[name].append(1e3 * timed(step, iters, 1 if r == 0 else 0))
            m.params.copy_(params0); m.state.copy_(state0)
    res = dict(plain_ms=round(min(ms['plain']), 2), bucket_path_ms=round(min(ms['bucket_path']), 2),
               plain_ms_blocks=[round(v, 2) for v in ms['plain']], bucket_path_ms_blocks=[round(v, 2) for v in ms['bucket_path']],
               buckets=len(tr.reducer.launched), comm_mode=tr.comm_mode, bucket_mib=tr.bucket_bytes >> 20)
    tr.shutdown()
    dist.destroy_process_group()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    m = FidModel(S, 0)
    m.init_synthetic(seed=7)
    m.init_dense()
    g = torch.Generator(device='cuda').manual_seed(0)
    out = dict(image_size=S)
    for B in (1, 48):
        x = torch.rand((B, S, S, 3), generator=g, device='cuda')
        dt = timed(lambda: m.extract_device(x), args.iters, 2)
        out['extract_img_per_s_b%d' % B] = round(B / dt, 2)
    state0, params0 = m.state.clone(), m.params.clone()
    for B in (1, 13):
        xs = [torch.rand((B, S, S, 3), generator=g, device='cuda') for _ in range(3)]
        dt = timed(lambda: m.train_on_batch(*xs, 1e-6, 0.99, 0.99), args.iters, 1)
        out['train_triplets_per_s_b%d' % B] = round(B / dt, 3)
        out['train_step_ms_b%d' % B] = round(dt * 1e3, 2)
        m.params.copy_(params0); m.state.copy_(state0)
    bw = copy_bandwidth()
    out['copy_bandwidth_tb_s'] = round(bw / 1e12, 3)
    xs = [torch.rand((13, S, S, 3), generator=g, device='cuda') for _ in range(3)]
    m.forward_backward(*xs)
    torch.cuda.synchronize()
    m.ctx.profile(True)
    m.forward_backward(*xs)
    recs = m.ctx.profile_collect()
    m.ctx.profile(False)
    dense = {}
    for k in DENSE_KERNELS:
        r = recs.get(k)
        if r:
            dense[k] = dict(us=round(1e3 * r['ms'] / r['launches'], 2), floor_us=round(1e6 * r['bytes'] / r['launches'] / bw, 2))
    out['dense_kernels_b13'] = dense
    out['dense_total_us_b13'] = round(sum(v['us'] for v in dense.values()), 1)
    out['data_parallel_b13'] = bucket_path_cost(m, xs, args.iters, params0, state0)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
