"""FaceIdentifier throughput on one GPU at 416 x 416: facial-ID extraction (fv_fid_extract) at batch 1 and 48, triplet training
steps (fv_fid_train_step + fv_adam_step) at B = 1 and 13, and the per-launch time of the four dense-head kernels of a B = 13 step
against their byte floors at the measured device-to-device copy bandwidth; then, alternating in this process, the plain B = 13
step and the same step through parallel.DataParallelTrainer with the bucket path forced over a world-size-1 `nccl` group (RCCL
launches no kernel at one rank: what the callbacks and the stream traffic cost).  Prints one JSON line.

    python tools/fid_bench.py [--iters N]
    python tools/fid_bench.py --only batch_step [--iters N]

batch_step: alternating in this process, three blocks each of the three-tower B = 13 triplet step and of the
one-tower M = 39 labelled-batch step (fv_fid_batch_train_step + fv_adam_step; 13 subjects of 3 crops), the host clock around
blocks that end in a synchronise, all blocks reported; then the per-launch device time of the batch loss's three kernels at
M = 39, 96 and 1024 next to fid_triplet_kernel at B = 13, and the loss's share of the M = 39 step.

    python tools/fid_bench.py --only margin_step [--iters N] [--classes C]

margin_step: alternating in this process, three blocks each of the one-tower M = 39 labelled-batch step
(fv_fid_batch_train_step + fv_adam_step) and of the margin-softmax step on the same images (fv_fid_cls_train_step + two
fv_adam_step; C classes, default 1000), all blocks reported; then the per-launch device time of the loss's six kernels inside that
step and alone at (M, C) = (39, 1000), (96, 8631) and (1024, 8631) for both kinds, and of the class kernel's Adam launch.
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


BATCH_KERNELS = ('fid_batch_select_kernel', 'fid_batch_grad_kernel', 'fid_batch_finish_kernel')


def profiled_us(m, fn, names):
    """Per-launch device time (us) of the named kernels over one call of fn, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    m.ctx.profile(True)
    fn()
    recs = m.ctx.profile_collect()
    m.ctx.profile(False)
    return {k: round(1e3 * recs[k]['ms'] / recs[k]['launches'], 2) for k in names if k in recs}


def batch_step(m, g, iters, rounds=3):
    from face_vijnana_yolov3_amd import ops
    state0, params0 = m.state.clone(), m.params.clone()
    B, P, K = 13, 13, 3
    xs = [torch.rand((B, S, S, 3), generator=g, device='cuda') for _ in range(3)]
    x = torch.cat(xs)
    subjects = torch.arange(P, dtype=torch.int32, device='cuda').repeat_interleave(K)
    ms = dict(three_tower_b13=[], one_tower_m39=[])
    for r in range(rounds):
        for name, step in (('three_tower_b13', lambda: m.train_on_batch(*xs, 1e-6, 0.99, 0.99)),
                           ('one_tower_m39', lambda: m.train_on_labelled_batch(x, subjects, 'batch_semi_hard', 1e-6, 0.99, 0.99))):
            ms[name].append(round(1e3 * timed(step, iters, 1 if r == 0 else 0), 2))
            m.params.copy_(params0); m.state.copy_(state0)
    out = dict(image_size=S, iters_per_block=iters, step_ms_blocks=ms)
    out['triplet_kernel_us_b13'] = profiled_us(m, lambda: m.forward_backward(*xs), ('fid_triplet_kernel',))
    out['batch_loss_us_in_step_m39'] = profiled_us(m, lambda: m.forward_backward_batch(x, subjects, 'batch_semi_hard'), BATCH_KERNELS)
    m.params.copy_(params0); m.state.copy_(state0)
    loss_us = sum(out['batch_loss_us_in_step_m39'].values())
    out['batch_loss_share_of_step'] = round(loss_us / (1e3 * min(ms['one_tower_m39'])), 5)
    alone = {}
    for M in (39, 96, 1024):
        pre = torch.randn((M, 64), generator=g, device='cuda')
        r = torch.relu(pre)
        u = r / r.norm(dim=1, keepdim=True).clamp_min(1e-6)
        sub = (torch.arange(M, device='cuda') % max(1, M // 6)).to(torch.int32)
        for mode in (0, 1):
            us = profiled_us(m, lambda: ops.fid_batch_triplet_loss_grad(m.ctx, pre, u, sub, 0.2, mode), BATCH_KERNELS)
            us['total'] = round(sum(us.values()), 2)
            alone['m%d_mode%d' % (M, mode)] = us
    out['batch_loss_us_alone'] = alone
    return out


MARGIN_KERNELS = ('fid_margin_cos_kernel', 'fid_margin_row_kernel', 'fid_margin_du_kernel', 'fid_margin_dw_kernel',
                  'fid_margin_rows_kernel', 'fid_margin_finish_kernel')


def margin_step(m, g, iters, C, rounds=3):
    from face_vijnana_yolov3_amd import ops
    state0, params0 = m.state.clone(), m.params.clone()
    P, K = 13, 3
    x = torch.rand((P * K, S, S, 3), generator=g, device='cuda')
    subjects = torch.arange(P, dtype=torch.int32, device='cuda').repeat_interleave(K)
    m.init_classes(C, 0)
    ms = dict(batch_mining_m39=[], margin_softmax_m39=[])
    for r in range(rounds):
        for name, step in (('batch_mining_m39', lambda: m.train_on_labelled_batch(x, subjects, 'batch_semi_hard', 1e-6, 0.99, 0.99)),
                           ('margin_softmax_m39', lambda: m.train_on_classified_batch(x, subjects, 'cosface', 30.0, None, 1e-6, 0.99, 0.99))):
            ms[name].append(round(1e3 * timed(step, iters, 1 if r == 0 else 0), 2))
            m.params.copy_(params0); m.state.copy_(state0)
    out = dict(image_size=S, classes=C, iters_per_block=iters, step_ms_blocks=ms)
    out['margin_loss_us_in_step_m39'] = profiled_us(m, lambda: m.forward_backward_classes(x, subjects, 'cosface'), MARGIN_KERNELS)
    out['margin_loss_us_in_step_m39']['total'] = round(sum(out['margin_loss_us_in_step_m39'].values()), 2)
    m.params.copy_(params0); m.state.copy_(state0)
    adam = lambda: ops.adam_step(m.ctx, m.class_kernel, m.class_grads, m.class_m, m.class_v, 0, 1e-6, 0.99, 0.99)
    out['class_adam_us'] = profiled_us(m, adam, ('adam_kernel',))
    alone = {}
    for M, Cc in ((39, 1000), (96, 8631), (1024, 8631)):
        pre = torch.randn((M, 64), generator=g, device='cuda')
        r = torch.relu(pre)
        u = r / r.norm(dim=1, keepdim=True).clamp_min(1e-6)
        W = 0.1 * torch.randn((Cc, 64), generator=g, device='cuda')
        labels = (torch.arange(M, device='cuda') % Cc).to(torch.int32)
        ws = torch.empty(int(ops.lib().fv_fid_margin_workspace_bytes(M, Cc)), dtype=torch.uint8, device='cuda')
        for kind in (0, 1):
            us = profiled_us(m, lambda: ops.fid_margin_softmax_loss_grad(m.ctx, pre, u, labels, W, kind, 30.0, 0.35 if kind == 0 else 0.5,
                                                                         workspace=ws), MARGIN_KERNELS)
            us['total'] = round(sum(us.values()), 2)
            alone['m%d_c%d_kind%d' % (M, Cc, kind)] = us
    out['margin_loss_us_alone'] = alone
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--only', choices=['batch_step', 'margin_step'], default=None)
    ap.add_argument('--classes', type=int, default=1000)
    args = ap.parse_args()
    m = FidModel(S, 0)
    m.init_synthetic(seed=7)
    m.init_dense()
    g = torch.Generator(device='cuda').manual_seed(0)
    if args.only == 'batch_step':
        print(json.dumps(batch_step(m, g, args.iters)))
        return
    if args.only == 'margin_step':
        print(json.dumps(margin_step(m, g, args.iters, args.classes)))
        return
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
