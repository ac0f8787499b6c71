"""The reconstruction model on one GPU at 416 x 416: images/s of ReconModel.predict_device at batch 1 and
48 beside facial-ID extraction (FidModel.extract_device) in the same process -- the same conv kernels and about the same FLOPs
run the other way --, the normalise stage's bytes/s per channel count against a device-to-device copy, the per-kernel times of a
batch-48 pass, and the five stride-2 transposed convs in Keras' (0, 1) alignment beside the existing (1, 1) data-gradient of the
same layers.  Prints one JSON line.

    python tools/recon_bench.py [--iters N]
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

from face_vijnana_yolov3_amd import ops  # noqa: E402
from face_vijnana_yolov3_amd._lib import lib, ptr  # noqa: E402
from face_vijnana_yolov3_amd.face_identification import FidModel, ReconModel  # noqa: E402

S = 416
NULL = None


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    fid = FidModel(S, 0)
    fid.init_synthetic(seed=7)
    fid.init_dense()
    rec = ReconModel.from_identifier(fid, seed=0)
    ctx = rec.ctx
    g = torch.Generator(device='cuda').manual_seed(0)
    out = dict(image_size=S)

    # ---- whole passes, alternating extraction and reconstruction
    for B in (1, 48):
        x = torch.rand((B, S, S, 3), generator=g, device='cuda')
        ids = fid.extract_device(x)
        ex, rc = [], []
        for _ in range(3):
            ex.append(timed(lambda: fid.extract_device(x), args.iters, 2))
            rc.append(timed(lambda: rec.predict_device(ids), args.iters, 2))
        out['extract_img_per_s_b%d' % B] = round(B / min(ex), 2)
        out['recon_img_per_s_b%d' % B] = round(B / min(rc), 2)
        out['recon_ms_b%d_blocks' % B] = [round(1e3 * v, 3) for v in rc]
        out['extract_ms_b%d_blocks' % B] = [round(1e3 * v, 3) for v in ex]
        out['recon_over_extract_b%d' % B] = round(min(ex) / min(rc), 3)

    # ---- per-kernel times of one batch-48 pass (event pairs around every launch)
    ids = fid.extract_device(torch.rand((48, S, S, 3), generator=g, device='cuda'))
    rec.predict_device(ids)
    torch.cuda.synchronize()
    ctx.profile(True)
    rec.predict_device(ids)
    recs = ctx.profile_collect()
    ctx.profile(False)
    groups = {}
    for k, r in recs.items():
        name = k.split('<')[0].split(' ')[0]
        e = groups.setdefault(name, dict(launches=0, ms=0.0))
        e['launches'] += r['launches']; e['ms'] += r['ms']
    out['kernels_b48'] = {k: dict(launches=v['launches'], ms=round(v['ms'], 3)) for k, v in sorted(groups.items())}
    out['kernels_b48_total_ms'] = round(sum(v['ms'] for v in groups.values()), 3)

    # ---- the normalise stage alone, at the rows of a batch-48 pass, against a copy
    bw = copy_bandwidth()
    out['copy_bandwidth_tb_s'] = round(bw / 1e12, 3)
    norm = {}
    for C, div in ((32, 1), (64, 2), (128, 4), (256, 8), (512, 16), (1024, 32)):
        rows = 48 * (S // div) ** 2
        x = torch.randn((rows, C), generator=g, device='cuda')
        sk = torch.randn((rows, C), generator=g, device='cuda')
        d = torch.empty_like(x); y = torch.empty_like(x)
        sc = torch.rand(C, generator=g, device='cuda') + 0.5
        sh = torch.randn(C, generator=g, device='cuda')
        L = lib()
        t2 = timed(lambda: L.fv_l2norm_affine(ctx.handle, ptr(x), NULL, NULL, ptr(sc), ptr(sh), ptr(y), rows, C, 0.1), args.iters, 3)
        t4 = timed(lambda: L.fv_l2norm_affine(ctx.handle, ptr(x), ptr(sk), ptr(d), ptr(sc), ptr(sh), ptr(y), rows, C, 0.1), args.iters, 3)
        nbytes = 4.0 * rows * C
        norm[str(C)] = dict(rows=rows, plain_us=round(1e6 * t2, 1), plain_tb_s=round(2 * nbytes / t2 / 1e12, 3),
                            subtract_us=round(1e6 * t4, 1), subtract_tb_s=round(4 * nbytes / t4 / 1e12, 3))
        del x, sk, d, y
    out['l2norm_affine_b48'] = norm

    # ---- the stride-2 transposed convs: the new (0, 1) alignment beside the (1, 1) data-gradient of the same layers
    s2 = {}
    B = 48
    for d in rec.layers:
        if d['stride'] != 2:
            continue
        Hin = S // d['out_div']
        xin = torch.randn((B, Hin, Hin, d['cout']), generator=g, device='cuda')
        w = torch.randn((d['cout'], 3, 3, d['cin']), generator=g, device='cuda') * 0.05
        wt = ops.transpose_weights(ctx, w)
        o = torch.empty((B, 2 * Hin, 2 * Hin, d['cin']), dtype=torch.float32, device='cuda')
        L = lib()
        ta, tb = [], []
        for _ in range(3):
            ta.append(timed(lambda: L.fv_conv2d_transpose(ctx.handle, ptr(xin), ptr(wt), B, Hin, Hin, d['cin'], d['cout'], 3, 2, ptr(o)), args.iters, 2))
            tb.append(timed(lambda: L.fv_conv2d_dgrad(ctx.handle, ptr(xin), ptr(wt), B, 2 * Hin, 2 * Hin, d['cin'], d['cout'], 3, 2, NULL, ptr(o)), args.iters, 2))
        flops = 2.0 * B * Hin * Hin * d['cin'] * 9 * d['cout']
        s2['conv_%d' % d['darknet_index']] = dict(transpose_ms=round(1e3 * min(ta), 3), dgrad_ms=round(1e3 * min(tb), 3),
                                                  transpose_tf=round(flops / min(ta) / 1e12, 1), dgrad_tf=round(flops / min(tb) / 1e12, 1))
        del xin, w, wt, o
    out['stride2_b48'] = s2
    print(json.dumps(out))


if __name__ == '__main__':
    main()
