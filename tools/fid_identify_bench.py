"""Face identification on one GPU at 416 x 416: fv_letterbox_crops and fv_fid_match per call (n = 2 880 crops / queries; registry
m = 1 085 and 8 631) against their byte floors at the measured device-to-device copy bandwidth, and FaceIdentifier.test() frames/s
on synthetic 1920 x 1080 JPEGs with 60 face boxes per frame (the detector runs for real; its boxes are then replaced by 60 preset
ones, so the identification half does the work of a crowded frame).  Prints one JSON line.

    python tools/fid_identify_bench.py [--frames N] [--iters N]
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import face_identification as fi  # noqa: E402
from face_vijnana_yolov3_amd._lib import Context  # noqa: E402
from face_vijnana_yolov3_amd.postproc import BoundBox, letterbox_batch_device  # noqa: E402

S = 416
H, W = 1080, 1920


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def copy_bandwidth():
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
    b = torch.empty_like(a)
    dt = timed(lambda: b.copy_(a), 10)
    return 2 * a.numel() * 4 / dt


def preset_boxes(rng, n=60):
    out = []
    for _ in range(n):
        w, h = int(rng.integers(40, 220)), int(rng.integers(40, 220))
        x, y = int(rng.integers(2, W - w)), int(rng.integers(2, H - h))
        out.append((x, y, x + w, y + h, float(rng.uniform(0.5, 1.0))))
    return out


def kernels(bw, iters):
    rng = np.random.default_rng(0)
    ctx = Context(0)
    raws = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(48)]
    keep = []
    letterbox_batch_device(ctx, raws, S, torch.device('cuda', 0), keep=keep)
    crops = []
    for i in range(48):
        for b in preset_boxes(rng):
            crops.append((i, b[1], b[0], b[3] - b[1], b[2] - b[0]))
    n = len(crops)
    out = torch.empty((n, S, S, 3), dtype=torch.float32, device='cuda')
    t_lb = timed(lambda: fi.letterbox_crops(ctx, keep[0], crops, S, out=out), iters)
    lb_bytes = sum(c[3] * c[4] * 3 for c in crops) + 12.0 * S * S * n
    res = {'crops_n': n, 'letterbox_crops_ms': t_lb * 1e3, 'letterbox_crops_floor_ms': lb_bytes / bw * 1e3}
    q = torch.randn((n, 64), device='cuda')
    for m in (1085, 8631):
        r = torch.randn((m, 64), device='cuda')
        t = timed(lambda: fi.fid_match(ctx, q, r), iters)
        res['match_m%d_ms' % m] = t * 1e3
        res['match_m%d_floor_ms' % m] = ((n + m) * 256 + 12 * n) / bw * 1e3
        res['match_m%d_gflops_fp64' % m] = 3.0 * n * m * 64 / t / 1e9
    return res


def identify(frames, reps):
    from PIL import Image
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        rng = np.random.default_rng(1)
        os.makedirs('frames')
        for k in range(frames):
            base = rng.integers(0, 256, (H // 16, W // 16, 3)).astype(np.uint8)
            Image.fromarray(np.kron(base, np.ones((16, 16, 1), np.uint8))).save('frames/f%03d.jpg' % k, quality=90)
        reg = rng.normal(size=(1085, 64)).astype(np.float32)
        with open('ref_facial_id_db.pickle', 'wb') as f:
            pickle.dump({k: reg[k] for k in range(len(reg))}, f)
        conf = {'fi_conf': dict(mode='test', resource_type='uccs', raw_data_path=tmp, test_path=os.path.join(tmp, 'frames'),
                                output_file_path=os.path.join(tmp, 'solution_fi.csv'), multi_gpu=False, num_gpus=1,
                                yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64),
                                hps=dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=1, sim_th=100.0)),
                'fd_conf': {'mode': 'test', 'raw_data_path': tmp, 'test_path': os.path.join(tmp, 'frames'), 'output_file_path': 'x.csv',
                            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
                            'hps': {'face_conf_th': 0.5, 'nms_iou_th': 0.5, 'num_cands': 60, 'eval_batch_size': 48},
                            'nn_arch': {'image_size': S, 'bb_info_c_size': 6}}}
        ident = fi.FaceIdentifier(conf)
        fd = ident.fd
        boxes = preset_boxes(np.random.default_rng(2))
        orig = fd._detect_files

        def crowded(files, need_raw=True, _with_images=False):
            for item in orig(files, need_raw, _with_images):
                yield (item[0], item[1], [BoundBox(np.float64(b[0]), np.float64(b[1]), np.float64(b[2]), np.float64(b[3]),
                                                   objness=b[4], classes=[np.float32(b[4])]) for b in boxes]) + tuple(item[3:])
        fd._detect_files = crowded
        ident.test()                                    # warm-up: workspaces, pinned buffers, code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            ident.test()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / reps
        rows = open(conf['fi_conf']['output_file_path']).read().count('\n')
        return {'test_frames': frames, 'test_rows': rows, 'test_frames_per_s': frames / dt, 'test_crops_per_s': rows / dt}
    finally:
        os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    bw = copy_bandwidth()
    res = {'device': torch.cuda.get_device_name(0), 'image_size': S, 'copy_GBps': bw / 1e9}
    res.update(kernels(bw, a.iters))
    res.update(identify(a.frames, a.reps))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
