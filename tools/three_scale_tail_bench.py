"""The three-scale head's inference tail on one GPU, one JSON line:

  kernel     fv_yolo_select_cands alone between device events at 48 images x capacity 4225 x num_cands 60 and at 1 image, on lists
             with few (a trained detector's) and with all rows kept: median and range over the repetitions of a block of launches
             (with --kernel; needs the entry point)
  test_loop  bench.py's `detect.test_loop_three_scale_head` measurement (FaceDetector.test() over 256 JPEGs at eval batch 16 / 32 /
             default, and device_only), repeated --loops times
  collect    FaceDetector._detect_collect alone on a finished batch (the host's share of the tail) at batch 16 / 48, host clock

Without --kernel it runs on any commit that has bench.test_loop_bench (copied into that checkout's tools/), so that two checkouts can
be measured alternately on the same box.

    python tools/three_scale_tail_bench.py [--kernel] [--loops N] [--tag NAME]
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


def kernel_bench(blocks=7, launches=50):
    from face_vijnana_yolov3_amd._lib import Context
    from face_vijnana_yolov3_amd.yolov3 import select_cands, select_cands_buffers
    ctx, dev = Context(0), torch.device('cuda', 0)
    out = {}
    for nimg in (48, 1):
        for name, share in (('sparse', 0.02), ('dense', 1.0)):
            rng = np.random.default_rng(nimg)
            cap = 4225
            cls = rng.uniform(0.05, 1.0, (nimg, cap, 1)).astype(np.float32)
            cls[rng.random((nimg, cap)) >= share] = 0.0
            res = dict(boxes=torch.from_numpy(rng.integers(0, 416, (nimg, cap, 4)).astype(np.int32)).to(dev),
                       objness=torch.from_numpy(rng.uniform(0.5, 1, (nimg, cap)).astype(np.float32)).to(dev),
                       classes=torch.from_numpy(cls).to(dev), count=torch.full((nimg,), cap, dtype=torch.int32, device=dev))
            buf = select_cands_buffers(nimg, 60, 1, dev)
            for _ in range(10):
                select_cands(ctx, res, 60, 13, out=buf)
            torch.cuda.synchronize()
            us = []
            for _ in range(blocks):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    select_cands(ctx, res, 60, 13, out=buf)
                e1.record()
                e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / launches)
            out['%d_images_%s' % (nimg, name)] = dict(kept_per_image=int((cls[..., 0] > 0).sum() / nimg), us_median=round(float(np.median(us)), 2),
                                                     us_min=round(min(us), 2), us_max=round(max(us), 2), blocks=blocks, launches_per_block=launches)
    return out


def collect_bench():
    import bench
    from face_vijnana_yolov3_amd import face_detection
    face_detection.DEBUG = False
    conf = {'mode': 'test', 'raw_data_path': '.', 'test_path': '.', 'output_file_path': os.devnull, 'multi_gpu': False, 'num_gpus': 1,
            'yolov3_base_model_load': False, 'model_loading': False,
            'hps': dict(bench.HPS, epochs=1, step=1, batch_size=40, face_conf_th=0.5, nms_iou_th=0.5, num_cands=60),
            'nn_arch': {'image_size': 416, 'bb_info_c_size': 6, 'head': 'three_scale'}}
    fd = face_detection.FaceDetector(conf, 0)
    for d in fd.model.layers:                             # as bench.test_loop_bench: objectness logits around -2, a few cells fire
        if not d['has_bn']:
            fd.model.params[d['w_off']:d['beta_off']] *= 0.05
            fd.model.params[d['beta_off'] + 4:d['beta_off'] + d['cout']:6] = -2.0
    out = {}
    for B in (16, 48):
        x = torch.rand((B, 416, 416, 3), device='cuda', generator=torch.Generator('cuda').manual_seed(B))
        fd._detect_collect(fd._detect_launch(x))
        ms, copied = [], 0
        for _ in range(9):
            launched = fd._detect_launch(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            boxes = fd._detect_collect(launched)
            ms.append((time.perf_counter() - t0) * 1e3)
            copied = sum(t.numel() * t.element_size() for t in launched[1].values())
        out['batch_%d' % B] = dict(collect_ms_median=round(float(np.median(ms)), 3), collect_ms_min=round(min(ms), 3), collect_ms_max=round(max(ms), 3),
                                   bytes_copied_per_image=copied // B, boxes_per_image=round(sum(len(b) for b in boxes) / B, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--loops', type=int, default=1)
    ap.add_argument('--tag', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('three_scale_tail_bench needs the GPU: there is nothing to measure without one')
    out = {'tag': a.tag}
    if a.kernel:
        out['kernel'] = kernel_bench()
    if a.loops > 0:
        import bench
        out['test_loop'] = [bench.test_loop_bench(0, 416, n_img=256, head='three_scale') for _ in range(a.loops)]
    out['collect'] = collect_bench()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
