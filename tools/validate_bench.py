"""hps['validate'] on one GPU.  Two measurements, one JSON line:

  metric   the device metric stage (fv_det_rows_from_nms + fv_det_match_rows + fv_det_ap_sweep, ten thresholds) over synthetic
           decode/NMS results of n_img images with 60 detections each (N ~ 6 000, 60 000, 600 000 counted detections), three
           ground-truth boxes per image: median ms over the rounds between two HIP events, against cal_mAP_sweep (pandas + NumPy +
           SciPy, the host clock) on the csv files that hold the same rows.  The two mean APs are printed side by side.
  pass     FaceDetector.validate() against FaceDetector.test() over the same folder of JPEG files (S = 416, the default
           eval_batch_size), alternating, wall ms per pass ending in a device synchronise.

    python tools/validate_bench.py [--rounds R] [--images N] [--alternations A] [--skip-host-above N] [--skip-pass] [--skip-metric]
                                   [--head single|three_scale]

--head three_scale: the pass with nn_arch.head = three_scale (fv_yolo_decode_nms_batch -> fv_yolo_select_cands in fv_decode_nms' place).
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

from face_vijnana_yolov3_amd import data, det_metric, evaluate  # noqa: E402

S, K = 416, 60


def synthetic_set(n_img, seed=0):
    """decode/NMS-shaped results whose boxes sit near three ground-truth boxes per image, so that matches exist."""
    rng = np.random.default_rng(seed)
    h, w = 480, 640
    geom = np.tile(np.array([(h, w) + tuple(data.letterbox_geometry(h, w, S)[2:])], np.int32), (n_img, 1))
    cx = rng.integers(40, S - 40, (n_img, K)); cy = rng.integers(80, S - 80, (n_img, K))
    hw_ = rng.integers(8, 40, (n_img, K, 2))
    boxes = np.stack([cx - hw_[..., 0], cy - hw_[..., 1], cx + hw_[..., 0], cy + hw_[..., 1]], axis=2).astype(np.int32)
    score = np.sort(rng.uniform(0.05, 1.0, (n_img, K)).astype(np.float32), axis=1)
    count = np.full(n_img, K, np.int32)
    scale = w / S
    pad_t = int(geom[0, 2])
    sel = boxes[:, :3].astype(np.float64)                  # ground truth: three of the detections, back-projected and jittered
    gt = np.stack([sel[..., 0] * scale, np.maximum(sel[..., 1] - pad_t, 0) * scale, (sel[..., 2] - sel[..., 0]) * scale,
                   (sel[..., 3] - sel[..., 1]) * scale], axis=2) + rng.normal(0, 3, (n_img, 3, 4))
    gt[..., 2:] = np.maximum(gt[..., 2:], 4)
    return boxes, score, count, geom, np.round(gt, 1)


def metric_bench(ctx, dev, n_img, rounds, host):
    boxes, score, count, geom, gt = synthetic_set(n_img)
    res = dict(boxes=torch.from_numpy(boxes).to(dev), score=torch.from_numpy(score).to(dev), count=torch.from_numpy(count).to(dev))
    d_geom = torch.from_numpy(geom).to(dev)
    d_gt = torch.from_numpy(gt.reshape(-1, 4)).to(dev)
    d_off = torch.arange(0, 3 * n_img + 1, 3, dtype=torch.int64, device=dev)
    ths = np.arange(0.5, 1.0, 0.05)
    rows = torch.empty((n_img, det_metric.ROWS, 5), dtype=torch.float64, device=dev)
    nrows = torch.empty((n_img,), dtype=torch.int32, device=dev)
    iou = torch.empty((n_img, det_metric.ROWS), dtype=torch.float64, device=dev)
    flag = torch.empty((n_img,), dtype=torch.int32, device=dev)

    def stage():
        det_metric.rows_from_nms(ctx, res, d_geom, S, rows, nrows)
        det_metric.match_rows(ctx, rows, nrows, d_gt, d_off, 3, iou, flag)
        return det_metric.ap_sweep(ctx, rows, nrows, iou, flag, ths, 3 * n_img)

    out = stage()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = stage(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    n_det = int(out['n_det'].cpu()[0])
    r = dict(n_img=n_img, n_det=n_det, device_ms=float(np.median(ms)), device_ms_min=float(np.min(ms)),
             device_mean_ap=float(out['result'][0].mean().cpu()))
    if host:
        with tempfile.TemporaryDirectory() as tmp:
            h_rows, h_nrows = rows.cpu().numpy(), nrows.cpu().numpy()
            gt_csv, sol_csv = os.path.join(tmp, 'validation.csv'), os.path.join(tmp, 'solution.csv')
            with open(gt_csv, 'w') as f:
                f.write('FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT\n')
                for i in range(n_img):
                    for j in range(3):
                        f.write('%d,img_%07d.jpg,1,%r,%r,%r,%r\n' % ((3 * i + j,  i) + tuple(float(v) for v in gt[i, j])))
            with open(sol_csv, 'w') as f:
                for i in range(n_img):
                    for j in range(int(h_nrows[i])):
                        f.write('img_%07d.jpg,%s\n' % (i, ','.join(repr(float(v)) for v in h_rows[i, j])))
            t0 = time.perf_counter()
            _res, mean = evaluate.cal_mAP_sweep(gt_csv, sol_csv)
            r['host_ms'] = (time.perf_counter() - t0) * 1e3
            r['host_mean_ap'] = mean
    return r


def pass_bench(n_images, alternations, head='single'):
    from face_vijnana_yolov3_amd import face_detection
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    face_detection.DEBUG = False
    with tempfile.TemporaryDirectory() as tmp:
        data.make_synthetic_uccs(tmp, n_images=n_images, seed=0, csv_name='validation.csv')
        conf = {'mode': 'test', 'raw_data_path': tmp, 'test_path': tmp, 'output_file_path': os.path.join(tmp, 'solution_fd.csv'),
                'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
                'hps': {'face_conf_th': 0.5, 'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'validate': True},
                'nn_arch': {'image_size': S, 'bb_info_c_size': 6, 'head': head}}
        fd = FaceDetector(conf)
        if head == 'single':
            d = fd.model.layers[-1]
            fd.model.params[d['beta_off']] = 1.0; fd.model.params[d['beta_off'] + 5] = 1.0  # some cells pass the threshold
        else:
            for d in fd.model.layers:                     # the three detection convs: objectness logits around -2, a few cells fire
                if not d['has_bn']:
                    fd.model.params[d['w_off']:d['beta_off']] *= 0.05
                    fd.model.params[d['beta_off'] + 4:d['beta_off'] + d['cout']:6] = -2.0
        times = {'test': [], 'validate': []}
        fd.test(); fd.validate()                                                           # warm-up of both paths
        for _ in range(alternations):
            for name in ('test', 'validate'):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = getattr(fd, name)()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        return dict(head=head, images=n_images, eval_batch_size=face_detection.default_eval_batch(S), test_ms=float(np.median(times['test'])),
                    validate_ms=float(np.median(times['validate'])), n_det=out['n_det'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--images', type=int, default=480)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--skip-host-above', type=int, default=10 ** 9, help='no cal_mAP_sweep run for sets of more images than this')
    ap.add_argument('--skip-pass', action='store_true')
    ap.add_argument('--skip-metric', action='store_true')
    ap.add_argument('--head', choices=('single', 'three_scale'), default='single', help='nn_arch.head of the pass measurement')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('validate_bench needs the GPU: there is nothing to measure without one')
    from face_vijnana_yolov3_amd._lib import Context
    ctx = Context(0)
    dev = torch.device('cuda', 0)
    out = {}
    if not a.skip_metric:
        out['metric'] = [metric_bench(ctx, dev, n, a.rounds, n <= a.skip_host_above) for n in (100, 1000, 10000)]
    if not a.skip_pass:
        out['pass'] = pass_bench(a.images, a.alternations, a.head)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
