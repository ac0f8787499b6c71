"""The detection metric of evaluate.cal_mAP_fd on the device (csrc/det_metric.hip): thin wrappers over
fv_det_rows_from_nms / fv_det_match_rows / fv_det_ap_sweep, and the Validator FaceDetector.validate() runs them through.

Buffers: rows (n, 60, 5) float64 = x, y, w, h, conf per detection (what FaceDetector._write_rows writes, as float() reads it
back), nrows (n,) int32, iou (n, 60) float64 (assigned IoU, -1 without one), flag (n,) int32 (1: some pair of the image overlapped;
0: none did and the image's detections count nowhere, as in the reference)."""
import ctypes
import os

import numpy as np

from ._lib import lib, ptr

ROWS = 60                 # FV_DET_ROWS: _write_rows' boxes[:60]
MAX_GT = 4096             # FV_DET_MAX_GT


def rows_from_nms(ctx, res, geom, image_size, rows=None, nrows=None):
    """decode_nms' device dict + geom (n, 6) int32 CUDA tensor (h, w, pad_t, pad_b, pad_l, pad_r) -> (rows, nrows), written into
    the given tensors (views of a whole-set buffer) when there are any.  No host sync."""
    import torch
    boxes = res['boxes']
    n, k = int(boxes.shape[0]), int(boxes.shape[1])
    dev = boxes.device
    if rows is None:
        rows = torch.empty((n, ROWS, 5), dtype=torch.float64, device=dev)
        nrows = torch.empty((n,), dtype=torch.int32, device=dev)
    assert geom.dtype == torch.int32 and tuple(geom.shape) == (n, 6) and tuple(rows.shape) == (n, ROWS, 5)
    ctx.check(lib().fv_det_rows_from_nms(ctx.handle, ptr(boxes), ptr(res['score']), ptr(res['count']), ptr(geom), n, k, int(image_size),
                                         ptr(rows), ptr(nrows)), 'fv_det_rows_from_nms')
    return rows, nrows


def match_rows(ctx, rows, nrows, gt, gt_off, max_gt, iou=None, flag=None):
    """rows / nrows of n images, gt (total, 4) float64 x, y, w, h and gt_off (n + 1,) int64 CUDA tensors (a view into a longer
    offsets tensor is fine: offsets are absolute) -> (iou, flag).  max_gt: the largest group (host); > MAX_GT raises."""
    import torch
    n = int(rows.shape[0])
    if iou is None:
        iou = torch.empty((n, ROWS), dtype=torch.float64, device=rows.device)
        flag = torch.empty((n,), dtype=torch.int32, device=rows.device)
    assert gt.dtype == torch.float64 and gt_off.dtype == torch.int64 and gt_off.numel() >= n + 1
    ctx.check(lib().fv_det_match_rows(ctx.handle, ptr(rows), ptr(nrows), ptr(gt), ptr(gt_off), n, int(max_gt), ptr(iou), ptr(flag)),
              'fv_det_match_rows')
    return iou, flag


def ap_sweep(ctx, rows, nrows, iou, flag, iou_ths, gt_count, want_curve=False, workspace=None):
    """One fv_det_ap_sweep over n images -> dict of CUDA tensors: result (3, T) float64 (AP, final precision, final recall per
    threshold), n_det (1,) int32 and, with want_curve, order (n * 60,) int32 and counts (T, n * 60) int32 (their first n_det entries
    hold the ranking and the running true-positive counts).  workspace: a CUDA tensor of at least
    fv_det_ap_sweep_workspace_bytes(n) bytes to work in (its contents are ignored); default: a fresh one.  No host sync."""
    import torch
    n = int(rows.shape[0])
    dev = rows.device
    ths = np.ascontiguousarray(np.asarray(iou_ths, np.float64).reshape(-1))
    T = len(ths)
    need = int(lib().fv_det_ap_sweep_workspace_bytes(n))
    ws = workspace if workspace is not None else torch.empty(max(need, 8) // 8 + 1, dtype=torch.float64, device=dev)
    assert ws.numel() * ws.element_size() >= need
    out = dict(result=torch.empty((3, T), dtype=torch.float64, device=dev), n_det=torch.empty((1,), dtype=torch.int32, device=dev))
    if want_curve:
        out['order'] = torch.empty((max(n * ROWS, 1),), dtype=torch.int32, device=dev)
        out['counts'] = torch.empty((T, max(n * ROWS, 1)), dtype=torch.int32, device=dev)
    ctx.check(lib().fv_det_ap_sweep(ctx.handle, ptr(rows), ptr(nrows), ptr(iou), ptr(flag), n,
                                    ths.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, int(gt_count), ptr(ws), need,
                                    ptr(out['result']), ptr(out['n_det']), ptr(out['order']) if want_curve else None,
                                    ptr(out['counts']) if want_curve else None), 'fv_det_ap_sweep')
    return out


def group_ground_truth(gt_df, names, what):
    """Ground truth rows of a validation.csv frame grouped per name of `names` (in that order) -> (boxes (total, 4) float64 x, y, w,
    h, offsets (len(names) + 1,) int64, largest group).  ValueError naming `what` (the file) for a group beyond MAX_GT."""
    groups = {k: v.iloc[:, 3:7].to_numpy(dtype=np.float64) for k, v in gt_df.groupby('FILE', sort=True)}
    parts, offs = [], [0]
    for name in names:
        g = groups.get(name)
        if g is not None and len(g) > MAX_GT:
            raise ValueError('%s: %d ground-truth rows for %s (the device metric takes at most %d per image)' % (what, len(g), name, MAX_GT))
        if g is not None:
            parts.append(g)
        offs.append(offs[-1] + (len(g) if g is not None else 0))
    boxes = np.concatenate(parts).reshape(-1, 4) if parts else np.zeros((0, 4))
    sizes = np.diff(offs)
    return np.ascontiguousarray(boxes), np.asarray(offs, np.int64), int(sizes.max()) if len(sizes) else 0


def summarise(iou_ths, result, n_det):
    """result (3, T) and n_det as host arrays -> the metric part of validate()'s dict."""
    ap = [float(v) for v in result[0]]
    return dict(iou_ths=[float(t) for t in iou_ths], ap=ap, mean_ap=float(np.mean(ap)) if ap else 0.0,
                precision=[float(v) for v in result[1]], recall=[float(v) for v in result[2]], n_det=int(n_det))


class Validator(object):
    """The held-out set of hps['validate'] (data.validate_conf's dict): sorted(glob(path/*.jpg)), validation.csv grouped per file
    in that order and uploaded once, the whole set's rows / iou buffers, and the recall denominator = ALL rows of the csv
    (gt_df.shape[0] in cal_mAP_fd).  Built once at the start of train() (or at the first validate())."""

    def __init__(self, ctx, device, conf):
        import glob

        import pandas as pd
        import torch
        self.conf = conf
        self.iou_ths = list(conf['iou_ths'])
        path = conf['path']
        self.files = sorted(glob.glob(os.path.join(path, '*.jpg')))
        csv = os.path.join(path, 'validation.csv')
        gt_df = pd.read_csv(csv)
        self.n_gt = int(gt_df.shape[0])
        if self.n_gt < 1:
            raise ValueError('%s holds no ground-truth row: nothing to validate against' % csv)
        boxes, offs, self.max_gt = group_ground_truth(gt_df, [os.path.basename(f) for f in self.files], csv)
        n = len(self.files)
        self.gt = torch.from_numpy(boxes).to(device)
        self.gt_off = torch.from_numpy(offs).to(device)
        self.rows = torch.empty((n, ROWS, 5), dtype=torch.float64, device=device)
        self.nrows = torch.empty((n,), dtype=torch.int32, device=device)
        self.iou = torch.empty((n, ROWS), dtype=torch.float64, device=device)
        self.flag = torch.empty((n,), dtype=torch.int32, device=device)

    def match(self, ctx, i0, n):
        """Images i0 .. i0 + n of the set: their rows are in place -> iou / flag."""
        match_rows(ctx, self.rows[i0:i0 + n], self.nrows[i0:i0 + n], self.gt, self.gt_off[i0:i0 + n + 1], self.max_gt,
                   self.iou[i0:i0 + n], self.flag[i0:i0 + n])

    def finish(self, ctx):
        """One sweep over the whole set and one small D2H copy -> the metric part of validate()'s dict."""
        import torch
        out = ap_sweep(ctx, self.rows, self.nrows, self.iou, self.flag, self.iou_ths, self.n_gt)
        host = torch.cat([out['result'].reshape(-1), out['n_det'].to(torch.float64)]).cpu().numpy()
        T = len(self.iou_ths)
        res = summarise(self.iou_ths, host[:3 * T].reshape(3, T), int(host[3 * T]))
        res.update(n_images=len(self.files), n_gt=self.n_gt)
        return res
