"""The contract of fv_det_rows_from_nms / fv_det_match_rows / fv_det_ap_sweep restated in numpy, float64 throughout, each value
formed by the operations the device runs in their order, so rows, assigned IoUs, the ranking and the running counts are compared
for equality and AP within the rounding of a sum.  Test infrastructure: the product does not import it.  Also the generators of
the cases the CPU and GPU tests share."""
import numpy as np

ROWS = 60
MAX_GT = 4096


def rows_from_nms(boxes, score, count, geom, image_size):
    """boxes (n, K, 4) int, score (n, K) float32, count (n,), geom (n, 6) = h, w, pad_t, pad_b, pad_l, pad_r -> (rows (n, 60, 5),
    nrows (n,)): FaceDetector._project_back on the first min(count, 60) boxes, then _write_rows' five values."""
    n, K = boxes.shape[0], boxes.shape[1]
    rows = np.zeros((n, ROWS, 5), np.float64)
    nrows = np.zeros(n, np.int32)
    S = int(image_size)
    for i in range(n):
        c = min(max(int(count[i]), 0), min(ROWS, K))
        nrows[i] = c
        h, w, pad_t, _pb, pad_l, _pr = (int(v) for v in geom[i])
        b = boxes[i, :c].astype(np.float64)
        if w >= h:
            xs = np.minimum(b[:, (0, 2)] * w / S, w)
            ys = np.minimum(np.maximum(b[:, (1, 3)] - pad_t, 0) * w / S, h)
        else:
            xs = np.minimum(np.maximum(b[:, (0, 2)] - pad_l, 0) * h / S, w)
            ys = np.minimum(b[:, (1, 3)] * h / S, h)
        rows[i, :c, 0] = xs[:, 0]; rows[i, :c, 1] = ys[:, 0]
        rows[i, :c, 2] = xs[:, 1] - xs[:, 0]; rows[i, :c, 3] = ys[:, 1] - ys[:, 0]
        rows[i, :c, 4] = np.minimum(score[i, :c], np.float32(1.0)).astype(np.float64)
    return rows, nrows


def _overlap(a1, a2, b1, b2):
    """yd.py:165-178 over arrays: the branch structure of evaluate._interval_overlap."""
    lo = np.where(b1 < a1, a1, b1)
    none = np.where(b1 < a1, b2 < a1, a2 < b1)
    return np.where(none, 0.0, np.minimum(a2, b2) - lo)


def iou_matrix(gt, det):
    """gt (G, 4), det (D, 4) as x, y, w, h -> (G, D) float64, bbox_iou's operations in order; a zero union divides as NumPy does
    (nan or +-inf), which is what fv_bbox_iou_pairs gives."""
    g = np.asarray(gt, np.float64).reshape(-1, 4); d = np.asarray(det, np.float64).reshape(-1, 4)
    gx0, gy0, gx1, gy1 = (v[:, None] for v in (g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]))
    dx0, dy0, dx1, dy1 = (v[None, :] for v in (d[:, 0], d[:, 1], d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]))
    with np.errstate(invalid='ignore', divide='ignore'):
        inter = _overlap(gx0, gx1, dx0, dx1) * _overlap(gy0, gy1, dy0, dy1)
        union = (gx1 - gx0) * (gy1 - gy0) + (dx1 - dx0) * (dy1 - dy0) - inter
        return inter / union


def match_image(gt, det):
    """evaluate.match_image on the matrix: -> ((D,) assigned IoU, -1 without one; flag).  Pairs with IoU > 0 in descending IoU
    order, equal IoUs by ground-truth index then detection index (the stable sort of the row-major pair list)."""
    m = iou_matrix(gt, det)
    out = np.full(m.shape[1], -1.0)
    with np.errstate(invalid='ignore'):
        gi, di = np.nonzero(m > 0.0)
    if len(gi) == 0:
        return out, 0
    v = m[gi, di]
    order = np.argsort(-v, kind='stable')
    used_g, used_d = set(), set()
    for k in order:
        i, j = int(gi[k]), int(di[k])
        if i in used_g or j in used_d:
            continue
        out[j] = v[k]
        used_g.add(i); used_d.add(j)
    return out, 1


def match_rows(rows, nrows, gt, gt_off):
    n = len(nrows)
    iou = np.full((n, ROWS), -1.0)
    flag = np.zeros(n, np.int32)
    for i in range(n):
        c = int(nrows[i])
        iou[i, :c], flag[i] = match_image(gt[gt_off[i]:gt_off[i + 1]], rows[i, :c, :4])
    return iou, flag


def compact(rows, nrows, iou, flag):
    """-> (conf, iou) of the detections that count: images with the flag, in image order then row order."""
    keep = [(rows[i, :nrows[i], 4], iou[i, :nrows[i]]) for i in range(len(nrows)) if flag[i] > 0]
    if not keep:
        return np.zeros(0), np.zeros(0)
    return np.concatenate([k[0] for k in keep]), np.concatenate([k[1] for k in keep])


def ap_sweep(conf, ious, iou_ths, gt_count):
    """-> (order (N,), counts (T, N), ap (T,), precision (T,), recall (T,)): np.argsort(-conf, kind='stable'), the inclusive running
    count of iou >= th, and the trapezoid sum of (r_k - r_{k-1}) * (p_k + p_{k-1}) / 2 with pr_curve's divisions."""
    N = len(conf)
    order = np.argsort(-conf, kind='stable')
    T = len(iou_ths)
    counts = np.zeros((T, N), np.int64)
    ap, prec, rec = np.zeros(T), np.zeros(T), np.zeros(T)
    for t, th in enumerate(iou_ths):
        tp = np.cumsum(ious[order] >= th)
        counts[t] = tp
        if N == 0:
            continue
        ps, rs = tp / np.arange(1, N + 1), tp / float(gt_count)
        ap[t] = trapezoid(ps, rs)
        prec[t], rec[t] = ps[-1], rs[-1]
    return order, counts, ap, prec, rec


def trapezoid(ps, rs):
    """The exact integral of the linear interpolant of (rs, ps) from rs[0] to rs[-1], term by term in float64."""
    if len(rs) < 2:
        return 0.0
    return float(np.sum((rs[1:] - rs[:-1]) * (ps[1:] + ps[:-1]) / 2.0))


def quad_with_error(ps, rs):
    """integrate_pr's SciPy calls on the same interpolant -> (value, quad's own absolute error estimate); (0, 0) where integrate_pr
    returns 0 without integrating."""
    from scipy.integrate import quad
    from scipy.interpolate import interp1d
    if len(rs) < 2 or rs[0] == rs[-1]:
        return 0.0, 0.0
    func = interp1d(rs, ps)
    v, err = quad(lambda x: func(x), rs[0], rs[-1])
    return float(v), float(err)


def loop_oracle_rows(seed):
    """The generator of tests/test_evaluate_cpu.py::test_matches_loop_oracle: -> (gt_rows, sol_rows) for its csv writer."""
    rng = np.random.default_rng(seed)
    gt_rows, sol_rows = [], []
    for k in range(40):
        name = 'img_%03d.jpg' % k
        n = int(rng.integers(1, 6))
        for _ in range(n):
            x, y = rng.uniform(1, 800, 2); w, h = rng.uniform(20, 120, 2)
            gt_rows.append((name, round(x, 1), round(y, 1), round(w, 1), round(h, 1)))
            if rng.random() < 0.8:
                j = rng.normal(0, 12, 4)
                sol_rows.append((name, x + j[0], y + j[1], max(w + j[2], 4), max(h + j[3], 4), rng.uniform(0.3, 1.0)))
        for _ in range(int(rng.integers(0, 4))):
            sol_rows.append((name, rng.uniform(1, 900), rng.uniform(1, 900), rng.uniform(10, 80), rng.uniform(10, 80), rng.uniform(0.1, 0.9)))
    sol_rows.append(('not_in_gt.jpg', 1, 1, 10, 10, 0.99))
    return gt_rows, sol_rows


def write_csv_pair(tmp_path, gt_rows, sol_rows):
    import os
    gt = os.path.join(tmp_path, 'validation.csv'); sol = os.path.join(tmp_path, 'solution_fd.csv')
    with open(gt, 'w') as f:
        f.write('FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT\n')
        for k, r in enumerate(gt_rows):
            f.write('%d,%s,%d,%s,%s,%s,%s\n' % (k, r[0], 1, r[1], r[2], r[3], r[4]))
    with open(sol, 'w') as f:
        for r in sol_rows:
            f.write('%s,%s,%s,%s,%s,%s\n' % tuple(r))
    return gt, sol


def golden_cases(tmp_path):
    """tests/golden/cal_map_fd.npz -> (case, gt csv, sol csv, thresholds, {th: (ps, rs, map)}) per case, the csv files written
    under tmp_path."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cal_map_fd.npz'))
    for ci in range(int(g['ncases'])):
        gt = os.path.join(str(tmp_path), 'gt%d.csv' % ci); sol = os.path.join(str(tmp_path), 'sol%d.csv' % ci)
        open(gt, 'wb').write(g['case%d_gt' % ci].tobytes()); open(sol, 'wb').write(g['case%d_sol' % ci].tobytes())
        want = {float(th): (g['case%d_th%g_ps' % (ci, th)], g['case%d_th%g_rs' % (ci, th)], float(g['case%d_th%g_map' % (ci, th)]))
                for th in g['thresholds']}
        yield ci, gt, sol, [float(th) for th in g['thresholds']], want


def frames_from_csv(gt_path, sol_path):
    """Two csv files -> (rows, nrows, gt, gt_off, gt_count) over the ground-truth images in sorted order, the layout the device
    calls take; an image's solution rows in file order."""
    import pandas as pd
    sol_df = pd.read_csv(sol_path, header=None)
    gt_df = pd.read_csv(gt_path)
    sol_groups = {k: v for k, v in sol_df.groupby(0, sort=True)}
    names, parts, offs = [], [], [0]
    for name, df in gt_df.groupby('FILE', sort=True):
        names.append(name)
        parts.append(df.iloc[:, 3:7].to_numpy(dtype=np.float64))
        offs.append(offs[-1] + len(df))
    rows = np.zeros((len(names), ROWS, 5)); nrows = np.zeros(len(names), np.int32)
    for i, name in enumerate(names):
        rel = sol_groups.get(name)
        if rel is not None:
            nrows[i] = len(rel)
            rows[i, :len(rel)] = rel.iloc[:, 1:6].to_numpy(dtype=np.float64)
    return rows, nrows, np.concatenate(parts).reshape(-1, 4), np.asarray(offs, np.int64), int(gt_df.shape[0])
