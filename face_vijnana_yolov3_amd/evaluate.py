"""Detection accuracy of FaceDetector.evaluate's output: the reference's `cal_mAP_fd`
(evaluate.py:27-127) and the IoU-threshold sweep of its `main` (evaluate.py:337-355); identification accuracy of
FaceIdentifier.test's output: `cal_acc_fi` (evaluate.py:225-329) and its sweep (evaluate.py:362-387); face verification:
`cal_face_pairs_dists` and `cal_VAL_FAR` (evaluate.py:129-223), whose pair distances run on the device (fv_fid_pair_dists,
DESIGN.md section 15).

The detection / identification metrics are host code, as in the reference (pandas/NumPy/SciPy on a few thousand boxes);
cal_mAP_sweep_device is the detection metric with everything after the csv parsing on the device (det_metric.py, DESIGN.md
section 28), the form FaceDetector.validate runs per epoch.  What they restate, line by line:

* solution csv (no header): FILE, x, y, w, h, confidence  -- what `FaceDetector.evaluate` writes
  (face_detection.py:733-737); ground truth csv (header): FACE_ID, FILE, SUBJECT_ID, FACE_X,
  FACE_Y, FACE_WIDTH, FACE_HEIGHT.  Boxes are (x, y, x + w, y + h) (evaluate.py:50-53, 61-64).
* per image: IoU of every (gt, detection) pair with `bbox_iou` (yd.py:165-194; pairs with IoU <= 0
  are dropped, evaluate.py:67), greedy one-to-one assignment in descending IoU order
  (evaluate.py:81-95); a detection's IoU is that of its assigned gt, -1 if it got none;
* images without detections, and images where no (gt, detection) pair overlaps, are skipped -- their
  detections never enter the result, false positives included (evaluate.py:43-47, 77); neither do
  detections on images that are not in the ground truth (the loop runs over ground-truth images);
* detections sorted by confidence, descending (evaluate.py:104); precision / recall after each one
  with TP = "IoU >= iou_th" and the recall denominator = ALL ground-truth rows (evaluate.py:108-119);
* mAP = integral of the linear interpolant precision(recall) from rs[0] to rs[-1]
  (`interp1d` + `quad`, evaluate.py:124-125) -- the same SciPy calls are made here.

Parity unpinned: the reference function cannot be executed -- `sol_df.iat[:, 6] = -1.0`
(evaluate.py:31, 36) raises "iAt based indexing can only have integer indexers" in every pandas
release, so no golden vectors can be minted; `bbox_iou` itself is pinned (tests/golden/iou_cases.npz).
Two places where the committed text is ill-defined are resolved as follows: (1) the initial IoU of an
unmatched detection is the -1.0 those two lines try to assign; (2) `res_df` is assigned at loop index
k == 0 only (evaluate.py:97-100), which raises NameError when the first ground-truth image has no
detections -- here results are simply collected over all images.  Ties in IoU / confidence keep file
order (stable sorts; the reference's `sort_values` default is not stable)."""
import numpy as np


def _interval_overlap(a1, a2, b1, b2):
    """yd.py:165-178 with its branch structure (the result may be negative for touching boxes)."""
    if b1 < a1:
        return 0 if b2 < a1 else min(a2, b2) - a1
    return 0 if a2 < b1 else min(a2, b2) - b1


def bbox_iou_xyxy(b1, b2):
    """yd.py:183-194 on (xmin, ymin, xmax, ymax) tuples; ZeroDivisionError/nan behaviour not reproduced:
    a zero union gives nan."""
    iw = _interval_overlap(b1[0], b1[2], b2[0], b2[2])
    ih = _interval_overlap(b1[1], b1[3], b2[1], b2[3])
    inter = iw * ih
    union = (b1[2] - b1[0]) * (b1[3] - b1[1]) + (b2[2] - b2[0]) * (b2[3] - b2[1]) - inter
    return float(inter) / union if union != 0 else float('nan')


def iou_matrix_device(ctx, gt_boxes, det_boxes):
    """All (gt, detection) IoUs of one or many images in ONE kernel launch (fv_bbox_iou_pairs): gt_boxes (n,4),
    det_boxes (m,4) as x, y, w, h -> (n, m) float64, bit-identical to bbox_iou_xyxy on the same pairs."""
    import torch
    from ._lib import lib, ptr
    g = np.asarray(gt_boxes, np.float64).reshape(-1, 4); d = np.asarray(det_boxes, np.float64).reshape(-1, 4)
    n, m = len(g), len(d)
    if n == 0 or m == 0:
        return np.zeros((n, m))
    gx = np.stack([g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]], 1)
    dx = np.stack([d[:, 0], d[:, 1], d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]], 1)
    dev = torch.device('cuda', ctx.device)
    a = torch.from_numpy(np.repeat(gx, m, axis=0)).to(dev); b = torch.from_numpy(np.tile(dx, (n, 1))).to(dev)
    out = torch.empty(n * m, dtype=torch.float64, device=dev)
    ctx.check(lib().fv_bbox_iou_pairs(ctx.handle, ptr(a), ptr(b), n * m, ptr(out)), 'fv_bbox_iou_pairs')
    return out.cpu().numpy().reshape(n, m)


def match_image(gt_boxes, det_boxes, ctx=None):
    """Greedy assignment of one image (evaluate.py:46-95).  gt_boxes (n,4), det_boxes (m,4) as
    x, y, w, h.  Returns the (m,) IoU assigned to each detection (-1 = unmatched), or None when no pair
    overlaps (the reference then drops the image's detections, false positives included).  ctx: an fv
    Context -> the pair IoUs come from the device kernel (same values)."""
    out = np.full(len(det_boxes), -1.0)
    pairs = []
    if ctx is not None:
        with np.errstate(invalid='ignore'):
            m = iou_matrix_device(ctx, gt_boxes, det_boxes)
            pairs = [(int(i), int(j), float(m[i, j])) for i, j in zip(*np.nonzero(m > 0.))]
    for i, g in enumerate(gt_boxes if ctx is None else []):
        gb = (g[0], g[1], g[0] + g[2], g[1] + g[3])
        for j, d in enumerate(det_boxes):
            iou = bbox_iou_xyxy(gb, (d[0], d[1], d[0] + d[2], d[1] + d[3]))
            if iou > 0.:
                pairs.append((i, j, iou))
    if not pairs:
        return None                           # evaluate.py:77: the image then contributes nothing at all
    pairs.sort(key=lambda t: -t[2])          # stable: ties keep (gt, detection) order
    used_g, used_d = set(), set()
    for i, j, iou in pairs:
        if i in used_g or j in used_d:
            continue
        out[j] = iou
        used_g.add(i); used_d.add(j)
    return out


def detection_ious(gt_df, sol_df, ctx=None):
    """-> (confidences, assigned IoUs) of every detection on a ground-truth image that has detections,
    in ground-truth image order (evaluate.py:39-101)."""
    sol_groups = {k: v for k, v in sol_df.groupby(0, sort=True)}
    conf, ious = [], []
    for image_id, df in gt_df.groupby('FILE', sort=True):
        rel = sol_groups.get(image_id)
        if rel is None or len(rel) == 0:
            continue
        iou = match_image(df.iloc[:, 3:7].to_numpy(dtype=np.float64), rel.iloc[:, 1:5].to_numpy(dtype=np.float64), ctx)
        if iou is None:
            continue
        conf.append(rel.iloc[:, 5].to_numpy(dtype=np.float64))
        ious.append(iou)
    if not conf:
        return np.zeros(0), np.zeros(0)
    return np.concatenate(conf), np.concatenate(ious)


def pr_curve(conf, ious, gt_count, iou_th):
    """evaluate.py:104-122."""
    order = np.argsort(-conf, kind='stable')
    tp = np.cumsum(ious[order] >= iou_th)
    n = np.arange(1, len(order) + 1)
    return tp / n, tp / float(gt_count)


def integrate_pr(ps, rs):
    """evaluate.py:124-125: quad over the linear interpolant of (rs, ps)."""
    from scipy.integrate import quad
    from scipy.interpolate import interp1d
    if len(rs) < 2 or rs[0] == rs[-1]:
        return 0.0
    func = interp1d(rs, ps)
    return quad(lambda x: func(x), rs[0], rs[-1])[0]


def cal_mAP_fd(gt_path, sol_path, iou_th, ctx=None):
    """-> (ps, rs, mAP) exactly as the reference's signature (evaluate.py:27, 127); ctx: optional fv Context
    (pair IoUs on the device)."""
    import pandas as pd
    sol_df = pd.read_csv(sol_path, header=None)
    gt_df = pd.read_csv(gt_path)
    conf, ious = detection_ious(gt_df, sol_df, ctx)
    ps, rs = pr_curve(conf, ious, gt_df.shape[0], iou_th)
    return ps, rs, integrate_pr(ps, rs)


def cal_mAP_sweep(gt_path, sol_path, iou_ths=None):
    """The sweep of evaluate.py:337-347 (IoU 0.50 ... 0.95): -> list of (iou_th, mAP) and their mean
    (the README's "mAP" is the mean of AP50..AP95).  The matching does not depend on the threshold and
    is done once."""
    import pandas as pd
    iou_ths = np.arange(0.5, 1.0, 0.05) if iou_ths is None else iou_ths
    sol_df = pd.read_csv(sol_path, header=None)
    gt_df = pd.read_csv(gt_path)
    conf, ious = detection_ious(gt_df, sol_df)
    res = []
    for th in iou_ths:
        ps, rs = pr_curve(conf, ious, gt_df.shape[0], th)
        res.append((float(th), integrate_pr(ps, rs)))
    return res, float(np.mean([m for _, m in res])) if res else 0.0


def sweep_device(gt_path, sol_path, iou_ths=None, ctx=None, want_curve=False):
    """cal_mAP_sweep's metric with everything after the csv parsing on the device (det_metric.py: fv_det_match_rows, one
    fv_det_ap_sweep) -> dict: iou_ths, ap, mean_ap, precision, recall (final), n_det and, with want_curve, ps / rs: one float64
    array per threshold, rebuilt from the device's ranking and running counts with pr_curve's two divisions.  AP is the trapezoid sum
    over the (recall, precision) points -- the exact integral of the interpolant integrate_pr hands to quad.  An image with more
    than 60 solution rows (FaceDetector.evaluate never writes more) or more than 4096 ground-truth rows is a ValueError naming the
    file."""
    import pandas as pd
    import torch
    from . import det_metric
    from ._lib import Context
    iou_ths = np.arange(0.5, 1.0, 0.05) if iou_ths is None else np.asarray(iou_ths, np.float64)
    sol_df = pd.read_csv(sol_path, header=None)
    gt_df = pd.read_csv(gt_path)
    names = sorted(gt_df['FILE'].unique())
    boxes, offs, max_gt = det_metric.group_ground_truth(gt_df, names, gt_path)
    sol_groups = {k: v for k, v in sol_df.groupby(0, sort=True)}
    rows = np.zeros((len(names), det_metric.ROWS, 5), np.float64)
    nrows = np.zeros(len(names), np.int32)
    for i, name in enumerate(names):
        rel = sol_groups.get(name)
        if rel is None:
            continue
        if len(rel) > det_metric.ROWS:
            raise ValueError('%s: %d rows for %s (the device metric takes at most %d per image)' % (sol_path, len(rel), name, det_metric.ROWS))
        nrows[i] = len(rel)
        rows[i, :len(rel)] = rel.iloc[:, 1:6].to_numpy(dtype=np.float64)
    ctx = ctx if ctx is not None else Context(0)
    dev = torch.device('cuda', ctx.device)
    d_rows, d_nrows = torch.from_numpy(rows).to(dev), torch.from_numpy(nrows).to(dev)
    iou, flag = det_metric.match_rows(ctx, d_rows, d_nrows, torch.from_numpy(boxes).to(dev), torch.from_numpy(offs).to(dev), max_gt)
    out = det_metric.ap_sweep(ctx, d_rows, d_nrows, iou, flag, iou_ths, gt_df.shape[0], want_curve=want_curve)
    n = int(out['n_det'].cpu()[0])
    res = det_metric.summarise(iou_ths, out['result'].cpu().numpy(), n)
    if want_curve:
        counts = out['counts'][:, :n].cpu().numpy()
        res['order'] = out['order'][:n].cpu().numpy()
        res['ps'] = [c / np.arange(1, n + 1) for c in counts]
        res['rs'] = [c / float(gt_df.shape[0]) for c in counts]
    return res


def cal_mAP_sweep_device(gt_path, sol_path, iou_ths=None, ctx=None):
    """cal_mAP_sweep with the matching, the ranking and the precision / recall sweep on the device (sweep_device): -> list of
    (iou_th, mAP) and their mean.  ctx: an fv Context (default: device 0)."""
    r = sweep_device(gt_path, sol_path, iou_ths, ctx)
    return [(t, m) for t, m in zip(r['iou_ths'], r['ap'])], r['mean_ap']


def acc_fi_image(gt_sids, gt_boxes, det_sids, det_boxes):
    """The greedy assignment of one ground-truth image that has detections (evaluate.py:246-304): pairs with IoU > 0, taken in
    descending IoU order (ties: gt, then detection order), each gt and detection at most once -> (assigned [(i, j, iou)],
    unassigned gt indices, unassigned detection indices), or None when no pair overlaps (the image then counts nothing,
    evaluate.py:275).  gt_sids / det_sids: subject ids (-1 = unknown); boxes (n,4) as x, y, w, h."""
    pairs = []
    for i, g in enumerate(gt_boxes):
        gb = (g[0], g[1], g[0] + g[2], g[1] + g[3])
        for j, d in enumerate(det_boxes):
            iou = bbox_iou_xyxy(gb, (d[0], d[1], d[0] + d[2], d[1] + d[3]))
            if iou > 0.:
                pairs.append((i, j, iou))
    if not pairs:
        return None
    pairs.sort(key=lambda t: -t[2])          # stable
    used_g, used_d, assigned = set(), set(), []
    for i, j, iou in pairs:
        if i in used_g or j in used_d:
            continue
        assigned.append((i, j, iou))
        used_g.add(i); used_d.add(j)
    return assigned, [i for i in range(len(gt_boxes)) if i not in used_g], [j for j in range(len(det_boxes)) if j not in used_d]


def cal_acc_fi(gt_path, sol_path, iou_th):
    """The reference's cal_acc_fi (evaluate.py:225-329) -> (tp, fp, tn, fn, acc), acc = (tp + tn) / (tp + tn + fp + fn).
    Solution csv (no header): FILE, SUBJECT_ID, x, y, w, h, score (FaceIdentifier.test); ground truth as cal_mAP_fd.  Per
    ground-truth image (sorted): without detections every gt row is tn (SUBJECT_ID -1) or fn; otherwise the greedy assignment of
    acc_fi_image, an assigned pair counting tp when IoU >= iou_th and both ids are the same known subject, fp when IoU >= iou_th,
    the detection is known and the ids differ, else tn when the gt is unknown, else fn.  Detections on images outside the
    ground truth are not counted."""
    import pandas as pd
    sol_df = pd.read_csv(sol_path, header=None)
    gt_df = pd.read_csv(gt_path)
    sol_groups = {k: v for k, v in sol_df.groupby(0, sort=True)}
    tp = fp = tn = fn = 0
    for image_id, df in gt_df.groupby('FILE', sort=True):
        g_sid = df.iloc[:, 2].to_numpy()
        rel = sol_groups.get(image_id)
        if rel is None:
            tn += int(np.sum(g_sid == -1)); fn += int(np.sum(g_sid != -1))
            continue
        d_sid = rel.iloc[:, 1].to_numpy()
        res = acc_fi_image(g_sid, df.iloc[:, 3:7].to_numpy(dtype=np.float64), d_sid, rel.iloc[:, 2:6].to_numpy(dtype=np.float64))
        if res is None:
            continue
        assigned, free_g, free_d = res
        for i, j, iou in assigned:
            if iou >= iou_th and g_sid[i] != -1 and d_sid[j] != -1 and g_sid[i] == d_sid[j]:
                tp += 1
            elif iou >= iou_th and d_sid[j] != -1 and g_sid[i] != d_sid[j]:
                fp += 1
            elif g_sid[i] == -1:
                tn += 1
            else:
                fn += 1
        for i in free_g:
            if g_sid[i] == -1:
                tn += 1
            else:
                fn += 1
        for j in free_d:
            if d_sid[j] == -1:
                tn += 1
            else:
                fp += 1
    acc = (tp + tn) / (tp + tn + fp + fn)
    return tp, fp, tn, fn, acc


def cal_acc_fi_sweep(gt_path, sol_path, iou_ths=None):
    """The sweep of evaluate.py:362-387 (IoU 0.50 ... 0.95): -> list of (iou_th, tp, fp, tn, fn, acc)."""
    iou_ths = np.arange(0.5, 1.0, 0.05) if iou_ths is None else iou_ths
    return [(float(th),) + tuple(cal_acc_fi(gt_path, sol_path, th)) for th in iou_ths]


# ----------------------------------------------------------------------------- face verification (evaluate.py:129-223)
SIM_TH_RANGE = np.arange(0.1, 1.1, 0.1)      # main's cal_VAL_FAR thresholds (evaluate.py:359)


def face_pairs(db_csv=None, resource_type='uccs'):
    """The pair sets of cal_face_pairs_dists (evaluate.py:129-194) as a block table over one facial-ID matrix.  Reads the subject
    db (default: db_files(resource_type)'s csv), groups it by subject_id (sorted keys, -1 included in the list the random draw
    indexes) and draws the different-identity subject pairs with np.random.choice(range(S), size=(S // 2, 2), replace=False) from
    NumPy's global RandomState, exactly as the reference.  -> dict:
      names    face files in matrix-row order: every known subject's files (csv order), subjects in key order;
      blocks   (k, 6) int64 rows (a0, na, b0, nb, out_off, kind) for fv_fid_pair_dists: one i < j triangle per subject with >= 2
               files (out_off into same_dists), then one rectangle per drawn pair without -1 (out_off into diff_dists, offset by
               n_same: one buffer holds both);
      n_same, n_diff, subject_ids, draw (the (S // 2, 2) array np.random.choice returned)."""
    import pandas as pd
    from .face_identification import PAIR_RECTANGLE, PAIR_TRIANGLE, db_files
    db = pd.read_csv(db_files(resource_type)[0] if db_csv is None else db_csv).iloc[:, 1:]
    groups = {k: list(df.iloc[:, 1]) for k, df in db.groupby('subject_id')}
    subject_ids = list(groups.keys())
    names, start = [], {}
    for sid in subject_ids:
        if sid == -1:
            continue
        start[sid] = len(names)
        names += groups[sid]
    blocks, off = [], 0
    for sid in subject_ids:                           # evaluate.py:143-159
        n = len(groups[sid])
        if sid == -1 or n < 2:
            continue
        blocks.append((start[sid], n, start[sid], n, off, PAIR_TRIANGLE))
        off += n * (n - 1) // 2
    n_same = off
    draw = np.random.choice(range(len(subject_ids)), size=(len(subject_ids) // 2, 2), replace=False)   # evaluate.py:164-166
    for k, l in draw:                                 # evaluate.py:170-187
        sk, sl = subject_ids[k], subject_ids[l]
        if sk == -1 or sl == -1:
            continue
        nk, nl = len(groups[sk]), len(groups[sl])
        blocks.append((start[sk], nk, start[sl], nl, off, PAIR_RECTANGLE))
        off += nk * nl
    return {'names': names, 'blocks': np.asarray(blocks, np.int64).reshape(-1, 6), 'n_same': n_same, 'n_diff': off - n_same,
            'subject_ids': subject_ids, 'draw': draw}


def gather_facial_ids(names, h5_path):
    """The float32 (len(names), 64) matrix of the facial IDs of subject_facial_ids.h5 (FaceIdentifier.make_facial_ids_db), in
    `names` order; a file missing from the h5 raises KeyError, as the reference's f[name] does."""
    from .face_identification import DENSE1_DIM, read_facial_ids_h5
    fids = read_facial_ids_h5(h5_path)
    out = np.zeros((len(names), DENSE1_DIM), np.float32)
    for r, name in enumerate(names):
        out[r] = fids[name][0]
    return out


def face_pair_dists_device(pairs, ids, thresholds, materialise=True, ctx=None):
    """One fv_fid_pair_dists launch over face_pairs()'s table: -> (same_dists, diff_dists) float32 arrays (None, None when not
    materialise: no distance buffer exists on the device or the host) and counts (2, n_th) int64, counts[0][t] / counts[1][t] the
    same / different pairs with float32 distance <= thresholds[t] (ascending float32)."""
    import torch
    from ._lib import Context
    from .face_identification import fid_pair_dists
    n_same, n_diff = pairs['n_same'], pairs['n_diff']
    th = np.asarray(thresholds, np.float32).reshape(-1)
    if n_same + n_diff == 0:
        empty = np.zeros(0, np.float32)
        return (empty, empty) if materialise else (None, None), np.zeros((2, len(th)), np.int64)
    ctx = ctx if ctx is not None else Context(0)
    x = torch.from_numpy(np.ascontiguousarray(ids, np.float32)).to(torch.device('cuda', ctx.device))
    d, c = fid_pair_dists(ctx, x, pairs['blocks'], th, n_dists=(n_same + n_diff) if materialise else None)
    counts = c.cpu().numpy()
    if not materialise:
        return (None, None), counts
    d = d.cpu().numpy()
    return (d[:n_same].copy(), d[n_same:].copy()), counts


def _run_pairs(resource_type, thresholds, materialise, ctx):
    from .face_identification import db_files
    db_csv, _faces, h5, _pickle = db_files(resource_type)
    pairs = face_pairs(db_csv)
    ids = gather_facial_ids(pairs['names'], h5)
    return pairs, face_pair_dists_device(pairs, ids, thresholds, materialise, ctx)


def write_face_pairs_dists(path, same_dists, diff_dists):
    """face_pairs_dists.h5 (evaluate.py:191-193): float32 same_dists and diff_dists."""
    from .hdf5_lite import write_hdf5
    write_hdf5(path, {'/same_dists': np.asarray(same_dists, np.float32), '/diff_dists': np.asarray(diff_dists, np.float32)})


def cal_face_pairs_dists(resource_type='uccs', ctx=None):
    """The reference's cal_face_pairs_dists (evaluate.py:129-194) in the current directory: subject_image_db.csv and
    subject_facial_ids.h5 (vggface2: db_files' names) -> every same-identity pair and the different-identity pairs of the random
    subject draw, on the device (fv_fid_pair_dists); writes face_pairs_dists.h5 and returns (same_dists, diff_dists), float32 in
    the reference's order.  Distances are fp64 sums rounded once to float32 (the reference: scipy.linalg.norm of the float32
    difference, snrm2), within 1 float32 ulp of it."""
    _pairs, ((same, diff), _counts) = _run_pairs(resource_type, [np.inf], True, ctx)
    write_face_pairs_dists('face_pairs_dists.h5', same, diff)
    return same, diff


def val_far(counts, n_same, n_diff):
    """VAL and FAR of evaluate.py:205-214 from pair counts: count / number of pairs, float64 (NaN for an empty pair set)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return (np.asarray(counts[0], np.float64) / np.float64(n_same), np.asarray(counts[1], np.float64) / np.float64(n_diff))


def cal_VAL_FAR(sim_th_range, counts_only=False, resource_type='uccs', ctx=None):
    """The reference's cal_VAL_FAR (evaluate.py:196-223) -> (sim_ths, vals, fars) float64: VAL / FAR = share of the same /
    different pairs with float32(distance) <= float32(threshold) (what `float32 array <= float64 scalar` compares under NumPy < 2),
    the counts taken from the launch that computes the distances.  Writes face_pairs_dists.h5 (as cal_face_pairs_dists) and
    val_far.h5 (sim_ths, vals, fars -- the reference writes the builtin `vars` as vals, a bug not reproduced).  counts_only: no
    distance array anywhere and no face_pairs_dists.h5 (the path for VGGFace2, where the two arrays are several GB)."""
    from .hdf5_lite import write_hdf5
    sim_ths = np.asarray(list(sim_th_range), np.float64).reshape(-1)
    th32 = sim_ths.astype(np.float32)
    uniq = np.unique(th32[~np.isnan(th32)])                # the kernel takes ascending thresholds; NaN counts nothing
    if len(uniq) > 4096:
        raise ValueError('cal_VAL_FAR takes at most 4096 distinct float32 thresholds, got %d' % len(uniq))
    pairs, ((same, diff), counts) = _run_pairs(resource_type, uniq if len(uniq) else [np.inf], not counts_only, ctx)
    if not counts_only:
        write_face_pairs_dists('face_pairs_dists.h5', same, diff)
    full = np.zeros((2, len(sim_ths)), np.int64)
    ok = ~np.isnan(th32)
    full[:, ok] = counts[:, np.searchsorted(uniq, th32[ok])]
    vals, fars = val_far(full, pairs['n_same'], pairs['n_diff'])
    write_hdf5('val_far.h5', {'/sim_ths': sim_ths, '/vals': vals, '/fars': fars})
    return sim_ths, vals, fars


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='Face detection / identification / verification metrics (reference evaluate.py)')
    ap.add_argument('--mode', default='cal_map_fd', help='cal_map_fd, cal_acc_fi, cal_face_pairs_dists or cal_VAL_FAR')
    ap.add_argument('--gt_path', help='ground-truth csv (cal_map_fd, cal_acc_fi)')
    ap.add_argument('--sol_path', help='solution csv (cal_map_fd, cal_acc_fi)')
    ap.add_argument('--seed', type=int, default=None, help='np.random.seed before the random subject draw (verification modes)')
    ap.add_argument('--resource_type', default='uccs', help='uccs or vggface2: which subject db / facial-ID h5 (verification modes)')
    ap.add_argument('--device', action='store_true', help='cal_map_fd: matching, ranking and the sweep on the GPU (cal_mAP_sweep_device)')
    ap.add_argument('--counts_only', action='store_true', help='cal_VAL_FAR without the distance arrays (no face_pairs_dists.h5)')
    a = ap.parse_args(argv)
    if a.mode in ('cal_face_pairs_dists', 'cal_VAL_FAR'):
        if a.seed is not None:
            np.random.seed(a.seed)
        if a.mode == 'cal_face_pairs_dists':
            same, diff = cal_face_pairs_dists(a.resource_type)
            print('same pairs', len(same), 'different pairs', len(diff))
            return
        sim_ths, vals, fars = cal_VAL_FAR(SIM_TH_RANGE, counts_only=a.counts_only, resource_type=a.resource_type)
        for th, v, f in zip(sim_ths, vals, fars):
            print('{0:1.2f}'.format(th), v, f)
        return
    if a.mode not in ('cal_map_fd', 'cal_acc_fi'):
        raise SystemExit('unknown mode %r: cal_map_fd, cal_acc_fi, cal_face_pairs_dists and cal_VAL_FAR are implemented here'
                         % a.mode)
    if a.gt_path is None or a.sol_path is None:
        ap.error('--gt_path and --sol_path are required for --mode %s' % a.mode)
    if a.mode == 'cal_acc_fi':
        from .hdf5_lite import write_hdf5
        res = cal_acc_fi_sweep(a.gt_path, a.sol_path)
        for r in res:
            print('{0:1.2f}'.format(r[0]), r[1], r[2], r[3], r[4], r[5])
        cols = np.asarray([r[1:] for r in res], dtype=np.float64).reshape(-1, 5)
        write_hdf5('fi_acc.h5', {'/tp_ls': cols[:, 0].astype(np.int64), '/fp_ls': cols[:, 1].astype(np.int64),
                                 '/tn_ls': cols[:, 2].astype(np.int64), '/fn_ls': cols[:, 3].astype(np.int64),
                                 '/acc_ls': cols[:, 4]})          # evaluate.py:382-387
        return
    res, mean = (cal_mAP_sweep_device if a.device else cal_mAP_sweep)(a.gt_path, a.sol_path)
    for th, m in res:
        print('{0:1.2f}'.format(th), m)
    print('mean', mean)


if __name__ == '__main__':
    main()
