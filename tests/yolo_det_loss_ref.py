"""fv_yolo_det_loss_grad's contract (include/fv_hotpath.h) restated in torch on the CPU: float64 by default,
or with every operation in another dtype (the accuracy yardstick of the GIoU gradient).  The gradient comes from autograd; the
ignore mask is detached.  Shapes: y_s, t_s (B, g_s, g_s, 3*(5+ncls)), scale 0 = the coarsest grid first."""
import numpy as np
import torch
import torch.nn.functional as F

STATS = ('box', 'obj', 'noobj', 'cls', 'positives', 'ignored', 'iou_sum', 'iou_gt_50', 'iou_gt_75', 'max_count', 'dropped', 'spare')


def f32(v):
    """A configuration value as the C struct holds it (float32)."""
    return float(np.float32(v))


def bce(x, z):
    """max(x,0) - x z + log1p(e^-|x|) on the logit x; through logsigmoid, whose autograd is sigma(x) - z without cancellation
    and right at x = 0."""
    return -F.logsigmoid(-x) - x * z


def decode(v, s, image_size, anchors, clamp):
    """v (B,g,g,3,>=4) -> (cx, cy, w, h) in network pixels.  clamp: sizes from clamp(v, -20, 20), gradient 0 where |v| >= 20."""
    g = v.shape[1]
    cell = image_size // g
    col = torch.arange(g, dtype=v.dtype).view(1, 1, g, 1)
    row = torch.arange(g, dtype=v.dtype).view(1, g, 1, 1)
    aw = torch.tensor([anchors[s][2 * a] for a in range(3)], dtype=v.dtype).view(1, 1, 1, 3)
    ah = torch.tensor([anchors[s][2 * a + 1] for a in range(3)], dtype=v.dtype).view(1, 1, 1, 3)
    e2, e3 = v[..., 2], v[..., 3]
    if clamp:
        e2 = torch.where(e2.abs() < 20, e2, e2.detach().clamp(-20, 20))
        e3 = torch.where(e3.abs() < 20, e3, e3.detach().clamp(-20, 20))
    return torch.stack([(col + torch.sigmoid(v[..., 0])) * cell, (row + torch.sigmoid(v[..., 1])) * cell,
                        aw * torch.exp(e2), ah * torch.exp(e3)], -1)


def corners(b):
    return b[..., 0] - 0.5 * b[..., 2], b[..., 0] + 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 1] + 0.5 * b[..., 3]


def iou_parts(a, b):
    """-> I, U, and the (min, max) argument pairs whose ties the GPU test excludes."""
    x1, x2, y1, y2 = corners(a)
    X1, X2, Y1, Y2 = corners(b)
    iw = torch.minimum(x2, X2) - torch.maximum(x1, X1)
    ih = torch.minimum(y2, Y2) - torch.maximum(y1, Y1)
    inter = iw.clamp(min=0) * ih.clamp(min=0)
    union = a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter
    return inter, union, (x1, x2, y1, y2, X1, X2, Y1, Y2, iw, ih)


def iou(a, b):
    inter, union, _ = iou_parts(a, b)
    return inter / union


def giou(a, b):
    inter, union, (x1, x2, y1, y2, X1, X2, Y1, Y2, _, _) = iou_parts(a, b)
    c = (torch.maximum(x2, X2) - torch.minimum(x1, X1)) * (torch.maximum(y2, Y2) - torch.minimum(y1, Y1))
    return inter / union - (c - union) / c


def giou_tie_margin(a, b):
    """The smallest |difference| among the min / max argument pairs of GIoU(a, b) (and iw, ih against 0)."""
    _, _, (x1, x2, y1, y2, X1, X2, Y1, Y2, iw, ih) = iou_parts(a, b)
    return torch.stack([(x1 - X1).abs(), (x2 - X2).abs(), (y1 - Y1).abs(), (y2 - Y2).abs(), iw.abs(), ih.abs()], -1).min(-1).values


def gather(ts, image_size, ncls, anchors, max_boxes=None):
    """Per image: the boxes (n,4) float64 of the slots with t4 == 1 in slot order (scale, row, column, anchor), cut to max_boxes,
    and the true counts."""
    E = 5 + ncls
    B = ts[0].shape[0]
    lists = [[] for _ in range(B)]
    for s, t in enumerate(ts):
        t5 = torch.as_tensor(t).double().reshape(B, t.shape[1], t.shape[2], 3, E)
        boxes = decode(t5, s, image_size, anchors, clamp=False).reshape(B, -1, 4)
        flag = (t5[..., 4] == 1).reshape(B, -1)
        for b in range(B):
            lists[b].append(boxes[b][flag[b]])
    lists = [torch.cat(l, 0) for l in lists]
    counts = [int(l.shape[0]) for l in lists]
    if max_boxes is not None:
        lists = [l[:max_boxes] for l in lists]
    return lists, counts


def det_loss(ys, ts, image_size, ncls, conf, dtype=torch.float64, detail=False):
    """-> loss (a scalar of `dtype`, differentiable in ys), stats (12 floats) [, detail: per scale `best` of the unassigned slots,
    the assigned mask, GIoU tie margins of the assigned slots].  conf: data.det_loss_conf's dict (its floats as float32)."""
    E = 5 + ncls
    B = ys[0].shape[0]
    anchors = conf['anchors']
    thr, bw, nw = f32(conf['ignore_thresh']), f32(conf['box_weight']), f32(conf['noobj_weight'])
    max_boxes = int(conf['max_boxes'])
    lists, counts = gather([torch.as_tensor(t) for t in ts], image_size, ncls, anchors, max_boxes)
    M = max(1, max(l.shape[0] for l in lists))
    listed = torch.zeros((B, M, 4), dtype=dtype)
    valid = torch.zeros((B, M), dtype=torch.bool)
    for b, l in enumerate(lists):
        listed[b, :l.shape[0]] = l.to(dtype)
        valid[b, :l.shape[0]] = True
    listed[~valid] = torch.tensor([-1e6, -1e6, 1.0, 1.0], dtype=dtype)        # far away: IoU 0
    parts = [torch.zeros((), dtype=dtype) for _ in range(4)]
    npos = nign = n50 = n75 = 0
    iou_sum = 0.0
    bests, masks, margins, pos_ious = [], [], [], []
    for s, (y, t) in enumerate(zip(ys, ts)):
        g = y.shape[1]
        y5 = y.to(dtype).reshape(B, g, g, 3, E)
        t5 = torch.as_tensor(t).to(dtype).reshape(B, g, g, 3, E)
        pos = t5[..., 4] == 1
        pred = decode(y5, s, image_size, anchors, clamp=True)
        with torch.no_grad():
            best = iou(pred.detach().unsqueeze(-2), listed.view(B, 1, 1, 1, M, 4)).max(-1).values
            ignore = (best > thr) & ~pos
        noobj = nw * bce(y5[..., 4], torch.zeros_like(y5[..., 4]))
        parts[2] = parts[2] + noobj[~pos & ~ignore].sum()
        nign += int(ignore.sum())
        yp, tp = y5[pos], t5[pos]                                              # (n, E)
        gt = decode(t5, s, image_size, anchors, clamp=False)[pos]
        pb = pred[pos]
        parts[1] = parts[1] + bce(yp[:, 4], torch.ones_like(yp[:, 4])).sum()
        parts[3] = parts[3] + bce(yp[:, 5:], tp[:, 5:]).sum()
        if conf['box_loss'] == 'l2':
            sc = 2.0 - gt[:, 2] * gt[:, 3] / float(image_size * image_size)
            box = sc * (bce(yp[:, 0], torch.sigmoid(tp[:, 0])) + bce(yp[:, 1], torch.sigmoid(tp[:, 1]))) \
                + 0.5 * sc * ((yp[:, 2] - tp[:, 2]) ** 2 + (yp[:, 3] - tp[:, 3]) ** 2)
        else:
            assert conf['box_loss'] == 'giou'
            box = 1.0 - giou(pb, gt)
        parts[0] = parts[0] + bw * box.sum()
        with torch.no_grad():
            io = iou(pb, gt)
            npos += int(pos.sum()); iou_sum += float(io.sum()); n50 += int((io > 0.5).sum()); n75 += int((io > 0.75).sum())
            bests.append(best); masks.append(pos); margins.append(giou_tie_margin(pb, gt)); pos_ious.append(io)
    loss = (parts[0] + parts[1] + parts[2] + parts[3]) / B
    stats = [float(p.detach()) / B for p in parts] + [npos, nign, iou_sum, n50, n75, max(counts), sum(max(0, c - max_boxes) for c in counts), 0.0]
    if detail:
        return loss, stats, dict(best=bests, pos=masks, margin=margins, pos_iou=pos_ious)
    return loss, stats


def det_loss_grad(ys, ts, image_size, ncls, conf, loss_weight=1.0, dtype=torch.float64, detail=False):
    """-> loss (float), [dy_s (B,g,g,3*(5+ncls)) of `dtype`] = loss_weight * d loss / d y, stats [, detail]."""
    yv = [torch.as_tensor(y).to(dtype).clone().requires_grad_(True) for y in ys]
    out = det_loss(yv, ts, image_size, ncls, conf, dtype=dtype, detail=detail)
    grads = torch.autograd.grad(out[0], yv, allow_unused=True)
    grads = [(torch.zeros_like(y) if g is None else g) * loss_weight for g, y in zip(grads, yv)]
    return (float(out[0].detach()), grads) + tuple(out[1:])


# ----------------------------------------------------------------------------- planted inputs of the GPU tests
SPECIAL_LOGITS = (0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4)
PLAN = ((0, 0, 0, 0), (0, 0, 0, 2), (1, 1, 2, 1), (2, 3, 5, 0), (2, 6, 1, 2))     # (scale, row, column, anchor); two share a cell


def planted_case(image_size, counts, ncls, seed, anchors):
    """counts[b] boxes in image b (0..5), planted at PLAN's slots (a single box: at scale b % 3) -> ys, ts: lists of float32
    arrays (B, g, g, 3*(5+ncls)).  Targets: random offsets, sizes 0.2 .. 0.45 of the image, one class; an image with at least
    four boxes has tw = +30 in one and th = -30 in another.  Predictions: the assigned slots hold their target's box entries
    plus N(0, 0.3) jitter (so +-30 reaches the +-20 clamp); an unassigned slot imitates, with probability 0.9, the nearest box of its
    image as well as its cell allows, so that both sides of the ignore threshold occur; 35 % of all objectness and class logits
    are drawn from SPECIAL_LOGITS."""
    rng = np.random.default_rng(seed)
    S, E, B = image_size, 5 + ncls, len(counts)
    gs = [S // 32 << s for s in range(3)]
    ts = [np.zeros((B, g, g, 3, E), np.float32) for g in gs]
    ys = [rng.normal(0, 0.5, (B, g, g, 3, E)).astype(np.float32) for g in gs]
    logit = lambda p: np.log(p / (1.0 - p))
    for b, n in enumerate(counts):
        plan = [PLAN[(0, 2, 3)[b % 3]]] if n == 1 else PLAN[:n]
        boxes = []
        for k, (s, r, c, a) in enumerate(plan):
            cell = S // gs[s]
            size = rng.uniform(0.2, 0.45, 2) * S
            t = ts[s][b, r, c, a]
            t[0:2] = rng.normal(0, 1, 2)
            t[2] = np.log(size[0] / anchors[s][2 * a]); t[3] = np.log(size[1] / anchors[s][2 * a + 1])
            t[4] = 1.0
            t[5 + int(rng.integers(ncls))] = 1.0
            if n >= 4 and k == 1:
                t[2] = 30.0
            elif n >= 4 and k == 2:
                t[3] = -30.0
            else:
                sg = 1.0 / (1.0 + np.exp(-t[0:2].astype(np.float64)))
                boxes.append(((c + sg[0]) * cell, (r + sg[1]) * cell, size[0], size[1]))
            ys[s][b, r, c, a, 0:4] = t[0:4] + rng.normal(0, 0.3, 4)
        for s, g in enumerate(gs):
            cell = S // g
            for r in range(g):
                for c in range(g):
                    for a in range(3):
                        if ts[s][b, r, c, a, 4] == 1.0 or not boxes or rng.random() >= 0.9:
                            continue
                        cx, cy, w, h = min(boxes, key=lambda q: abs(q[0] - (c + 0.5) * cell) + abs(q[1] - (r + 0.5) * cell))
                        y = ys[s][b, r, c, a]
                        y[0] = logit(min(max(cx / cell - c, 0.05), 0.95)) + rng.normal(0, 0.2)
                        y[1] = logit(min(max(cy / cell - r, 0.05), 0.95)) + rng.normal(0, 0.2)
                        y[2] = np.log(w / anchors[s][2 * a]) + rng.normal(0, 0.15)
                        y[3] = np.log(h / anchors[s][2 * a + 1]) + rng.normal(0, 0.15)
    for y in ys:
        tail = y[..., 4:]
        pick = rng.random(tail.shape) < 0.35
        tail[pick] = rng.choice(np.asarray(SPECIAL_LOGITS, np.float32), int(pick.sum()))
    return [y.reshape(B, g, g, 3 * E) for y, g in zip(ys, gs)], [t.reshape(B, g, g, 3 * E) for t, g in zip(ts, gs)]
