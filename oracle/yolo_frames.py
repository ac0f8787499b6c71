"""ORACLE -- test infrastructure only.

Random three-scale head outputs for the decode + per-class NMS tests (tests/test_yolo_postproc_cpu.py checks on the oracle
alone that every case holds what it claims; tests/test_yolo_postproc_gpu.py compares the kernels with the oracle on them),
and the diagnostics that show a frame has NMS work of the intended kind.
"""
import math

import numpy as np

from . import host_oracle

ANCHORS = ((116, 90, 156, 198, 373, 326), (30, 61, 62, 45, 59, 119), (10, 13, 16, 30, 33, 23))
KEPT = ((1,), (0, 2), (1,))


def slot_count(grid0):
    """Candidate slots of one image: 1 kept anchor at g, 2 at 2g, 1 at 4g."""
    return 25 * grid0 * grid0


def make_frame(rng, grid0, nclass, density, net_hw=(416, 416), centres=6, dup_cls=False, zero_prob=0.0, at_thresh=0.0,
               zero_area=0.0):
    """Three float32 head outputs (g,g,3*(5+nclass)), g = grid0, 2 grid0, 4 grid0.

    density: share of the kept-anchor slots whose objectness logit is high (+3 +- 0.5); the others sit at -6 +- 0.5, below any
    threshold used.  The hot slots are those nearest (with jitter) to `centres` random points, and a hot slot's box takes the
    size of its nearest centre (+- 10 %), so neighbouring boxes overlap heavily and chains of partial overlaps form at the
    rim of a cluster.  Class logits: N(0, 1.5), +3 on the centre's favourite class.
    dup_cls: class logits snapped to a palette of 6 values -> many candidates share a probability bit for bit.
    zero_prob: share of class logits set to -200 (probability exactly 0).
    at_thresh: share of hot slots with objectness logit exactly 0 (objectness exactly 0.5).
    zero_area: share of hot slots with t2 = t3 = -30 (integer corners collapse to one point)."""
    net_h, net_w = net_hw
    C = 5 + nclass
    cen = rng.uniform(0.15, 0.85, (centres, 2))
    size = rng.uniform(0.12, 0.4, (centres, 2))                  # w, h relative to the net
    fav = rng.integers(0, nclass, centres)
    # a slot's distance to its nearest centre, over all scales, to choose the hot ones
    info = []
    for s in range(3):
        g = grid0 << s
        rr, cc = np.meshgrid(np.arange(g), np.arange(g), indexing='ij')
        pos = np.stack([(cc + 0.5) / g, (rr + 0.5) / g], -1).reshape(-1, 1, 2)
        d = np.abs(pos - cen[None]).max(-1)                      # (cells, centres)
        info.append((d.argmin(1), d.min(1)))
    nslots = slot_count(grid0)
    nhot = int(round(density * nslots))
    score = np.concatenate([np.repeat(d, len(KEPT[s])) for s, (_, d) in enumerate(info)]) + rng.normal(0, 0.03, nslots)
    hot_all = np.zeros(nslots, bool)
    if nhot:
        hot_all[np.argsort(score, kind='stable')[:nhot]] = True
    outs = []
    o = 0
    for s in range(3):
        g = grid0 << s
        near = info[s][0]
        no = rng.normal(0, 1.0, (g * g, 3, C)).astype(np.float32)
        no[..., 4] = rng.normal(-6, 0.5, (g * g, 3))
        nk = len(KEPT[s])
        hot = hot_all[o:o + g * g * nk].reshape(g * g, nk); o += g * g * nk
        for j, b in enumerate(KEPT[s]):
            h = hot[:, j]
            n = int(h.sum())
            no[h, b, 4] = rng.normal(3, 0.5, n)
            sz = size[near[h]] * rng.uniform(0.9, 1.1, (n, 2))
            no[h, b, 2] = np.log(sz[:, 0] * net_w / ANCHORS[s][2 * b])
            no[h, b, 3] = np.log(sz[:, 1] * net_h / ANCHORS[s][2 * b + 1])
            cl = rng.normal(0, 1.5, (n, nclass))
            cl[np.arange(n), fav[near[h]]] += 3.0
            if dup_cls:
                cl = np.round(cl / 1.5).clip(-2, 3) * 1.5
            if zero_prob:
                cl[rng.random((n, nclass)) < zero_prob] = -200.0
            no[h, b, 5:] = cl
            if at_thresh:
                idx = np.nonzero(h)[0][rng.random(n) < at_thresh]
                no[idx, b, 4] = 0.0
            if zero_area:
                idx = np.nonzero(h)[0][rng.random(n) < zero_area]
                no[idx, b, 2] = -30.0; no[idx, b, 3] = -30.0
        outs.append(no.reshape(g, g, 3 * C))
    return outs


def exact_threshold_frame(nclass=1, grid0=13):
    """A sparse frame for a 416 x 416 image on a 416 net (identity correction), nms_thresh = 0.5: in six cells of scale 1 the two
    kept anchors hold concentric boxes whose corners fall on half pixels (centre at 16 c + 8.5, even sizes), so the integer
    boxes are known: three pairs 100 x 200 / 100 x 100 (IoU exactly 1/2: suppressed) and three pairs 100 x 202 / 100 x 100
    (IoU 100/202: kept); all corners are positive, so int() truncates them the same way.  Anchor 0 carries the larger class
    probability.  Returns (netouts, cells_exact, cells_below)."""
    assert grid0 == 13
    C = 5 + nclass
    outs = []
    for s in range(3):
        g = grid0 << s
        no = np.zeros((g, g, 3, C), np.float32)
        no[..., 4] = -8.0
        outs.append(no)
    t_c = np.float32(math.log((17 / 32) / (15 / 32)))            # sigmoid = 17/32: centre 16 (c + 17/32) = 16 c + 8.5
    cells_exact = [(7, 4), (7, 12), (7, 20)]
    cells_below = [(18, 4), (18, 12), (18, 20)]
    for cells, big_h in ((cells_exact, 200), (cells_below, 202)):
        for (r, c) in cells:
            for b, (w, h, cl) in ((0, (100, big_h, 4.0)), (2, (100, 100, 2.0))):
                v = outs[1][r, c, b]
                v[0] = t_c; v[1] = t_c
                v[2] = math.log(w / ANCHORS[1][2 * b]); v[3] = math.log(h / ANCHORS[1][2 * b + 1])
                v[4] = 5.0
                v[5:] = cl
    return [o.reshape(o.shape[0], o.shape[1], 3 * C) for o in outs], cells_exact, cells_below


# ----------------------------------------------------------------------------- the cases of the wrapper-level matrix
LANDSCAPE, PORTRAIT, SQUARE = (1440, 1920), (1920, 1440), (416, 416)      # image (h, w)
NET = (416, 416)
NET_NONSQUARE = (320, 416)                                                # (h, w): the grids stay square, as in the kernel


def _case(name, grid0, nclass, density, obj, nms, image, frames, net=NET, min_count=0, clustered=True, **knobs):
    return dict(name=name, grid0=grid0, nclass=nclass, density=density, obj_thresh=obj, nms_thresh=nms, image_hw=image, net_hw=net,
                frames=frames, min_count=min_count, clustered=clustered, knobs=knobs)


# grid0 3 / 7 / 10 / 13 reach the NMS widths 1024 / 2048 / 4096 / 8192 through the wrappers (capacity = 25 grid0^2).
# min_count: what the case claims about its candidate count; clustered: NMS must suppress >= 20 % and hold a chain.
CASES = [
    _case('g3_c4_few', 3, 4, 0.3, 0.5, 0.45, LANDSCAPE, 12, clustered=False),
    _case('g3_c1_all', 3, 1, 1.0, 0.3, 0.3, PORTRAIT, 12, min_count=225),
    _case('g3_c80', 3, 80, 0.5, 0.5, 0.45, SQUARE, 6, min_count=100),
    _case('g7_c4_300', 7, 4, 0.25, 0.5, 0.5, LANDSCAPE, 8, min_count=290),
    _case('g7_c1_dense', 7, 1, 1.0, 0.5, 0.45, PORTRAIT, 8, min_count=1025),
    _case('g7_c80', 7, 80, 0.25, 0.3, 0.3, SQUARE, 4, min_count=290),
    _case('g10_c4_dense', 10, 4, 0.9, 0.6, 0.7, SQUARE, 6, min_count=2049),
    _case('g10_c1_300', 10, 1, 0.12, 0.5, 0.5, PORTRAIT, 8, min_count=290),
    _case('g10_c80_1100', 10, 80, 0.45, 0.5, 0.45, LANDSCAPE, 3, min_count=1025),
    _case('g13_empty', 13, 4, 0.0, 0.5, 0.45, SQUARE, 4, clustered=False),
    _case('g13_few', 13, 4, 0.002, 0.5, 0.45, LANDSCAPE, 12, clustered=False),
    _case('g13_c80_300', 13, 80, 0.07, 0.5, 0.45, LANDSCAPE, 4, min_count=290),
    _case('g13_c80_1100', 13, 80, 0.27, 0.5, 0.5, SQUARE, 3, min_count=1025),
    _case('g13_c4_3000', 13, 4, 0.75, 0.5, 0.45, PORTRAIT, 6, min_count=3001),
    _case('g13_c1_all', 13, 1, 1.0, 0.3, 0.3, SQUARE, 6, min_count=4225),
    _case('g13_c4_all', 13, 4, 1.0, 0.5, 0.5, LANDSCAPE, 4, min_count=4225),
    _case('g13_c1_3500_hi', 13, 1, 0.85, 0.6, 0.7, PORTRAIT, 6, min_count=3001),
    _case('g13_ties', 13, 4, 0.08, 0.5, 0.45, SQUARE, 8, min_count=290, dup_cls=True),
    _case('g13_ties_dense', 13, 1, 0.4, 0.5, 0.5, PORTRAIT, 6, min_count=1025, dup_cls=True),
    _case('g13_zero_prob', 13, 4, 0.45, 0.5, 0.45, SQUARE, 6, min_count=1025, zero_prob=0.3),
    _case('g13_at_thresh', 13, 4, 0.1, 0.5, 0.45, LANDSCAPE, 8, min_count=290, at_thresh=0.2),
    _case('g13_zero_area', 13, 4, 0.3, 0.5, 0.45, SQUARE, 6, min_count=1025, zero_area=0.2),
    _case('net320x416_portrait', 13, 4, 0.3, 0.5, 0.45, PORTRAIT, 6, net=NET_NONSQUARE, min_count=1025),
    _case('net320x416_landscape', 13, 4, 0.3, 0.5, 0.45, LANDSCAPE, 6, net=NET_NONSQUARE, min_count=1025),
    _case('net320x416_square', 13, 1, 0.08, 0.3, 0.3, SQUARE, 6, net=NET_NONSQUARE, min_count=290),
    # grids past 13: 6400 slots at 16 (512 input), 9025 at 19 (608 input) of which the kernel holds 8192
    _case('g16_c4_300', 16, 4, 0.05, 0.5, 0.45, SQUARE, 4, net=(512, 512), min_count=290),
    _case('g16_c1_all', 16, 1, 1.0, 0.5, 0.5, (512, 512), 3, net=(512, 512), min_count=6400),
    _case('g19_c4_1500', 19, 4, 0.17, 0.5, 0.45, (608, 608), 3, net=(608, 608), min_count=1025),
    _case('g19_c1_8000', 19, 1, 0.89, 0.5, 0.5, (608, 608), 3, net=(608, 608), min_count=8000),
]


def case_frames(case):
    """The frames of a case, from a seed that depends on its name only."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    return [make_frame(rng, case['grid0'], case['nclass'], case['density'], net_hw=case['net_hw'], **case['knobs'])
            for _ in range(case['frames'])]


def case_oracle(case, netouts, capacity=None):
    return host_oracle.decode_frame(netouts, ANCHORS, case['obj_thresh'], case['nms_thresh'], case['net_hw'], case['image_hw'],
                                    capacity=capacity)


def case_report(case, netouts, capacity=None):
    return nms_report(netouts, case['obj_thresh'], case['nms_thresh'], case['net_hw'], case['image_hw'], capacity=capacity)


# ----------------------------------------------------------------------------- what a frame holds (on the oracle's output)
def nms_report(netouts, obj_thresh, nms_thresh, net_hw, image_hw, anchors=ANCHORS, capacity=None, max_probe=300):
    """Decode with and without NMS and count what the tests rely on."""
    pre = host_oracle.decode_frame(netouts, anchors, obj_thresh, nms_thresh, net_hw, image_hw, capacity=capacity, nms=False)
    post = host_oracle.decode_frame(netouts, anchors, obj_thresh, nms_thresh, net_hw, image_hw, capacity=capacity)
    bx = pre['boxes']
    n = len(bx)
    pos = pre['classes'] > 0
    rep = dict(count=n, positive=int(pos.sum()), max_positive_per_class=int(pos.sum(0).max()) if n else 0,
               suppressed=int((pos & (post['classes'] == 0)).sum()), chains=0, tie_pairs=0, exact_pairs=0, zero_union_pairs=0,
               zero_prob=int((pre['classes'] == 0).sum()), at_thresh=int((pre['objness'] == np.float32(obj_thresh)).sum()))
    area0 = np.nonzero((bx[:, 2] == bx[:, 0]) | (bx[:, 3] == bx[:, 1]))[0]
    for c in range(pre['classes'].shape[1] if n else 0):
        p0, p1 = pre['classes'][:, c], post['classes'][:, c]
        surv = np.nonzero(p1 > 0)[0]
        dead = np.nonzero((p0 > 0) & (p1 == 0))[0]
        # chains: a suppressed box that two survivors overlap at or above the threshold (one of them suppressed it; two
        # survivors never overlap each other that much, or the later one would be gone)
        for b in dead[:max_probe]:
            inter, uni = host_oracle.box_iou_int(bx[b], bx[surv])
            hit = host_oracle.suppresses(inter, uni, nms_thresh)
            rep['chains'] += int(hit.sum() >= 2)
            rep['exact_pairs'] += int(np.any((uni != 0) & (inter.astype(np.float64) / np.where(uni == 0, 1, uni) == nms_thresh)))
        # ties: pairs with the same positive probability, bit for bit, that overlap at or above the threshold
        live = np.nonzero(p0 > 0)[0]
        bits = p0[live].view(np.uint32)
        for v in np.unique(bits):
            grp = live[bits == v][:max_probe]
            if len(grp) < 2:
                continue
            inter, uni = host_oracle.box_iou_int(bx[grp][:, None, :], bx[grp][None, :, :])
            rep['tie_pairs'] += int(np.triu(host_oracle.suppresses(inter, uni, nms_thresh), 1).sum())
        z = np.intersect1d(area0, live)[:max_probe]
        if len(z) >= 2:
            inter, uni = host_oracle.box_iou_int(bx[z][:, None, :], bx[z][None, :, :])
            rep['zero_union_pairs'] += int(np.triu(uni == 0, 1).sum())
    return rep
