"""The oracle side of the three-scale decode + per-class NMS tests (tests/test_yolo_postproc_gpu.py), on the CPU: the array
form of the chain against the loop form that the reference-minted goldens pin, and the proof that every generated case
holds what it claims -- so that a change of a generator cannot quietly empty a case."""

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import yolo_frames as yf
from test_oracle_golden import GOLDEN_CASES, load_decode_case

MAX_EXCLUDED = 0.01          # share of the frames of one test that fragile() may leave out


def _loop_chain(netouts, anchors, obj, nms, net_hw, image_hw, exp, run_nms=True):
    rows = []
    for s in range(3):
        rows += ho.decode_netout(netouts[s], list(anchors[s]), s, obj, net_hw[0], net_hw[1], exp=exp)
    ho.correct_yolo_boxes(rows, image_hw[0], image_hw[1], net_hw[0], net_hw[1])
    if run_nms:
        ho.do_nms(rows, nms)
    a = np.array(rows, np.float64).reshape(len(rows), -1)
    return a[:, :4].astype(np.int64), a[:, 4].astype(np.float32), a[:, 5:].astype(np.float32)


def _same(res, loop):
    assert np.array_equal(res['boxes'], loop[0])
    assert np.array_equal(res['objness'].view(np.int32), loop[1].view(np.int32))
    assert np.array_equal(res['classes'].view(np.int32), loop[2].view(np.int32))


@pytest.mark.parametrize('fixture', GOLDEN_CASES)
@pytest.mark.parametrize('exp', [np.exp, ho.exp_rounded], ids=['numpy_exp', 'rounded_exp'])
def test_array_chain_equals_loop_chain_on_goldens(golden_dir, fixture, exp):
    netouts, g, ih, iw, post, nms = load_decode_case(golden_dir, fixture)
    res = ho.decode_frame(netouts, g['anchors'].tolist(), 0.5, nms, (416, 416), (ih, iw), exp=exp)
    _same(res, _loop_chain(netouts, g['anchors'], 0.5, nms, (416, 416), (ih, iw), exp))
    if exp is np.exp:      # and so the array chain is pinned to the reference's own output too
        assert np.array_equal(res['boxes'], post[:, :4].astype(np.int64))
        assert np.array_equal(res['classes'] == 0, post[:, 5:] == 0)


def test_array_nms_equals_loop_nms_on_small_random_frames():
    """n <= 60, 1-4 classes, clustered integer boxes, duplicated probabilities, zeros; no zero-area box (the loop raises)."""
    rng = np.random.default_rng(2024)
    suppressed = ties = 0
    for k in range(400):
        n = int(rng.integers(1, 61)); ncls = int(rng.integers(1, 5))
        cen = rng.integers(20, 300, (3, 2))
        c = cen[rng.integers(0, 3, n)] + rng.integers(-12, 13, (n, 2))
        wh = rng.integers(1, 60, (n, 2))
        boxes = np.concatenate([c - wh, c + wh], 1)
        cls = rng.choice(np.array([0, 0.125, 0.3, 0.5, 0.7, 0.9], np.float32), (n, ncls)) if k % 2 else rng.random((n, ncls), np.float32)
        th = float(rng.choice([0.3, 0.45, 0.5, 0.7]))
        rows = [[int(v) for v in boxes[i]] + [0.9] + [float(v) for v in cls[i]] for i in range(n)]
        ho.do_nms(rows, th)
        got = cls.copy()
        ho.do_nms_arrays(boxes, got, th)
        assert np.array_equal(got, np.array([r[5:] for r in rows], np.float32)), k
        suppressed += int(((cls > 0) & (got == 0)).sum())
        ties += int(k % 2)
    assert suppressed > 2000 and ties == 200


def test_zero_union_pair_does_not_suppress():
    boxes = np.array([[5, 5, 5, 5], [5, 5, 5, 5], [9, 9, 9, 20]])
    cls = np.array([[0.9], [0.8], [0.7]], np.float32)
    ho.do_nms_arrays(boxes, cls, 0.5)
    assert np.array_equal(cls, np.array([[0.9], [0.8], [0.7]], np.float32))
    with pytest.raises(ZeroDivisionError):
        ho.do_nms([[5, 5, 5, 5, 1.0, 0.9], [5, 5, 5, 5, 1.0, 0.8]], 0.5)


def test_fragile_flags_exactly_the_midpoint_neighbourhood():
    """Search float32 inputs whose float64 exp lies next to a float32 rounding midpoint; fragile() must flag them, and must
    not flag their neighbours nor ordinary frames."""
    x = np.random.default_rng(3).normal(0, 1.5, 4_000_000).astype(np.float32)
    low = np.exp(-x.astype(np.float64)).view(np.uint64) & np.uint64((1 << 29) - 1)
    dist = np.abs(low.astype(np.int64) - (1 << 28))
    assert (dist <= 4).sum() == 0                      # none in 4 M samples: the exclusion is rare by construction
    near = x[np.argmin(dist)]
    frame = [np.full((g, g, 18), -8.0, np.float32) for g in (1, 2, 4)]
    assert not ho.fragile(frame, 0.5)
    frame[0][0, 0, 6 + 4] = near                       # anchor 1, objectness: feeds membership
    assert ho.fragile(frame, 0.5, ulps=int(dist.min())) and not ho.fragile(frame, 0.5, ulps=int(dist.min()) - 1)
    frame[0][0, 0, 0 + 4] = near; frame[0][0, 0, 6 + 4] = -8.0      # anchor 0 is on the skip list at scale 0: feeds nothing
    assert not ho.fragile(frame, 0.5, ulps=int(dist.min()))


@pytest.mark.parametrize('case', yf.CASES, ids=[c['name'] for c in yf.CASES])
def test_cases_hold_what_they_claim(case):
    frames = yf.case_frames(case)
    excluded = sum(ho.fragile(f, case['obj_thresh']) for f in frames)
    assert excluded <= MAX_EXCLUDED * len(frames)
    kn = case['knobs']
    for f in frames:
        rep = yf.case_report(case, f)
        assert rep['count'] >= case['min_count']
        assert rep['count'] <= min(yf.slot_count(case['grid0']), 8192)
        if case['density'] == 0:
            assert rep['count'] == 0
        if case['min_count'] > 1024:
            assert rep['max_positive_per_class'] > 1024
        if case['clustered']:
            assert rep['suppressed'] >= 0.2 * rep['positive'] and rep['chains'] >= 1
        if kn.get('dup_cls'):
            assert rep['tie_pairs'] >= 50
        if kn.get('zero_prob'):
            assert rep['zero_prob'] >= 0.2 * rep['count'] * case['nclass']
        if kn.get('at_thresh'):
            assert rep['at_thresh'] >= 10
        if kn.get('zero_area'):
            assert rep['zero_union_pairs'] >= 1
        res = yf.case_oracle(case, f)
        assert np.abs(res['boxes']).max(initial=0) < 2 ** 24       # far inside int32, and exact in float32


def test_matrix_covers_the_axes():
    by = lambda k: {c[k] for c in yf.CASES}
    assert by('grid0') >= {3, 7, 10, 13, 16, 19} and by('nclass') == {1, 4, 80}
    assert {(c['obj_thresh'], c['nms_thresh']) for c in yf.CASES} >= {(0.3, 0.3), (0.5, 0.45), (0.5, 0.5), (0.6, 0.7)}
    for net in (yf.NET, yf.NET_NONSQUARE):
        assert {c['image_hw'] for c in yf.CASES if c['net_hw'] == net} >= {yf.LANDSCAPE, yf.PORTRAIT, yf.SQUARE}
    # the non-square net takes both branches of correct_yolo_boxes
    br = {(float(w) / c['image_hw'][1]) < (float(h) / c['image_hw'][0]) for c in yf.CASES for (h, w) in [c['net_hw']] if h != w}
    assert br == {True, False}


def test_exact_threshold_frame():
    netouts, cells_exact, cells_below = yf.exact_threshold_frame(1)
    assert not ho.fragile(netouts, 0.5)
    pre = ho.decode_frame(netouts, yf.ANCHORS, 0.5, 0.5, (416, 416), (416, 416), nms=False)
    post = ho.decode_frame(netouts, yf.ANCHORS, 0.5, 0.5, (416, 416), (416, 416))
    assert len(pre['boxes']) == 12
    for k in range(6):                                  # list order: cells row-major, anchor 0 then anchor 2
        big, small = pre['boxes'][2 * k], pre['boxes'][2 * k + 1]
        inter, uni = ho.box_iou_int(big, small[None])
        assert pre['classes'][2 * k, 0] > pre['classes'][2 * k + 1, 0] > 0
        if k < 3:
            assert (int(inter[0]), int(uni[0])) == (10000, 20000) and inter[0] / uni[0] == 0.5
            assert post['classes'][2 * k, 0] > 0 and post['classes'][2 * k + 1, 0] == 0          # IoU == nms_thresh suppresses
        else:
            assert (int(inter[0]), int(uni[0])) == (10000, 20200)
            assert post['classes'][2 * k, 0] > 0 and post['classes'][2 * k + 1, 0] > 0           # 0.495: kept
    # nothing else reaches the threshold: the pairs decide alone
    inter, uni = ho.box_iou_int(pre['boxes'][:, None, :], pre['boxes'][None, :, :])
    assert int(np.triu(ho.suppresses(inter, uni, 0.5), 1).sum()) == 3


def test_truncated_oracle_is_a_prefix_with_its_own_nms():
    case = next(c for c in yf.CASES if c['name'] == 'g13_c4_all')
    f = yf.case_frames(case)[0]
    full = ho.decode_frame(f, yf.ANCHORS, 0.5, 0.5, yf.NET, yf.LANDSCAPE, nms=False)
    cut = yf.case_oracle(case, f, capacity=1025)
    assert len(cut['boxes']) == 1025 and np.array_equal(cut['boxes'], full['boxes'][:1025])
    want = full['classes'][:1025].copy()
    ho.do_nms_arrays(full['boxes'][:1025], want, 0.5)
    assert np.array_equal(cut['classes'], want)
    assert not np.array_equal(cut['classes'], yf.case_oracle(case, f)['classes'][:1025])     # candidates past the cut play no part
