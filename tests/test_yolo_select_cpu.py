"""fv_yolo_select_cands without a GPU: its NumPy restatement (tests/yolo_select_ref.py) against a literal transcription of the
reference's detect() tail over BoundBox objects, the exported symbol, and the refusal threshold yolov3.select_cands passes."""
import ctypes

import numpy as np
import pytest

import yolo_select_ref as ref


def _lists(seed, nclass, n, capacity, zeroed=0.3):
    """Seeded candidate lists: scores on a lattice of 12 float32 values (ties are the rule), a share of rows zeroed as NMS leaves
    suppressed ones, some values above 1 (capped)."""
    rng = np.random.default_rng(seed)
    lattice = np.concatenate([rng.uniform(0.05, 1.0, 10), [1.25, 1.5]]).astype(np.float32)
    cls = lattice[rng.integers(0, 12, (1, capacity, nclass))]
    cls[rng.random((1, capacity, nclass)) < zeroed] = 0.0
    cls[0, rng.random(capacity) < 0.15] = 0.0                             # whole rows suppressed
    boxes = rng.integers(-20, 500, (1, capacity, 4)).astype(np.int32)
    obj = rng.uniform(0.5, 1.0, (1, capacity)).astype(np.float32)
    return boxes, obj, cls, np.array([n], np.int32)


@pytest.mark.parametrize('nclass', [1, 3])
@pytest.mark.parametrize('K', [1, 7, 60])
def test_select_ref_is_the_reference_tail(nclass, K):
    """Fewer, exactly and more than K survivors; tied scores; zeroed rows."""
    seen, tied = set(), 0
    for seed, n, zeroed in [(0, 0, 0.3), (1, 1, 0.0), (2, 5, 0.0), (3, 40, 0.3), (4, 200, 0.3), (5, 200, 0.9), (6, 64, 0.0), (7, 90, 0.2)]:
        cap = 225
        boxes, obj, cls, count = _lists(seed, nclass, n, cap, zeroed)
        if seed == 6:                                                         # exactly K survivors
            cls[0, K:] = 0.0
            cls[0, :K] = np.maximum(cls[0, :K], np.float32(0.25))
        got = ref.select_ref(boxes, obj, cls, count, cap, ref.INT_MAX, K)
        kept, rows = ref.reference_tail(boxes[0], obj[0], cls[0], n, K)
        k = int(got['count'][0])
        assert k == len(kept) and got['cell'][0, :k].tolist() == rows
        survivors = int(((cls[0, :n].max(axis=1) if n else np.zeros(0)) > 0).sum())
        seen.add('fewer' if survivors < K else 'exactly' if survivors == K else 'more')
        for s, bb in enumerate(kept):
            assert (bb.xmin, bb.ymin, bb.xmax, bb.ymax) == tuple(got['boxes'][0, s]) and bb.objness == got['obj'][0, s]
            assert bb.get_score() == got['score'][0, s] and bb.classes == list(got['classes'][0, s])
        assert np.all(got['boxes'][0, k:] == -1) and np.all(got['cell'][0, k:] == -1)
        assert not got['obj'][0, k:].any() and not got['score'][0, k:].any() and not got['classes'][0, k:].any()
        assert np.all(np.diff(got['score'][0, :k]) >= 0)
        tied += ref.ties(got)
    assert seen == {'fewer', 'exactly', 'more'}
    assert K == 1 or tied > 0


def test_select_ref_edge_values_and_refusal():
    cap, K = 25, 8
    boxes, obj, cls, _ = _lists(9, 2, cap, cap, 0.0)
    cls[0, :] = 0.0
    cls[0, 3] = [0.2, np.nan]                                             # a NaN anywhere: dropped
    cls[0, 4] = [1e-40, 0.0]                                              # a positive denormal: kept, ranked first
    cls[0, 5] = [-0.0, -0.0]                                              # dropped
    cls[0, 6] = [1.5, 0.1]; cls[0, 2] = [0.3, 1.0]; cls[0, 9] = [2.0, 3.0]  # capped: tie at 1.0, ordered by row
    cls[0, 7] = [0.5, 0.25]
    cls[0, 11] = [-1.0, -2.0]                                            # negative: dropped
    out = ref.select_ref(boxes, obj, cls, np.array([cap], np.int32), cap, ref.INT_MAX, K)
    assert out['count'][0] == 5 and out['cell'][0, :5].tolist() == [4, 7, 2, 6, 9]
    assert out['score'][0, :5].tolist() == [np.float32(1e-40), 0.5, 1.0, 1.0, 1.0] and out['score'][0, 0] > 0
    both = ref.select_ref(np.repeat(boxes, 3, 0), np.repeat(obj, 3, 0), np.repeat(cls, 3, 0), np.array([cap, cap - 1, 99], np.int32), cap, cap, K)
    assert both['count'].tolist() == [-1, 5, -1] and np.all(both['boxes'][0] == -1) and not both['score'][0].any()
    low = ref.select_ref(boxes, obj, cls, np.array([-7], np.int32), cap, cap, K)
    assert low['count'][0] == 0 and np.all(low['cell'] == -1)
    assert ref.select_ref(boxes, obj, cls, np.array([cap], np.int32), cap, ref.INT_MAX, K, with_classes=False)['classes'] is None


def test_library_exports_the_entry_point():
    from face_vijnana_yolov3_amd.build import build_library
    L = ctypes.CDLL(build_library())
    assert hasattr(L, 'fv_yolo_select_cands')
    L.fv_yolo_select_cands.restype = ctypes.c_int
    # a NULL context is refused without touching anything
    assert L.fv_yolo_select_cands(*([None] * 5), 1, 25, 1, 25, 1, *([None] * 6)) == -1


class _Recorder(object):
    def __init__(self):
        self.args = None

    def fv_yolo_select_cands(self, *args):
        self.args = args
        return 0


class _Ctx(object):
    handle = None

    def check(self, rc, what):
        assert rc == 0, what


@pytest.mark.parametrize('grid, want', [(19, 8192), (13, 2 ** 31 - 1), (3, 2 ** 31 - 1)])
def test_select_cands_passes_the_refusal_threshold(monkeypatch, grid, want):
    """Grid 19 has 9025 slots, the candidate list 8192: a full list may have been cut and is refused.  Grid 13 (4225 slots) and
    below: the list holds every slot and a full one is served."""
    import torch
    from face_vijnana_yolov3_amd import yolov3
    rec = _Recorder()
    monkeypatch.setattr(yolov3, 'lib', lambda: rec)
    cap = min(yolov3.candidate_slots(grid), yolov3.MAX_CANDIDATES)
    assert yolov3.select_refuse_at(cap, grid) == want
    res = dict(boxes=torch.zeros((2, cap, 4), dtype=torch.int32), objness=torch.zeros((2, cap)), classes=torch.zeros((2, cap, 1)),
               count=torch.zeros((2,), dtype=torch.int32))
    out = yolov3.select_cands(_Ctx(), res, 60, grid)
    nimg, capacity, nclass, refuse_at, K = rec.args[5:10]
    assert (nimg, capacity, nclass, refuse_at, K) == (2, cap, 1, want, 60)
    assert sorted(out) == ['boxes', 'cell', 'classes', 'count', 'obj', 'score']
    assert tuple(out['boxes'].shape) == (2, 60, 4) and tuple(out['classes'].shape) == (2, 60, 1) and out['cell'].dtype == torch.int32


def test_a_refused_count_raises_the_candidate_error():
    from face_vijnana_yolov3_amd._lib import FvError
    from face_vijnana_yolov3_amd.yolov3 import MAX_CANDIDATES, check_candidate_count, check_selected_count
    check_selected_count(0, 19)
    check_selected_count(60, 19)
    with pytest.raises(FvError) as today:
        check_candidate_count(MAX_CANDIDATES, MAX_CANDIDATES, 19)
    with pytest.raises(FvError) as now:
        check_selected_count(-1, 19)
    assert str(now.value) == str(today.value) and '8192' in str(now.value)
