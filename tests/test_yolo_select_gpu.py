"""fv_yolo_select_cands on the GPU against its NumPy restatement (tests/yolo_select_ref.py), every output byte for byte: sizes,
counts, the sort's power-of-two boundaries, ties, score edge values, refusal, poisoned outputs, invalid arguments, the stream
contract; then the three-scale FaceDetector tail that runs through it (detect_batch, test(), validate()) against the composition
decode_nms_batch -> select_ref at image size 96, and saturation at grid 19 with crafted head tensors."""
import io
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import data, det_metric as dm, postproc
from face_vijnana_yolov3_amd._lib import Context, FvError, lib, ptr
from face_vijnana_yolov3_amd.yolov3 import decode_nms_batch, select_cands
import stream_order as so
import yolo_select_ref as ref

pytestmark = pytest.mark.gpu

OUT = ('boxes', 'cell', 'obj', 'score', 'classes', 'count')
INT_MAX = ref.INT_MAX


@pytest.fixture(scope='module')
def ctx():
    c = Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', ctx.device))


def _problem(seed, nimg, capacity, nclass, zeroed=0.3):
    """Seeded candidate lists: class values on a lattice of 12 float32 values (two of them above 1, capped to a tie at 1.0), so
    ties are the rule; a share of the entries and of whole rows zeroed, as NMS leaves suppressed ones."""
    rng = np.random.default_rng(seed)
    lattice = np.concatenate([rng.uniform(0.05, 1.0, 10), [1.25, 1.5]]).astype(np.float32)
    cls = lattice[rng.integers(0, 12, (nimg, capacity, nclass))]
    cls[rng.random((nimg, capacity, nclass)) < zeroed] = 0.0
    cls[rng.random((nimg, capacity)) < 0.15] = 0.0
    return dict(boxes=rng.integers(-50, 700, (nimg, capacity, 4)).astype(np.int32),
                objness=rng.uniform(0.5, 1.0, (nimg, capacity)).astype(np.float32), classes=cls,
                count=np.full(nimg, capacity, np.int32))


def _buffers(nimg, K, nclass, dev, poison):
    """Output tensors pre-filled: 'ff' every byte 0xFF, 'nan' float NaN (the integers its pattern), 'seven' the value 7."""
    shapes = dict(boxes=((nimg, K, 4), torch.int32), cell=((nimg, K), torch.int32), obj=((nimg, K), torch.float32),
                  score=((nimg, K), torch.float32), classes=((nimg, K, nclass), torch.float32), count=((nimg,), torch.int32))
    out = {}
    for k, (shape, dt) in shapes.items():
        t = torch.empty(shape, dtype=dt, device=dev)
        if poison == 'ff':
            t.view(torch.uint8).fill_(0xFF)
        elif poison == 'nan':
            t.view(torch.int32).fill_(0x7FC00000)
        else:
            t.fill_(7)
        out[k] = t
    return out


def _run(ctx, p, K, refuse_at=INT_MAX, poison='ff', with_classes=True):
    """The raw entry point on the problem -> the outputs as host arrays (classes: the poison when with_classes is off)."""
    dev = torch.device('cuda', ctx.device)
    nimg, capacity, nclass = p['classes'].shape
    d = {k: _dev(v, ctx) for k, v in p.items()}
    out = _buffers(nimg, K, nclass, dev, poison)
    rc = lib().fv_yolo_select_cands(ctx.handle, ptr(d['boxes']), ptr(d['objness']), ptr(d['classes']), ptr(d['count']), nimg, capacity,
                                    nclass, refuse_at, K, ptr(out['boxes']), ptr(out['cell']), ptr(out['obj']), ptr(out['score']),
                                    ptr(out['classes']) if with_classes else None, ptr(out['count']))
    ctx.check(rc, 'fv_yolo_select_cands')
    return {k: v.cpu().numpy() for k, v in out.items()}


def _want(p, K, refuse_at=INT_MAX, with_classes=True):
    return ref.select_ref(p['boxes'], p['objness'], p['classes'], p['count'], p['classes'].shape[1], refuse_at, K, with_classes)


def _assert_equal(got, want, what):
    for k in OUT:
        if want[k] is None:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), '%s: %s differs (count %s, reference %s)' % (what, k, got['count'], want['count'])


# ----------------------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize('capacity', [25, 225, 4225, 8192])
def test_sizes(ctx, capacity):
    """nimg 1 and 5, nclass 1 / 2 / 80, K 1 / 60 / 512 at each capacity (grid 1, grid 3, grid 13, the bound); the counts of the five
    images differ: full, partial, above the capacity, empty, full."""
    tied = 0
    for nclass in (1, 2, 80):
        p5 = _problem(capacity + nclass, 5, capacity, nclass)
        p5['count'] = np.array([capacity, capacity // 2 + 1, capacity + 9, 0, capacity], np.int32)
        p1 = {k: v[:1].copy() for k, v in p5.items()}
        for K in (1, 60, 512):
            for p in (p1, p5):
                want = _want(p, K)
                _assert_equal(_run(ctx, p, K), want, (capacity, nclass, K, len(p['count'])))
                tied += ref.ties(want)
    print('capacity %d: %d adjacent selected rows share their score' % (capacity, tied))
    assert tied > 0


@pytest.mark.parametrize('K', [1, 60, 512])
def test_count_values(ctx, K):
    """count 0, 1, K - 1, K, K + 1, capacity, above the capacity and negative, one image each; every row is a survivor, so the
    selected number is min(clamped count, K)."""
    capacity = 1000
    counts = np.array([0, 1, K - 1, K, K + 1, capacity, capacity + 1, 2 ** 30, -1, -2 ** 31], np.int32)
    p = _problem(K, len(counts), capacity, 2, zeroed=0.0)
    p['classes'] = np.maximum(p['classes'], np.float32(0.01))
    p['count'] = counts
    want = _want(p, K)
    assert want['count'].tolist() == [min(min(max(int(c), 0), capacity), K) for c in counts]
    _assert_equal(_run(ctx, p, K), want, K)


@pytest.mark.parametrize('K', [60, 512])
def test_kept_counts_at_the_sort_boundaries(ctx, K):
    """Exactly 2, 1024, 1025, 4096, 4097 and 8192 kept rows among 8192: the padded power of two and the strided passes change
    there; 0 and 1 (no sort at all) ride along."""
    capacity, kept = 8192, [2, 1024, 1025, 4096, 4097, 8192, 0, 1]
    p = _problem(77, len(kept), capacity, 1, zeroed=0.0)
    p['classes'] = np.maximum(p['classes'], np.float32(0.01))
    rng = np.random.default_rng(78)
    for b, n in enumerate(kept):
        p['classes'][b, rng.permutation(capacity)[n:]] = 0.0
    want = _want(p, K)
    assert want['count'].tolist() == [min(n, K) for n in kept]
    tied = ref.ties(want)
    print('%d adjacent selected rows share their score' % tied)
    assert tied > 0
    _assert_equal(_run(ctx, p, K), want, K)


def test_a_whole_image_of_suppressed_rows(ctx):
    p = _problem(3, 3, 4225, 2)
    p['classes'][1] = 0.0
    want = _want(p, 60)
    assert want['count'].tolist() == [60, 0, 60] and np.all(want['boxes'][1] == -1) and not want['score'][1].any()
    _assert_equal(_run(ctx, p, 60), want, 'zeroed image')


def test_score_edge_values(ctx):
    """1.5 is capped, and the rows then tied at 1.0 order by their index; a NaN class anywhere drops the row; 1e-40 (a positive
    denormal) is kept and ranked first; -0.0 and negatives are dropped."""
    capacity, K = 225, 60
    p = _problem(4, 2, capacity, 2)
    c = p['classes']
    c[0] = 0.0
    c[0, 100] = [0.2, np.nan]; c[0, 101] = [np.nan, 0.9]; c[0, 102] = [-np.nan, 0.0]
    c[0, 50] = [1e-40, 0.0]
    c[0, 60] = [-0.0, -0.0]; c[0, 61] = [-0.5, -1.0]; c[0, 62] = [0.0, -0.0]
    c[0, 200] = [1.5, 0.1]; c[0, 7] = [0.3, 1.0]; c[0, 150] = [np.inf, 3.0]; c[0, 8] = [1.5, 1.5]
    c[0, 30] = [0.5, 0.25]; c[0, 31] = [0.25, 0.5]
    c[1, 17] = [np.nan, np.nan]
    want = _want(p, K)
    assert want['count'][0] == 7 and want['cell'][0, :7].tolist() == [50, 30, 31, 7, 8, 150, 200]
    assert want['score'][0, :7].view(np.uint32).tolist() == [np.float32(1e-40).view(np.uint32)] + [0x3F000000] * 2 + [0x3F800000] * 4
    assert 17 not in want['cell'][1].tolist()
    _assert_equal(_run(ctx, p, K), want, 'edge values')


def test_refusal_serves_the_neighbours(ctx):
    """count == refuse_at and above: -1 and filled slots; the images beside them are served, count == refuse_at - 1 included."""
    capacity, K = 225, 60
    p = _problem(6, 5, capacity, 1)
    p['count'] = np.array([capacity, capacity - 1, capacity + 4, 3, capacity], np.int32)
    want = _want(p, K, refuse_at=capacity)
    assert want['count'].tolist()[::2] == [-1, -1, -1] and want['count'][1] == 60 and 0 < want['count'][3] <= 3
    assert np.all(want['boxes'][0] == -1) and np.all(want['cell'][2] == -1) and not want['classes'][4].any()
    _assert_equal(_run(ctx, p, K, refuse_at=capacity), want, 'refusal')
    served = _want(p, K)                                                      # the same lists with no threshold: all served
    assert served['count'].min() >= 0
    _assert_equal(_run(ctx, p, K), served, 'no refusal')


@pytest.mark.parametrize('with_classes', [True, False])
def test_poisoned_outputs_and_null_classes(ctx, with_classes):
    """Outputs pre-filled with 0xFF bytes and with NaN give the same bytes: every slot is written.  out_classes NULL: the other
    five outputs are the same and nothing else is written."""
    p = _problem(8, 3, 4225, 2)
    p['count'] = np.array([4225, 40, 0], np.int32)
    want = _want(p, 60, with_classes=with_classes)
    a = _run(ctx, p, 60, poison='ff', with_classes=with_classes)
    b = _run(ctx, p, 60, poison='nan', with_classes=with_classes)
    _assert_equal(a, want, 'ff')
    _assert_equal(b, want, 'nan')
    if not with_classes:
        assert np.all(a['classes'].view(np.uint32) == 0xFFFFFFFF) and np.all(b['classes'].view(np.uint32) == 0x7FC00000)


def test_invalid_arguments_enqueue_nothing(ctx):
    p = _problem(5, 2, 225, 2)
    dev = torch.device('cuda', ctx.device)
    d = {k: _dev(v, ctx) for k, v in p.items()}
    out = _buffers(2, 60, 2, dev, 'seven')

    def call(nimg=2, capacity=225, nclass=2, refuse_at=INT_MAX, K=60, null=None):
        a = [ptr(d['boxes']), ptr(d['objness']), ptr(d['classes']), ptr(d['count'])]
        o = [ptr(out[k]) for k in OUT]
        if null is not None:
            if null < 4:
                a[null] = None
            else:
                o[null - 4] = None
        return lib().fv_yolo_select_cands(ctx.handle, *a, nimg, capacity, nclass, refuse_at, K, *o)
    bad = [dict(nimg=0), dict(nimg=-1), dict(capacity=0), dict(capacity=8193), dict(nclass=0), dict(K=0), dict(K=513), dict(refuse_at=0),
           dict(refuse_at=-5)] + [dict(null=i) for i in (0, 1, 2, 3, 4, 5, 6, 7, 9)]           # 8 is out_classes, which may be NULL
    for kw in bad:
        assert call(**kw) == -1, kw                                           # FV_ERR_INVALID
        assert b'fv_yolo_select_cands' in lib().fv_last_error(ctx.handle), kw
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())                    # nothing was enqueued
    assert call(null=8) == 0 and call() == 0                                  # and the good calls go through
    torch.cuda.synchronize()
    assert out['count'].min().item() >= 0 and not bool((out['cell'] == 7).all())


def test_select_cands_wrapper(ctx):
    """yolov3.select_cands on decode_nms_batch's dict: fv_decode_nms' key names plus classes, refusal from the grid, views of a
    longer buffer as outputs."""
    p = _problem(12, 3, 8192, 1)
    p['count'] = np.array([8192, 400, 8191], np.int32)
    res = {k: _dev(v, ctx) for k, v in p.items()}
    got = select_cands(ctx, res, 60, 19)                                      # 9025 slots in 8192 rows: a full list is refused
    assert sorted(got) == sorted(OUT)
    _assert_equal({k: v.cpu().numpy() for k, v in got.items()}, _want(p, 60, refuse_at=8192), 'grid 19')
    small = {k: _dev(v[:, :4225] if v.ndim > 1 else np.minimum(v, 4225), ctx) for k, v in p.items()}
    whole = {k: torch.zeros((5,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device) for k, v in got.items()}
    select_cands(ctx, {k: v.contiguous() for k, v in small.items()}, 60, 13, out={k: v[1:4] for k, v in whole.items()})
    want = _want({k: v.cpu().numpy() for k, v in small.items()}, 60)          # grid 13: 4225 slots in 4225 rows, never refused
    assert want['count'].tolist() == [60, 60, 60]
    _assert_equal({k: v[1:4].cpu().numpy() for k, v in whole.items()}, want, 'grid 13')
    assert not any(bool(v[0].any()) or bool(v[4].any()) for v in whole.values())


# ----------------------------------------------------------------------------- stream contract
def test_select_cands_on_a_delayed_stream():
    """The harness of tests/stream_order.py on fv_yolo_select_cands: exact, no host_sync.  Boxes, objectness and classes differ
    between the two problems, the counts do not; with more than 60 survivors per image the selected number ties at 60."""
    def make(seed, dev):
        p = _problem(seed, 3, 4225, 2)
        p['count'] = np.array([4225, 900, 61], np.int32)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.items()}

    def call(ctx, p):
        return select_cands(ctx, p, 60, 13)
    case = so.Case('yolo_select_cands', ('fv_yolo_select_cands',), make, call, may_tie=('count',))
    assert case.exact and not case.host_sync
    so.run_delayed(case)


# ----------------------------------------------------------------------------- the detector's tail at image size 96
S = 96
SHAPES = [(120, 160), (160, 120), (128, 128), (100, 200), (150, 180)]


def _conf(root, image_size=S, eval_batch=4):
    return {'mode': 'test', 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False, 'bn_zero_debias': False,
            'hps': {'lr': 1e-3, 'beta_1': 0.9, 'beta_2': 0.999, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2,
                    'face_conf_th': 0.0, 'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'eval_batch_size': eval_batch},
            'nn_arch': {'image_size': image_size, 'bb_info_c_size': 6, 'head': 'three_scale', 'num_classes': 1}}


def _held_out_set(root, shapes):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(31)
    lines = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    names = []
    for k, (h, w) in enumerate(shapes):
        names.append(os.path.join(root, 'held_%02d.jpg' % k))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(names[-1], quality=90)
        lines.append('%d,%s,%d,%.1f,%.1f,%.1f,%.1f' % (k, os.path.basename(names[-1]), k + 1, 0.1 * w, 0.1 * h, 0.8 * w, 0.8 * h))
    open(os.path.join(root, 'validation.csv'), 'w').write('\n'.join(lines) + '\n')
    return names


def _small_head(fd, scale):
    """The synthetic initialisation gives head logits of +-1e4, where exp overflows; scaled, they are of order 1."""
    for d in fd.model.layers:
        if d['role'] == 5:
            n = d['cout'] * d['ksize'] * d['ksize'] * d['cin']
            fd.model.params[d['w_off']:d['w_off'] + n] *= scale


@pytest.fixture(scope='module')
def detector(tmp_path_factory):
    from face_vijnana_yolov3_amd import face_detection
    root = str(tmp_path_factory.mktemp('three_scale_tail'))
    names = _held_out_set(root, SHAPES)
    old, cwd = face_detection.DEBUG, os.getcwd()
    face_detection.DEBUG = False
    os.chdir(root)
    try:
        fd = face_detection.FaceDetector(_conf(root))
        assert fd.three_scale and fd.hps['face_conf_th'] == 0.0
        _small_head(fd, 3e-4)
        yield fd, root, names
    finally:
        face_detection.DEBUG = old
        os.chdir(cwd)


def _compose(fd, files):
    """One batch through the public pieces: letterbox, network, decode_nms_batch, then the restatement on the decode's own result
    -> (x, geoms, the decode's dict, select_ref's dict)."""
    ctx = fd.model.ctx
    raws = [data._pil_loader(f) for f in files]
    x, geoms = postproc.letterbox_batch_device(ctx, raws, S, fd.model.dev)
    ys = fd.model.predict_device(x)
    res = decode_nms_batch(ctx, ys[0], ys[1], ys[2], (S, S), (S, S), obj_thresh=fd.hps['face_conf_th'], nms_thresh=fd.hps['nms_iou_th'])
    host = {k: v.cpu().numpy() for k, v in res.items()}
    assert host['boxes'].shape[1] == 225 and np.all(host['count'] == 225)       # face_conf_th 0: every slot is a candidate
    return x, geoms, res, ref.select_ref(host['boxes'], host['objness'], host['classes'], host['count'], 225, INT_MAX, fd.hps['num_cands'])


def _boundboxes(want, b):
    n = int(want['count'][b])
    bx = want['boxes'][b, :n].astype(np.int64)
    return [postproc.BoundBox(bx[k, 0], bx[k, 1], bx[k, 2], bx[k, 3], objness=want['obj'][b, k], classes=list(want['classes'][b, k]))
            for k in range(n)]


def test_decode_then_select_equals_the_restatement(detector):
    fd, root, names = detector
    _x, _geoms, res, want = _compose(fd, names[:4])
    got = select_cands(fd.model.ctx, res, fd.hps['num_cands'], S // 32)
    _assert_equal({k: v.cpu().numpy() for k, v in got.items()}, want, 'composition')
    suppressed = int((res['classes'].cpu().numpy()[..., 0] == 0).sum())
    print('selected per image %s, %d of %d candidates suppressed' % (want['count'].tolist(), suppressed, 4 * 225))
    assert want['count'].min() >= 2 and suppressed > 0                        # the selection has something to drop and to order


def test_detect_batch_equals_the_boundboxes_of_the_composition(detector):
    fd, root, names = detector
    x, _geoms, _res, want = _compose(fd, names[:4])
    got = fd.detect_batch(x)
    assert len(got) == 4
    for b in range(4):
        exp = _boundboxes(want, b)
        assert len(got[b]) == len(exp) >= 2
        for g, e in zip(got[b], exp):
            for name in ('xmin', 'ymin', 'xmax', 'ymax'):
                assert type(getattr(g, name)) is np.int64 and getattr(g, name) == getattr(e, name)
            assert type(g.objness) is np.float32 and g.objness.tobytes() == e.objness.tobytes()
            assert type(g.classes) is list and len(g.classes) == 1 and type(g.classes[0]) is np.float32
            assert g.classes[0].tobytes() == e.classes[0].tobytes()
        assert [float(g.get_score()) for g in got[b]] == [float(s) for s in want['score'][b, :len(exp)]]


def test_pinned_copies_hold_the_selected_rows_only(detector):
    fd, root, names = detector
    x, _geoms, _res, want = _compose(fd, names[:3])
    tag, host, ev, n = fd._detect_launch(x)
    ev.synchronize()
    assert tag == 'three_scale' and n == 3 and sorted(host) == sorted(OUT)
    K = fd.hps['num_cands']
    assert tuple(host['boxes'].shape) == (3, K, 4) and tuple(host['classes'].shape) == (3, K, 1)
    assert all(tuple(host[k].shape) == (3, K) for k in ('cell', 'obj', 'score')) and tuple(host['count'].shape) == (3,)
    assert all(t.is_pinned() for t in host.values())
    _assert_equal({k: v.numpy() for k, v in host.items()}, want, 'pinned')


@pytest.mark.parametrize('eval_batch', [1, 4])
def test_csv_of_test_equals_the_composition(detector, eval_batch):
    fd, root, names = detector
    files = sorted(names)
    fd.hps['eval_batch_size'] = eval_batch
    fd.conf = dict(fd.conf, test_path=root, output_file_path=os.path.join(root, 'solution_%d.csv' % eval_batch))
    f = io.StringIO()
    for c0 in range(0, len(files), eval_batch):
        chunk = files[c0:c0 + eval_batch]
        _x, geoms, _res, want = _compose(fd, chunk)
        for b, name in enumerate(chunk):
            boxes = _boundboxes(want, b)
            fd._project_back(boxes, geoms[b])
            fd._write_rows(f, name, boxes)
    want_lines = f.getvalue().splitlines(True)
    assert len(want_lines) >= 2 * len(files)
    fd.test()
    assert open(fd.conf['output_file_path']).readlines() == want_lines


def test_validate_rows_are_rows_from_nms_on_the_composition(detector):
    fd, root, names = detector
    fd.hps['eval_batch_size'] = 4
    fd.conf = dict(fd.conf, test_path=root)
    fd._validator = None
    res = fd.validate()
    v = fd._validator
    assert res['n_images'] == len(names) and v.files == sorted(names)
    ctx = fd.model.ctx
    for c0 in range(0, len(v.files), 4):
        chunk = v.files[c0:c0 + 4]
        _x, geoms, _res, want = _compose(fd, chunk)
        dev_res = {k: _dev(want[k], ctx) for k in ('boxes', 'score', 'count')}
        geom = torch.tensor(geoms, dtype=torch.int32).reshape(len(chunk), 6).to(fd.model.dev)
        rows, nrows = dm.rows_from_nms(ctx, dev_res, geom, S)
        assert torch.equal(v.nrows[c0:c0 + len(chunk)], nrows) and int(nrows.min()) >= 2
        assert v.rows[c0:c0 + len(chunk)].cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()


def test_a_saturated_image_raises_in_detect_batch_and_in_validate(tmp_path, monkeypatch):
    """Grid 19 without running a 608 network: predict_device hands back crafted 19 / 38 / 76-grid tensors, one sparse image and
    one where every slot is a candidate (9025 > 8192).  The error names the kernel's bound; validate() returns no metric."""
    from oracle import yolo_frames as yf
    from face_vijnana_yolov3_amd import face_detection
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(face_detection, 'DEBUG', False)
    root = str(tmp_path / 'val')
    _held_out_set(root, SHAPES[:2])
    conf = _conf(root, image_size=608, eval_batch=2)
    conf['hps']['face_conf_th'] = 0.5
    fd = face_detection.FaceDetector(conf)
    dense = yf.make_frame(np.random.default_rng(608), 19, 1, 1.0, net_hw=(608, 608))
    sparse = yf.make_frame(np.random.default_rng(609), 19, 1, 0.1, net_hw=(608, 608))
    fake = [torch.from_numpy(np.stack([a, b])).cuda() for a, b in zip(sparse, dense)]
    monkeypatch.setattr(fd.model, 'predict_device', lambda images: fake)
    x = torch.zeros((2, 8, 8, 3), device=fd.model.dev)                        # never read: the network is patched out
    tag, host, ev, n = fd._detect_launch(x)
    ev.synchronize()
    assert host['count'][1] == -1 and 0 < host['count'][0] <= 60               # the neighbour was served
    with pytest.raises(FvError, match='at least 8192 candidates.*handles 8192'):
        fd.detect_batch(x)
    with pytest.raises(FvError, match='at least 8192 candidates.*handles 8192'):
        fd.validate()
    monkeypatch.setattr(fd.model, 'predict_device', lambda images: [t[:1].repeat(2, 1, 1, 1) for t in fake])
    assert [len(b) for b in fd.detect_batch(x)] == [int(host['count'][0])] * 2  # two sparse images: served
