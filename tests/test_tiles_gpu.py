"""hps['tiles'] on the GPU: fv_tile_merge against its float64 restatement (tests/tile_merge_ref.py), bit for bit; its safety
checks; the stream contract on a delayed stream; FaceDetector.detect_frame / test() / validate() with tiles against the composition
of the public pieces (tile_grid -> letterbox_crops -> predict_device -> decode_nms -> tile_merge_ref)."""
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import data, det_metric as dm, postproc
from face_vijnana_yolov3_amd._lib import Context, FvError, lib, ptr
import det_metric_ref as mref
import stream_order as so
import tile_merge_ref as ref

pytestmark = pytest.mark.gpu

S = 96
OUT = ('corners', 'rows', 'nrows', 'src')


@pytest.fixture(scope='module')
def ctx():
    c = Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', ctx.device))


# ----------------------------------------------------------------------------- problems
# view geometries: the identity (96 x 96 at image size 96) at lattice offsets, so that views of one frame share exact coordinates;
# tw > th and tw < th with their paddings; a big odd tile whose scale is no integer
GEOMS = [(0, 0, 96, 96), (8, 16, 96, 96), (16, 8, 96, 96), (0, 0, 48, 96), (0, 0, 96, 48), (40, 24, 96, 192), (24, 40, 192, 96), (3, 5, 517, 333),
         (0, 0, 333, 517)]


def _problem(seed, views_per_frame, K, full_frame=None):
    """Seeded views on a coarse lattice: corners are multiples of 8 network pixels, scores come from 12 float32 values -- exact
    threshold overlaps and score ties are common.  Counts cycle through 0, partial, K, above K and negative.  full_frame: index of
    a frame whose every slot is a candidate (count K, score > 0)."""
    rng = np.random.default_rng(seed)
    T = int(sum(views_per_frame))
    lo = 8 * rng.integers(0, 10, (T, K, 2))
    hi = np.minimum(lo + 8 * rng.integers(1, 5, (T, K, 2)), S - 1 + 0 * lo)
    boxes = np.concatenate([lo, hi], axis=2).astype(np.int32)
    values = rng.uniform(0.05, 1.2, 12).astype(np.float32)                # some above 1: conf is capped, the ranking is not
    score = values[rng.integers(0, 12, (T, K))]
    score[rng.random((T, K)) < 0.1] = 0.0                                 # no candidate
    score[rng.random((T, K)) < 0.02] = np.nan                             # never > 0
    off = np.concatenate([[0], np.cumsum(views_per_frame)]).astype(np.int32)
    tiles = np.zeros((T, 5), np.int32)
    count = np.zeros(T, np.int32)
    for f, nv in enumerate(views_per_frame):
        cap = min(K, 4096 // nv)                                          # a frame stays within the kernel's 4096 candidates
        kinds = [0, max(1, cap // 2), cap, K + 5 if cap == K else cap, -3, max(1, cap // 3)]
        for t in range(off[f], off[f + 1]):
            count[t] = kinds[(t + seed) % len(kinds)]
            tiles[t] = (f,) + GEOMS[(t + seed) % (3 if (t - off[f]) % 2 else len(GEOMS))]
    if full_frame is not None:
        sl = slice(off[full_frame], off[full_frame + 1])
        count[sl] = K
        score[sl] = np.where(score[sl] > 0, score[sl], values[0])
    return dict(boxes=boxes, score=score, count=count, tiles=tiles, frame_off=off)


def _run(ctx, p, metric, th, workspace=None, out=None):
    res = dict(boxes=_dev(p['boxes'], ctx), score=_dev(p['score'], ctx), count=_dev(p['count'], ctx))
    got = postproc.tile_merge(ctx, res, _dev(p['tiles'], ctx), _dev(p['frame_off'], ctx), S, metric, th, workspace=workspace, out=out)
    return {k: got[k].cpu().numpy() for k in OUT}


def _assert_equal(got, want, what):
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), '%s: %s differs (nrows %s, reference %s)' % (what, k, got['nrows'], want['nrows'])


CASES = [  # (views per frame, K, frame made full)
    ([1], 1, None), ([30], 1, None), ([1, 2, 30], 1, None),
    ([1], 60, None), ([30], 60, None), ([1, 2, 30], 60, None), ([2, 30, 1], 60, 1),
    ([1], 512, None), ([8], 512, 0), ([1, 2, 30], 512, None),
]


@pytest.mark.parametrize('metric', ['ios', 'iou'])
def test_kernel_equals_the_reference(ctx, metric):
    """F of 1 and 3; 1, 2 and 30 views per frame, mixed in one call; K of 1, 60 and 512; counts 0, partial, full, above K and
    negative; a frame with no candidate; a frame at exactly 4096 candidates; tw >= th and tw < th; lattice boxes and few score
    values, so that the reference meets exact-threshold overlaps, score ties and kills in both view directions."""
    stats = {}
    seen_4096 = seen_empty = False
    for n, (views, K, full) in enumerate(CASES):
        p = _problem(100 + n, views, K, full)
        if n == 5:
            p['count'][p['frame_off'][1]:p['frame_off'][2]] = 0            # the two-view frame: no candidate at all
        want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, metric, 0.5, stats=stats)
        for f in range(len(views)):
            t0, t1 = p['frame_off'][f], p['frame_off'][f + 1]
            cands = sum(int((p['score'][t, :min(max(int(p['count'][t]), 0), K)] > 0).sum()) for t in range(t0, t1))
            seen_4096 = seen_4096 or cands == 4096
            seen_empty = seen_empty or cands == 0
        assert (want['nrows'] >= 0).all()
        _assert_equal(_run(ctx, p, metric, 0.5), want, 'case %d %r K %d' % (n, views, K))
    print('reference statistics (%s): %r' % (metric, stats))
    assert seen_4096 and seen_empty
    assert stats['ties'] >= 1 and stats['at_threshold'] >= 1 and stats['late_kills_early'] >= 1 and stats['early_kills_late'] >= 1


def test_other_thresholds_and_the_hand_built_cases(ctx):
    p = _problem(7, [3, 30], 60)
    for metric in ('ios', 'iou'):
        for th in (1.0, 0.25, float(np.nextafter(0.5, 1.0))):
            want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, metric, th)
            _assert_equal(_run(ctx, p, metric, th), want, '%s at %r' % (metric, th))
    # IoU exactly 0.5; a point against a doubly inverted box (x / 0 = inf: merged); identical points (0 / 0 = nan: kept);
    # 62 candidates of which the 61st is suppressed and the 62nd never decided
    disjoint = [(8 * (i % 10), 8 * (i // 10), 8 * (i % 10) + 5, 8 * (i // 10) + 5) for i in range(60)]
    hand = [([(0, 0, 10, 10), (0, 0, 10, 5)], [0.9, 0.8]), ([(5, 5, 5, 5), (5, 5, 3, 2)], [0.9, 0.8]), ([(5, 5, 5, 5), (5, 5, 5, 5)], [0.9, 0.8]),
            (disjoint[:59] + [disjoint[0], disjoint[59], (88, 88, 93, 93)], list(np.arange(62, 0, -1) / 100))]
    for metric in ('ios', 'iou'):
        for th in (0.5, float(np.nextafter(0.5, 1.0)), 1.0):
            for boxes, score in hand:
                K = len(boxes)
                p = dict(boxes=np.array(boxes, np.int32)[None], score=np.array(score, np.float32)[None], count=np.array([K], np.int32),
                         tiles=np.array([(0, 0, 0, 96, 96)], np.int32), frame_off=np.array([0, 1], np.int32))
                want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, metric, th)
                _assert_equal(_run(ctx, p, metric, th), want, 'hand-built %s at %r, %d boxes' % (metric, th, K))


# ----------------------------------------------------------------------------- safety
def test_a_frame_beyond_the_cap_is_flagged_and_the_others_are_served(ctx):
    p = _problem(3, [9, 2, 30], 512, full_frame=0)                      # 9 x 512 = 4608 candidates in frame 0
    want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, 'ios', 0.5)
    assert want['nrows'][0] == -1 and (want['nrows'][1:] >= 0).all() and want['nrows'][2] > 0
    assert not want['rows'][0].any() and (want['src'][0] == -1).all()
    _assert_equal(_run(ctx, p, 'ios', 0.5), want, 'frame beyond the cap')
    # a hand-made table whose ranges do not fit the views: flagged, nothing of them is read
    p2 = dict(p, frame_off=np.array([0, 2, 1, 99], np.int32))
    want = ref.merge(p2['boxes'], p2['score'], p2['count'], p2['tiles'], p2['frame_off'], S, 'ios', 0.5)
    assert want['nrows'].tolist()[1:] == [-1, -1] and want['nrows'][0] >= 0
    _assert_equal(_run(ctx, p2, 'ios', 0.5), want, 'ranges outside the views')


def test_outputs_and_workspace_contents_do_not_matter(ctx):
    p = _problem(11, [30, 1, 2], 60)
    dev = torch.device('cuda', ctx.device)
    need = int(lib().fv_tile_merge_workspace_bytes(3))
    assert need == 3 * 4096 * 32
    runs = []
    for fill in ('ff', 'nan', 'zero'):
        ws = torch.zeros(need // 8 + 512, dtype=torch.float64, device=dev)
        out = dict(corners=torch.zeros((3, 60, 4), dtype=torch.float64, device=dev), rows=torch.zeros((3, 60, 5), dtype=torch.float64, device=dev),
                   nrows=torch.zeros(3, dtype=torch.int32, device=dev), src=torch.zeros((3, 60), dtype=torch.int32, device=dev))
        if fill == 'ff':
            for t in [ws] + list(out.values()):
                t.view(torch.uint8).fill_(0xFF)
        elif fill == 'nan':
            ws.fill_(float('nan')); out['corners'].fill_(float('nan')); out['rows'].fill_(float('nan'))
        ws[need // 8:] = 12345.0                                              # guard behind the workspace
        got = _run(ctx, p, 'ios', 0.5, workspace=ws, out=out)
        assert bool((ws[need // 8:] == 12345.0).all())
        runs.append(b''.join(got[k].tobytes() for k in OUT))
    assert runs[0] == runs[1] == runs[2]
    want = ref.merge(p['boxes'], p['score'], p['count'], p['tiles'], p['frame_off'], S, 'ios', 0.5)
    assert runs[2] == b''.join(want[k].tobytes() for k in OUT)


def test_invalid_arguments_enqueue_nothing(ctx):
    p = _problem(5, [2, 1], 60)
    dev = torch.device('cuda', ctx.device)
    d = {k: _dev(v, ctx) for k, v in p.items()}
    ws = postproc.tile_merge_workspace(2, dev)
    out = dict(corners=torch.full((2, 60, 4), 7.0, dtype=torch.float64, device=dev), rows=torch.full((2, 60, 5), 7.0, dtype=torch.float64, device=dev),
               nrows=torch.full((2,), 7, dtype=torch.int32, device=dev), src=torch.full((2, 60), 7, dtype=torch.int32, device=dev))

    def call(T=3, F=2, K=60, size=S, metric=0, th=0.5, ws_bytes=None, null=None):
        a = [ptr(d['boxes']), ptr(d['score']), ptr(d['count']), ptr(d['tiles']), ptr(d['frame_off'])]
        o = [ptr(out['corners']), ptr(out['rows']), ptr(out['nrows']), ptr(out['src'])]
        w = ptr(ws)
        if null is not None:
            if null < 5:
                a[null] = None
            elif null == 5:
                w = None
            else:
                o[null - 6] = None
        return lib().fv_tile_merge(ctx.handle, *a, T, F, K, size, metric, th, w, ws.numel() * 8 if ws_bytes is None else ws_bytes, *o)
    bad = [dict(T=0), dict(F=0), dict(K=0), dict(K=513), dict(size=0), dict(metric=2), dict(metric=-1), dict(th=0.0), dict(th=-0.5),
           dict(th=1.0000001), dict(th=float('nan')), dict(ws_bytes=2 * 4096 * 32 - 1), dict(ws_bytes=0)] + [dict(null=i) for i in range(10)]
    for kw in bad:
        assert call(**kw) == -1, kw                                           # FV_ERR_INVALID
        assert b'fv_tile_merge' in lib().fv_last_error(ctx.handle), kw
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())                    # nothing was enqueued
    with pytest.raises(FvError, match=r'\(-1\).*merge_th'):
        postproc.tile_merge(ctx, d, d['tiles'], d['frame_off'], S, 'ios', 1.5)
    with pytest.raises(ValueError, match='metric'):
        postproc.tile_merge(ctx, d, d['tiles'], d['frame_off'], S, 'giou', 0.5)
    assert call() == 0                                                        # and the good call goes through
    torch.cuda.synchronize()
    assert out['nrows'].min().item() >= 0 and not bool((out['src'] == 7).all())


# ----------------------------------------------------------------------------- stream contract
def test_tile_merge_on_a_delayed_stream():
    """The harness of tests/stream_order.py on fv_tile_merge: exact, no host_sync.  Boxes and scores differ between the two
    problems, the geometry and counts do not.  nrows may tie: two random problems can keep the same number of boxes in every frame
    (60 of them in a crowded frame); src, the ranking, cannot."""
    def make(seed, dev):
        p = _problem(seed, [2, 30, 1], 60)
        shared = _problem(1, [2, 30, 1], 60)
        p['count'], p['tiles'] = shared['count'], shared['tiles']
        p['score'] = np.nan_to_num(p['score'], nan=0.0)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.items()}

    def call(ctx, p):
        return postproc.tile_merge(ctx, p, p['tiles'], p['frame_off'], S, 'ios', 0.5)
    case = so.Case('tile_merge', ('fv_tile_merge',), make, call, may_tie=('nrows',))
    assert case.exact and not case.host_sync
    so.run_delayed(case)


# ----------------------------------------------------------------------------- end to end at small size
SHAPES = [(200, 330), (330, 200), (150, 150), (260, 130)]
TILES = {'size': 128, 'overlap': 0.25}


def _conf(root, tiles=TILES, eval_batch=5, validate=None):
    hps = {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2, 'face_conf_th': 0.5,
           'nms_iou_th': 0.5, 'num_cands': 60, 'eval_batch_size': eval_batch}
    if tiles is not None:
        hps['tiles'] = tiles
    if validate is not None:
        hps['validate'] = validate
    return {'mode': 'test', 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False, 'hps': hps,
            'nn_arch': {'image_size': S, 'bb_info_c_size': 6}}


def _frames(root, n):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(21)
    names = []
    for k, (h, w) in enumerate(SHAPES[:n]):
        # smooth blobs rather than noise, so that the views differ in what the head makes of them
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 120 * np.sin(xx / rng.uniform(5, 30) + c) * np.cos(yy / rng.uniform(5, 30) - c) for c in range(3)], axis=2)
        names.append(os.path.join(root, 'frame_%02d.jpg' % k))
        Image.fromarray(img.astype(np.uint8)).save(names[-1], quality=92)
    return names


def _tune_head(fd, names):
    """Random weights, the head calibrated on every view of the test frames: every output channel is centred (a random head has a
    channel mean of several spatial spreads) and scaled to a spread of 0.25 around its bias -- objectness and class logits
    1.2 +- 0.25 (scores around 0.59 against the threshold 0.5: most cells of a view pass, not all), centres 0.5 +- 0.25 of a cell,
    sides 0.3 +- 0.25 of the view (positive widths and heights: the validation needs boxes that overlap something)."""
    d = fd.model.layers[-1]
    raws, keep = [data._pil_loader(n) for n in names], []
    postproc.letterbox_batch_device(fd.model.ctx, raws, S, fd.model.dev, keep=keep)
    crops = [(i,) + g for i, r in enumerate(raws) for g in data.tile_grid(r.shape[0], r.shape[1], fd.tiles)]
    x = postproc.letterbox_crops(fd.model.ctx, keep[0], crops, S)           # every view of every frame: tiles and whole frames
    fd.model.params[d['beta_off']:d['beta_off'] + 6] = 0
    y0 = fd.model.predict_device(x).cpu().numpy().astype(np.float64)
    k = 0.25 / float((y0 - y0.mean(axis=(0, 1, 2))).std())
    fd.model.params[d['w_off']:d['beta_off']] *= k
    for c, v in enumerate((1.2, 0.5, 0.5, 0.3, 0.3, 1.2)):
        fd.model.params[d['beta_off'] + c] = v - k * float(y0[..., c].mean())


def _compose(fd, raws, bs):
    """The public pieces in a row for one frame batch: the batch's frames on the device, tile_grid, ONE letterbox_crops over every
    view (the whole-frame views included), predict_device + decode_nms per chunk of `bs` views in view order (the network's fp32
    sums depend on the batch size -- tests/test_face_detector_gpu.py -- so the composition uses the chunks the contract names:
    at most eval_batch_size views, full wherever the count allows), the float64 merge on the host."""
    ctx, dev = fd.model.ctx, fd.model.dev
    keep = []
    postproc.letterbox_batch_device(ctx, raws, S, dev, keep=keep)
    grids = [data.tile_grid(r.shape[0], r.shape[1], fd.tiles) for r in raws]
    crops = [(i,) + g for i, grid in enumerate(grids) for g in grid]
    x = postproc.letterbox_crops(ctx, keep[0], crops, S)
    parts = []
    for c0 in range(0, len(crops), bs):
        y = fd.model.predict_device(x[c0:c0 + bs])
        r = postproc.decode_nms(ctx, y, S, fd.hps['face_conf_th'], fd.hps['nms_iou_th'], fd.hps['num_cands'])
        parts.append({k: v.cpu().numpy() for k, v in r.items()})
    res = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
    off = np.concatenate([[0], np.cumsum([len(g) for g in grids])])
    merged = ref.merge(res['boxes'], res['score'], res['count'], np.array(crops, np.int32), off, S, fd.tiles['metric'], fd.tiles['merge_th'])
    return merged, res, grids


def _csv_lines(name, merged, f):
    out = []
    for r in range(int(merged['nrows'][f])):
        x, y, w, h, s = merged['rows'][f, r]
        out.append(os.path.basename(name) + ',' + str(x) + ',' + str(y) + ',' + str(w) + ',' + str(h) + ',' + str(s) + '\n')
    return out


@pytest.fixture(scope='module')
def detector(tmp_path_factory):
    from face_vijnana_yolov3_amd import face_detection
    root = str(tmp_path_factory.mktemp('tiles'))
    names = _frames(root, 4)
    lines = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    for k, (h, w) in enumerate(SHAPES):          # six boxes of the detections' size per frame, on a 2 x 3 grid
        for j, (fx, fy) in enumerate((a, b) for b in (0.1, 0.4, 0.7) for a in (0.1, 0.5)):
            lines.append('%d,%s,%d,%.1f,%.1f,%.1f,%.1f' % (6 * k + j, os.path.basename(names[k]), j + 1, fx * w, fy * h, 36.0, 36.0))
    open(os.path.join(root, 'validation.csv'), 'w').write('\n'.join(lines) + '\n')
    old, cwd = face_detection.DEBUG, os.getcwd()
    face_detection.DEBUG = False
    os.chdir(root)
    try:
        fd = face_detection.FaceDetector(_conf(root))
        _tune_head(fd, names)
        yield fd, root, names
    finally:
        face_detection.DEBUG = old
        os.chdir(cwd)


def test_detect_frame_equals_the_composition(detector):
    fd, root, names = detector
    fd.hps['eval_batch_size'] = 5
    for name in names[:2]:
        raw = data._pil_loader(name)
        merged, res, grids = _compose(fd, [raw], 5)
        assert len(grids[0]) >= 7 and grids[0][-1] == (0, 0) + raw.shape[:2]
        assert int(merged['nrows'][0]) >= 2 and int((res['count'] > 0).sum()) >= 3           # several views saw something
        boxes = fd.detect_frame(raw)
        n = int(merged['nrows'][0])
        assert len(boxes) == n
        got = np.array([[b.xmin, b.ymin, b.xmax, b.ymax] for b in boxes], np.float64)
        assert got.tobytes() == merged['corners'][0, :n].tobytes()
        assert all(type(b.xmin) is np.float64 for b in boxes)
        src = merged['src'][0, :n]
        assert np.array_equal(np.array([b.classes[0] for b in boxes], np.float32), res['score'].reshape(-1)[src])
        assert np.array_equal(np.array([b.objness for b in boxes], np.float32), res['obj'].reshape(-1)[src])
        assert [float(b.get_score()) for b in boxes] == list(merged['rows'][0, :n, 4])
        assert len({int(s) // 60 for s in src}) >= 2                                          # boxes of more than one view survive


@pytest.mark.parametrize('eval_batch', [1, 5, 64])
def test_csv_of_test_equals_the_composition(detector, eval_batch):
    """test() over the 200 x 330 and the 330 x 200 frame, string for string, at eval_batch_size 1 (one frame per batch, one view
    per chunk), 5 (both frames in one batch, chunks that straddle the frames and a short last one) and 64 (one chunk)."""
    fd, root, names = detector
    sub = os.path.join(root, 'two_%d' % eval_batch)
    os.makedirs(sub)
    files = []
    for n in names[:2]:
        files.append(os.path.join(sub, os.path.basename(n)))
        open(files[-1], 'wb').write(open(n, 'rb').read())
    fd.hps['eval_batch_size'] = eval_batch
    fd.conf = dict(fd.conf, test_path=sub, output_file_path=os.path.join(sub, 'solution.csv'))
    want = []
    for c0 in range(0, len(files), eval_batch):
        chunk = files[c0:c0 + eval_batch]
        merged, _res, _grids = _compose(fd, [data._pil_loader(f) for f in chunk], eval_batch)
        for f, name in enumerate(chunk):
            want += _csv_lines(name, merged, f)
    assert len(want) >= 4
    fd.test()
    assert open(fd.conf['output_file_path']).readlines() == want


def test_a_frame_batch_cut_into_groups_gives_the_same_rows(detector, monkeypatch):
    """TILE_MAX_VIEWS below the batch's views: the frame batch is merged in two launches; rows as from the composition with the
    chunks restarted at the group boundary."""
    fd, root, names = detector
    fd.hps['eval_batch_size'] = 64
    raws = [data._pil_loader(n) for n in names[:2]]
    keep = []
    x, _ = postproc.letterbox_batch_device(fd.model.ctx, raws, S, fd.model.dev, keep=keep)
    n0 = len(data.tile_grid(raws[0].shape[0], raws[0].shape[1], fd.tiles))
    monkeypatch.setattr(type(fd), 'TILE_MAX_VIEWS', n0)
    got = fd._tiles_run(x, keep[0])
    for f in range(2):
        merged, _res, _g = _compose(fd, [raws[f]], 64)
        for k in OUT:
            assert got[k][f].cpu().numpy().tobytes() == merged[k][0].tobytes(), (f, k)


def test_csv_without_the_key_is_detect_batch_and_project_back(detector):
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    fd, root, names = detector
    sub = os.path.join(root, 'plain')
    os.makedirs(sub)
    files = []
    for n in names[:2]:
        files.append(os.path.join(sub, os.path.basename(n)))
        open(files[-1], 'wb').write(open(n, 'rb').read())
    conf = _conf(sub, tiles=None, eval_batch=5)
    plain = FaceDetector(conf)
    assert plain.tiles is None
    plain.model.params.copy_(fd.model.params); plain.model.state.copy_(fd.model.state)
    plain.test()
    raws = [data._pil_loader(f) for f in files]
    x, geoms = postproc.letterbox_batch_device(plain.model.ctx, raws, S, plain.model.dev)
    want = []
    for name, boxes, geom in zip(files, plain.detect_batch(x), geoms):
        plain._project_back(boxes, geom)
        for b in boxes[:60]:
            want.append(os.path.basename(name) + ',' + str(b.xmin) + ',' + str(b.ymin) + ',' + str(b.xmax - b.xmin) + ','
                        + str(b.ymax - b.ymin) + ',' + str(b.get_score()) + '\n')
    assert len(want) >= 2 and open(conf['output_file_path']).readlines() == want
    # detect_frame without the key: letterbox -> detect -> project back
    boxes = plain.detect_frame(raws[0])
    one = plain.detect_batch(x[:1])[0]
    plain._project_back(one, geoms[0])
    assert [(b.xmin, b.ymin, b.xmax, b.ymax, b.classes[0]) for b in boxes] == [(b.xmin, b.ymin, b.xmax, b.ymax, b.classes[0]) for b in one]
    assert len(boxes) >= 1


def test_validate_with_tiles_is_the_sweep_over_the_composition(detector):
    """Four frames and a synthetic validation.csv: validate() = tests/det_metric_ref.py's matching and sweep over the rows of the
    composition (precision and recall equal; AP within the rounding of the device's N-term trapezoid sum, the bound
    tests/test_validate_gpu.py holds fv_det_ap_sweep to)."""
    import pandas as pd
    fd, root, names = detector
    val = os.path.join(root, 'val')
    os.makedirs(val)
    for n in names:
        open(os.path.join(val, os.path.basename(n)), 'wb').write(open(n, 'rb').read())
    open(os.path.join(val, 'validation.csv'), 'w').write(open(os.path.join(root, 'validation.csv')).read())
    bs = 3
    fd.hps['eval_batch_size'] = bs
    ths = [0.05, 0.1, 0.2, 0.3, 0.5, 0.75]
    fd.validation = data.validate_conf({'path': val, 'iou_ths': ths}, val)
    fd._validator = None
    got = fd.validate()
    files = sorted(os.path.join(val, os.path.basename(n)) for n in names)
    rows = np.zeros((4, 60, 5)); nrows = np.zeros(4, np.int32)
    for c0 in range(0, 4, bs):
        chunk = files[c0:c0 + bs]
        merged, _res, _g = _compose(fd, [data._pil_loader(f) for f in chunk], bs)
        rows[c0:c0 + len(chunk)] = merged['rows']; nrows[c0:c0 + len(chunk)] = merged['nrows']
    gt_df = pd.read_csv(os.path.join(val, 'validation.csv'))
    gt, off, _m = dm.group_ground_truth(gt_df, [os.path.basename(f) for f in files], 'validation.csv')
    iou, flag = mref.match_rows(rows, nrows, gt, off)
    conf, ious = mref.compact(rows, nrows, iou, flag)
    _order, _counts, ap, prec, rec = mref.ap_sweep(conf, ious, ths, len(gt_df))
    N = len(conf)
    print('validate with tiles: rows per frame %r, frames with an overlapping pair %r' % (nrows.tolist(), flag.tolist()))
    assert N >= 4 and (ious > 0).sum() >= 1                                   # not vacuous
    assert got['n_det'] == N and got['n_images'] == 4 and got['n_gt'] == 24 and got['iou_ths'] == ths
    assert got['precision'] == [float(v) for v in prec] and got['recall'] == [float(v) for v in rec]
    err = np.abs(np.array(got['ap']) - ap)
    print('validate with tiles: N %d, AP %r, largest |AP - reference| %.3e' % (N, got['ap'], err.max()))
    assert (err <= N * 2.0 ** -53 * 4).all()
    assert got['ap'][0] > 0 and got['recall'][0] > 0                          # and the numbers are not all zero
