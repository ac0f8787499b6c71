"""The workspace contract of every network-level entry point (include/fv_hotpath.h at fv_workspace_bytes): the contents of the
workspace on entry are ignored, and nothing outside [workspace, workspace + bytes) is written.

Each entry point runs on guarded workspaces (tests/workspace_poison.py) from four states -- zero-filled twice, filled with
0xFF (NaN / -1), and left as a complete call of the same shape with other parameters, another input and another target left
it -- and every run is compared with the first zero-filled one.  There is no float64 oracle in here: test_net_gpu.py,
test_yolov3_gpu.py, test_fid_gpu.py and test_recon_gpu.py pin the same calls to it; this file pins them to themselves under
a workspace an ordinary test never sees.  The shapes are the smallest at which the schedules differ; the two training graphs
run under every option set that changes who writes or reads a kept tensor.

Bounds (two orders of the same atomics, as test_early_bn_fused_gpu.py uses them): inference is bit-identical; loss, BN state
and the published z / mean / invstd / scale / shift lie within 1e-6 of each tensor's largest magnitude; every parameter
tensor's gradient within 1e-5 of its own largest entry + 1e-9.
"""
import ctypes

import numpy as np
import pytest
import torch

import workspace_poison as wp

pytestmark = pytest.mark.gpu

STAT_REL = 1e-6
GRAD_REL, GRAD_FLOOR = 1e-5, 1e-9
OUT = 18                                  # three-scale head: 3 * (5 + 1 class)

# (name, options) -- one pytest parameter each; the mixed sets are the states in which exactly one of the two readers of
# a(0) / a(2) stages from z.  virt: a(0) and a(2) are not written (schedule.h EarlyIn::virt(): both readers apply the BN on load).
OPTION_SETS = [
    ('defaults', {}, True),
    ('early_bn_fused=0', {'early_bn_fused': 0}, False),
    ('early_bn_fused=2', {'early_bn_fused': 2}, False),          # the forward alone reads z
    ('early_bn_fused=4', {'early_bn_fused': 4}, False),          # the weight-gradient alone
    ('early_bn_fused=8', {'early_bn_fused': 8}, False),          # dz(0) formed on load alone
    ('early_bn_fused=6', {'early_bn_fused': 6}, True),           # both readers, dz(0) written
    ('conv_halo=0', {'conv_halo': 0}, False),
    ('wgrad_fused_taps=0', {'wgrad_fused_taps': 0}, False),
    ('conv_halo=0,wgrad_fused_taps=0', {'conv_halo': 0, 'wgrad_fused_taps': 0}, False),
    ('bn_in_1x1=0', {'bn_in_1x1': 0}, True),
    ('bn_in_1x1=2', {'bn_in_1x1': 2}, True),
    ('conv1x1_persist=0', {'conv1x1_persist': 0}, True),
    ('overlap=0', {'overlap': 0}, True),
    ('tail_split=0', {'tail_split': 0}, True),
]
OPTION_IDS = [o[0] for o in OPTION_SETS]


class _Options(object):
    """Set the context's options for a block and put back what they were."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.before = {k: self.ctx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            self.ctx.set_option(k, v)


_MODELS = {}
_PARAMS = {}


def _model(kind):
    if kind not in _MODELS:
        if kind == 'engine':
            from face_vijnana_yolov3_amd.engine import Engine
            _MODELS[kind] = Engine(0)
        elif kind == 'yolov3':
            from face_vijnana_yolov3_amd.yolov3 import Yolov3
            _MODELS[kind] = Yolov3(0, out_channels=OUT)
        elif kind == 'fid':
            from face_vijnana_yolov3_amd import face_identification as fi
            _MODELS[kind] = fi.FidModel(64, 0)
        else:
            from face_vijnana_yolov3_amd import face_identification as fi
            _MODELS[kind] = fi.ReconModel(32, 0)
    return _MODELS[kind]


def _set_params(kind, seed):
    """Synthetic parameters of `seed` (made once, kept on the device): gamma in [0.8, 1.2], |beta| in [0.5, 0.8] with both signs,
    so that a padding slot that received LeakyReLU(shift) instead of 0 would change every border output; the BN state at its
    initial values; for FidModel the dense layer too."""
    m = _model(kind)
    if (kind, seed) not in _PARAMS and kind == 'recon':
        # the snapshot create_face_reconst_model takes of an identifier, then BN vectors away from their fresh values
        from face_vijnana_yolov3_amd import face_identification as fi
        fid = fi.FidModel(m.image_size, 0)
        fid.init_synthetic(seed)
        fid.init_dense(seed)
        rec = fi.ReconModel.from_identifier(fid, seed=seed)
        g = torch.Generator().manual_seed(seed + 1000)
        for l in range(len(rec.layers)):
            for which in range(4):
                sl = rec.bn_slice(l, which)
                rec.params[sl] = (0.5 + torch.rand(sl.stop - sl.start, generator=g)).to(rec.dev)
        _PARAMS[(kind, seed)] = (rec.params.clone(), rec.state.clone())
    if (kind, seed) not in _PARAMS:
        m.init_synthetic(seed)
        g = torch.Generator().manual_seed(seed + 1000)
        p = m.params.cpu()
        for d in m.layers:
            if d['has_bn']:
                c = d['cout']
                p[d['gamma_off']:d['gamma_off'] + c] = 0.8 + 0.4 * torch.rand(c, generator=g)
                p[d['beta_off']:d['beta_off'] + c] = torch.where(torch.rand(c, generator=g) > 0.5, 1.0, -1.0) * (0.5 + 0.3 * torch.rand(c, generator=g))
        m.params.copy_(p)
        if kind == 'fid':
            m.init_dense(seed)
            m.dense_bias().copy_(0.1 * torch.rand(64, generator=g))
        _PARAMS[(kind, seed)] = (m.params.clone(), m.state.clone())
    p, st = _PARAMS[(kind, seed)]
    m.params.copy_(p)
    m.state.copy_(st)
    m.bn_updates = 0
    return m


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).cuda()


# ------------------------------------------------------------------------------------------------------- kept tensors of a step
_KEPT = {}


def _kept(model, ws, B, S):
    """{(layer, code): view} of z, a, mean, invstd, scale, shift (codes 0..5) of every BN layer inside `ws`, a training workspace
    of the model or a copy of one."""
    key = (id(model), B, S)
    if key not in _KEPT:
        # FidModel: the plan of its (first) tower lies first in the workspace, at fv_train_workspace_tensor's offsets
        tensor = getattr(model, '_workspace_tensor', None) or _model('engine')._workspace_tensor
        where = {}
        for l, d in enumerate(model.layers):
            if d['has_bn']:
                for code in range(6):
                    off, cnt = ctypes.c_size_t(0), ctypes.c_int64(0)
                    assert tensor(B, S, l, code, ctypes.byref(off), ctypes.byref(cnt)) == 0
                    where[(l, code)] = (off.value, cnt.value)
        _KEPT[key] = where
    return {k: ws[o:o + 4 * n].view(torch.float32) for k, (o, n) in _KEPT[key].items()}


CODES = ('z', 'a', 'mean', 'invstd', 'scale', 'shift')


def _check_training(model, B, S, outs, virt, extra=(), exact=(), hows=('zero2', 'nan', 'stale'), grown=False):
    """outs: contract_runs' result of a training call whose outputs are loss, state, grads, ws (a copy of the workspace) and the
    names in `extra` (float tensors held to STAT_REL) and `exact` (integer tensors that must be equal).  virt: a(0) and a(2) are
    expected unwritten (True), written (False), or either as long as each is one of the two wholly (None).  grown: the 'stale'
    call ran another batch size in the same buffer.

    Measured on the MI355X over all option sets and shapes of this file: the statistics, z and the loss came out bit-identical in
    every run (ratio 0); over two runs of the file the worst gradient ratio of two zero-filled runs was 2.6e-6 (dW(0) at B = 6,
    S = 128), of a poisoned run against the zero-filled one 2.9e-6 (the same tensor) -- the 1e-5 bound holds for every tensor
    without the head-room rule."""
    clean = outs['zero']
    ckept = _kept(model, clean['ws'], B, S)
    segs = wp.grad_segments(model)
    for how in hows:
        o = outs[how]
        kept = _kept(model, o['ws'], B, S)
        # ---- which a(l) hold no data: a(0) / a(2) alone, wholly, and exactly where both of their readers apply the BN on load.
        # Both poisoned states start from 0xFF: a tensor that still holds it was not written, and -- the outputs being finite --
        # not read either (in a zero-filled workspace an unwritten a(l) holds zeros, which are finite).
        holds_none = set()
        if how == 'stale' and grown:
            holds_none = {0, 2} if virt else set()   # the longer batch wrote there in its own layout: nothing to tell
        elif how != 'zero2':
            holds_none = {l for (l, code), t in kept.items() if code == 1 and wp.untouched(t)}
            assert holds_none <= {0, 2}, (how, sorted(holds_none))
            if virt is not None:
                assert holds_none == ({0, 2} if virt else set()), (how, sorted(holds_none), virt)
        # ---- finite: every output, every tensor the step documents as written
        for name in ('loss', 'state', 'grads') + tuple(extra):
            wp.assert_finite('%s: %s' % (how, name), o[name])
        for (l, code), t in kept.items():
            if not (code == 1 and l in holds_none):
                wp.assert_finite('%s: %s(%d)' % (how, CODES[code], l), t)
        # ---- close to the zero-filled run
        worst = dict(stat=(0.0, ''), grad=(0.0, ''))
        for name in ('loss', 'state') + tuple(extra):
            r = wp.assert_within('%s: %s' % (how, name), o[name], clean[name], STAT_REL)
            worst['stat'] = max(worst['stat'], (r, name))
        for name in exact:
            assert torch.equal(o[name], clean[name]), (how, name, o[name], clean[name])
        for (l, code), t in kept.items():
            if code != 1:
                name = '%s(%d)' % (CODES[code], l)
                r = wp.assert_within('%s: %s' % (how, name), t, ckept[(l, code)], STAT_REL)
                worst['stat'] = max(worst['stat'], (r, name))
        for name, s in segs:
            r = wp.assert_within('%s: %s' % (how, name), o['grads'][s], clean['grads'][s], GRAD_REL, GRAD_FLOOR)
            worst['grad'] = max(worst['grad'], (r, name))
        print('B=%d S=%d %-5s to clean: statistics %.2e (%s), gradients %.2e (%s)'
              % (B, S, how, worst['stat'][0], worst['stat'][1], worst['grad'][0], worst['grad'][1]))


def _check_inference(outs):
    clean = outs['zero']
    for how in ('zero2', 'nan', 'stale'):
        for name, t in outs[how].items():
            wp.assert_finite('%s: %s' % (how, name), t)
            assert torch.equal(t, clean[name]), (how, name, wp.ratio(t, clean[name]))


# ------------------------------------------------------------------------------------------------------------------ Engine
def _engine_train(B, S, virt):
    """One fv_train_step at (B, S) from the four workspace states."""
    eng = _model('engine')
    wp.release(eng)
    x, yt = _rand((B, S, S, 3), 10 * B + S), _rand((B, S // 32, S // 32, 6), 10 * B + S + 1)
    x2, yt2 = _rand((B, S, S, 3), 10 * B + S + 2), _rand((B, S // 32, S // 32, 6), 10 * B + S + 3)
    eng.ensure_optimizer()
    ws = eng._workspace(B, S, True)
    assert ws.numel() == eng._workspace_bytes(B, S, 1)

    def call():
        _set_params('engine', 29)
        loss = eng.forward_backward(x, yt)
        torch.cuda.synchronize()
        return dict(loss=loss.clone(), state=eng.state.clone(), grads=eng.grads.clone(), ws=eng._workspace(B, S, True).clone())

    def stale():
        _set_params('engine', 31)
        eng.forward_backward(x2, yt2)
        torch.cuda.synchronize()
    outs = wp.contract_runs(eng, call, stale)
    _check_training(eng, B, S, outs, virt)
    wp.release(eng)


# (2, 64): 2 x 2 cells, every tile partial; (3, 96): odd grids; (6, 128): tail-split tile counts in the training forward
@pytest.mark.parametrize('name,opts,virt', OPTION_SETS, ids=OPTION_IDS)
def test_engine_train_step_ignores_what_the_workspace_held(name, opts, virt):
    eng = _model('engine')
    with _Options(eng.ctx, opts):
        for B, S in ((2, 64), (3, 96), (6, 128)):
            _engine_train(B, S, virt)


# (1, 96): the conv_small / conv_bm64 paths of a batch-1 call; (3, 64)
@pytest.mark.parametrize('B,S', [(1, 96), (3, 64)])
def test_engine_inference_is_bit_identical_whatever_the_workspace_held(B, S):
    eng = _model('engine')
    wp.release(eng)
    x, x2 = _rand((B, S, S, 3), 50 + B), _rand((B, S, S, 3), 60 + B)
    eng._workspace(B, S, False)

    def call():
        _set_params('engine', 29)
        y = eng.predict_device(x)
        feat, yh = eng.predict_base_device(x, with_head=True)
        torch.cuda.synchronize()
        return dict(y=y, feat=feat, y_of_base=yh)

    def stale():
        _set_params('engine', 31)
        eng.predict_device(x2)
        eng.predict_base_device(x2, with_head=True)
        torch.cuda.synchronize()
    outs = wp.contract_runs(eng, call, stale)
    _check_inference(outs)
    assert torch.equal(outs['zero']['y'], outs['zero']['y_of_base'])
    wp.release(eng)


# ------------------------------------------------------------------------------------------------------------------ Yolov3
def _yolo_heads(m, ws, B, S):
    """The raw head outputs and their padded gradients inside `ws` (fv_yolov3_train_workspace_head)."""
    from face_vijnana_yolov3_amd._lib import lib
    out = {}
    for scale in range(3):
        for which, name in ((0, 'y'), (1, 'dy')):
            off, cnt = ctypes.c_size_t(0), ctypes.c_int64(0)
            assert lib().fv_yolov3_train_workspace_head(B, S, OUT, scale, which, ctypes.byref(off), ctypes.byref(cnt)) == 0
            out['%s%d' % (name, scale)] = ws[off.value:off.value + 4 * cnt.value].view(torch.float32).clone()
    return out


def _det_targets(B, S, counts, seed):
    import yolo_det_loss_ref as ref
    from face_vijnana_yolov3_amd import data
    _, ts = ref.planted_case(S, counts, OUT // 3 - 5, seed, data.YOLO_ANCHORS)
    return [torch.from_numpy(t).cuda() for t in ts]


def _yolo_train(det, virt):
    from face_vijnana_yolov3_amd import data
    m = _model('yolov3')
    wp.release(m)
    B, S = 2, 64
    x, x2 = _rand((B, S, S, 3), 71), _rand((B, S, S, 3), 72)
    if det:
        m.det_loss = data.det_loss_conf({'yolo': dict(box_loss='giou', max_boxes=4)})
        t, t2 = _det_targets(B, S, (4, 1), 8), _det_targets(B, S, (1, 5), 9)
        m._det_buffers(B, S)                       # the detection scratch: guarded and poisoned with the workspace
        assert m._det_scratch is not None
    else:
        m.det_loss = None
        t = [_rand((B, S // d, S // d, OUT), 73 + d) for d in (32, 16, 8)]
        t2 = [_rand((B, S // d, S // d, OUT), 74 + d) for d in (32, 16, 8)]
    m.ensure_optimizer()
    m._workspace(B, S, True)

    def call():
        _set_params('yolov3', 33)
        loss = m.forward_backward(x, t)
        torch.cuda.synchronize()
        ws = m._workspace(B, S, True).clone()
        out = dict(loss=loss.clone(), state=m.state.clone(), grads=m.grads.clone(), ws=ws, **_yolo_heads(m, ws, B, S))
        if det:
            out['det_stats'] = m.det_stats.clone()
        return out

    def stale():
        _set_params('yolov3', 35)
        m.forward_backward(x2, t2)
        torch.cuda.synchronize()
    try:
        outs = wp.contract_runs(m, call, stale)
        assert len(wp.workspaces(m)) == (2 if det else 1)
        heads = tuple('%s%d' % (n, s) for n in ('y', 'dy') for s in range(3))
        _check_training(m, B, S, outs, virt, extra=heads + (('det_stats',) if det else ()))
    finally:
        m.det_loss = None
        wp.release(m)


@pytest.mark.parametrize('name,opts,virt', OPTION_SETS, ids=OPTION_IDS)
def test_yolov3_train_step_ignores_what_the_workspace_held(name, opts, virt):
    m = _model('yolov3')
    with _Options(m.ctx, opts):
        _yolo_train(False, virt)                   # the mse step
        _yolo_train(True, virt)                    # fv_yolov3_train_step_det: the detection scratch is covered too


def test_yolov3_inference_is_bit_identical_whatever_the_workspace_held():
    m = _model('yolov3')
    wp.release(m)
    B, S = 1, 64
    x, x2 = _rand((B, S, S, 3), 81), _rand((B, S, S, 3), 82)
    m._workspace(B, S, False)

    def call():
        _set_params('yolov3', 33)
        ys = m.predict_device(x)
        torch.cuda.synchronize()
        return dict(y13=ys[0], y26=ys[1], y52=ys[2])

    def stale():
        _set_params('yolov3', 35)
        m.predict_device(x2)
        torch.cuda.synchronize()
    _check_inference(wp.contract_runs(m, call, stale))
    wp.release(m)


# ---------------------------------------------------------------------------------------------------------------- FidModel
def test_fid_triplet_step_ignores_what_the_workspace_held():
    m = _model('fid')
    wp.release(m)
    B, S = 2, 64
    xs = [_rand((B, S, S, 3), 90 + i) for i in range(3)]
    xs2 = [_rand((B, S, S, 3), 95 + i) for i in range(3)]
    m.ensure_optimizer()
    m._workspace(B, S, True)

    def call():
        _set_params('fid', 41)
        loss = m.forward_backward(*xs)
        torch.cuda.synchronize()
        return dict(loss=loss.clone(), state=m.state.clone(), grads=m.grads.clone(), ws=m._workspace(B, S, True).clone())

    def stale():
        _set_params('fid', 43)
        m.forward_backward(*xs2)
        torch.cuda.synchronize()
    outs = wp.contract_runs(m, call, stale)
    _check_training(m, B, S, outs, True)         # the kept tensors of the anchor's tower
    wp.release(m)


def test_fid_extract_is_bit_identical_whatever_the_workspace_held():
    m = _model('fid')
    wp.release(m)
    B, S = 3, 64
    x, x2 = _rand((B, S, S, 3), 101), _rand((B, S, S, 3), 102)
    m._workspace(B, S, False)

    def call():
        _set_params('fid', 41)
        ids = m.extract_device(x)
        torch.cuda.synchronize()
        return dict(ids=ids)

    def stale():
        _set_params('fid', 43)
        m.extract_device(x2)
        torch.cuda.synchronize()
    _check_inference(wp.contract_runs(m, call, stale))
    wp.release(m)


def _labelled_step(m, step, alloc, x5, lab5, x8, lab8, names_f, names_i):
    """The 8-then-5 sequence of a PK epoch: the buffer is grown to 8 rows, then a short batch of 5 runs in it with another
    layout over the longer batch's data.  The M = 5 result on the grown buffer -- NaN-filled, zero-filled, and as the M = 8
    step with other data left it -- is compared with M = 5 on a zeroed buffer of its own."""
    S = 64
    m.ensure_optimizer()

    def call():
        _set_params('fid', 41)
        loss, sel = step(x5, lab5)
        torch.cuda.synchronize()
        out = dict(loss=loss.clone(), state=m.state.clone(), grads=m.grads.clone(), ws=m._ws[KEYS[alloc]].clone())
        out.update({k: v.clone() for k, v in sel.items()})
        if getattr(m, 'class_grads', None) is not None and alloc == 'cls':
            out['class_grads'] = m.class_grads.clone()
        return out

    def stale():
        _set_params('fid', 43)
        step(x8, lab8)
        torch.cuda.synchronize()
    wp.release(m)
    getattr(m, ALLOC[alloc])(5)
    own = wp.contract_runs(m, call, stale, hows=('zero', 'zero2'))
    n5 = m._ws[KEYS[alloc]].numel()
    wp.release(m)
    getattr(m, ALLOC[alloc])(8)
    grown = wp.contract_runs(m, call, stale, hows=('zero2', 'nan', 'stale'))
    n8 = m._ws[KEYS[alloc]].numel()
    assert n8 > n5 and getattr(m, ALLOC[alloc])(5).numel() == n8        # the short batch ran in the grown buffer
    outs = dict(zero=own['zero'], zero2=own['zero2'], nan=grown['nan'], stale=grown['stale'])
    for o in list(outs.values()) + [grown['zero2']]:
        o['ws'] = o['ws'][:n5]
    wp.release(m)
    _check_training(m, 5, S, outs, True, extra=names_f, exact=names_i, grown=True)
    outs['zero2'] = grown['zero2']                 # and the zero-filled grown buffer
    _check_training(m, 5, S, outs, True, extra=names_f, exact=names_i, grown=True)
    return outs


KEYS = dict(batch=(0, 64, 'labelled_batch'), cls=(0, 64, 'classified_batch'))
ALLOC = dict(batch='_batch_workspace', cls='_cls_workspace')
# every row of a known subject with a positive and a negative in the batch: every anchor is valid, every selection output finite
SUBJECTS8 = np.asarray([0, 0, 1, 1, 2, 2, 3, 3], np.int32)
SUBJECTS5 = np.asarray([4, 7, 7, 4, 7], np.int32)


@pytest.mark.parametrize('mode', ['batch_hard', 'batch_semi_hard'])
def test_fid_batch_step_on_a_grown_buffer(mode):
    m = _model('fid')
    x5, x8 = _rand((5, 64, 64, 3), 111), _rand((8, 64, 64, 3), 112)

    def step(x, sub):
        loss = m.forward_backward_batch(x, sub, mode)
        return loss, m.batch_selection
    outs = _labelled_step(m, step, 'batch', x5, SUBJECTS5, x8, SUBJECTS8, ('d_ap', 'd_an'), ('pos_index', 'neg_index', 'kind'))
    assert bool((outs['zero']['kind'] != 3).all())


def test_fid_class_step_on_a_grown_buffer():
    m = _model('fid')
    m.init_classes(7, 3)                           # an odd class count: the coefficient rows carry a pad column
    kernel = m.class_kernel.clone()
    x5, x8 = _rand((5, 64, 64, 3), 121), _rand((8, 64, 64, 3), 122)

    def step(x, lab):
        m.class_kernel.copy_(kernel if len(lab) == 5 else kernel.flip(0))
        loss = m.forward_backward_classes(x, lab, 'arcface')
        return loss, m.class_selection
    try:
        outs = _labelled_step(m, step, 'cls', x5, np.asarray([6, 0, 3, 3, 1], np.int32), x8, np.asarray([1, 2, 3, 4, 5, 6, 0, 0], np.int32),
                              ('cos_t',), ('pred',))
        clean = outs['zero']['class_grads']
        for how in ('zero2', 'nan', 'stale'):
            wp.assert_finite('%s: class_grads' % how, outs[how]['class_grads'])
            r = wp.assert_within('%s: class kernel gradient' % how, outs[how]['class_grads'], clean, GRAD_REL, GRAD_FLOOR)
            print('%-5s to clean: class kernel gradient %.2e' % (how, r))
    finally:
        m.class_kernel = m.class_grads = m.class_m = m.class_v = None


# -------------------------------------------------------------------------------------------------------------- ReconModel
def test_recon_forward_is_bit_identical_whatever_the_workspace_held():
    m = _model('recon')
    wp.release(m)
    N, S = 3, 32
    ids = torch.nn.functional.normalize(_rand((N, 64), 131), dim=1)
    ids2 = torch.nn.functional.normalize(_rand((N, 64), 132), dim=1)
    m._workspace(N, S, False)

    def call():
        _set_params('recon', 51)
        out = m.predict_device(ids)
        torch.cuda.synchronize()
        return dict(image=out)

    def stale():
        _set_params('recon', 53)
        m.predict_device(ids2)
        torch.cuda.synchronize()
    outs = wp.contract_runs(m, call, stale)
    _check_inference(outs)
    assert float(outs['zero']['image'].abs().max()) > 0
    wp.release(m)


# ------------------------------------------------------------------------------------------- memory lent to single operators
class _Lent(object):
    """A fake model around one lent buffer, so that the operator's scratch gets guards and fills like a workspace."""

    def __init__(self, t):
        self._ws = {'lent': t}

    @property
    def t(self):
        return self._ws['lent']


def _lent_runs(nbytes, run, fills=('zero', 'nan'), dtype=torch.uint8):
    """run(buffer) -> dict of outputs, once per fill of the guarded buffer; every output must equal the zero-filled run's."""
    holder = wp.guarded(_Lent(torch.empty(nbytes // torch.empty(0, dtype=dtype).element_size(), dtype=dtype, device='cuda')))
    outs = {}
    for how in fills:
        wp.poison(holder, how)
        outs[how] = run(holder.t)
        torch.cuda.synchronize()
        wp.check_guards(holder)
    for how in fills[1:]:
        for name, t in outs[how].items():
            wp.assert_finite('%s: %s' % (how, name), t)
            assert torch.equal(t, outs['zero'][name]), (how, name)
    return outs


def test_conv_tail_split_does_not_read_the_lent_scratch_before_writing_it():
    """fv_set_conv_scratch at H = 100 (157 output tiles, every one cut into K slices -- test_ops_gpu.py's
    test_conv_tail_split_with_lent_scratch pins these launches to float64): forward with statistics, the fused epilogue and the
    stride-1 data-gradient are bit-identical whether the scratch held zeros or 0xFF."""
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import Context
    ctx = Context(0)
    B, H, cin, cout = 2, 100, 256, 128
    x, w = _rand((B, H, H, cin), 141) * 2 - 1, _rand((cout, 3, 3, cin), 142) * 0.2 - 0.1
    scale, shift, skip = _rand((cout,), 143) + 0.5, _rand((cout,), 144) * 2 - 1, _rand((B, H, H, cout), 145)
    w2, dy = _rand((cin, 3, 3, cout), 146) * 0.2 - 0.1, _rand((B, H, H, cin), 147) * 2 - 1
    plain, _, _ = ops.conv2d_forward(ctx, x, w, stride=1, stats=True)

    def run(scratch):
        ctx.set_conv_scratch(scratch)
        try:
            out, psum, psq = ops.conv2d_forward(ctx, x, w, stride=1, stats=True)
            fused = ops.conv2d_forward(ctx, x, w, 1, scale, shift, 0.1, skip)
            dgrad = ops.conv2d_dgrad(ctx, dy, w2, (H, H), 1)
        finally:
            ctx.set_conv_scratch(None)
        return dict(out=out, psum=psum, psq=psq, fused=fused, dgrad=dgrad)
    outs = _lent_runs(64 << 20, run)
    assert not torch.equal(outs['zero']['out'], plain)       # the split really ran


def test_margin_softmax_does_not_read_its_workspace_before_writing_it():
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import Context, lib
    ctx = Context(0)
    M, C = 21, 301                                 # rows beyond one 16-row tile, an odd class count over two dU chunks
    pre = _rand((M, 64), 151) - 0.3
    u = torch.nn.functional.normalize(torch.relu(pre) + 1e-3, dim=1).contiguous()
    W = (_rand((C, 64), 152) - 0.5).contiguous()
    labels = torch.from_numpy(np.random.default_rng(153).integers(-1, C, M).astype(np.int32)).cuda()
    need = int(lib().fv_fid_margin_workspace_bytes(M, C))

    def run(ws):
        return ops.fid_margin_softmax_loss_grad(ctx, pre, u, labels, W, kind=1, margin=0.5, workspace=ws)
    _lent_runs(need, run)


def test_det_loss_does_not_read_its_scratch_before_writing_it():
    import yolo_det_loss_ref as ref
    from face_vijnana_yolov3_amd import data, ops
    from face_vijnana_yolov3_amd._lib import Context, lib
    ctx = Context(0)
    S, counts, ncls, cpad = 96, (1, 5, 4), 4, 32
    conf = data.det_loss_conf({'yolo': dict(box_loss='giou', max_boxes=4)})
    ys, ts = ref.planted_case(S, counts, ncls, 3, data.YOLO_ANCHORS)
    yd = [torch.from_numpy(y).cuda().reshape(-1, 3 * (5 + ncls)) for y in ys]
    td = [torch.from_numpy(t).cuda().reshape(-1, 3 * (5 + ncls)) for t in ts]
    need = int(lib().fv_yolo_det_scratch_bytes(len(counts), S, 4))

    def run(scratch):
        loss, dys, stats = ops.yolo_det_loss_grad(ctx, yd, td, len(counts), S, ncls, cpad, conf, scratch=scratch)
        return dict(loss=loss, stats=stats, dy0=dys[0], dy1=dys[1], dy2=dys[2])
    outs = _lent_runs((need + 7) // 8 * 8, run, dtype=torch.float64)
    assert float(outs['zero']['stats'][10]) == 1.0                     # the image with five boxes lost one to the cap


def test_jpeg_encoder_does_not_read_its_workspace_before_writing_it(monkeypatch):
    """The encoder's workspace carries counts and offsets the later launches index with: a pre-filled buffer (0xFF, then 0x00)
    gives the bytes of a fresh one -- Pillow's, where this Pillow is built on libjpeg-turbo."""
    import io
    from PIL import Image, features
    from face_vijnana_yolov3_amd import jpeg
    from face_vijnana_yolov3_amd._lib import Context
    ctx = Context(0)
    rng = np.random.default_rng(161)
    raws = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((17, 23), (64, 96), (1, 1), (40, 56))]
    raws.append(np.full((33, 16, 3), 255, np.uint8))                   # FF bytes in the scan: the stuffing pass has work
    offs = np.cumsum([0] + [r.size for r in raws])[:-1].tolist()
    hw = [v for r in raws for v in r.shape[:2]]
    buf = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws])).cuda()
    fresh = jpeg.encode_batch(ctx, buf, offs, hw, buf.device)
    make = jpeg.encode_workspace
    for fill in (0xFF, 0x00):
        holders = []

        def prefilled(hw_, device):
            h = wp.guarded(_Lent(make(hw_, device)))
            h.t.fill_(fill)
            holders.append(h)
            return h.t
        monkeypatch.setattr(jpeg, 'encode_workspace', prefilled)
        got = jpeg.encode_batch(ctx, buf, offs, hw, buf.device)
        monkeypatch.setattr(jpeg, 'encode_workspace', make)
        assert len(holders) == 1
        wp.check_guards(holders[0])
        assert got == fresh, fill
    if features.check_feature('libjpeg_turbo'):
        for r, g in zip(raws, fresh):
            f = io.BytesIO()
            Image.fromarray(r).save(f, 'JPEG')
            assert g == f.getvalue(), r.shape
