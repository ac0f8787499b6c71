"""The margin softmax on the GPU: fv_fid_margin_softmax_loss_grad against its numpy restatement
(tests/margin_softmax_ref.py) on the same float inputs within the bounds of test_fid_batch_gpu.py::_compare, fv_fid_cls_train_step
against the float64 oracle with test_fid_gpu.py's rules, and FaceIdentifier.train() with hps['margin_softmax'] in the three input
tiers."""
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import crop_store as cs
from face_vijnana_yolov3_amd import face_identification as fi
import margin_softmax_ref as ref
import test_fid_gpu as fg
import test_fid_mining_gpu as mg

pytestmark = pytest.mark.gpu

U23, U24 = 2.0 ** -23, 2.0 ** -24
FV_ERR_INVALID, FV_ERR_WORKSPACE = -1, -3
ORDER = ('loss', 'dE', 'dbias', 'dW', 'pred', 'cos_t')
KINDS = [ref.KIND_COSFACE, ref.KIND_ARCFACE]


def _ctx():
    return fg._model(64).ctx


def _filled(M, C):
    """Outputs holding values the operator never writes: whatever is still there afterwards was not touched."""
    return dict(loss=torch.full((1,), float('nan')).cuda(), dE=torch.full((M, 64), float('nan')).cuda(),
                dbias=torch.full((64,), float('nan')).cuda(), dW=torch.full((C, 64), float('nan')).cuda(),
                pred=torch.full((M,), -7, dtype=torch.int32).cuda(), cos_t=torch.full((M,), -7.5, dtype=torch.float64).cuda())


def _run(pre, u, labels, W, kind, scale=30.0, margin=None, weight=1.0):
    from face_vijnana_yolov3_amd import ops
    margin = ref.DEFAULT_MARGIN[kind] if margin is None else margin
    o = ops.fid_margin_softmax_loss_grad(_ctx(), torch.from_numpy(pre).cuda(), torch.from_numpy(u).cuda(),
                                         torch.from_numpy(np.asarray(labels, np.int32)).cuda(), torch.from_numpy(W).cuda(), kind, scale,
                                         margin, weight, out=_filled(len(pre), len(W)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _compare(got, want, M, what):
    """pred: equality on every row.  cos_t 1e-12 absolute (NaN where the restatement has NaN).  Loss 2^-23 relative; dE and dW
    2^-23 |ref| + 1e-12 max|ref|; dbias M 2^-24 sum|dE column| + 2^-23 |ref|.  Every figure is printed before it is asserted."""
    nan = np.isnan(want['cos_t'])
    e_ct = np.abs(np.where(nan, 0.0, got['cos_t']) - np.where(nan, 0.0, want['cos_t']))
    loss, rl = float(got['loss'][0]), float(want['loss'])
    err, lim = {}, {}
    for k in ('dE', 'dW'):
        err[k] = np.abs(got[k].astype(np.float64) - want[k])
        lim[k] = U23 * np.abs(want[k]) + 1e-12 * np.abs(want[k]).max()
    e_db = np.abs(got['dbias'].astype(np.float64) - want['dbias'])
    lim_db = M * U24 * np.abs(want['dE']).sum(0) + U23 * np.abs(want['dbias'])
    worst = lambda e, l: float((e / np.maximum(l, 1e-300)).max()) if e.size else 0.0
    print('%s: loss %.9g ref %.9g; worst err/limit dE %.3g, dW %.3g, dbias %.3g; cos_t worst %.3g; pred differs in %d rows; V %d'
          % (what, loss, rl, worst(err['dE'], lim['dE']), worst(err['dW'], lim['dW']), worst(e_db, lim_db), e_ct.max(),
             int((got['pred'] != want['pred']).sum()), want['V']))
    assert np.array_equal(got['pred'], want['pred']), (what, np.flatnonzero(got['pred'] != want['pred'])[:8])
    assert np.array_equal(np.isnan(got['cos_t']), nan) and (e_ct <= 1e-12).all(), what
    assert abs(loss - rl) <= U23 * abs(rl), what
    for k in ('dE', 'dW'):
        assert np.isfinite(got[k]).all() and (err[k] <= lim[k]).all(), (what, k)
    assert (e_db <= lim_db).all(), what


# ----------------------------------------------------------------------------- 1. the operator on random batches
# a wave and a workgroup stride with one element to either side, VGGFace2's class count: the diagonal of the two lists and three more
SHAPES = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (257, 1000), (1024, 8631), (1024, 2), (1, 8631)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,C', SHAPES)
def test_margin_softmax_loss_and_gradient(M, C, kind):
    pre, u, labels, W, want, seed = ref.searched_case(M, C, kind)
    m = ref.DEFAULT_MARGIN[kind]
    # asserted on the restatement, before the device is looked at
    assert ref.well_separated(want, m, C, gap=1e-9, branch=1e-6), seed
    if M >= 63:
        assert M / 14 < (labels < 0).sum() < M / 4 and (pre[M // 2] <= 0).all() and labels[M // 2] >= 0 and not want['dE'][M // 2].any()
    if C >= 2:
        assert not W[C - 1].any() and labels[0] == C - 1 and want['cos_t'][0] == 0.0
    got = _run(pre, u, labels, W, kind)
    _compare(got, want, M, 'M=%d C=%d kind=%d seed=%d' % (M, C, kind, seed))
    # the gradient weight is a factor: 0.25 scales every stored bit pattern exactly and leaves the rest alone
    got4 = _run(pre, u, labels, W, kind, weight=0.25)
    for k in ('loss', 'pred', 'cos_t'):
        assert np.array_equal(got4[k].view(np.uint8), got[k].view(np.uint8)), k
    for k in ('dE', 'dbias', 'dW'):
        assert np.array_equal(got4[k], got[k] * np.float32(0.25)), k
    # the same inputs give the same bits
    again = _run(pre, u, labels, W, kind)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k


# ----------------------------------------------------------------------------- 2. hand cases
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', sorted(ref.hand_cases()))
def test_margin_softmax_hand_case(name, kind):
    c = ref.hand_cases()[name]
    u = ref.l2n_relu(c['pre'])
    want = ref.stored(ref.margin_softmax(c['pre'], u, c['labels'], c['W'], kind, 30.0, ref.DEFAULT_MARGIN[kind]))
    got = _run(c['pre'], u, c['labels'], c['W'], kind)
    _compare(got, want, len(u), '%s kind=%d' % (name, kind))
    if name in ('one_class', 'all_unknown'):
        assert got['loss'][0] == 0.0 and not got['dE'].any() and not got['dbias'].any() and not got['dW'].any()
    if name == 'dead_row':
        assert not got['dE'][1].any() and got['cos_t'][1] == 0.0
    if name == 'target_cosine_one':
        assert got['cos_t'][0] == 1.0
    if name == 'target_cosine_minus_one':
        assert got['cos_t'][0] == -1.0


def test_a_label_beyond_the_classes_is_an_unknown_row_with_pred_minus_2():
    pre, labels, W = ref.random_case(6, 4, 8, unknown=0.0)
    labels[3] = 4
    u = ref.l2n_relu(pre)
    want = ref.stored(ref.margin_softmax(pre, u, labels, W, 0, 30.0, 0.35))
    got = _run(pre, u, labels, W, 0)
    assert got['pred'][3] == -2 and np.isnan(got['cos_t'][3]) and not got['dE'][3].any()
    _compare(got, want, 6, 'label 4 of 4 classes')


# ----------------------------------------------------------------------------- 3. refused arguments
def test_refused_arguments_leave_the_outputs_untouched():
    from face_vijnana_yolov3_amd._lib import lib, ptr
    M, C = 6, 5
    pre, labels, W = ref.random_case(M, C, 5)
    pre, u = torch.from_numpy(pre).cuda(), torch.from_numpy(ref.l2n_relu(pre)).cuda()
    lab, W = torch.from_numpy(labels).cuda(), torch.from_numpy(W).cuda()
    o = _filled(1025, C)
    keep = {k: v.clone() for k, v in o.items()}
    ws = torch.empty(int(lib().fv_fid_margin_workspace_bytes(1024, C)), dtype=torch.uint8).cuda()
    big = torch.zeros((1025, 64)).cuda()

    def call(pre=pre, u=u, lab=lab, W=W, M=M, C=C, kind=0, scale=30.0, margin=0.35, weight=1.0, ws=ws, ws_bytes=None, null=None):
        outs = [None if k == null else ptr(o[k]) for k in ORDER]
        ins = [None if k == null else ptr(v) for k, v in (('pre', pre), ('u', u), ('lab', lab))]
        return lib().fv_fid_margin_softmax_loss_grad(_ctx().handle, ins[0], ins[1], ins[2], M, None if null == 'W' else ptr(W), C, kind,
                                                     scale, margin, weight, None if null == 'ws' else ptr(ws),
                                                     ws.numel() if ws_bytes is None else ws_bytes, *outs)
    nan, inf = float('nan'), float('inf')
    bad = [dict(M=0), dict(M=-1), dict(M=1025, pre=big, u=big, lab=torch.zeros(1025, dtype=torch.int32).cuda()), dict(C=0), dict(C=-1),
           dict(C=32769), dict(kind=2), dict(kind=-1), dict(scale=0.0), dict(scale=-30.0), dict(scale=nan), dict(scale=inf),
           dict(margin=0.0), dict(margin=-0.1), dict(margin=1.0), dict(margin=nan), dict(margin=inf), dict(kind=1, margin=1.6),
           dict(kind=1, margin=0.0), dict(weight=0.0), dict(weight=-1.0), dict(weight=nan), dict(weight=inf)]
    bad += [dict(null=k) for k in ORDER + ('pre', 'u', 'lab', 'W', 'ws')]
    for change in bad:
        assert call(**change) == FV_ERR_INVALID, change
    assert call(ws_bytes=int(lib().fv_fid_margin_workspace_bytes(M, C)) - 1) == FV_ERR_WORKSPACE
    assert call(ws_bytes=0) == FV_ERR_WORKSPACE
    torch.cuda.synchronize()
    for k in ORDER:
        assert np.array_equal(o[k].cpu().numpy().view(np.uint8), keep[k].cpu().numpy().view(np.uint8)), k
    assert call(kind=1, margin=1.5) == 0 and call(margin=0.999) == 0 and call(ws_bytes=int(lib().fv_fid_margin_workspace_bytes(M, C))) == 0
    torch.cuda.synchronize()                       # and the valid call, last: M rows are written, the rest is not
    assert bool((o['pred'][:M] != -7).all()) and int(o['pred'][M]) == -7 and float(o['cos_t'][M]) == -7.5
    assert bool(torch.isfinite(o['dE'][:M]).all()) and bool(torch.isnan(o['dE'][M:]).all()) and bool(torch.isfinite(o['dW']).all())
    # the step checks its batch before anything is enqueued
    m = fg._model(64)
    m.init_classes(3, 0)
    with pytest.raises(ValueError, match='1024'):
        m.forward_backward_classes(torch.zeros((1025, 64, 64, 3)), np.zeros(1025, np.int32))
    with pytest.raises(ValueError, match='kind'):
        m.forward_backward_classes(torch.zeros((2, 64, 64, 3)), np.zeros(2, np.int32), 'softmax')
    with pytest.raises(ValueError, match='one label per image'):
        m.forward_backward_classes(torch.zeros((2, 64, 64, 3)), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match='label 3 is not below the 3 classes'):
        m.forward_backward_classes(torch.zeros((2, 64, 64, 3)), np.asarray([0, 3], np.int32))
    with pytest.raises(fi.FvError, match='margin'):
        m.forward_backward_classes(torch.zeros((2, 64, 64, 3)), np.zeros(2, np.int32), 'cosface', 30.0, 1.0)
    assert m.bn_updates == 0


# ----------------------------------------------------------------------------- 4. the step against the float64 oracle
GAP = 1e-3


def _oracle_cls_step(p, s, x, labels, W, S, kind, scale, margin):
    sp = fg._SlicedParams(p)
    (u,), _, ns = fg.towers(sp, s, [x], S, training=True, ema_step=1)
    Wl = W.clone().requires_grad_(True)
    loss = ref.torch_loss_of_u(u, torch.as_tensor(labels, dtype=torch.int64), Wl, kind, scale, margin)
    dW, = torch.autograd.grad(loss, [Wl], retain_graph=True)
    cos = (u @ ref.torch_l2n(Wl).T).detach()
    return loss.detach(), sp.grad(loss), dW, ns.detach(), cos


# (labels, C, kind, seed)
STEP_CASES = [([0, 0, 1, 1], 3, 'cosface', 60), ([0, 0, 0, 1, 1, 2, 2, -1], 3, 'arcface', 60)]


@pytest.mark.parametrize('labels,C,kind,seed', STEP_CASES)
def test_fid_cls_train_step_matches_oracle(labels, C, kind, seed):
    from oracle import net_oracle as no
    S, M = 64, len(labels)
    code, margin, scale = fi.MARGIN_SOFTMAX_KINDS[kind], fi.MARGIN_SOFTMAX_MARGINS[kind], 30.0
    m = fg._model(S)
    m.init_classes(C, seed + 2)
    W64 = m.class_kernel.cpu().double()
    p64, s64 = fg.fid_params(S, seed)
    x = fg._images(M, S, seed + 1)
    l64, g64, dW64, ns64, cos = _oracle_cls_step(p64, s64, x, labels, W64, S, code, scale, margin)
    # asserted on the oracle first: the target cosines keep GAP from the branch points, the top-two cosines of a row differ
    valid = [i for i, y in enumerate(labels) if y >= 0]
    ct = cos[valid, [labels[i] for i in valid]]
    for point in (-1.0, 1.0, float(np.cos(np.pi - margin))):
        assert ((ct - point).abs() > GAP).all(), (ct, point)
    top = torch.sort(cos, dim=1).values[:, -2:]
    assert (top[:, 1] - top[:, 0] > GAP).all(), top
    l32, g32, dW32, ns32, _ = _oracle_cls_step(p64.float(), s64.float(), x.float(), labels, W64.float(), S, code, scale, margin)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    m.class_grads.fill_(float('nan'))                           # stored, not accumulated
    loss = m.forward_backward_classes(x.float(), np.asarray(labels, np.int32), kind, scale).item()
    assert m.bn_updates == 1
    sel = {k: v.cpu().numpy() for k, v in m.class_selection.items()}
    assert np.array_equal(sel['pred'], cos.argmax(1).numpy())
    assert np.array_equal(np.isnan(sel['cos_t']), np.asarray(labels) < 0)
    assert np.abs(sel['cos_t'][valid] - ct.numpy()).max() < GAP
    print('loss %.9g, float64 %.9g, float32 %.9g' % (loss, l64.item(), l32.item()))
    assert abs(loss - l64.item()) <= 4 * abs(l32.item() - l64.item()) + 1e-5 * min(1.0, abs(l64.item()))
    fg._within(m.state.cpu(), ns64, ns32, 'bn moving state after one update')
    g = m.grads.cpu()
    for e in no.param_layout()[0][:fi.NUM_BASE_LAYERS]:
        sl = slice(e['w_off'], e['w_off'] + e['cout'] * e['k'] * e['k'] * e['cin'])
        fg._grad_close(g[sl], g64[sl], g32[sl], 'dW ' + e['name'])
        for nm in ('gamma_off', 'beta_off'):
            sl = slice(e[nm], e[nm] + e['cout'])
            fg._grad_close(g[sl], g64[sl], g32[sl], nm + ' ' + e['name'])
    k, b = fi.dense_offsets(S)
    fg._grad_close(g[k:b], g64[k:b], g32[k:b], 'dense kernel')
    fg._grad_close(g[b:b + 64], g64[b:b + 64], g32[b:b + 64], 'dense bias')
    assert len(g) == b + 64 and torch.isfinite(g).all()
    cg = m.class_grads.cpu()
    assert torch.isfinite(cg).all()
    fg._grad_close(cg, dW64, dW32, 'class kernel')
    if C > len(set(labels) - {-1}):                             # a class without rows still gets the softmax's push
        assert cg[C - 1].abs().sum() > 0


# ----------------------------------------------------------------------------- 5. training and workspaces
def test_training_on_a_classified_batch_makes_progress():
    S = 64
    m = fg._model(S)
    p64, s64 = fg.fid_params(S, 51)
    x = torch.cat([fg._images(2, S, 52), fg._images(2, S, 53)]).float()
    labels = np.asarray([0, 0, 1, 1], np.int32)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    m.init_classes(2, 1)
    w0 = m.class_kernel.clone()
    losses = [m.train_on_classified_batch(x, labels, 'cosface', 30.0, None, 1e-5, 0.99, 0.99).item() for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[0] > 0 and m.bn_updates == 6 and m.iterations == 6
    assert losses[-1] < losses[0], losses
    assert not torch.equal(m.class_kernel, w0) and bool(torch.isfinite(m.class_kernel).all()) and bool(m.class_m.any()) and bool(m.class_v.any())


def test_the_class_workspace_does_not_evict_the_others():
    S = 64
    m = fg._model(S)
    m.ensure_optimizer()
    m.init_classes(5, 0)
    ws_train, ws_infer, ws_batch = m._workspace(2, S, True), m._workspace(3, S, False), m._batch_workspace(4)
    big = m._cls_workspace(6)
    assert m._cls_workspace(4) is big and m._workspace(2, S, True) is ws_train and m._workspace(3, S, False) is ws_infer
    assert m._batch_workspace(4) is ws_batch
    m._workspace(1, S, True)
    assert m._cls_workspace(6) is big and m._batch_workspace(4) is ws_batch


# ----------------------------------------------------------------------------- 6. end to end
def test_train_with_a_margin_softmax_end_to_end_in_the_three_tiers(tmp_path, monkeypatch, capsys):
    from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5
    mg._make_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    fed = []
    real = fi.FidModel.train_on_classified_batch

    def record(self, x, labels, kind, *a, **k):
        w = self.class_kernel.clone()
        loss = real(self, x, labels, kind, *a, **k)
        fed.append(dict(x=self._as_input(x).clone(), labels=labels.cpu().numpy().copy(), kind=kind, loss=float(loss.item()), w=w))
        return loss
    monkeypatch.setattr(fi.FidModel, 'train_on_classified_batch', record)
    tiers = {cs.RESIDENT: {}, cs.PER_BATCH: dict(crop_store_mb=0), cs.HOST: dict(crop_store=False)}
    made = []
    real_init = cs.TripletInputs.__init__
    monkeypatch.setattr(cs.TripletInputs, '__init__', lambda self, *a, **k: (real_init(self, *a, **k), made.append(self.tier))[0])
    first = {}
    for tier, more in tiers.items():
        del fed[:]
        for name in ('face_identifier.h5', 'face_identifier_classes.h5'):
            if os.path.exists(name):
                os.remove(name)
        ident = fi.FaceIdentifier(mg._conf(tmp_path, margin_softmax='arcface', ms_seed=3, pk_subjects=2, pk_crops=3, pk_seed=5, **more))
        ident.train()
        assert made[-1] == tier and os.path.exists('face_identifier.h5') and os.path.exists('face_identifier_classes.h5')
        out = capsys.readouterr().out
        lines = [line for line in out.splitlines() if line.startswith('Epoch')]
        assert len(lines) == 2 and all('margin softmax (arcface) accuracy:' in line and 'target cosine:' in line and 'nan' not in line
                                       for line in lines)
        tr_gen = fi.TrainingSequence(str(tmp_path), dict(ident.hps), ident.nn_arch, load_flag=True)
        codes = fi.subject_codes(list(tr_gen.db['subject_id']))
        rng = np.random.default_rng(5)
        want = [b for _ in range(2) for b in fi.pk_batches(codes, 2, 3, rng)]            # the very batches of batch_mining
        assert len(want) == 4 and all(len(b) == 6 for b in want)
        assert [b for e in ident.last_margin_softmax['batches'] for b in e] == want and ident.last_margin_softmax['classes'] == 4
        assert len(fed) == 4 and ident.model.iterations == 4 and ident.model.bn_updates == 4
        for f, b in zip(fed, want):
            assert np.array_equal(f['labels'], codes[b]) and f['kind'] == 'arcface' and tuple(f['x'].shape) == (6, mg.S5, mg.S5, 3)
        w = np.random.RandomState(3).standard_normal((4, 64))
        assert np.array_equal(fed[0]['w'].cpu().numpy(), (w / np.sqrt((w * w).sum(-1, keepdims=True))).astype(np.float32))
        data, _ = read_hdf5('face_identifier_classes.h5')
        assert data['/subject_ids'].tolist() == [0, 1, 2, 3] and np.array_equal(data['/class_kernel'], ident.model.class_kernel.cpu().numpy())
        assert not np.array_equal(data['/class_kernel'], fed[0]['w'].cpu().numpy())
        first[tier] = fed[0]['loss']
        print('%s: step losses %r' % (tier, [f['loss'] for f in fed]))
    # the first step has no earlier atomics in its history: the three tiers feed the same bits and get the same loss
    assert np.isfinite(list(first.values())).all() and len(set(first.values())) == 1, first
    # model_loading: the model and, the subject list being the same, the class kernel are read back
    conf = mg._conf(tmp_path, margin_softmax='arcface', ms_seed=9, pk_subjects=2, pk_crops=3, pk_seed=5, epochs=1)
    conf['fi_conf']['model_loading'] = True
    saved = read_hdf5('face_identifier_classes.h5')[0]['/class_kernel']
    del fed[:]
    fi.FaceIdentifier(conf).train()
    assert np.array_equal(fed[0]['w'].cpu().numpy(), saved)
