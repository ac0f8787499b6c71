"""The margin softmax without a device: the numpy restatement of fv_fid_margin_softmax_loss_grad
(tests/margin_softmax_ref.py) against torch float64 autograd of the definition and on cases worked out by hand, the configuration's
refusals before a device is touched, the header and the bindings, and train()'s loop with hps['margin_softmax'] over recorders."""
import json
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from face_vijnana_yolov3_amd import crop_store
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd import ops, parallel
import margin_softmax_ref as ref
import test_fid_mining_cpu as mining_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [ref.KIND_COSFACE, ref.KIND_ARCFACE]


# ----------------------------------------------------------------------------- 1. the restatement against autograd
def _against_autograd(pre, labels, W, kind, what, scale=30.0):
    m = ref.DEFAULT_MARGIN[kind]
    pre = np.asarray(pre, np.float64)
    got = ref.margin_softmax(pre, ref.l2n_relu64(pre), labels, W, kind, scale, m)
    loss, dpre, dW = ref.autograd(pre, labels, W, kind, scale, m)
    worst = 0.0
    for name, a, b in (('loss', got['loss'], loss), ('d pre', got['dpre'], dpre), ('dW', got['dW'], dW)):
        a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
        assert np.isfinite(a).all() and np.isfinite(b).all(), (what, name)
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) if np.abs(b).max() > 0 else np.abs(a).max()
        worst = max(worst, err)
        assert err <= 1e-12, (what, name, err)
    print('%s: worst error %.3g of the largest element' % (what, worst))
    return got


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,C', [(1, 1), (2, 2), (5, 3), (65, 65), (257, 1000), (64, 8631)])
def test_restatement_agrees_with_autograd(M, C, kind):
    pre, labels, W = ref.random_case(M, C, 100 + M + C)
    got = _against_autograd(pre, labels, W, kind, 'M=%d C=%d kind=%d' % (M, C, kind))
    if M >= 64:
        assert 0 < got['V'] < M                                # rows of label -1 are in


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', sorted(ref.hand_cases()))
def test_restatement_agrees_with_autograd_on_the_hand_cases(name, kind):
    c = ref.hand_cases()[name]
    _against_autograd(c['pre'], c['labels'], c['W'], kind, '%s kind=%d' % (name, kind))


# ----------------------------------------------------------------------------- 2. hand cases
def _hand(name, kind, **more):
    c = ref.hand_cases()[name]
    return c, ref.margin_softmax(c['pre'], ref.l2n_relu(c['pre']), c['labels'], c['W'], kind, 30.0, ref.DEFAULT_MARGIN[kind], **more)


@pytest.mark.parametrize('kind', KINDS)
def test_one_class_gives_zero_loss_and_zero_gradients(kind):
    c, out = _hand('one_class', kind)
    assert out['loss'] == 0.0 and out['V'] == 2 and not out['dE'].any() and not out['dW'].any()
    assert out['pred'].tolist() == [0, 0, 0] and np.isnan(out['cos_t'][2]) and np.isfinite(out['cos_t'][:2]).all()


@pytest.mark.parametrize('kind', KINDS)
def test_a_batch_without_labels_adds_nothing(kind):
    c, out = _hand('all_unknown', kind)
    assert out['loss'] == 0.0 and out['V'] == 0 and not out['dE'].any() and not out['dW'].any() and np.isnan(out['cos_t']).all()
    assert ((out['pred'] >= 0) & (out['pred'] < 5)).all()      # the prediction is made for every row


@pytest.mark.parametrize('kind', KINDS)
def test_a_dead_row_has_a_loss_and_no_gradient(kind):
    c, out = _hand('dead_row', kind)
    assert (c['pre'][1] <= 0).all() and not out['dE'][1].any() and out['cos_t'][1] == 0.0
    assert out['dE'][0].any() and out['dE'][2].any() and out['loss'] > 0 and np.isfinite(out['dW']).all()
    assert out['G'][1].any()                                   # its softmax still sends gradient to the class rows


@pytest.mark.parametrize('kind', KINDS)
def test_a_tiny_class_row_is_scaled_by_the_constant(kind):
    c, out = _hand('tiny_class_rows', kind)
    wh, inv, live = ref.normalise_classes(c['W'])
    assert live.tolist() == [True, True, False, False] and inv[2] == 1e6 and inv[3] == 1e6 and not wh[3].any()
    G, u = out['G'], ref.l2n_relu(c['pre']).astype(np.float64)
    assert np.array_equal(out['dW'][2], (G.T @ u)[2] * 1e6) and np.isfinite(out['dW']).all() and out['dW'][3].any()


def test_a_target_cosine_of_exactly_one_is_finite_for_arcface():
    c, out = _hand('target_cosine_one', ref.KIND_ARCFACE)
    assert out['cos_t'][0] == 1.0                               # q = 0: the 1e-12 branch, psi' = cos m
    assert np.isfinite(out['dE']).all() and np.isfinite(out['dW']).all() and np.isfinite(out['loss'])
    psi, dpsi = ref.margin_of(np.asarray([1.0]), ref.KIND_ARCFACE, 0.5)
    assert dpsi[0] == np.cos(0.5) and psi[0] == np.cos(0.5) - np.sqrt(1e-12) * np.sin(0.5)


def test_a_target_cosine_below_the_branch_point_takes_the_fallback():
    c, out = _hand('target_cosine_minus_one', ref.KIND_ARCFACE)
    assert out['cos_t'][0] == -1.0 and -1.0 <= np.cos(np.pi - 0.5)
    bp = np.cos(np.pi - 0.5)
    psi, dpsi = ref.margin_of(np.asarray([-1.0, bp, bp + 1e-9]), ref.KIND_ARCFACE, 0.5)
    assert psi[0] == -1.0 - 0.5 * np.sin(np.pi - 0.5) and dpsi[0] == 1.0 and dpsi[1] == 1.0
    assert psi[0] < psi[1] < psi[2] and abs(psi[2] + 1.0) < 1e-6        # monotone across the branch point, where cos(theta + m) = -1
    assert np.isfinite(out['dE']).all() and np.isfinite(out['dW']).all()


def test_the_weight_scales_the_gradients_and_leaves_the_loss():
    pre, labels, W = ref.random_case(9, 5, 3)
    u = ref.l2n_relu(pre)
    a = ref.margin_softmax(pre, u, labels, W, 0, 30.0, 0.35)
    b = ref.margin_softmax(pre, u, labels, W, 0, 30.0, 0.35, weight=0.25)
    assert a['loss'] == b['loss'] and np.array_equal(a['dE'] * 0.25, b['dE']) and np.array_equal(a['dW'] * 0.25, b['dW'])


def test_a_label_beyond_the_classes_is_an_unknown_row_with_pred_minus_2():
    pre, labels, W = ref.random_case(6, 4, 8, unknown=0.0)
    labels[3] = 4
    out = ref.margin_softmax(pre, ref.l2n_relu(pre), labels, W, 0, 30.0, 0.35)
    assert out['pred'][3] == -2 and np.isnan(out['cos_t'][3]) and out['V'] == 5 and not out['G'][3].any()


def test_the_searched_cases_are_well_separated():
    for kind in KINDS:
        pre, u, labels, W, want, seed = ref.searched_case(65, 65, kind)
        assert ref.well_separated(want, ref.DEFAULT_MARGIN[kind], 65)
        assert (labels < 0).sum() >= 3 and (pre[32] <= 0).all() and not W[64].any() and labels[0] == 64


# ----------------------------------------------------------------------------- 3. the header, the bindings
def test_header_and_bindings_agree():
    header = open(ROOT + '/include/fv_hotpath.h').read()
    assert re.search(r'int fv_fid_margin_softmax_loss_grad\(fv_ctx\* ctx, const float\* pre, const float\* u, const int32_t\* labels', header)
    for name in ('fv_fid_margin_workspace_bytes(', 'fv_fid_cls_workspace_bytes(', 'fv_fid_cls_train_step('):
        assert name in header
    assert fi.MARGIN_SOFTMAX_KINDS == dict(cosface=ref.KIND_COSFACE, arcface=ref.KIND_ARCFACE)
    assert fi.MARGIN_SOFTMAX_MARGINS == {'cosface': ref.DEFAULT_MARGIN[0], 'arcface': ref.DEFAULT_MARGIN[1]}
    from face_vijnana_yolov3_amd._lib import lib
    L = lib()
    assert len(L.fv_fid_margin_softmax_loss_grad.argtypes) == 19 and len(L.fv_fid_cls_train_step.argtypes) == 19
    # the size queries need no device: 0 for what the calls refuse
    q = L.fv_fid_margin_workspace_bytes
    assert q(0, 5) == 0 and q(1025, 5) == 0 and q(4, 0) == 0 and q(4, fi.CLASSES_MAX + 1) == 0
    assert 0 < q(1, 1) < q(39, 1000) < q(96, 8631) < q(1024, fi.CLASSES_MAX)
    assert q(39, 1000) >= 39 * 1000 * 8                          # it keeps the [M][C] coefficients
    c = L.fv_fid_cls_workspace_bytes
    assert c(4, 3, 65) == 0 and c(0, 3, 64) == 0 and c(4, 0, 64) == 0
    assert c(4, 3, 64) >= L.fv_fid_batch_workspace_bytes(4, 64) + q(4, 3)


# ----------------------------------------------------------------------------- 4. configuration
_conf, no_device = mining_cpu._conf, mining_cpu.no_device


@pytest.mark.parametrize('hps', [dict(margin_softmax='softmax'), dict(margin_softmax=1), dict(margin_softmax=True),
                                 dict(margin_softmax='cosface', ms_scale=0), dict(margin_softmax='cosface', ms_scale=-30.0),
                                 dict(margin_softmax='cosface', ms_scale='30'), dict(margin_softmax='arcface', ms_scale=float('inf')),
                                 dict(margin_softmax='arcface', ms_scale=float('nan')), dict(margin_softmax='cosface', ms_scale=True),
                                 dict(margin_softmax='cosface', ms_margin=0.0), dict(margin_softmax='cosface', ms_margin=1.0),
                                 dict(margin_softmax='arcface', ms_margin=1.6), dict(margin_softmax='arcface', ms_margin=-0.1),
                                 dict(margin_softmax='arcface', ms_margin='0.5'), dict(margin_softmax='cosface', ms_seed=-1),
                                 dict(margin_softmax='cosface', ms_seed=1.0), dict(margin_softmax='cosface', pk_crops=1),
                                 dict(margin_softmax='arcface', pk_subjects=513, pk_crops=2), dict(margin_softmax='cosface', pk_seed='0'),
                                 dict(margin_softmax='cosface', batch_mining='batch_hard'),
                                 dict(margin_softmax='arcface', triplet_mining='semi_hard')])
def test_a_bad_margin_softmax_configuration_is_refused_before_a_device_is_touched(tmp_path, no_device, hps):
    with pytest.raises(ValueError, match='margin_softmax|ms_scale|ms_margin|ms_seed|pk_crops|pk_subjects|pk_seed'):
        fi.FaceIdentifier(_conf(tmp_path, **dict(dict(batch_size=13), **hps)))


def test_margin_softmax_values_that_are_served():
    assert fi.margin_softmax_conf({}, 64) is None and fi.margin_softmax_conf(dict(margin_softmax=None), 64) is None
    assert fi.margin_softmax_conf(dict(margin_softmax='none', ms_scale=-1, batch_mining='batch_hard'), 64) is None   # off: nothing else is read
    assert fi.margin_softmax_conf(dict(margin_softmax='cosface', batch_size=13), 416) == \
        dict(kind='cosface', scale=30.0, margin=0.35, seed=0, P=9, K=4, pk_seed=0)
    assert fi.margin_softmax_conf(dict(margin_softmax='arcface', batch_size=13, ms_scale=64, ms_margin=1.5, ms_seed=3, pk_crops=3,
                                       pk_seed=5, batch_mining='none', triplet_mining=None), 416) == \
        dict(kind='arcface', scale=64.0, margin=1.5, seed=3, P=13, K=3, pk_seed=5)
    assert fi.margin_softmax_conf(dict(margin_softmax='cosface', batch_size=2, ms_margin=0.999), 64)['margin'] == 0.999


def test_more_subjects_than_the_class_kernel_takes_are_refused_before_a_device_is_touched(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    n = fi.CLASSES_MAX + 1
    pd.DataFrame(dict(subject_id=np.arange(n), face_file=['f.jpg'] * n)).to_csv('subject_image_db.csv')
    with pytest.raises(ValueError, match='margin_softmax.*32769 subjects'):
        fi.FaceIdentifier(_conf(tmp_path, batch_size=4, margin_softmax='cosface'))
    with pytest.raises(ValueError, match='32769 subjects'):
        fi.check_class_count(n)
    fi.check_class_count(fi.CLASSES_MAX)


def test_margin_softmax_on_two_ranks_is_refused_before_the_ranks_are_started(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(parallel, 'launch_ranks', lambda *a, **k: pytest.fail('ranks were started'))
    conf = _conf(tmp_path, batch_size=4, margin_softmax='arcface')
    conf['fi_conf'].update(multi_gpu=True, num_gpus=2)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match='margin_softmax'):
        fi.main()
    ident = object.__new__(fi.FaceIdentifier)
    ident.hps, ident.world, ident.rank, ident.conf = conf['fi_conf']['hps'], 2, 0, conf['fi_conf']
    monkeypatch.setattr(parallel, 'DataParallelTrainer', lambda *a, **k: pytest.fail('a process group was formed'))
    with pytest.raises(NotImplementedError, match='margin_softmax'):
        ident.train()


def test_the_bindings_refuse_labels_beyond_the_classes_before_any_device_call(monkeypatch):
    monkeypatch.setattr(ops, 'lib', lambda: pytest.fail('the library was called'))
    with pytest.raises(ValueError, match='labels below 3'):
        ops.fid_margin_softmax_loss_grad(None, torch.zeros((2, 64)), torch.zeros((2, 64)), np.asarray([0, 3]), torch.zeros((3, 64)))
    with pytest.raises(ValueError, match='labels below 3'):
        ops.fid_margin_softmax_loss_grad(None, torch.zeros((2, 64)), torch.zeros((2, 64)), np.asarray([0, 1, 2]), torch.zeros((3, 64)))


def test_init_classes_draws_unit_rows_from_the_seed():
    m = object.__new__(fi.FidModel)
    m.dev = torch.device('cpu')
    m.init_classes(5, 3)
    w = np.random.RandomState(3).standard_normal((5, 64))
    want = (w / np.sqrt((w * w).sum(-1, keepdims=True))).astype(np.float32)
    assert m.class_kernel.dtype == torch.float32 and np.array_equal(m.class_kernel.numpy(), want)
    assert np.abs(np.linalg.norm(m.class_kernel.numpy().astype(np.float64), axis=1) - 1).max() < 1e-6
    assert not m.class_grads.any() and not m.class_m.any() and not m.class_v.any()
    for C in (0, fi.CLASSES_MAX + 1):
        with pytest.raises(ValueError, match='classes'):
            m.init_classes(C)


# ----------------------------------------------------------------------------- 5. train()'s loop over recorders
SUBJECTS = [7, 7, 7, 3, 3, -1, 9, 9, 9, 9, 5, 5, -1, 4]          # db rows 100 ..; codes 0 0 0 1 1 -1 2 2 2 2 3 3 -1 4; 4: a single row


class _DbSequence(mining_cpu._Sequence):
    def __init__(self, raw_data_path, hps, nn_arch, load_flag=True):
        super(_DbSequence, self).__init__(raw_data_path, hps, nn_arch, load_flag)
        self.db = pd.DataFrame(dict(subject_id=SUBJECTS, face_file=['%d.jpg' % i for i in range(len(SUBJECTS))]),
                               index=[100 + i for i in range(len(SUBJECTS))])

    def path(self, label):
        return 'faces/%d.jpg' % label


class _Inputs(object):
    made = []

    def __init__(self, ctx, device, image_size, labels, path_of, batch_size, budget, threads, slots=None, tier=None):
        _Inputs.made.append(dict(labels=list(labels), slots=slots, tier=tier))
        self.closed = False

    def crop_batches(self, batches):
        for b in batches:
            yield list(b)

    def close(self):
        self.closed = True


class _ClsModel(mining_cpu._Model):
    """The host side of FidModel's classified step for real (train_on_classified_batch, init_classes, set_classes), the device
    calls recorded."""
    train_on_classified_batch = fi.FidModel.train_on_classified_batch
    init_classes = fi.FidModel.init_classes
    set_classes = fi.FidModel.set_classes

    def __init__(self):
        self.dev, self.ctx, self.iterations, self.fed, self.model_steps, self.workspaces = torch.device('cpu'), 'ctx', 0, [], [], []
        self.class_kernel = None

    def ensure_optimizer(self):
        pass

    def _cls_workspace(self, M):
        self.workspaces.append(M)

    def forward_backward_classes(self, x, labels, kind, scale, margin):
        self.fed.append(dict(x=x, labels=labels.numpy().copy(), kind=kind, scale=scale, margin=margin))
        lab = labels.to(torch.int64)
        pred = torch.where(torch.arange(len(lab)) % 2 == 0, lab, lab + 1).to(torch.int32)     # every other row is a hit
        self.class_selection = dict(pred=pred, cos_t=torch.full((len(lab),), 0.25, dtype=torch.float64))
        self.class_grads.fill_(0.5)
        return torch.full((1,), 2.0)

    def adam_step(self, lr, beta_1, beta_2, decay=0.0):
        self.model_steps.append((self.iterations, lr, beta_1, beta_2, decay))
        self.iterations += 1


@pytest.fixture
def cls_loop(loop, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(crop_store, 'TripletInputs', _Inputs)
    monkeypatch.setattr(crop_store, 'store_budget', lambda hps, dev: 0)
    _Inputs.made = []
    adam = []
    monkeypatch.setattr(ops, 'adam_step', lambda ctx, p, g, m, v, it, lr, b1, b2, eps=1e-7, decay=0.0:
                        (adam.append(dict(p=p, g=g, m=m, v=v, it=it, lr=lr, b1=b1, b2=b2, eps=eps, decay=decay)), p.sub_(0.125)))

    def make(**hps):
        ident = loop(**hps)
        ident.TrainingSequence, ident.model, ident.image_size, ident.model_loading = _DbSequence, _ClsModel(), 64, False
        return ident
    return make, adam


def test_with_the_key_train_runs_the_pk_batches_through_the_classified_step_and_writes_both_files(cls_loop, capsys):
    make, adam = cls_loop
    ident = make(margin_softmax='arcface', ms_scale=16, ms_seed=4, pk_subjects=2, pk_crops=2, pk_seed=6, decay=0.5, loader_threads=1)
    np.random.seed(11)
    before = np.random.get_state()[1].copy()
    ident.train()
    assert np.array_equal(before, np.random.get_state()[1])             # the global stream is left alone
    m = ident.model
    codes = fi.subject_codes(SUBJECTS)
    assert codes.tolist() == [0, 0, 0, 1, 1, -1, 2, 2, 2, 2, 3, 3, -1, 4]
    rng = np.random.default_rng(6)
    want = [b for _ in range(2) for b in fi.pk_batches(codes, 2, 2, rng)]
    assert len(want) == 4 and all(len(b) == 4 for b in want) and [b for e in ident.last_margin_softmax['batches'] for b in e] == want
    assert ident.last_margin_softmax['classes'] == 5 and m.workspaces == [4]
    # every batch: the db labels of its rows as crops, the rows' codes as class labels, the configured loss
    assert len(m.fed) == 4
    for f, b in zip(m.fed, want):
        assert f['x'] == [100 + r for r in b] and np.array_equal(f['labels'], codes[b]) and f['labels'].dtype == np.int32
        assert (f['kind'], f['scale'], f['margin']) == ('arcface', 16.0, 0.5)
    # one Adam step over the class kernel per step, with its own m / v and the model's iteration, before the model's own
    assert len(adam) == 4 and [a['it'] for a in adam] == [0, 1, 2, 3] and [s[0] for s in m.model_steps] == [0, 1, 2, 3]
    for a in adam:
        assert a['p'] is m.class_kernel and a['g'] is m.class_grads and a['m'] is m.class_m and a['v'] is m.class_v
        assert (a['lr'], a['b1'], a['b2'], a['eps'], a['decay']) == (1e-4, 0.9, 0.99, 1e-7, 0.5)
    assert m.model_steps[0][1:] == (1e-4, 0.9, 0.99, 0.5)
    assert _Inputs.made == [dict(labels=[100 + i for i in range(14)], slots=None, tier=crop_store.HOST)]
    out = capsys.readouterr().out
    lines = [line for line in out.splitlines() if line.startswith('Epoch')]
    assert len(lines) == 2 and all('loss: 2.0000 - margin softmax (arcface) accuracy: 0.5000, target cosine: 0.2500' in line for line in lines)
    assert ident.last_margin_softmax['accuracy'] == 0.5 and ident.last_margin_softmax['cos_t'] == 0.25
    # the two files: the model as before, the class kernel as trained with the subject id of every class
    assert mining_cpu._Model.saved == ['face_identifier.h5'] and mining_cpu._Trainer.fed == []
    from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5
    data, _ = read_hdf5('face_identifier_classes.h5')
    assert data['/subject_ids'].tolist() == [7, 3, 9, 5, 4]
    w = np.random.RandomState(4).standard_normal((5, 64))
    first = (w / np.sqrt((w * w).sum(-1, keepdims=True))).astype(np.float32)
    for _ in range(4):
        first = first - np.float32(0.125)
    assert np.array_equal(data['/class_kernel'], first) and data['/class_kernel'].dtype == np.float32


def test_the_class_kernel_is_loaded_only_with_model_loading_and_the_same_subject_list(cls_loop):
    make, adam = cls_loop
    from face_vijnana_yolov3_amd.hdf5_lite import write_hdf5
    saved = np.arange(5 * 64, dtype=np.float32).reshape(5, 64)

    def first_kernel(subject_ids, loading):
        write_hdf5('face_identifier_classes.h5', {'/class_kernel': saved, '/subject_ids': np.asarray(subject_ids, np.int64)})
        ident = make(margin_softmax='cosface', epochs=1, pk_subjects=2, pk_crops=2)
        ident.model_loading = loading
        seen = []
        real = _ClsModel.forward_backward_classes
        ident.model.forward_backward_classes = lambda *a: (seen.append(ident.model.class_kernel.clone()), real(ident.model, *a))[1]
        ident.train()
        return seen[0].numpy()
    w = np.random.RandomState(0).standard_normal((5, 64))
    fresh = (w / np.sqrt((w * w).sum(-1, keepdims=True))).astype(np.float32)
    assert np.array_equal(first_kernel([7, 3, 9, 5, 4], True), saved)
    assert np.array_equal(first_kernel([7, 3, 9, 5, 4], False), fresh)
    assert np.array_equal(first_kernel([7, 3, 9, 4, 5], True), fresh)           # another subject list: initialised afresh
    assert np.array_equal(first_kernel([7, 3, 9, 5], True), fresh)


@pytest.mark.parametrize('hps', [{}, dict(margin_softmax=None), dict(margin_softmax='none')])
def test_without_the_key_train_makes_the_calls_it_made_and_draws_the_same_random_numbers(loop, monkeypatch, capsys, hps):
    monkeypatch.setattr(fi, 'pk_batches', lambda *a, **k: pytest.fail('the sampler was called'))
    monkeypatch.setattr(fi.FaceIdentifier, '_train_classes', lambda *a, **k: pytest.fail('the class loop was entered'))
    ident = loop(**hps)
    np.random.seed(11)
    ident.train()
    after = np.random.get_state()[1].copy()
    np.random.seed(11)
    want = []
    for _ in range(2):
        for i in np.random.permutation(4)[:4]:
            want.append(mining_cpu.TRIPLETS[2 * i:2 * i + 2])
    assert np.array_equal(after, np.random.get_state()[1])
    assert mining_cpu._Trainer.fed == want and mining_cpu._Model.saved == ['face_identifier.h5']
    out = capsys.readouterr().out
    assert 'margin softmax' not in out and out.count('Epoch') == 2 and not os.path.exists('face_identifier_classes.h5')


loop = mining_cpu.loop
