"""Triplet mining, the parts that need no GPU: the group table and the mined rows (triplet_groups, mined_rows, subject_codes), the
numpy oracle of fv_fid_mine_negatives on cases worked out by hand, the configuration's refusals before a device is touched, the
argument checks of the binding, and train()'s loop with and without hps['triplet_mining'] over recorders."""
import json

import numpy as np
import pytest

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd import parallel
import mine_negatives_ref as ref


# ----------------------------------------------------------------------------- 1. the group table and the rows
def test_groups_of_a_hand_list_with_a_repeated_anchor():
    a, off, pos, order = fi.triplet_groups([(3, 1), (3, 2), (5, 0)])
    assert a.dtype == off.dtype == pos.dtype == np.int32
    assert a.tolist() == [3, 5] and off.tolist() == [0, 2, 3] and pos.tolist() == [1, 2, 0] and order.tolist() == [0, 1, 2]


def test_an_anchor_that_recurs_later_starts_another_group():
    pairs = [(3, 1), (3, 2), (5, 0), (3, 4)]
    a, off, pos, order = fi.triplet_groups(pairs)
    assert a.tolist() == [3, 5, 3] and off.tolist() == [0, 2, 3, 4] and pos.tolist() == [1, 2, 0, 4]
    # sorted by anchor first: one group per anchor, and order says where every output belongs
    a, off, pos, order = fi.triplet_groups(pairs, sort=True)
    assert a.tolist() == [3, 5] and off.tolist() == [0, 3, 4] and pos.tolist() == [1, 2, 4, 0] and order.tolist() == [0, 1, 3, 2]


@pytest.mark.parametrize('sort', [False, True])
def test_order_round_trips(sort):
    rng = np.random.RandomState(0)
    pairs = [(int(a), int(p)) for a, p in rng.randint(0, 6, (40, 2))]
    a, off, pos, order = fi.triplet_groups(pairs, sort=sort)
    assert off[0] == 0 and off[-1] == len(pairs) and (np.diff(off) >= 1).all() and sorted(order.tolist()) == list(range(40))
    back = [None] * len(pairs)
    for q in range(len(a)):
        for j in range(off[q], off[q + 1]):
            back[order[j]] = (int(a[q]), int(pos[j]))
    assert back == pairs
    if sort:
        assert len(set(a.tolist())) == len(a)


def test_groups_of_nothing():
    a, off, pos, order = fi.triplet_groups([])
    assert len(a) == 0 and off.tolist() == [0] and len(pos) == 0 and len(order) == 0


def test_mined_rows_drop_easy_on_and_off_and_kind_3_always():
    labels = [10, 11, 12, 13, 14]
    pairs = [(10, 11), (10, 12), (13, 14), (12, 10)]
    neg, kind = [4, 3, 0, -1], [fi.KIND_SEMI_HARD, fi.KIND_EASY, fi.KIND_VIOLATING, fi.KIND_NONE]
    assert fi.mined_rows(pairs, neg, kind, labels, False) == [(10, 11, 14), (10, 12, 13), (13, 14, 10)]
    assert fi.mined_rows(pairs, neg, kind, labels, True) == [(10, 11, 14), (13, 14, 10)]


def test_subject_codes_keep_the_unknown_identity():
    assert fi.subject_codes([5, -1, 7, 5]).tolist() == [0, -1, 1, 0]
    assert fi.subject_codes(['n2', 'n1', 'n2']).tolist() == [0, 1, 0] and fi.subject_codes([]).dtype == np.int32


def test_the_scan_width_is_the_headers():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fv_hotpath.h')).read()
    assert int(re.search(r'#define\s+FV_MINE_PB\s+(\d+)', header).group(1)) == fi.MINE_PB


def test_the_margin_has_one_name():
    assert fi.TRIPLET_MARGIN == fi.ALPHA
    assert (fi.KIND_SEMI_HARD, fi.KIND_VIOLATING, fi.KIND_EASY, fi.KIND_NONE) == (0, 1, 2, 3) == (
        ref.KIND_SEMI_HARD, ref.KIND_VIOLATING, ref.KIND_EASY, ref.KIND_NONE)


# ----------------------------------------------------------------------------- 2. the oracle on hand cases
CASES = ref.hand_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_on_a_hand_case(name):
    c = CASES[name]
    neg, kind, d_ap, d_an = ref.mine_negatives(c['ids'], c['subjects'], c['pairs'], c['margin'], c['mode'])
    assert list(zip(neg.tolist(), kind.tolist())) == c['want']
    for j, (a, p) in enumerate(c['pairs']):
        if kind[j] == ref.KIND_NONE:
            assert neg[j] == -1 and d_an[j] == np.inf
        else:
            assert c['subjects'][neg[j]] >= 0 and c['subjects'][neg[j]] != c['subjects'][a]
            assert d_an[j] == np.sqrt(((c['ids'][a].astype(np.float64) - c['ids'][neg[j]].astype(np.float64)) ** 2).sum())


def test_hand_cases_cover_every_kind():
    kinds = {k for c in CASES.values() for _, k in c['want']}
    assert kinds == {0, 1, 2, 3}
    assert np.isnan(ref.mine_negatives(**{k: CASES['nan_anchor'][k] for k in ('ids', 'subjects', 'pairs', 'margin', 'mode')})[2]).all()


def test_oracle_random_case_has_both_common_kinds():
    ids, subjects, pairs = ref.random_case(257)
    _, kind, d_ap, d_an = ref.mine_negatives(ids, subjects, pairs, 0.2, 0)
    assert (kind == 0).sum() > 100 and (kind == 2).sum() > 100
    band = kind == 0
    assert (d_an[band] > d_ap[band]).all() and (d_an[band] < d_ap[band] + 0.2).all()
    assert (d_an[kind == 2] >= d_ap[kind == 2] + 0.2).all() and (d_an[kind == 1] <= d_ap[kind == 1]).all()


# ----------------------------------------------------------------------------- 3. configuration
def _conf(tmp_path, **hps):
    return {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(tmp_path), multi_gpu=False, num_gpus=1,
                            model_loading=False, nn_arch=dict(image_size=64, dense1_dim=64), hps=hps), 'fd_conf': {}}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        pytest.fail('a device was touched')
    monkeypatch.setattr(fi, 'Context', touched)
    monkeypatch.setattr(fi, 'FidModel', touched)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('hps', [dict(triplet_mining='hard'), dict(triplet_mining=1), dict(triplet_mining='semi_hard', mining_every=0),
                                 dict(triplet_mining='hardest', mining_every='2')])
def test_an_unknown_mining_value_is_refused_before_a_device_is_touched(tmp_path, no_device, hps):
    with pytest.raises(ValueError, match='triplet_mining|mining_every'):
        fi.FaceIdentifier(_conf(tmp_path, **hps))


def test_mining_values_that_are_served():
    assert fi.mining_mode({}) is None and fi.mining_mode(dict(triplet_mining=None)) is None
    assert fi.mining_mode(dict(triplet_mining='none', mining_every=0)) is None         # off: the other keys are not read
    assert fi.mining_mode(dict(triplet_mining='semi_hard')) == 'semi_hard'
    assert fi.mining_mode(dict(triplet_mining='hardest', mining_every=3)) == 'hardest'


def test_mining_on_two_ranks_is_refused_before_the_ranks_are_started(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(parallel, 'launch_ranks', lambda *a, **k: pytest.fail('ranks were started'))
    conf = _conf(tmp_path, triplet_mining='semi_hard')
    conf['fi_conf'].update(multi_gpu=True, num_gpus=2)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match='triplet_mining'):
        fi.main()
    # inside a rank (someone started them by hand): train() itself, before its first collective
    ident = object.__new__(fi.FaceIdentifier)
    ident.hps, ident.world, ident.rank, ident.conf = conf['fi_conf']['hps'], 2, 0, conf['fi_conf']
    monkeypatch.setattr(parallel, 'DataParallelTrainer', lambda *a, **k: pytest.fail('a process group was formed'))
    with pytest.raises(NotImplementedError, match='triplet_mining'):
        ident.train()


def test_two_ranks_without_mining_are_still_started(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(parallel, 'launch_ranks', lambda n, target, **k: 41)
    conf = _conf(tmp_path, triplet_mining='none')
    conf['fi_conf'].update(multi_gpu=True, num_gpus=2)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(SystemExit) as e:
        fi.main()
    assert e.value.code == 41


# ----------------------------------------------------------------------------- 4. the binding's argument checks
class _NoCtx(object):
    device = 0

    def __getattr__(self, name):
        pytest.fail('the device was called')


@pytest.mark.parametrize('what', ['ids dtype', 'ids shape', 'subjects dtype', 'subjects length', 'anchors dtype', 'positives shape',
                                  'offsets length', 'mode', 'unhashable mode', 'host tensors'])
def test_binding_refuses_wrong_dtypes_and_shapes_before_any_device_call(monkeypatch, what):
    import torch
    monkeypatch.setattr(fi, 'lib', lambda: pytest.fail('the library was called'))
    a = dict(ids=torch.zeros((4, 64)), subjects=torch.zeros(4, dtype=torch.int32), anchors=np.zeros(1, np.int32),
             pos_off=np.asarray([0, 1], np.int32), positives=np.ones(1, np.int32), mode='semi_hard')
    if what == 'ids dtype':
        a['ids'] = a['ids'].double()
    elif what == 'ids shape':
        a['ids'] = torch.zeros((4, 32))
    elif what == 'subjects dtype':
        a['subjects'] = a['subjects'].long()
    elif what == 'subjects length':
        a['subjects'] = torch.zeros(3, dtype=torch.int32)
    elif what == 'anchors dtype':
        a['anchors'] = np.zeros(1, np.int64)
    elif what == 'positives shape':
        a['positives'] = np.ones((1, 1), np.int32)
    elif what == 'offsets length':
        a['pos_off'] = np.asarray([0], np.int32)
    elif what == 'mode':
        a['mode'] = 'hard'
    elif what == 'unhashable mode':
        a['mode'] = [0]
    match = {'host tensors': 'device', 'mode': 'mode', 'unhashable mode': 'mode'}.get(what, 'expects')      # each by its own check
    with pytest.raises(ValueError, match='fid_mine_negatives.*' + match):
        fi.fid_mine_negatives(_NoCtx(), **a)


# ----------------------------------------------------------------------------- 5. train()'s loop over recorders
TRIPLETS = [(0, 1, 4), (0, 2, 5), (1, 2, 3), (3, 4, 0), (3, 5, 1), (4, 5, 2), (6, 7, 0)]


class _Sequence(object):
    PICKLE_FILE = 'img_triplet_pairs.pickle'

    def __init__(self, raw_data_path, hps, nn_arch, load_flag=True):
        self.img_triplet_pairs = list(TRIPLETS)
        self.batch_size = int(hps['batch_size'])
        hps['step'] = fi.num_batches(len(TRIPLETS), self.batch_size)
        self.hps = hps

    def __len__(self):
        return self.hps['step']

    rows = fi._TripletSequence.rows

    def load(self, rows):
        return {'input_a': list(rows), 'input_p': None, 'input_n': None}, None


class _Trainer(object):
    fed = []

    def __init__(self, model, world_size=1, rank=0):
        pass

    def barrier(self):
        pass

    def train_on_inputs(self, xs, lr, beta_1, beta_2, decay, weight=1.0):
        _Trainer.fed.append(list(xs[0]))
        return 0.25

    def merged_loss(self, loss, weight):
        return loss

    def shutdown(self):
        pass


class _Model(object):
    saved = []

    def save(self, path):
        _Model.saved.append(path)


@pytest.fixture
def loop(monkeypatch):
    """A FaceIdentifier whose train() meets recorders only: -> make(**hps)."""
    monkeypatch.setattr(parallel, 'DataParallelTrainer', _Trainer)
    _Trainer.fed, _Model.saved = [], []

    def make(**hps):
        ident = object.__new__(fi.FaceIdentifier)
        ident.conf = dict(resource_type='uccs')
        ident.hps = dict(dict(lr=1e-4, beta_1=0.9, beta_2=0.99, epochs=2, batch_size=2, crop_store=False), **hps)
        ident.raw_data_path, ident.nn_arch, ident.world, ident.rank = '.', {}, 1, 0
        ident.mining, ident.last_mining, ident.model = fi.mining_mode(ident.hps), None, _Model()
        ident.TrainingSequence = _Sequence
        return ident
    return make


@pytest.mark.parametrize('hps', [{}, dict(triplet_mining=None), dict(triplet_mining='none')])
def test_without_the_key_train_never_mines_and_draws_the_same_random_numbers(loop, monkeypatch, capsys, hps):
    monkeypatch.setattr(fi.FaceIdentifier, 'mine_triplets', lambda *a, **k: pytest.fail('mine_triplets was called'))
    monkeypatch.setattr(fi, 'fid_mine_negatives', lambda *a, **k: pytest.fail('the binding was called'))
    ident = loop(**hps)
    np.random.seed(11)
    ident.train()
    after = np.random.get_state()[1].copy()
    # what the loop drew before this feature: one permutation of the batch count per epoch, from the global stream
    np.random.seed(11)
    want = []
    for _ in range(2):
        for i in np.random.permutation(4)[:4]:
            want.append(TRIPLETS[2 * i:2 * i + 2])
    assert np.array_equal(after, np.random.get_state()[1])
    assert _Trainer.fed == want and _Model.saved == ['face_identifier.h5']
    out = capsys.readouterr().out
    assert 'Mining' not in out and out.count('Epoch') == 2


def test_with_the_key_the_batches_are_cut_from_the_mined_rows(loop, monkeypatch, capsys):
    mined = [(0, 1, 3), (0, 2, 6), (3, 4, 7), (3, 5, 2), (6, 7, 5)]
    calls = []

    def mine(self, drop_easy=False, tr_gen=None, inputs=None):
        calls.append((drop_easy, tr_gen is not None))
        self.last_mining = dict(counts=[3, 2, 2, 0], seconds=0.0)
        return list(mined), np.zeros(len(mined), np.int32)
    monkeypatch.setattr(fi.FaceIdentifier, 'mine_triplets', mine)
    ident = loop(triplet_mining='semi_hard', epochs=3, mining_every=2)
    ident.train()
    assert calls == [(True, True)] * 2                                  # epochs 0 and 2; drop_easy is on by default
    assert len(_Trainer.fed) == 9                                       # min(step = 4, 3 batches) per epoch
    for e in range(3):
        got = _Trainer.fed[3 * e:3 * e + 3]
        assert sorted(got) == sorted([mined[0:2], mined[2:4], mined[4:5]])       # batch_size rows each, the last one short
    out = capsys.readouterr().out
    assert out.count('Mining (semi_hard) - semi-hard: 3, violating: 2, easy: 2, no negative: 0') == 2


def test_an_epoch_whose_triplets_are_all_easy_runs_no_step(loop, monkeypatch, capsys):
    def mine(self, drop_easy=False, tr_gen=None, inputs=None):
        self.last_mining = dict(counts=[0, 0, 7, 0], seconds=0.0)
        return [], np.zeros(0, np.int32)
    monkeypatch.setattr(fi.FaceIdentifier, 'mine_triplets', mine)
    ident = loop(triplet_mining='hardest', mining_drop_easy=True, epochs=1)
    ident.train()
    assert _Trainer.fed == [] and 'loss: nan' in capsys.readouterr().out and _Model.saved == ['face_identifier.h5']
