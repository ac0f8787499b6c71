"""In-batch triplet mining without a device: the numpy restatement of fv_fid_batch_triplet_loss_grad on cases
worked out by hand, the PK sampler, the configuration's refusals before a device is touched, and train() over recorders: with the
key absent it makes the calls and draws the random numbers it made before the feature existed."""
import json
import os
import re

import numpy as np
import pytest

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd import parallel
import batch_triplet_ref as ref
import test_fid_mining_cpu as mining_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- 1. the restatement on hand cases
@pytest.mark.parametrize('name', sorted(ref.hand_cases()))
def test_restatement_on_a_hand_case(name):
    c = ref.hand_cases()[name]
    u = ref.l2n_relu(c['pre'])
    out = ref.batch_triplet(c['pre'], u, c['subjects'], c['margin'], c['mode'])
    got = [(int(p), int(n), int(k)) for p, n, k in zip(out['pos_index'], out['neg_index'], out['kind'])]
    assert got == c['want']
    invalid = out['kind'] == 3
    assert np.isnan(out['d_ap'][invalid]).all() and np.isinf(out['d_an'][invalid]).all()
    assert (out['d_ap'][invalid].view(np.uint64) == 0x7ff8000000000000).all()          # one quiet NaN, sign and payload clear
    assert np.isfinite(out['dE']).all() and np.isfinite(out['loss'])
    assert out['V'] == int((~invalid).sum())
    # the kind is the class of the chosen distance, in both modes
    for i in np.flatnonzero(~invalid):
        dap, dan = out['d_ap'][i], out['d_an'][i]
        assert out['kind'][i] == (0 if dap < dan < dap + c['margin'] else 1 if dan <= dap else 2)


def test_m1_and_the_one_sided_batches_have_no_valid_anchor():
    for name in ('m1', 'one_subject', 'no_positive'):
        c = ref.hand_cases()[name]
        out = ref.batch_triplet(c['pre'], ref.l2n_relu(c['pre']), c['subjects'])
        assert out['V'] == 0 and out['loss'] == 0.0 and not out['dE'].any() and not out['dbias'].any()


def test_two_and_one_row_two_receives_negative_terms_only():
    """Subjects [0, 0, 1] with the negative made violating (margin 2: every hinge passes): V = 2, loss the mean of the two hinges,
    and row 2 -- no anchor -- gets exactly the two negative terms, in anchor order."""
    c = ref.hand_cases()['two_and_one']
    u = ref.l2n_relu(c['pre'])
    out = ref.batch_triplet(c['pre'], u, c['subjects'], margin=2.0)
    assert out['V'] == 2 and out['active'].tolist() == [True, True, False]
    assert out['loss'] == ((out['h'][0] + out['h'][1]) / 2)
    u64 = u.astype(np.float64)
    want = (0.0 + (1.0 / (2 * out['d_an'][0])) * (u64[0] - u64[2])) + (1.0 / (2 * out['d_an'][1])) * (u64[1] - u64[2])
    assert np.array_equal(out['du'][2], want)
    # rows 0 and 1: the own term, then the positive term the other anchor sends
    own0 = (1.0 / (2 * out['d_ap'][0])) * (u64[0] - u64[1]) - (1.0 / (2 * out['d_an'][0])) * (u64[0] - u64[2])
    assert np.array_equal(out['du'][0], own0 - (1.0 / (2 * out['d_ap'][1])) * (u64[1] - u64[0]))
    # with the contract's margin both hinges are negative: no gradient at all, yet both anchors are valid and counted
    easy = ref.batch_triplet(c['pre'], u, c['subjects'], margin=0.2)
    assert easy['V'] == 2 and not easy['active'].any() and easy['loss'] == 0.0 and not easy['dE'].any()


def test_a_zero_distance_has_gradient_zero_and_the_lower_index_wins():
    c = ref.hand_cases()['dap_zero']
    u = ref.l2n_relu(c['pre'])
    out = ref.batch_triplet(c['pre'], u, c['subjects'], c['margin'], c['mode'])
    assert out['d_ap'][0] == 0.0 and out['d_ap'][1] == 0.0 and out['active'][:2].all()
    u64 = u.astype(np.float64)
    # rows 0 and 1 get their negative term only; row 2 both anchors' negative terms
    assert np.array_equal(out['du'][0], -(1.0 / (2 * out['d_an'][0])) * (u64[0] - u64[2]))
    assert np.isfinite(out['dE']).all() and out['dE'][2].any()
    d = ref.hand_cases()['duplicates']
    sel = ref.select(ref.l2n_relu(d['pre']), d['subjects'], 0.2, 0)
    assert sel[0][2] == 0 and sel[1][0] == 3                       # equal distances: the lower row, positive and negative alike


def test_rows_of_subject_minus_one_take_no_part():
    c = ref.hand_cases()['unknown_rows']
    out = ref.batch_triplet(c['pre'], ref.l2n_relu(c['pre']), c['subjects'], margin=2.0)
    assert out['active'].tolist() == [True, True, False, False, False]
    assert not out['dE'][2].any() and not out['dE'][3].any() and out['dE'][4].any()
    assert 2 not in out['neg_index'] and 3 not in out['pos_index']


def test_hand_cases_cover_every_kind_in_mode_1():
    kinds = set()
    for c in ref.hand_cases().values():
        if c['mode'] == 1:
            kinds |= set(ref.select(ref.l2n_relu(c['pre']), c['subjects'], c['margin'], 1)[2].tolist())
    assert kinds == {0, 1, 2, 3}


def test_random_case_has_several_rows_per_subject_and_all_common_kinds():
    pre, u, subjects = ref.random_case(257, 3)
    assert np.bincount(subjects).min() >= 2
    hard = ref.select(u, subjects, 0.2, 0)
    semi = ref.select(u, subjects, 0.2, 1)
    assert (hard[2] != 3).all() and (semi[2] != 3).all()
    assert np.array_equal(hard[0], semi[0]) and np.array_equal(hard[3], semi[3])       # the positive does not depend on the mode
    assert (semi[4] >= hard[4]).all() and (semi[4] > hard[4]).any()                    # batch hard takes the nearest


# ----------------------------------------------------------------------------- 2. the header, the bindings
def test_header_binding_and_modes_agree():
    header = open(ROOT + '/include/fv_hotpath.h').read()
    assert re.search(r'int fv_fid_batch_triplet_loss_grad\(fv_ctx\* ctx, const float\* pre, const float\* u, const int32_t\* subjects', header)
    assert 'fv_fid_batch_train_step(' in header and 'fv_fid_batch_workspace_bytes(' in header
    assert fi.BATCH_MINING_MODES == dict(batch_hard=ref.MODE_BATCH_HARD, batch_semi_hard=ref.MODE_BATCH_SEMI_HARD)
    from face_vijnana_yolov3_amd._lib import lib
    L = lib()
    assert len(L.fv_fid_batch_triplet_loss_grad.argtypes) == 16 and len(L.fv_fid_batch_train_step.argtypes) == 18
    # the size query needs no device: 0 for what the step refuses, one tower's worth otherwise
    assert L.fv_fid_batch_workspace_bytes(0, 64) == 0 and L.fv_fid_batch_workspace_bytes(1025, 64) == 0
    assert L.fv_fid_batch_workspace_bytes(4, 65) == 0
    assert 0 < L.fv_fid_batch_workspace_bytes(2, 64) < L.fv_fid_batch_workspace_bytes(6, 64) < L.fv_fid_batch_workspace_bytes(1024, 64)


def test_the_training_workspaces_keep_their_sizes():
    """The three training steps carve one workspace layout (1 or 3 tower plans, then the dense rows); the sizes are those the
    three separate layouts had before they were merged, read from that build."""
    from face_vijnana_yolov3_amd._lib import lib
    L = lib()
    assert [L.fv_fid_workspace_bytes(B, S, 1) for B, S in ((1, 32), (2, 64), (3, 96))] == [193323776, 236910080, 355215872]
    assert L.fv_fid_workspace_bytes(3, 64, 0) == 10891264
    assert [L.fv_fid_batch_workspace_bytes(M, S) for M, S in ((1, 32), (4, 64), (6, 64), (1024, 64))] == \
        [173359360, 204493568, 221099008, 8697090304]
    for (M, C, S), want in (((4, 3, 64), 204496128), ((6, 1000, 64), 221159680)):
        assert L.fv_fid_cls_workspace_bytes(M, C, S) == want
        # one tower's workspace rounded up to 256 bytes, then the loss's region
        assert want == (L.fv_fid_batch_workspace_bytes(M, S) + 255) // 256 * 256 + L.fv_fid_margin_workspace_bytes(M, C)


# ----------------------------------------------------------------------------- 3. the PK sampler
CODES = np.asarray([0, 0, 0, 1, 1, -1, 2, 3, 3, 3, 3, 3, -1, 4, 4, 5, 5, 5, 6, 6], np.int32)     # 2: a single row; -1: unknown


@pytest.mark.parametrize('P,K', [(2, 2), (3, 4), (4, 3), (6, 2), (7, 5)])
def test_pk_batches_hold_p_subjects_of_k_rows(P, K):
    for seed in range(5):
        batches = fi.pk_batches(CODES, P, K, np.random.default_rng(seed))
        eligible = {0, 1, 3, 4, 5, 6}
        seen = []
        for b in batches:
            assert len(set(b)) == len(b)
            subjects = CODES[b]
            assert (subjects >= 0).all() and 2 not in subjects
            counts = np.bincount(subjects)
            assert 2 <= len(set(subjects.tolist())) <= P and counts.max() <= K
            for s in set(subjects.tolist()):
                assert counts[s] == min(K, int((CODES == s).sum()))
            seen += sorted(set(subjects.tolist()))
        assert len(seen) == len(set(seen))                              # a subject appears in one batch of an epoch
        left = len(eligible) % P
        assert set(seen) == eligible if left != 1 else len(seen) == len(eligible) - 1      # only a last group of one is dropped
        assert len(batches) == len(eligible) // P + (1 if left >= 2 else 0)


def test_pk_batches_are_a_pure_function_of_the_seed_and_leave_the_global_stream_alone():
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    a = fi.pk_batches(CODES, 3, 2, np.random.default_rng(7))
    b = fi.pk_batches(CODES, 3, 2, np.random.default_rng(7))
    c = fi.pk_batches(CODES, 3, 2, np.random.default_rng(8))
    assert a == b and a != c
    assert np.array_equal(before, np.random.get_state()[1])
    rng = np.random.default_rng(7)
    assert fi.pk_batches(CODES, 3, 2, rng) == a and fi.pk_batches(CODES, 3, 2, rng) != a   # the next epoch draws on
    assert fi.pk_batches(np.asarray([0, 1, -1, -1], np.int32), 2, 2, np.random.default_rng(0)) == []
    assert fi.pk_batches(np.asarray([0, 0, 1], np.int32), 2, 2, np.random.default_rng(0)) == []   # one eligible subject: no negatives


# ----------------------------------------------------------------------------- 4. configuration
_conf, no_device = mining_cpu._conf, mining_cpu.no_device


@pytest.mark.parametrize('hps', [dict(batch_mining='hard'), dict(batch_mining=1), dict(batch_mining='semi_hard'),
                                 dict(batch_mining='batch_hard', pk_crops=1), dict(batch_mining='batch_hard', pk_crops='4'),
                                 dict(batch_mining='batch_hard', pk_crops=True), dict(batch_mining='batch_semi_hard', pk_subjects=1),
                                 dict(batch_mining='batch_semi_hard', pk_subjects=2.0), dict(batch_mining='batch_hard', pk_seed=-1),
                                 dict(batch_mining='batch_hard', pk_seed='0'),
                                 dict(batch_mining='batch_hard', triplet_mining='semi_hard'),
                                 dict(batch_mining='batch_semi_hard', triplet_mining='hardest'),
                                 dict(batch_mining='batch_hard', pk_subjects=513, pk_crops=2)])
def test_a_bad_batch_mining_configuration_is_refused_before_a_device_is_touched(tmp_path, no_device, hps):
    with pytest.raises(ValueError, match='batch_mining|pk_crops|pk_subjects|pk_seed'):
        fi.FaceIdentifier(_conf(tmp_path, **dict(dict(batch_size=13), **hps)))


def test_a_pk_batch_beyond_one_call_at_the_image_size_is_refused(tmp_path, no_device):
    conf = _conf(tmp_path, batch_size=13, batch_mining='batch_hard', pk_subjects=25, pk_crops=4)
    conf['fi_conf']['nn_arch']['image_size'] = 416                      # one call takes 96 images of 416 x 416
    with pytest.raises(ValueError, match='pk_subjects'):
        fi.FaceIdentifier(conf)
    assert fi.batch_mining_conf(dict(batch_size=13, batch_mining='batch_hard', pk_subjects=24, pk_crops=4), 416)['P'] == 24


def test_batch_mining_values_that_are_served():
    assert fi.batch_mining_conf({}, 64) is None and fi.batch_mining_conf(dict(batch_mining=None), 64) is None
    assert fi.batch_mining_conf(dict(batch_mining='none', pk_crops=0, triplet_mining='semi_hard'), 64) is None   # off: nothing else is read
    assert fi.batch_mining_conf(dict(batch_mining='batch_hard', batch_size=13), 416) == dict(mode='batch_hard', P=9, K=4, seed=0)
    assert fi.batch_mining_conf(dict(batch_mining='batch_semi_hard', batch_size=13, pk_crops=3, pk_seed=5), 416) == \
        dict(mode='batch_semi_hard', P=13, K=3, seed=5)                 # 3 * 13 // 3: the reference's 39 tower images
    assert fi.batch_mining_conf(dict(batch_mining='batch_hard', batch_size=1, pk_crops=8), 64)['P'] == 2
    assert fi.batch_mining_conf(dict(batch_mining='batch_hard', batch_size=2, pk_subjects=512, pk_crops=2), 64)['P'] == 512
    assert fi.batch_mining_conf(dict(batch_mining='batch_hard', batch_size=2, triplet_mining='none'), 64)['K'] == 4


def test_batch_mining_on_two_ranks_is_refused_before_the_ranks_are_started(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(parallel, 'launch_ranks', lambda *a, **k: pytest.fail('ranks were started'))
    conf = _conf(tmp_path, batch_size=4, batch_mining='batch_semi_hard')
    conf['fi_conf'].update(multi_gpu=True, num_gpus=2)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match='batch_mining'):
        fi.main()
    ident = object.__new__(fi.FaceIdentifier)
    ident.hps, ident.world, ident.rank, ident.conf = conf['fi_conf']['hps'], 2, 0, conf['fi_conf']
    monkeypatch.setattr(parallel, 'DataParallelTrainer', lambda *a, **k: pytest.fail('a process group was formed'))
    with pytest.raises(NotImplementedError, match='batch_mining'):
        ident.train()


def test_two_ranks_without_batch_mining_are_still_started(tmp_path, monkeypatch, no_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(parallel, 'launch_ranks', lambda n, target, **k: 43)
    conf = _conf(tmp_path, batch_size=4, batch_mining='none')
    conf['fi_conf'].update(multi_gpu=True, num_gpus=2)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(SystemExit) as e:
        fi.main()
    assert e.value.code == 43


# ----------------------------------------------------------------------------- 5. train()'s loop over recorders
loop = mining_cpu.loop


@pytest.mark.parametrize('hps', [{}, dict(batch_mining=None), dict(batch_mining='none')])
def test_without_the_key_train_makes_the_calls_it_made_and_draws_the_same_random_numbers(loop, monkeypatch, capsys, hps):
    monkeypatch.setattr(fi, 'pk_batches', lambda *a, **k: pytest.fail('the sampler was called'))
    monkeypatch.setattr(fi.FaceIdentifier, '_train_pk', lambda *a, **k: pytest.fail('the PK loop was entered'))
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
    assert 'anchors' not in out and out.count('Epoch') == 2


def test_with_the_key_train_hands_over_to_the_pk_loop_and_leaves_the_global_stream(loop, monkeypatch):
    calls = []
    monkeypatch.setattr(fi.FaceIdentifier, '_train_pk', lambda self, tr_gen, pk, steps, epochs: calls.append((pk, steps, epochs)))
    ident = loop(batch_mining='batch_semi_hard', pk_crops=2, pk_seed=3)
    ident.image_size = 64
    np.random.seed(11)
    before = np.random.get_state()[1].copy()
    ident.train()
    assert np.array_equal(before, np.random.get_state()[1])
    assert calls == [(dict(mode='batch_semi_hard', P=3, K=2, seed=3), 4, 2)]
    assert mining_cpu._Trainer.fed == [] and mining_cpu._Model.saved == ['face_identifier.h5']
