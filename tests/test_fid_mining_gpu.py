"""Triplet mining on the GPU: fv_fid_mine_negatives against its numpy restatement (tests/mine_negatives_ref.py) -- the chosen
row and its kind equal, both distances bit for bit -- on random facial IDs around the scan's stride, on the hand cases, with
unknown subjects and exact ties, under every grouping of the same triplets; its refusals; and FaceIdentifier.mine_triplets() /
train() with hps['triplet_mining'] on a small synthetic subject db, in both tiers of the crop store."""
import ctypes
import os
import pickle
import random

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import crop_store as cs
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError, lib, ptr
import mine_negatives_ref as ref

pytestmark = pytest.mark.gpu

FV_ERR_INVALID = -1
PB = fi.MINE_PB
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _mine(ids, subjects, pairs, margin, mode, table=None):
    """The operator on `pairs` (grouped by runs of equal anchors, or as `table` says) -> the four outputs in the pairs' order."""
    anchors, pos_off, positives, order = fi.triplet_groups(pairs) if table is None else table
    out = fi.fid_mine_negatives(_ctx(), torch.from_numpy(ids).cuda(), torch.from_numpy(subjects).cuda(), anchors, pos_off, positives,
                                margin, mode)
    back = []
    for o in out:
        v = o.cpu().numpy()
        w = np.empty_like(v)
        w[order] = v
        back.append(w)
    return back


def _assert_equal(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64 and got[3].dtype == np.float64
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what
    assert np.array_equal(_bits(got[3]), _bits(want[3])), what


# ----------------------------------------------------------------------------- 1. random cases
_REF = {}


def _random(n, mode, **kw):
    """The case and its oracle outputs, computed once."""
    key = (n, mode, tuple(sorted(kw.items())))
    if key not in _REF:
        ids, subjects, pairs = ref.random_case(n, **kw)
        _REF[key] = (ids, subjects, pairs, ref.mine_negatives(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode))
    return _REF[key]


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [255, 256, 257, 1000])
def test_random_ids_against_the_oracle(n, mode):
    ids, subjects, pairs, want = _random(n, mode)
    kinds = np.bincount(want[1], minlength=4)
    print('n %d mode %d: %d pairs, kinds %s' % (n, mode, len(pairs), kinds.tolist()))
    assert len(pairs) > n and kinds[0] > 0 and kinds[2] > 0           # the oracle first: both common kinds occur
    _assert_equal(_mine(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode), want, (n, mode))


# ----------------------------------------------------------------------------- 2. hand cases, unknown subjects, exact ties
CASES = ref.hand_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_case(name):
    c = CASES[name]
    want = ref.mine_negatives(c['ids'], c['subjects'], c['pairs'], c['margin'], c['mode'])
    assert list(zip(want[0].tolist(), want[1].tolist())) == c['want']
    _assert_equal(_mine(c['ids'], c['subjects'], c['pairs'], c['margin'], c['mode']), want, name)


def test_hand_cases_reach_kinds_1_and_3_and_the_smallest_tables():
    assert {1, 3} <= {k for c in CASES.values() for _, k in c['want']}
    assert {1, 2} <= {len(c['ids']) for c in CASES.values()}


@pytest.mark.parametrize('mode', [0, 1])
def test_a_tenth_of_the_rows_of_unknown_subject(mode):
    ids, subjects, pairs, want = _random(300, mode, unknown=0.1)
    assert 15 <= (subjects < 0).sum() <= 45
    got = _mine(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode)
    _assert_equal(got, want, mode)
    assert (got[0] >= 0).all() and (subjects[got[0]] >= 0).all()
    assert (subjects[got[0]] != subjects[[a for a, _ in pairs]]).all()


def duplicated_case(mode):
    """Twenty of the rows that are chosen most often, each copied over another row of its subject: a twin is eligible whenever its
    twin is and lies at the same distance, bit for bit.  -> (ids, subjects, pairs, lower twins, higher twins)"""
    ids, subjects, pairs = ref.random_case(300, seed=1)
    first = ref.mine_negatives(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode)[0]
    chosen, counts = np.unique(first[first >= 0], return_counts=True)
    src = chosen[np.argsort(-counts, kind='stable')][:20]
    dst = []
    for r in src:
        own = [int(k) for k in np.flatnonzero(subjects == subjects[r]) if k not in src and k not in dst]
        dst.append(own[-1])
    dst = np.asarray(dst)
    ids = ids.copy()
    ids[dst] = ids[src]
    return ids, subjects, pairs, np.minimum(src, dst), np.maximum(src, dst)


@pytest.mark.parametrize('mode', [0, 1])
def test_twenty_duplicated_rows_resolve_to_the_lower_index(mode):
    ids, subjects, pairs, lo, hi = duplicated_case(mode)
    assert len(lo) == 20 and len(set(lo) | set(hi)) == 40
    want = ref.mine_negatives(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode)
    assert np.isin(want[0], lo).sum() > 100 and not np.isin(want[0], hi).any()      # the oracle first: the ties decide many triplets
    _assert_equal(_mine(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode), want, mode)


# ----------------------------------------------------------------------------- 3. the grouping does not matter
@pytest.mark.parametrize('mode', [0, 1])
def test_outputs_do_not_depend_on_the_grouping(mode):
    ids, subjects, _ = ref.random_case(257)
    rng = np.random.RandomState(5)
    sizes = [1, PB, PB + 1, 3 * PB + 2]
    anchors = [3, 250, 256, 100]
    pairs = [(a, int(p)) for a, k in zip(anchors, sizes) for p in rng.randint(0, 257, k)]
    want = ref.mine_negatives(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode)
    grouped = fi.triplet_groups(pairs)
    assert np.diff(grouped[1]).tolist() == sizes
    got = _mine(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode, grouped)
    _assert_equal(got, want, 'grouped')
    # every triplet a group of its own, in reversed order
    t = len(pairs)
    rev = pairs[::-1]
    single = (np.asarray([a for a, _ in rev], np.int32), np.arange(t + 1, dtype=np.int32), np.asarray([p for _, p in rev], np.int32),
              np.arange(t)[::-1].copy())
    alone = _mine(ids, subjects, pairs, fi.TRIPLET_MARGIN, mode, single)
    for g, s in zip(got, alone):
        assert np.array_equal(g.view(np.int64 if g.dtype == np.float64 else np.int32), s.view(np.int64 if s.dtype == np.float64 else np.int32))
    # an empty group between two others changes nothing either
    gap = (np.asarray([3, 7, 3], np.int32), np.asarray([0, 1, 1, 2], np.int32), np.asarray([pairs[0][1], pairs[0][1]], np.int32),
           np.arange(2))
    twice = _mine(ids, subjects, [pairs[0], pairs[0]], fi.TRIPLET_MARGIN, mode, gap)
    for g, s in zip(got, twice):
        assert g[0] == s[0] == s[1] or (np.isnan(g[0]) and np.isnan(s).all())


# ----------------------------------------------------------------------------- 4. refusals
def _raw(ids, subjects, n, anchors, pos_off, positives, t, margin, mode, outs):
    i32p = ctypes.POINTER(ctypes.c_int32)
    arr = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(i32p)
    keep = [np.ascontiguousarray(v, np.int32) for v in (anchors, pos_off, positives)]
    return lib().fv_fid_mine_negatives(_ctx().handle, ptr(ids), ptr(subjects), n, keep[0].ctypes.data_as(i32p), keep[1].ctypes.data_as(i32p),
                                       len(keep[0]), keep[2].ctypes.data_as(i32p), t, float(margin), mode, *[ptr(o) for o in outs])


def test_refusals_leave_the_outputs_untouched():
    n = 10
    ids = torch.from_numpy(ref.random_case(n)[0]).cuda()
    subjects = torch.arange(n, dtype=torch.int32, device='cuda') % 3
    outs = [torch.full((4,), -7, dtype=torch.int32, device='cuda'), torch.full((4,), -7, dtype=torch.int32, device='cuda'),
            torch.full((4,), -7.5, dtype=torch.float64, device='cuda'), torch.full((4,), -7.5, dtype=torch.float64, device='cuda')]
    ok = dict(anchors=[0, 1], pos_off=[0, 2, 3], positives=[3, 6, 4], t=3, margin=0.2, mode=0)
    bad = [dict(positives=[3, n, 4]), dict(anchors=[0, n]), dict(positives=[3, -1, 4]), dict(anchors=[-1, 1]),
           dict(pos_off=[0, 3, 2]), dict(pos_off=[1, 2, 3]), dict(pos_off=[0, 2, 4]), dict(margin=0.0), dict(margin=-0.2),
           dict(margin=float('nan')), dict(margin=float('inf')), dict(mode=2), dict(mode=-1), dict(t=-1)]
    for change in bad:
        a = dict(ok, **change)
        rc = _raw(ids, subjects, n, a['anchors'], a['pos_off'], a['positives'], a['t'], a['margin'], a['mode'], outs)
        assert rc == FV_ERR_INVALID, change
    assert _raw(ids, subjects, 0, ok['anchors'], ok['pos_off'], ok['positives'], 3, 0.2, 0, outs) == FV_ERR_INVALID       # n < 1
    with pytest.raises(FvError, match='outside'):
        fi.fid_mine_negatives(_ctx(), ids, subjects, np.asarray([0], np.int32), np.asarray([0, 1], np.int32), np.asarray([n], np.int32))
    # no triplets: nothing is written, with groups or without
    assert _raw(ids, subjects, n, [0, 1], [0, 0, 0], [], 0, 0.2, 0, outs) == 0
    assert _raw(ids, subjects, n, [], [0], [], 0, 0.2, 1, outs) == 0
    assert [o.numel() for o in fi.fid_mine_negatives(_ctx(), ids, subjects, np.zeros(0, np.int32), np.zeros(1, np.int32),
                                                     np.zeros(0, np.int32))] == [0, 0, 0, 0]
    torch.cuda.synchronize()
    assert all(bool((o == (-7 if o.dtype == torch.int32 else -7.5)).all()) for o in outs)
    # and the valid table, last: the three triplets are written, the fourth slot is not
    assert _raw(ids, subjects, n, ok['anchors'], ok['pos_off'], ok['positives'], 3, 0.2, 0, outs) == 0
    torch.cuda.synchronize()
    assert bool((outs[1][:3] != -7).all()) and int(outs[1][3]) == -7 and float(outs[3][3]) == -7.5


# ----------------------------------------------------------------------------- 5. end to end on a small subject db
S5 = 32
N_SUBJECTS, PER_SUBJECT, N_UNKNOWN = 4, 3, 2


def _smooth(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(1, w - 1)), (y * 255 // max(1, h - 1)), ((x + y) * 255 // max(1, h + w - 2))], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def _make_tree(root):
    """4 subjects x 3 JPEG crops (one of them a PNG, which only Pillow reads) and two crops of unknown identity (-1)."""
    import pandas as pd
    from PIL import Image
    rng = np.random.RandomState(1)
    os.makedirs(os.path.join(root, 'subject_faces'))
    rows = []
    for sid in [0, 1, 2, 3, -1]:
        base = _smooth(np.random.default_rng(sid + 5), S5, S5).astype(np.int64)
        for j in range(PER_SUBJECT if sid >= 0 else N_UNKNOWN):
            img = np.clip(base + rng.randint(-20, 21, (S5, S5, 3)), 0, 255).astype(np.uint8)
            name = 'f%d_%d.%s' % (sid, j, 'png' if (sid, j) == (1, 1) else 'jpg')
            Image.fromarray(img).save(os.path.join(root, 'subject_faces', name))
            rows.append(dict(subject_id=sid, face_file=name))
    pd.DataFrame(rows).to_csv(os.path.join(root, 'subject_image_db.csv'))


def _conf(root, **hps):
    h = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=2, step=1, batch_size=4, loader_threads=2)
    h.update(hps)
    return {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(root), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S5, dense1_dim=64), hps=h),
            'fd_conf': {}}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('mining_db')
    _make_tree(str(root))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        ident = fi.FaceIdentifier(_conf(root, triplet_mining='semi_hard'))           # synthetic weights
        tr_gen = fi.TrainingSequence(str(root), dict(ident.hps), ident.nn_arch, load_flag=False)     # writes the pickle
        # the oracle's side: the extractor's IDs of the same crops, in two calls of other sizes than mining's one chunk
        labels = list(tr_gen.db.index)
        x = np.asarray([fi._imread(tr_gen.path(label)) for label in labels])
        ids = np.concatenate([ident.fid_extractor.predict(x[:5]), ident.fid_extractor.predict(x[5:])])
    finally:
        os.chdir(cwd)
    return root, ident, tr_gen, ids


def _want_rows(tr_gen, ids, mode):
    labels = list(tr_gen.db.index)
    subjects = np.asarray(tr_gen.db['subject_id'], np.int32)
    pairs = [(int(t[0]), int(t[1])) for t in tr_gen.img_triplet_pairs if subjects[int(t[0])] >= 0]
    neg, kind, _, _ = ref.mine_negatives(ids, fi.subject_codes(list(subjects)), pairs, fi.TRIPLET_MARGIN, mode)
    return pairs, neg, kind


@pytest.mark.parametrize('how', ['alone', 'alone_per_chunk', 'resident_inputs', 'per_batch_inputs', 'host'])
def test_mine_triplets_equals_the_oracle_on_the_extractors_ids(tree, monkeypatch, how):
    root, ident, tr_gen, ids = tree
    monkeypatch.chdir(root)
    more = {'alone_per_chunk': dict(crop_store_mb=0), 'per_batch_inputs': dict(crop_store_mb=0), 'host': dict(crop_store=False)}.get(how, {})
    monkeypatch.setattr(ident, 'hps', dict(ident.hps, **more))
    n_pairs = N_SUBJECTS * 3 + 1
    assert len(tr_gen.img_triplet_pairs) == n_pairs
    pairs, neg, kind = _want_rows(tr_gen, ids, 0)
    assert len(pairs) == n_pairs - 1                                  # the pair of the two unknown crops is left out
    want = [(a, p, int(n)) for (a, p), n, k in zip(pairs, neg, kind) if k != ref.KIND_NONE]
    assert len(want) == len(pairs)
    inputs = ident._triplet_inputs(tr_gen) if how.endswith('_inputs') else None
    try:
        if inputs is not None:
            assert inputs.tier == (cs.RESIDENT if how == 'resident_inputs' else cs.PER_BATCH)
            rows, kinds = ident.mine_triplets(False, tr_gen, inputs)
        else:
            rows, kinds = ident.mine_triplets()                       # reads the pickle
    finally:
        if inputs is not None:
            inputs.close()
    assert [tuple(int(v) for v in r) for r in rows] == want
    assert np.array_equal(kinds, kind) and ident.last_mining['counts'] == np.bincount(kind, minlength=4).tolist()
    easy = kind == ref.KIND_EASY
    rows2, kinds2 = ident.mine_triplets(True, tr_gen)
    assert [tuple(int(v) for v in r) for r in rows2] == [w for w, e in zip(want, easy) if not e] and np.array_equal(kinds2, kind[~easy])


def _epoch_losses(text):
    return [line.split('loss:')[1].strip() for line in text.splitlines() if line.startswith('Epoch')]


def test_train_with_mining_end_to_end(tmp_path, monkeypatch, capsys):
    _make_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    seen, loads, fed = [], [], []
    real_imread, real_load, real_batches = fi._imread, cs.CropStore.load, cs.TripletInputs.batches
    monkeypatch.setattr(fi, '_imread', lambda path: (seen.append(os.path.basename(path)), real_imread(path))[1])
    monkeypatch.setattr(cs.CropStore, 'load', lambda self, paths, *a, **k: (loads.append(len(paths)), real_load(self, paths, *a, **k))[1])

    def batches(self, batches_of_rows):
        fed.extend(batches_of_rows)
        return real_batches(self, batches_of_rows)
    monkeypatch.setattr(cs.TripletInputs, 'batches', batches)
    ident = fi.FaceIdentifier(_conf(tmp_path, triplet_mining='semi_hard', mining_every=1, mining_drop_easy=False))
    ident.train()
    n_crops, n_pairs = N_SUBJECTS * PER_SUBJECT + N_UNKNOWN, N_SUBJECTS * 3
    assert loads == [n_crops] and seen == ['f1_1.png']               # one load of the store; Pillow saw the one file it must, once
    assert os.path.exists('face_identifier.h5')
    assert ident.model.iterations == 2 * 3 and len(fed) == 6         # 12 mined rows in batches of 4, step = 4 (13 triplets)
    db = ident_db = fi.TrainingSequence(str(tmp_path), dict(ident.hps), ident.nn_arch, load_flag=True).db
    subject = {label: int(s) for label, s in zip(db.index, db['subject_id'])}
    for e in range(2):
        rows = [r for b in fed[3 * e:3 * e + 3] for r in b]
        assert len(rows) == n_pairs and len({(r[0], r[1]) for r in rows}) == n_pairs
        for a, p, n in rows:
            assert subject[a] >= 0 and subject[p] == subject[a] and subject[n] >= 0 and subject[n] != subject[a]
    out = capsys.readouterr().out
    assert out.count('Mining (semi_hard)') == 2 and len(_epoch_losses(out)) == 2 and 'nan' not in _epoch_losses(out)
    # the pickle is the reference's list: 13 triplets with the random negatives, the unknown pair among them
    with open('img_triplet_pairs.pickle', 'rb') as f:
        assert len(pickle.load(f)) == n_pairs + 1
    # the default, mining_drop_easy on: only the triplets that still have a loss are cut into batches, fewer than hps['step']
    del fed[:]
    ident = fi.FaceIdentifier(_conf(tmp_path, triplet_mining='semi_hard', epochs=1))
    ident.train()
    counts = ident.last_mining['counts']
    kept = counts[fi.KIND_SEMI_HARD] + counts[fi.KIND_VIOLATING]
    assert sum(counts) == n_pairs and counts[fi.KIND_NONE] == 0
    assert len(fed) == fi.num_batches(kept, 4) <= 3 and sum(len(b) for b in fed) == kept and ident.model.iterations == len(fed)
    assert sorted(len(b) for b in fed) == sorted([4] * (kept // 4) + ([kept % 4] if kept % 4 else []))    # shuffled: the short one anywhere
    print('kinds %r: %d batches' % (counts, len(fed)))


# The parent's own run-to-run error on this test's configuration: five runs of the key-absent train() from these seeds on one
# MI355X, per step the largest minus the smallest loss (steps in the seeded batch order), and the same for the two epoch means.
# The weight-gradient kernels add with float atomics, so the last bits of dW differ between two runs of the SAME configuration
# (DESIGN.md section 4.2); this small network (S = 32: one pixel after the base, batch statistics over four triplets) amplifies
# that from step to step.  The five runs' last step: 0.206, 0.103, 0.125, 0.147, 0.081; epoch means 0.1681 .. 0.1690 and 0.1099 ..
# 0.1414.
STEP_SPREAD = [0.0, 0.0, 4.1e-5, 3.361e-3, 1.1943e-2, 6.6466e-2, 1.006e-3, 1.25178e-1]
EPOCH_SPREAD = [8.4e-4, 3.158e-2]
SPREAD_FACTOR = 4                 # two runs against the range of five: room for a tail the five did not show


def test_train_without_the_key_is_what_it_was(tmp_path, monkeypatch, capsys):
    """Two runs from the same seeds, the key absent and 'none': the same pickle, the same batches in the same order, the same
    number of steps, no call into the mining code, and the same losses as far as two runs of ONE configuration have them: the
    first step sees the initial weights only and must agree bit for bit; step k within SPREAD_FACTOR x STEP_SPREAD[k] (at least
    1e-6: the second step was equal in all five runs, but its weights already carry dW's last bits), the printed epoch means within
    SPREAD_FACTOR x EPOCH_SPREAD plus one unit of the last printed digit.  Steps 2 to 5 are the tight ones (1e-6, 1.6e-4, 1.3e-2,
    4.8e-2 on losses between 0.03 and 0.24): a change of the feed or of the optimiser state shows there."""
    from face_vijnana_yolov3_amd import parallel
    _make_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(fi, 'fid_mine_negatives', lambda *a, **k: pytest.fail('the binding was called'))
    monkeypatch.setattr(fi.FaceIdentifier, 'mine_triplets', lambda *a, **k: pytest.fail('mine_triplets was called'))
    fed, losses = [], []
    real_batches, real_loss = cs.TripletInputs.batches, parallel.DataParallelTrainer.merged_loss

    def batches(self, batches_of_rows):
        fed.extend([tuple(int(v) for v in r) for r in rows] for rows in batches_of_rows)
        return real_batches(self, batches_of_rows)

    def merged_loss(self, loss, weight=None):
        losses.append(real_loss(self, loss, weight))
        return losses[-1]
    monkeypatch.setattr(cs.TripletInputs, 'batches', batches)
    monkeypatch.setattr(parallel.DataParallelTrainer, 'merged_loss', merged_loss)
    runs = []
    for hps in ({}, dict(triplet_mining='none')):
        np.random.seed(3)
        random.seed(3)
        del fed[:], losses[:]
        ident = fi.FaceIdentifier(_conf(tmp_path, **hps))
        ident.train()
        with open('img_triplet_pairs.pickle', 'rb') as f:
            data = f.read()
        os.remove('face_identifier.h5')
        out = capsys.readouterr().out
        assert 'Mining' not in out
        print('epoch losses %r, step losses %r' % (_epoch_losses(out), losses))
        runs.append(dict(pickle=data, fed=list(fed), losses=list(losses), epochs=_epoch_losses(out), iterations=ident.model.iterations))
    a, b = runs
    assert a['pickle'] == b['pickle'] and a['fed'] == b['fed'] and len(a['fed']) == 2 * 4
    assert a['iterations'] == b['iterations'] == 2 * 4 and len(a['losses']) == len(b['losses']) == 8
    assert np.isfinite(a['losses']).all() and np.isfinite(b['losses']).all()
    assert a['losses'][0] == b['losses'][0]
    for k in range(1, 8):
        assert abs(a['losses'][k] - b['losses'][k]) <= max(SPREAD_FACTOR * STEP_SPREAD[k], 1e-6), (k, a['losses'], b['losses'])
    for e in range(2):
        assert abs(float(a['epochs'][e]) - float(b['epochs'][e])) <= SPREAD_FACTOR * EPOCH_SPREAD[e] + 1e-4, (a['epochs'], b['epochs'])
