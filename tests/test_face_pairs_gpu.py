"""Face verification on the GPU: cal_VAL_FAR against the reference's own output (tests/golden/face_pairs.npz), fv_fid_pair_dists
against a sequential fp64 restatement on random block tables, its determinism over block order, launch split and counts-only,
its argument checks, and the CLI modes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import evaluate as ev
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError, PairBlock, lib, ptr
from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'face_pairs.npz')
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def restated_dists(ids, ra, rb):
    """The kernel's contract: sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences -> float32."""
    a = np.asarray(ids, np.float64)[ra]
    b = np.asarray(ids, np.float64)[rb]
    s = np.zeros(len(ra))
    for k in range(a.shape[1]):
        d = a[:, k] - b[:, k]
        s = s + d * d
    return np.sqrt(s).astype(np.float32)


def ulp_diff(x, y):
    return np.abs(np.asarray(x, np.float32).view(np.int32).astype(np.int64) - np.asarray(y, np.float32).view(np.int32).astype(np.int64))


def host_counts(d, kinds, th):
    return np.asarray([[int(np.sum(d[kinds == k] <= t)) for t in th] for k in (0, 1)], np.int64)


def _unit_ids(n, rng):
    x = rng.normal(size=(n, 64))
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(0.3, 0.8, (n, 1))
    return x.astype(np.float32)


def _table(rng, n_ids, shapes):
    """Blocks of the given shapes ((kind, na, nb)) at random rows, packed in order -> (blocks, n_pairs, per-pair kind)."""
    rows, off, kinds = [], 0, []
    for kind, na, nb in shapes:
        a0 = int(rng.integers(0, n_ids - na + 1))
        b0 = a0 if kind == 0 else int(rng.integers(0, n_ids - nb + 1))
        m = na * (na - 1) // 2 if kind == 0 else na * nb
        rows.append((a0, na, b0, na if kind == 0 else nb, off, kind))
        kinds += [kind] * m
        off += m
    return np.asarray(rows, np.int64), off, np.asarray(kinds)


def _run(ids_dev, blocks, th, n_dists):
    d, c = fi.fid_pair_dists(_ctx(), ids_dev, blocks, th, n_dists=n_dists)
    torch.cuda.synchronize()
    return (None if d is None else d.cpu().numpy()), c.cpu().numpy()


# ----------------------------------------------------------------------------- 1. the reference's own output
def test_cal_val_far_matches_reference(tmp_path, monkeypatch):
    z = np.load(GOLDEN)
    for c in range(int(z['ncases'])):
        d = tmp_path / ('case%d' % c)
        d.mkdir()
        monkeypatch.chdir(d)
        (d / 'subject_image_db.csv').write_bytes(z['case%d_csv' % c].tobytes())
        names = [str(n) for n in z['case%d_names' % c]]
        fi.write_facial_ids_h5('subject_facial_ids.h5', names, z['case%d_ids' % c], [0] * len(names))
        np.random.seed(int(z['case%d_seed' % c]))
        sim_ths, vals, fars = ev.cal_VAL_FAR(np.arange(0.1, 1.1, 0.1), ctx=_ctx())
        assert np.array_equal(sim_ths, z['case%d_sim_ths' % c])
        assert vals.dtype == np.float64 and np.array_equal(vals, z['case%d_vals' % c]), (c, vals)
        assert fars.dtype == np.float64 and np.array_equal(fars, z['case%d_fars' % c]), (c, fars)
        data, _ = read_hdf5('face_pairs_dists.h5')
        assert sorted(data) == ['/diff_dists', '/same_dists']
        for k in ('same_dists', 'diff_dists'):
            got, want = data['/' + k], z['case%d_%s' % (c, k)]
            assert got.dtype == np.float32 and got.shape == want.shape, (c, k)
            assert ulp_diff(got, want).max() <= 1, (c, k)
        data, _ = read_hdf5('val_far.h5')
        assert sorted(data) == ['/fars', '/sim_ths', '/vals']
        assert all(v.dtype == np.float64 for v in data.values())
        assert np.array_equal(data['/vals'], vals) and np.array_equal(data['/fars'], fars)
        # counts only: the same VAL / FAR, no distance file
        os.remove('face_pairs_dists.h5')
        np.random.seed(int(z['case%d_seed' % c]))
        s2, v2, f2 = ev.cal_VAL_FAR(np.arange(0.1, 1.1, 0.1), counts_only=True, ctx=_ctx())
        assert np.array_equal(v2, vals) and np.array_equal(f2, fars) and not os.path.exists('face_pairs_dists.h5')


# ----------------------------------------------------------------------------- 2. kernel vs the fp64 restatement
def test_kernel_against_restatement():
    rng = np.random.default_rng(5)
    n_ids = 2400
    ids = _unit_ids(n_ids, rng)
    shapes = [(0, 1, 1), (0, 2, 2), (0, 63, 63), (0, 64, 64), (0, 65, 65), (0, 1000, 1000), (0, 7, 7),
              (1, 1, 1), (1, 1, 300), (1, 300, 1), (1, 64, 65), (1, 129, 63), (1, 700, 900), (1, 5, 3)]
    shapes += [(int(k), int(rng.integers(1, 40)), int(rng.integers(1, 40))) for k in rng.integers(0, 2, 30)]
    blocks, n, kinds = _table(rng, n_ids, shapes)
    x = torch.from_numpy(ids).cuda()
    ra, rb = fi.expand_pair_blocks(blocks)
    want = restated_dists(ids, ra, rb)
    for th in (np.asarray([0.7], np.float32), np.sort(rng.uniform(0.0, 1.7, 4096)).astype(np.float32)):
        d, c = _run(x, blocks, th, n)
        assert ulp_diff(d, want).max() <= 1
        assert np.array_equal(c, host_counts(d, kinds, th))
    # duplicate thresholds, one above every distance, and distances exactly at a threshold
    th = np.asarray([want[0], want[0], want[5], 10.0], np.float32)
    d, c = _run(x, blocks, th, n)
    assert np.array_equal(c, host_counts(d, kinds, th)) and c[:, -1].sum() == n


# ----------------------------------------------------------------------------- 3. determinism
def test_order_split_and_counts_only_are_deterministic():
    rng = np.random.default_rng(9)
    n_ids = 1500
    x = torch.from_numpy(_unit_ids(n_ids, rng)).cuda()
    shapes = [(int(k), int(rng.integers(1, 150)), int(rng.integers(1, 150))) for k in rng.integers(0, 2, 40)]
    blocks, n, kinds = _table(rng, n_ids, shapes)
    th = np.linspace(0.2, 1.4, 25).astype(np.float32)
    d0, c0 = _run(x, blocks, th, n)
    perm = rng.permutation(len(blocks))
    d1, c1 = _run(x, blocks[perm], th, n)
    assert np.array_equal(d0.view(np.int32), d1.view(np.int32)) and np.array_equal(c0, c1)
    h = len(blocks) // 2
    da, ca = _run(x, blocks[:h], th, n)
    db, cb = _run(x, blocks[h:], th, n)
    split = np.where(np.arange(n) < int(blocks[h, 4]), da, db)
    assert np.array_equal(d0.view(np.int32), split.view(np.int32)) and np.array_equal(c0, ca + cb)
    _, c2 = _run(x, blocks, th, None)
    assert np.array_equal(c0, c2)


# ----------------------------------------------------------------------------- 4. argument checks
def test_rejections_leave_buffers_untouched():
    rng = np.random.default_rng(2)
    x = torch.from_numpy(_unit_ids(100, rng)).cuda()
    good = np.asarray([[0, 10, 0, 10, 0, 0], [10, 5, 20, 6, 45, 1]], np.int64)
    th = np.asarray([0.5, 10.0], np.float32)
    n = 75
    bad_tables = {
        'row range': np.asarray([[95, 10, 95, 10, 0, 0]], np.int64),
        'b range': np.asarray([[0, 5, 98, 6, 0, 1]], np.int64),
        'triangle shape': np.asarray([[0, 10, 1, 10, 0, 0]], np.int64),
        'triangle nb': np.asarray([[0, 10, 0, 9, 0, 0]], np.int64),
        'kind': np.asarray([[0, 10, 0, 10, 0, 2]], np.int64),
        'out_off overflow': np.asarray([[0, 10, 0, 10, 40, 0]], np.int64),
        'negative out_off': np.asarray([[0, 10, 0, 10, -1, 0]], np.int64),
    }
    cases = [(t, th, n) for t in bad_tables.values()]
    cases += [(good, np.asarray([1.0, 0.5], np.float32), n), (good, np.zeros(0, np.float32), n),
              (good, np.linspace(0, 1, 4097).astype(np.float32), n), (good, th, n - 1)]
    for blocks, t, nd in cases:
        counts = torch.full((2, max(1, len(t))), 7, dtype=torch.int64, device='cuda')
        dists = torch.full((n,), -3.0, dtype=torch.float32, device='cuda')
        with pytest.raises(FvError):
            table = (PairBlock * len(blocks))(*[PairBlock(*r[:5].tolist(), int(r[5]), 0) for r in blocks])
            _ctx().check(lib().fv_fid_pair_dists(_ctx().handle, ptr(x), 100, table, len(blocks),
                                                 np.ascontiguousarray(t).ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                 len(t), ptr(dists), nd, ptr(counts)), 'fv_fid_pair_dists')
        torch.cuda.synchronize()
        assert bool((counts == 7).all()) and bool((dists == -3.0).all())
    d, c = _run(x, good, th, n)                       # the good table runs
    assert c[:, -1].tolist() == [45, 30]


# ----------------------------------------------------------------------------- 5. CLI and a UCCS-sized database
def _synth_db(rng, n_subjects, mean_faces, minus1=8):
    import pandas as pd
    rows, id_of = [], {}
    for sid in [-1] + list(range(1, n_subjects)):
        n = minus1 if sid == -1 else int(rng.integers(1, 2 * mean_faces))
        c = rng.normal(size=64)
        for f in range(n):
            name = 's%05d_%03d.jpg' % (sid if sid >= 0 else 99999, f)
            v = c + 0.4 * rng.normal(size=64)
            rows.append((sid, name, 40, 40))
            if sid != -1:
                id_of[name] = (v / np.linalg.norm(v)).astype(np.float32)
    pd.DataFrame(rows, columns=['subject_id', 'face_file', 'w', 'h']).to_csv('subject_image_db.csv')
    return id_of


def _write_db(rng, n_subjects, mean_faces):
    id_of = _synth_db(rng, n_subjects, mean_faces)
    names = list(id_of)
    fi.write_facial_ids_h5('subject_facial_ids.h5', names, [id_of[n] for n in names], [0] * len(names))
    return id_of


def test_cli_writes_both_files(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    _write_db(np.random.default_rng(4), 30, 5)
    ev.main(['--mode', 'cal_VAL_FAR', '--seed', '7'])
    assert os.path.exists('face_pairs_dists.h5') and os.path.exists('val_far.h5')
    v = read_hdf5('val_far.h5')[0]
    assert np.array_equal(v['/sim_ths'], np.arange(0.1, 1.1, 0.1)) and len(v['/vals']) == 10
    assert len(capsys.readouterr().out.strip().splitlines()) == 10
    os.remove('face_pairs_dists.h5')
    ev.main(['--mode', 'cal_face_pairs_dists', '--seed', '7'])
    d = read_hdf5('face_pairs_dists.h5')[0]
    np.random.seed(7)
    pairs = ev.face_pairs('subject_image_db.csv')
    assert len(d['/same_dists']) == pairs['n_same'] and len(d['/diff_dists']) == pairs['n_diff']


def test_uccs_sized_database(tmp_path, monkeypatch):
    # 1 085 subjects, ~8 600 IDs (more face files than hdf5_lite writes into one group: the IDs go in directly)
    monkeypatch.chdir(tmp_path)
    id_of = _synth_db(np.random.default_rng(8), 1085, 8)
    np.random.seed(1)
    pairs = ev.face_pairs('subject_image_db.csv')
    assert len(pairs['names']) > 7000
    ids = np.asarray([id_of[n] for n in pairs['names']], np.float32)
    th = np.arange(0.1, 1.1, 0.1).astype(np.float32)
    (same, diff), counts = ev.face_pair_dists_device(pairs, ids, th, True, _ctx())
    assert same.dtype == np.float32 and len(same) == pairs['n_same'] and len(diff) == pairs['n_diff']
    ra, rb = fi.expand_pair_blocks(pairs['blocks'])
    want = restated_dists(ids, ra, rb)
    assert ulp_diff(np.concatenate([same, diff]), want).max() <= 1
    assert np.array_equal(counts, np.asarray([[np.sum(same <= t) for t in th], [np.sum(diff <= t) for t in th]]))
