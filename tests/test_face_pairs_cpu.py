"""Face verification on the host: face_pairs()'s subject enumeration, random draw and block table against the reference's own
cal_VAL_FAR output (tests/golden/face_pairs.npz, minted by tests/golden/make_pairs_golden.py), a sequential fp64 restatement of
the kernel's distance contract against the reference's snrm2 distances, the two h5 files, and the new CLI modes' arguments."""
import os

import numpy as np
import pytest

from face_vijnana_yolov3_amd import evaluate as ev
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'face_pairs.npz')


def _golden():
    z = np.load(GOLDEN)
    return z, int(z['ncases'])


def restated_dists(ids, ra, rb):
    """fv_fid_pair_dists' contract: sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences, rounded to
    float32."""
    a = np.asarray(ids, np.float64)[ra]
    b = np.asarray(ids, np.float64)[rb]
    s = np.zeros(len(ra))
    for k in range(a.shape[1]):
        d = a[:, k] - b[:, k]
        s = s + d * d
    return np.sqrt(s).astype(np.float32)


def ulp_diff(x, y):
    """Distance in float32 ulps of two arrays of non-negative float32 values."""
    return np.abs(np.asarray(x, np.float32).view(np.int32).astype(np.int64) - np.asarray(y, np.float32).view(np.int32).astype(np.int64))


def _case_pairs(z, c, tmp_path):
    p = tmp_path / ('case%d.csv' % c)
    p.write_bytes(z['case%d_csv' % c].tobytes())
    np.random.seed(int(z['case%d_seed' % c]))
    pairs = ev.face_pairs(str(p))
    id_of = dict(zip([str(n) for n in z['case%d_names' % c]], z['case%d_ids' % c]))
    ids = np.asarray([id_of[n] for n in pairs['names']], np.float32)
    return pairs, ids


def test_enumeration_and_draw_match_golden(tmp_path):
    z, n = _golden()
    for c in range(n):
        pairs, ids = _case_pairs(z, c, tmp_path)
        assert np.array_equal(pairs['draw'], z['case%d_draw' % c]), c
        assert pairs['n_same'] == len(z['case%d_same_dists' % c]) and pairs['n_diff'] == len(z['case%d_diff_dists' % c]), c
        assert -1 in pairs['subject_ids']
        b = pairs['blocks']
        assert b.dtype == np.int64 and b.shape[1] == 6
        ra, rb = fi.expand_pair_blocks(b)
        assert len(ra) == pairs['n_same'] + pairs['n_diff'] and np.all(ra >= 0) and np.all(rb >= 0)
        kinds = b[:, 5]
        assert np.all(b[kinds == 0, 4] < max(pairs['n_same'], 1)) and np.all(b[kinds == 1, 4] >= pairs['n_same'])
    # case 0 has subject -1 drawn into a pair: that row is skipped, so fewer rectangles than draws
    p0, _ = _case_pairs(z, 0, tmp_path)
    assert np.any(p0['draw'] == 0) and int(np.sum(p0['blocks'][:, 5] == 1)) < len(p0['draw'])


def test_restatement_matches_reference_distances_and_val_far(tmp_path):
    z, n = _golden()
    for c in range(n):
        pairs, ids = _case_pairs(z, c, tmp_path)
        ra, rb = fi.expand_pair_blocks(pairs['blocks'])
        d = restated_dists(ids, ra, rb)
        ns = pairs['n_same']
        want_s, want_d = z['case%d_same_dists' % c], z['case%d_diff_dists' % c]
        assert np.all(want_s.astype(np.float32) == want_s) and np.all(want_d.astype(np.float32) == want_d)   # float32 values
        assert ulp_diff(d[:ns], want_s).max() <= 1, c
        assert ulp_diff(d[ns:], want_d).max() <= 1, c
        ths = z['case%d_sim_ths' % c]
        th32 = ths.astype(np.float32)
        counts = np.asarray([[np.sum(d[:ns] <= t) for t in th32], [np.sum(d[ns:] <= t) for t in th32]])
        vals, fars = ev.val_far(counts, ns, pairs['n_diff'])
        assert np.array_equal(vals, z['case%d_vals' % c]) and np.array_equal(fars, z['case%d_fars' % c]), c
        assert np.array_equal(ths, ev.SIM_TH_RANGE)


def test_block_table_pair_order_small():
    # a triangle of 4 rows at 10, then a 2 x 3 rectangle: the reference's append order
    b = np.asarray([[10, 4, 10, 4, 0, 0], [0, 2, 5, 3, 6, 1]], np.int64)
    ra, rb = fi.expand_pair_blocks(b)
    assert list(zip(ra.tolist(), rb.tolist())) == [(10, 11), (10, 12), (10, 13), (11, 12), (11, 13), (12, 13),
                                                  (0, 5), (0, 6), (0, 7), (1, 5), (1, 6), (1, 7)]
    assert fi.pair_block_pairs(b).tolist() == [6, 6]


def test_val_far_empty_is_nan():
    vals, fars = ev.val_far(np.zeros((2, 3), np.int64), 0, 5)
    assert np.all(np.isnan(vals)) and np.array_equal(fars, np.zeros(3))


def test_h5_files_round_trip(tmp_path):
    same = np.asarray([0.25, 0.5, 1.0], np.float32)
    diff = np.asarray([0.75], np.float32)
    p = str(tmp_path / 'face_pairs_dists.h5')
    ev.write_face_pairs_dists(p, same, diff)
    data, _ = read_hdf5(p)
    assert sorted(data) == ['/diff_dists', '/same_dists']
    assert data['/same_dists'].dtype == np.float32 and np.array_equal(data['/same_dists'], same)
    assert data['/diff_dists'].dtype == np.float32 and np.array_equal(data['/diff_dists'], diff)
    p = str(tmp_path / 'empty.h5')
    ev.write_face_pairs_dists(p, np.zeros(0, np.float32), diff)
    data, _ = read_hdf5(p)
    assert data['/same_dists'].shape == (0,) and data['/same_dists'].dtype == np.float32


def test_cli_arguments(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    # the existing modes still need both csvs
    for mode in ('cal_map_fd', 'cal_acc_fi'):
        with pytest.raises(SystemExit):
            ev.main(['--mode', mode])
        with pytest.raises(SystemExit):
            ev.main(['--mode', mode, '--gt_path', 'gt.csv'])
    with pytest.raises(SystemExit):
        ev.main(['--mode', 'no_such_mode', '--gt_path', 'a', '--sol_path', 'b'])
    # the verification modes take neither: with no database in the cwd they get as far as reading it
    for mode in ('cal_face_pairs_dists', 'cal_VAL_FAR'):
        with pytest.raises(FileNotFoundError):
            ev.main(['--mode', mode, '--seed', '3'])
    with pytest.raises(FileNotFoundError):
        ev.main(['--mode', 'cal_VAL_FAR', '--counts_only', '--resource_type', 'vggface2'])
    with pytest.raises(ValueError):
        ev.main(['--mode', 'cal_VAL_FAR', '--resource_type', 'nope'])
