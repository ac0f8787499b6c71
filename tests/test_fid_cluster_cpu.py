"""fv_fid_cluster without a GPU: its NumPy restatement (tests/fid_cluster_ref.py) against scikit-learn's DBSCAN and against
outputs written out by hand on an exact lattice, and the host side around it: hps['cluster'], register_clusters, main()."""
import json
import pickle

import numpy as np
import pytest

from face_vijnana_yolov3_amd import face_identification as fi
import fid_cluster_ref as ref


def _partition(labels, rows):
    """The sets of `rows` that share a label."""
    groups = {}
    for i in rows:
        groups.setdefault(int(labels[i]), set()).add(int(i))
    return sorted(sorted(g) for g in groups.values())


@pytest.fixture(scope='module')
def mixed_cases():
    out = []
    for seed in range(3):
        ids = ref.mixed(1200, seed)
        out.append((ids, ref.distances(ids)))
    return out


@pytest.mark.parametrize('eps,min_pts', [(0.9, 4), (1.0, 6)])
def test_reference_equals_scikit_learn_where_dbscan_is_order_independent(mixed_cases, eps, min_pts):
    cluster = pytest.importorskip('sklearn.cluster')
    for ids, D in mixed_cases:
        out = ref.cluster(ids, eps, min_pts, D)
        core = out['core'].astype(bool)
        n_clusters, n_core, n_border, n_noise = ref.classes(out)
        print('clusters %d, core %d, border %d, noise %d, smallest |D - eps| %.3e' % (n_clusters, n_core, n_border, n_noise,
                                                                                     np.abs(D - eps).min()))
        assert n_clusters >= 2 and n_core and n_border and n_noise
        assert np.abs(D - eps).min() > 1e-9              # scikit-learn rounds its distances differently: no pair near the threshold
        sk = cluster.DBSCAN(eps=eps, min_samples=min_pts, algorithm='brute').fit(ids.astype(np.float64))
        assert np.array_equal(sk.core_sample_indices_, np.flatnonzero(core))
        assert np.array_equal(sk.labels_ == -1, out['labels'] == -1)
        rows = np.flatnonzero(core)
        assert _partition(sk.labels_, rows) == _partition(out['labels'], rows)
        for i in np.flatnonzero(~core & (out['labels'] >= 0)):
            near = np.flatnonzero(core & (D[i] <= eps))
            assert sk.labels_[i] in set(sk.labels_[near])
            assert out['via'][i] in near and out['labels'][i] == out['labels'][out['via'][i]]


@pytest.mark.parametrize('case', ref.hand_cases(), ids=lambda c: c[0])
def test_reference_on_the_hand_built_cases(case):
    name, ids, eps, min_pts, want = case
    got = ref.cluster(ids, eps, min_pts)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


def test_hand_built_distances_are_exact():
    for name, ids, eps, min_pts, want in ref.hand_cases():
        x = ids[np.isfinite(ids)].astype(np.float64) * 8
        assert (x == np.round(x)).all() and np.abs(x).max() < 2 ** 20, name      # small multiples of 1 / 8: every D ** 2 is exact
    D = ref.distances(ref.points([(0.0,), (1.0,)]))
    assert D[0, 1] == 1.0 and D[0, 1] > np.nextafter(1.0, 0.0)


def test_permuting_the_rows_permutes_the_result():
    ids = ref.mixed(700, 5)
    D = ref.distances(ids)
    out = ref.cluster(ids, 0.9, 4, D)
    assert len(ref.tied_borders(out, D)) == 0            # a border row with an index tie may move with the order: none here
    n_clusters, n_core, n_border, n_noise = ref.classes(out)
    assert n_clusters >= 2 and n_core and n_border and n_noise
    perm = np.random.default_rng(11).permutation(len(ids))
    pout = ref.cluster(ids[perm], 0.9, 4)
    assert np.array_equal(pout['core'], out['core'][perm])
    assert np.array_equal(pout['n_nbr'], out['n_nbr'][perm])
    assert np.array_equal(pout['labels'] == -1, (out['labels'] == -1)[perm])
    assert pout['n_clusters'][0] == out['n_clusters'][0]
    # row k of the permuted problem is row perm[k]: the same sets of original rows, core and border rows alike
    rows = np.flatnonzero(out['labels'] >= 0)
    plabel_of = np.empty(len(ids), np.int64)
    plabel_of[perm] = pout['labels']
    assert _partition(plabel_of, rows) == _partition(out['labels'], rows)
    assert np.array_equal(perm[pout['via'][pout['via'] >= 0]], out['via'][perm][pout['via'] >= 0])


def test_chain_and_copies_closed_forms_are_the_reference():
    ids, pos = ref.chain(257, 0.125, 3)
    for min_pts in (2, 3, 4):
        got, want = ref.cluster(ids, 0.125, min_pts), ref.chain_expected(pos, min_pts)
        for k in want:
            assert np.array_equal(got[k], want[k]), (min_pts, k)
    ids, g = ref.copies(40, 5, 2)
    for min_pts in (5, 6):
        got, want = ref.cluster(ids, 0.5, min_pts), ref.copies_expected(g, 5, min_pts)
        for k in want:
            assert np.array_equal(got[k], want[k]), (min_pts, k)


# ------------------------------------------------------------------------------------------------------------------ cluster_conf
def test_cluster_conf_defaults_and_accepted_forms():
    assert fi.cluster_conf({}) is None
    assert fi.cluster_conf({'cluster': None}) is None and fi.cluster_conf({'cluster': False}) is None
    assert fi.cluster_conf({'cluster': True, 'sim_th': 0.75}) == dict(eps=0.75, min_pts=3, register=False)
    assert fi.cluster_conf({'cluster': {}, 'sim_th': 1}) == dict(eps=1.0, min_pts=3, register=False)
    assert fi.cluster_conf({'cluster': {'eps': 0}}) == dict(eps=0.0, min_pts=3, register=False)
    assert fi.cluster_conf({'cluster': {'eps': 0.5, 'min_pts': 1, 'register': True}, 'sim_th': 0.9}) == dict(eps=0.5, min_pts=1, register=True)
    assert fi.cluster_conf({'cluster': {'min_pts': np.int64(7)}, 'sim_th': np.float32(0.5)}) == dict(eps=0.5, min_pts=7, register=False)


@pytest.mark.parametrize('hps', [
    {'cluster': True},                                               # no eps and no sim_th to take it from
    {'cluster': 'dbscan', 'sim_th': 0.9},
    {'cluster': 1, 'sim_th': 0.9},
    {'cluster': {'epsilon': 0.5}, 'sim_th': 0.9},
    {'cluster': {'eps': True}}, {'cluster': {'eps': '0.5'}}, {'cluster': {'eps': -0.1}}, {'cluster': {'eps': float('nan')}},
    {'cluster': {'eps': float('inf')}}, {'cluster': True, 'sim_th': float('inf')},
    {'cluster': {'min_pts': 0}, 'sim_th': 0.9}, {'cluster': {'min_pts': True}, 'sim_th': 0.9}, {'cluster': {'min_pts': 2.0}, 'sim_th': 0.9},
    {'cluster': {'register': 1}, 'sim_th': 0.9}, {'cluster': {'register': 'yes'}, 'sim_th': 0.9},
], ids=repr)
def test_cluster_conf_refuses_and_names_the_key(hps):
    with pytest.raises(ValueError, match='cluster'):
        fi.cluster_conf(hps)


def test_face_identifier_validates_the_key_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(fi, 'FidModel', lambda *a, **k: pytest.fail('a model was built'))
    conf = {'fi_conf': dict(mode='cluster', resource_type='uccs', raw_data_path='.', nn_arch=dict(image_size=64, dense1_dim=64),
                            hps={'sim_th': 0.9, 'cluster': {'min_pts': 0}}, model_loading=False)}
    with pytest.raises(ValueError, match='cluster'):
        fi.FaceIdentifier(conf)


def test_cluster_csv_text():
    text = fi.cluster_csv_text(['a.jpg', 'b.jpg', 'c.jpg'], np.int32([0, -1, 0]), np.uint8([1, 0, 0]), np.int32([3, 1, 2]), np.int32([0, -1, 0]))
    assert text == 'face_file,cluster,core,n_neighbours,via_face_file\na.jpg,0,1,3,a.jpg\nb.jpg,-1,0,1,\nc.jpg,0,0,2,a.jpg\n'
    assert fi.cluster_csv_text([], [], [], [], []) == 'face_file,cluster,core,n_neighbours,via_face_file\n'
    assert fi.cluster_files('uccs') == 'subject_clusters.csv' and fi.cluster_files('vggface2') == 'subject_clusters_vggface2.csv'


# ------------------------------------------------------------------------------------------------------------------ register_clusters
def _bare_identifier(resource_type='uccs'):
    obj = fi.FaceIdentifier.__new__(fi.FaceIdentifier)
    obj.conf = dict(resource_type=resource_type)
    return obj


def test_register_clusters_appends_one_subject_per_cluster(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    ids = rng.standard_normal((7, 64)).astype(np.float32)
    result = dict(names=['f%d.jpg' % k for k in range(7)], ids=ids, labels=np.int32([1, 0, -1, 1, 0, 1, -1]), n_clusters=2)
    old = {np.int64(9): np.full(64, 0.5), np.int64(4): np.full(64, 0.25)}
    with open('ref_facial_id_db.pickle', 'wb') as f:
        pickle.dump(old, f)
    obj = _bare_identifier()
    assert obj.register_clusters(result) == [10, 11]
    with open('ref_facial_id_db.pickle', 'rb') as f:
        db = pickle.load(f)
    assert list(db.keys()) == [9, 4, 10, 11]                           # the old entries in their order, then cluster order
    assert np.array_equal(db[9], old[9]) and np.array_equal(db[4], old[4])
    assert np.array_equal(db[10], fi.subject_mean(ids[[1, 4]])) and np.array_equal(db[11], fi.subject_mean(ids[[0, 3, 5]]))
    # an explicit first_id; one that runs into a registered id is refused and the file stays
    before = open('ref_facial_id_db.pickle', 'rb').read()
    for first in (3, 4, 8, 9, 10, 11):
        with pytest.raises(ValueError, match='registered already'):
            obj.register_clusters(result, first_id=first)
    assert open('ref_facial_id_db.pickle', 'rb').read() == before
    assert obj.register_clusters(result, first_id=100) == [100, 101]
    with open('ref_facial_id_db.pickle', 'rb') as f:
        assert list(pickle.load(f).keys()) == [9, 4, 10, 11, 100, 101]


def test_register_clusters_starts_an_empty_registry_at_zero(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ids = np.arange(3 * 64, dtype=np.float32).reshape(3, 64)
    obj = _bare_identifier('vggface2')
    assert obj.register_clusters(dict(ids=ids, labels=np.int32([0, 0, -1]), n_clusters=1)) == [0]
    with open('ref_facial_id_vggface2_db.pickle', 'rb') as f:
        db = pickle.load(f)
    assert list(db.keys()) == [0] and np.array_equal(db[0], fi.subject_mean(ids[:2]))
    assert obj.register_clusters(dict(ids=ids, labels=np.int32([-1, -1, -1]), n_clusters=0)) == []


# ------------------------------------------------------------------------------------------------------------------ main()
class _Recorder(object):
    calls = []

    def __init__(self, conf):
        self.cluster = fi.cluster_conf(conf['fi_conf']['hps'])
        _Recorder.calls.append('init')

    def cluster_unknown(self):
        _Recorder.calls.append('cluster_unknown')
        return 'the result'

    def register_clusters(self, result):
        _Recorder.calls.append(('register_clusters', result))


@pytest.mark.parametrize('cluster,want', [(None, ['init', 'cluster_unknown']), (True, ['init', 'cluster_unknown']),
                                          ({'register': False}, ['init', 'cluster_unknown']),
                                          ({'register': True}, ['init', 'cluster_unknown', ('register_clusters', 'the result')])])
def test_main_dispatches_the_cluster_mode(tmp_path, monkeypatch, cluster, want):
    monkeypatch.chdir(tmp_path)
    hps = {'sim_th': 0.9}
    if cluster is not None:
        hps['cluster'] = cluster
    conf = {'fi_conf': dict(mode='cluster', resource_type='uccs', raw_data_path=str(tmp_path), nn_arch=dict(image_size=64, dense1_dim=64),
                            hps=hps, model_loading=False, multi_gpu=True, num_gpus=4)}      # multi_gpu is ignored: no ranks are started
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    _Recorder.calls = []
    monkeypatch.setattr(fi, 'FaceIdentifier', _Recorder)
    fi.main()
    assert _Recorder.calls == want


def test_main_still_names_the_modes_for_an_unknown_one(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps({'fi_conf': {'mode': 'evaluate'}}))
    monkeypatch.setattr(fi, 'FaceIdentifier', lambda conf: pytest.fail('no model for an unknown mode'))
    with pytest.raises(NotImplementedError, match='available: data, train, fid_db, test, cluster'):
        fi.main()


def test_library_exports_the_entry_points():
    import ctypes
    from face_vijnana_yolov3_amd.build import build_library
    L = ctypes.CDLL(build_library())
    L.fv_fid_cluster_workspace_bytes.restype = ctypes.c_size_t
    L.fv_fid_cluster_workspace_bytes.argtypes = [ctypes.c_int]
    sizes = [L.fv_fid_cluster_workspace_bytes(n) for n in (0, -1, ref.MAX_N + 1)]
    assert sizes == [0, 0, 0]
    sizes = [L.fv_fid_cluster_workspace_bytes(n) for n in (1, 2, 63, 64, 65, 1000, 4097, ref.MAX_N)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= ref.MAX_N * ref.MAX_N // 8
    L.fv_fid_cluster.restype = ctypes.c_int
    assert L.fv_fid_cluster(*([None] * 2), 1, ctypes.c_double(0.5), 1, *([None] * 6)) == -1      # no context: refused on the host
