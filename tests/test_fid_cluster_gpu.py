"""fv_fid_cluster on the device: every output byte against the NumPy restatement (tests/fid_cluster_ref.py) and against closed
forms, the workspace and stream contracts, and FaceIdentifier.cluster_unknown / register_clusters end to end."""
import ctypes
import hashlib
import os
import pickle

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, lib, ptr
import fid_cluster_ref as ref
import stream_order as so

pytestmark = pytest.mark.gpu

NAMES = ('labels', 'via', 'n_nbr', 'core', 'n_clusters')


@pytest.fixture(scope='module')
def ctx():
    c = Context(0)
    yield c
    c.close()


def _run(ctx, ids, eps, min_pts, workspace=None):
    out = fi.fid_cluster(ctx, torch.from_numpy(np.ascontiguousarray(ids)).cuda(), eps, min_pts, workspace=workspace)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_equal(got, want, what):
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, '%s: %s differs in %d of %d places, first at %d: %r, reference %r' % (
            what, k, len(bad), len(want[k]), bad[0], got[k][bad[0]], want[k][bad[0]])


# ----------------------------------------------------------------------------- 1. sizes and parameters on the mixed generator
EPS3 = (0.05, 0.9, 2.5)          # nothing within 0.05; a mix at 0.9; unit vectors are at most 2 apart


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 257, 1000, 4097])
def test_kernel_equals_the_reference(ctx, n):
    ids = ref.mixed(n, n)
    D = ref.distances(ids)
    for eps in EPS3:
        for min_pts in (1, 2, 4, n + 1):
            want = ref.cluster(ids, eps, min_pts, D)
            n_clusters, n_core, n_border, n_noise = ref.classes(want)
            if min_pts == n + 1:
                assert n_core == 0 and n_noise == n
            if min_pts == 4 and n >= 63:                 # the three regimes, on the reference alone
                if eps == EPS3[0]:
                    assert n_noise == n
                if eps == EPS3[2]:
                    assert (n_clusters, n_core) == (1, n)
                if eps == EPS3[1] and n >= 255:
                    assert n_clusters >= 2 and n_core and n_border and n_noise
            _assert_equal(_run(ctx, ids, eps, min_pts), want, 'n %d eps %g min_pts %d' % (n, eps, min_pts))


# ----------------------------------------------------------------------------- 2. ties, the chain, the largest size
def test_lattice_with_pairs_at_the_threshold_and_tied_borders(ctx):
    ids = ref.lattice(2048, 1, side=16)
    eps = float(np.sqrt(2.0 / 64.0))                     # a lattice distance: two steps of 1/8 in different dimensions
    D = ref.distances(ids)
    want = ref.cluster(ids, eps, 12, D)
    at_threshold = int((D == eps).sum()) // 2
    tied = len(ref.tied_borders(want, D))
    print('pairs exactly at eps %d, border rows with tied core distances %d, classes %r' % (at_threshold, tied, ref.classes(want)))
    assert at_threshold >= 100 and tied >= 100
    _assert_equal(_run(ctx, ids, eps, 12), want, 'lattice')


@pytest.mark.parametrize('min_pts', [2, 3, 4])
def test_chain_of_4096_in_shuffled_order(ctx, min_pts):
    ids, pos = ref.chain(4096, 0.125, 7)
    want = ref.chain_expected(pos, min_pts)              # tests/test_fid_cluster_cpu.py holds the closed form to the reference
    n_clusters, n_core, n_border, n_noise = ref.classes(want)
    assert (n_clusters, n_core, n_border, n_noise) == {2: (1, 4096, 0, 0), 3: (1, 4094, 2, 0), 4: (0, 0, 0, 4096)}[min_pts]
    _assert_equal(_run(ctx, ids, 0.125, min_pts), want, 'chain min_pts %d' % min_pts)


def test_largest_size_against_the_closed_form(ctx):
    ids, g = ref.copies(4096, 16, 3)
    assert len(ids) == ref.MAX_N
    want = ref.copies_expected(g, 16, 4)
    assert int(want['n_clusters'][0]) == 4096
    _assert_equal(_run(ctx, ids, 0.5, 4), want, 'n 65536')


# ----------------------------------------------------------------------------- 3. robustness
@pytest.mark.parametrize('case', ref.hand_cases(), ids=lambda c: c[0])
def test_hand_built_cases_on_the_device(ctx, case):
    name, ids, eps, min_pts, want = case
    _assert_equal(_run(ctx, ids, eps, min_pts), want, name)


def _buffers(n, dev, fill):
    need = int(lib().fv_fid_cluster_workspace_bytes(n))
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
    outs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.empty((n + 3) // 4, dtype=torch.int32, device=dev),
                                                                                 torch.empty(1, dtype=torch.int32, device=dev)]
    for t in [ws] + outs:
        t.fill_(fill)
    return ws, outs


def _call(ctx, x, n, eps, min_pts, ws, outs):
    """The C entry point on caller-made buffers: outs = labels, via, n_nbr, core (as int32 words), n_clusters."""
    return lib().fv_fid_cluster(ctx.handle, x, n, float(eps), int(min_pts), ws, *[ptr(t) for t in outs])


def _bytes(outs, n):
    host = [t.cpu().numpy() for t in outs]
    return dict(labels=host[0], via=host[1], n_nbr=host[2], core=host[3].view(np.uint8)[:n].copy(), n_clusters=host[4])


def test_outputs_and_workspace_contents_do_not_matter(ctx):
    n = 257
    ids = ref.mixed(n, 21)
    want = ref.cluster(ids, 0.9, 4)
    x = torch.from_numpy(ids).cuda()
    for fill in (-1, 0x7FC00000, 0x7FF80000, 0):         # 0xFF bytes, float32 and float64 NaN patterns, zeros
        ws, outs = _buffers(n, x.device, fill)
        assert _call(ctx, ptr(x), n, 0.9, 4, ptr(ws), outs) == 0
        _assert_equal(_bytes(outs, n), want, 'fill %#x' % (fill & 0xFFFFFFFF))


def test_two_calls_on_one_workspace_give_each_its_own_result(ctx):
    a, b = ref.mixed(1000, 31), ref.mixed(300, 32)
    ws = torch.empty(int(lib().fv_fid_cluster_workspace_bytes(1000)), dtype=torch.uint8, device='cuda')
    xa, xb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    oa = fi.fid_cluster(ctx, xa, 0.9, 4, workspace=ws)
    ob = fi.fid_cluster(ctx, xb, 1.0, 3, workspace=ws)   # enqueued behind the first, no host wait between them
    oc = fi.fid_cluster(ctx, xa, 0.9, 4, workspace=ws)
    _assert_equal({k: v.cpu().numpy() for k, v in oa.items()}, ref.cluster(a, 0.9, 4), 'first call')
    _assert_equal({k: v.cpu().numpy() for k, v in ob.items()}, ref.cluster(b, 1.0, 3), 'second call')
    _assert_equal({k: v.cpu().numpy() for k, v in oc.items()}, ref.cluster(a, 0.9, 4), 'third call')
    with pytest.raises(ValueError, match='workspace'):
        fi.fid_cluster(ctx, xa, 0.9, 4, workspace=ws[:100])


def test_invalid_arguments_enqueue_nothing(ctx):
    n = 70
    x = torch.from_numpy(ref.mixed(n + 1, 41)).cuda()
    ws, outs = _buffers(n, x.device, 0x5A5A5A5A)
    before = [t.clone() for t in [ws] + outs]
    X, W = ptr(x), ptr(ws)
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    bad = [(None, n, 0.9, 4, W, outs), (X, n, 0.9, 4, None, outs),
           (X, 0, 0.9, 4, W, outs), (X, -1, 0.9, 4, W, outs), (X, ref.MAX_N + 1, 0.9, 4, W, outs),
           (X, n, float('nan'), 4, W, outs), (X, n, float('inf'), 4, W, outs), (X, n, -1e-300, 4, W, outs),
           (X, n, 0.9, 0, W, outs), (X, n, 0.9, -3, W, outs),
           (odd(x), n, 0.9, 4, W, outs), (X, n, 0.9, 4, odd(ws), outs)]
    for k in range(5):                                   # each output pointer NULL in turn
        class _Null(object):
            def is_contiguous(self):
                return True

            def data_ptr(self):
                return None
        bad.append((X, n, 0.9, 4, W, outs[:k] + [_Null()] + outs[k + 1:]))
    for args in bad:
        assert _call(ctx, *args) == -1, args[:4]
    torch.cuda.synchronize()
    for t, b in zip([ws] + outs, before):
        assert torch.equal(t, b)
    assert _call(ctx, X, n, 0.9, 4, W, outs) == 0        # and the same buffers serve a valid call
    _assert_equal(_bytes(outs, n), ref.cluster(x[:n].cpu().numpy(), 0.9, 4), 'after the refusals')


def test_workspace_bytes_and_the_host_wrapper(ctx):
    size = lib().fv_fid_cluster_workspace_bytes
    assert [size(n) for n in (0, -5, ref.MAX_N + 1)] == [0, 0, 0]
    sizes = [size(n) for n in range(1, 700)] + [size(n) for n in (1000, 4097, 10000, ref.MAX_N - 1, ref.MAX_N)]
    assert min(sizes) > 0 and sizes == sorted(sizes)
    empty = fi.fid_cluster(ctx, torch.zeros((0, 64), dtype=torch.float32, device='cuda'), 0.9, 4)
    assert [tuple(empty[k].shape) for k in NAMES] == [(0,), (0,), (0,), (0,), (1,)] and int(empty['n_clusters'][0]) == 0
    for wrong in (torch.zeros((3, 64), dtype=torch.float64, device='cuda'), torch.zeros((3, 63), device='cuda'), torch.zeros(64, device='cuda')):
        with pytest.raises(ValueError, match='float32'):
            fi.fid_cluster(ctx, wrong, 0.9, 4)


def test_fid_cluster_on_a_delayed_stream(ctx):
    """The harness of tests/stream_order.py on fv_fid_cluster: exact, no host_sync (the header declares no wait).  On this
    module's context, and the harness' cached sleep calibration is put back as it was found, so that the stream-order suite
    that runs later in the process starts from the state it starts from without this file."""
    def make(seed, dev):
        return dict(ids=torch.from_numpy(ref.mixed(600, seed)).to(dev))

    def call(ctx, p):
        return fi.fid_cluster(ctx, p['ids'], 0.9, 4)
    case = so.Case('fid_cluster', ('fv_fid_cluster',), make, call, may_tie=('n_clusters',), ctx=lambda: ctx)
    assert case.exact and not case.host_sync
    calibration = dict(so._CAL)
    try:
        so.run_delayed(case)
    finally:
        so._CAL.clear()
        so._CAL.update(calibration)


# ----------------------------------------------------------------------------- 4. end to end at image size 96
S = 96
N_SUBJECTS, PER_SUBJECT, N_SINGLE, N_GROUPS, PER_GROUP = 3, 3, 28, 3, 4
# sha256 of the two files the mode fid_db writes on this tree without the 'cluster' key, recorded on the commit before
# cluster_unknown existed: the key's absence leaves the other modes' bytes alone
FID_DB_SHA256 = {'subject_facial_ids.h5': '1eea33ab751b9e212cd8f7a6d2ac96dba6d99a2ece9d4fafbbbada4198e03b4b', 'ref_facial_id_db.pickle': '99060f66f8f528bc258705064ef41a57ec3d92a1de00140b797935b438efb77d'}


def _face(rng):
    y, x = np.mgrid[0:S, 0:S]
    f = rng.uniform(0.02, 0.25, 6)
    base = np.stack([127 + 120 * np.sin(f[0] * x + f[1] * y), 127 + 120 * np.cos(f[2] * x - f[3] * y), 127 + 120 * np.sin(f[4] * (x + y) + f[5])], -1)
    return np.clip(base + rng.integers(-25, 26, (S, S, 3)), 0, 255).astype(np.uint8)


def make_tree(root):
    """3 subjects x 3 crops and 40 crops of unknown identity, 12 of them three groups of four byte-identical files, interleaved.
    PNG throughout: the pixels do not depend on a codec."""
    import pandas as pd
    from PIL import Image
    rng = np.random.default_rng(17)
    os.makedirs(os.path.join(root, 'subject_faces'))
    rows = []
    for sid in range(N_SUBJECTS):
        for j in range(PER_SUBJECT):
            name = 's%d_%d.png' % (sid, j)
            Image.fromarray(_face(rng)).save(os.path.join(root, 'subject_faces', name))
            rows.append(dict(subject_id=sid, face_file=name))
    unknown = [('u%02d.png' % k, _face(rng)) for k in range(N_SINGLE)]
    for g in range(N_GROUPS):
        img = _face(rng)
        unknown += [('g%d_%d.png' % (g, j), img) for j in range(PER_GROUP)]
    for k in rng.permutation(len(unknown)):
        name, img = unknown[k]
        Image.fromarray(img).save(os.path.join(root, 'subject_faces', name))
        rows.insert(int(rng.integers(0, len(rows) + 1)), dict(subject_id=-1, face_file=name))
    pd.DataFrame(rows).to_csv(os.path.join(root, 'subject_image_db.csv'))


def conf_of(root, **hps):
    h = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=4, loader_threads=2, sim_th=0.5)
    h.update(hps)
    return {'fi_conf': dict(mode='cluster', resource_type='uccs', raw_data_path=str(root), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64), hps=h),
            'fd_conf': {}}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    import pandas as pd
    root = tmp_path_factory.mktemp('cluster_db')
    make_tree(str(root))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        ident = fi.FaceIdentifier(conf_of(root))         # synthetic weights
        db = pd.read_csv('subject_image_db.csv').iloc[:, 1:]
        names = [ff for ff, sid in zip(db['face_file'], db['subject_id']) if sid == -1]
        x = np.asarray([fi._imread(os.path.join(str(root), 'subject_faces', ff)) for ff in names])
        ids = ident.fid_extractor.predict(x)             # one chunk, as cluster_unknown's: which conv kernels run depends on the batch
    finally:
        os.chdir(cwd)
    return root, ident, names, ids


def _choose_eps(ids, min_pts):
    """The smallest of a few quantiles of the pairwise distances at which the reference shows clusters and noise."""
    D = ref.distances(ids)
    pairs = D[np.triu_indices(len(D), 1)]
    for q in (0.02, 0.05, 0.1, 0.2, 0.3, 0.5):
        eps = float(np.quantile(pairs, q))
        want = ref.cluster(ids, eps, min_pts, D)
        n_clusters, n_core, n_border, n_noise = ref.classes(want)
        if n_clusters >= 2 and n_noise >= 1:
            return eps, want
    pytest.fail('no quantile gives two clusters and a noise row')


def test_cluster_unknown_equals_the_reference_with_the_store_on_and_off(tree, monkeypatch):
    root, ident, names, ids = tree
    monkeypatch.chdir(root)
    assert len(names) == N_SINGLE + N_GROUPS * PER_GROUP
    eps, want = _choose_eps(ids, 3)
    assert int(want['n_clusters'][0]) >= 2 and int((want['labels'] < 0).sum()) >= 1
    for g in range(N_GROUPS):                            # identical pixels, identical IDs: each group of four lies in one cluster
        rows = [k for k, ff in enumerate(names) if ff.startswith('g%d_' % g)]
        assert len(set(want['labels'][rows])) == 1 and want['labels'][rows[0]] >= 0
    texts = []
    for store in (True, False):
        monkeypatch.setitem(ident.hps, 'crop_store', store)
        res = ident.cluster_unknown(eps=eps, min_pts=3)
        assert res['names'] == names and np.array_equal(res['ids'], ids)
        got = dict(res, n_clusters=np.array([res['n_clusters']], np.int32))
        _assert_equal(got, want, 'cluster_unknown, crop_store %r' % store)
        texts.append(open('subject_clusters.csv').read())
        assert texts[-1] == fi.cluster_csv_text(names, want['labels'], want['core'], want['n_nbr'], want['via'])
    assert texts[0] == texts[1] and texts[0].count('\n') == 1 + len(names)


def test_fid_db_bytes_without_the_key_and_the_registry_after_register_clusters(tree, monkeypatch):
    root, ident, names, ids = tree
    monkeypatch.chdir(root)
    assert 'cluster' not in ident.hps and ident.cluster is None
    ident.make_facial_ids_db()
    ident.register_facial_ids()
    got = {f: hashlib.sha256(open(f, 'rb').read()).hexdigest() for f in FID_DB_SHA256}
    print('fid_db sha256: %r' % got)
    assert got == FID_DB_SHA256
    with open('ref_facial_id_db.pickle', 'rb') as f:
        before = pickle.load(f)
    assert list(before.keys()) == list(range(N_SUBJECTS))
    eps, want = _choose_eps(ids, 3)
    res = ident.cluster_unknown(eps=eps, min_pts=3)
    C = int(want['n_clusters'][0])
    assert ident.register_clusters(res) == list(range(N_SUBJECTS, N_SUBJECTS + C))
    with open('ref_facial_id_db.pickle', 'rb') as f:
        after = pickle.load(f)
    assert list(after.keys()) == list(range(N_SUBJECTS + C))
    for sid in before:
        assert np.array_equal(after[sid], before[sid])
    for c in range(C):
        assert np.array_equal(after[N_SUBJECTS + c], fi.subject_mean(ids[want['labels'] == c]))
    with pytest.raises(ValueError, match='registered already'):
        ident.register_clusters(res, first_id=N_SUBJECTS + C - 1)
