"""Data-parallel FaceIdentifier training, the parts that need no GPU: main()'s self-launch of the ranks (fi_conf.multi_gpu /
num_gpus, the reference's keras.utils.multi_gpu_model at face_identification.py:303-312, 348-361), the per-rank slice of a
triplet batch as train() cuts it, and the ctypes declaration of fv_fid_train_step_dp against the header."""
import ctypes
import json
import os
import re

import pytest

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd import parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeIdentifier(object):
    made = []

    def __init__(self, conf):
        self.calls = []
        _FakeIdentifier.made.append(self)

    def __getattr__(self, name):
        if name not in ('train', 'make_facial_ids_db', 'register_facial_ids', 'test'):
            raise AttributeError(name)
        return lambda: self.calls.append(name)


@pytest.fixture
def fake_main(tmp_path, monkeypatch):
    """main() in tmp_path with the launcher, the identifier and the data mode replaced by recorders."""
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    launched = []
    _FakeIdentifier.made = []

    def launch(n, target, **kw):
        assert not _FakeIdentifier.made, 'the ranks must be started before anything is constructed'
        launched.append((n, list(target)))
        return 37
    monkeypatch.setattr(parallel, 'launch_ranks', launch)
    monkeypatch.setattr(fi, 'FaceIdentifier', _FakeIdentifier)
    monkeypatch.setattr(fi, 'create_db_fi', lambda conf: launched.append('data') and None)

    def run(mode, **fi_conf):
        conf = dict(mode=mode, resource_type='uccs', multi_gpu=True, num_gpus=2)
        conf.update(fi_conf)
        with open('face_vijnana_yolov3.json', 'w') as f:
            json.dump({'fi_conf': conf, 'fd_conf': {}}, f)
        fi.main()
    return run, launched


def test_main_train_starts_the_ranks_before_anything_else(fake_main):
    run, launched = fake_main
    with pytest.raises(SystemExit) as e:
        run('train')
    assert e.value.code == 37                                     # the launcher's return code
    assert launched == [(2, ['-m', 'face_vijnana_yolov3_amd.face_identification'])]
    assert not _FakeIdentifier.made


def test_main_train_single_gpu_configurations_do_not_launch(fake_main):
    run, launched = fake_main
    run('train', multi_gpu=False, num_gpus=8)
    run('train', multi_gpu=True, num_gpus=1)
    assert launched == []
    assert [m.calls for m in _FakeIdentifier.made] == [['train', 'make_facial_ids_db', 'register_facial_ids']] * 2


@pytest.mark.parametrize('rank,calls', [(0, ['train', 'make_facial_ids_db', 'register_facial_ids']), (1, ['train'])])
def test_main_inside_a_rank_trains_and_only_rank_0_builds_the_database(fake_main, monkeypatch, rank, calls):
    run, launched = fake_main
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', str(rank))
    run('train')
    assert launched == []
    assert [m.calls for m in _FakeIdentifier.made] == [calls]


@pytest.mark.parametrize('mode', ['data', 'fid_db', 'test'])
def test_main_other_modes_never_launch(fake_main, mode):
    run, launched = fake_main
    run(mode)
    assert [x for x in launched if x != 'data'] == []
    if mode == 'data':
        assert launched == ['data'] and not _FakeIdentifier.made
    else:
        want = ['make_facial_ids_db', 'register_facial_ids'] if mode == 'fid_db' else ['test']
        assert [m.calls for m in _FakeIdentifier.made] == [want]


def test_slice_of_a_triplet_batch_per_rank():
    """slice_triplets is what train() cuts every batch with: contiguous, disjoint, covering slices in rank order, weights n_r / n
    that sum to 1, the remainder on the last rank, and None on EVERY rank when the batch is shorter than the world."""
    for world in range(1, 5):
        for n in range(0, 10):
            rows = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(n)]
            parts = [fi.slice_triplets(rows, world, r) for r in range(world)]
            if n < world:
                assert parts == [None] * world, (world, n, parts)
                continue
            assert all(p is not None for p in parts)
            assert sum((p[0] for p in parts), []) == rows             # contiguous, disjoint, covering, in rank order
            assert all(len(p[0]) >= 1 for p in parts)
            assert abs(sum(p[1] for p in parts) - 1.0) < 1e-12
            for r, (mine, w) in enumerate(parts):
                assert w == len(mine) / float(n)
                assert len(mine) == (n // world if r < world - 1 else n - (world - 1) * (n // world))
                lo, hi, w2 = parallel.slice_batch(n, world, r)
                assert mine == rows[lo:hi] and w == w2


def _header_args(name):
    text = open(os.path.join(ROOT, 'include', 'fv_hotpath.h')).read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, text, re.S)
    assert m, '%s is not declared in the header' % name
    return [re.sub(r'\s+', ' ', a.strip()) for a in m.group(1).split(',')]


def test_ctypes_table_declares_the_data_parallel_entry_as_the_header_does():
    from face_vijnana_yolov3_amd._lib import BUCKET_FN, lib
    L = lib()
    assert L.fv_abi_version() == 4
    old, new = _header_args('fv_fid_train_step'), _header_args('fv_fid_train_step_dp')
    assert len(old) == 12 and len(new) == 15
    assert new[:12] == old                                        # the old entry's arguments, none dropped
    assert new[12:] == ['double loss_weight', 'fv_bucket_fn on_bucket', 'void* user']
    a_old, a_new = list(L.fv_fid_train_step.argtypes), list(L.fv_fid_train_step_dp.argtypes)
    assert len(a_new) == 15 and a_new[:12] == a_old
    assert a_new[12:] == [ctypes.c_double, BUCKET_FN, ctypes.c_void_p]
    assert L.fv_fid_train_step_dp.restype is ctypes.c_int
    for c_decl, ct in zip(new, a_new):                            # every argument: pointer / int / size_t / double as declared
        if c_decl.startswith('fv_bucket_fn'):
            assert ct is BUCKET_FN
        elif '*' in c_decl:
            assert ct is ctypes.c_void_p, c_decl
        elif c_decl.startswith('size_t'):
            assert ct is ctypes.c_size_t, c_decl
        elif c_decl.startswith('double'):
            assert ct is ctypes.c_double, c_decl
        else:
            assert c_decl.startswith('int ') and ct is ctypes.c_int, c_decl
