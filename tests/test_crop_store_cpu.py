"""The crop store without a GPU: the C entry point is declared and exported, plan_store's boundary, batch_slots' mapping, and the
refusals of fv_gather_u8_f32 that need no device (it checks its arguments before it looks at the context)."""
import ctypes
import os
import re

import numpy as np
import pytest

from face_vijnana_yolov3_amd import crop_store as cs
from face_vijnana_yolov3_amd import face_identification as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FV_ERR_INVALID = -1


def test_header_declares_and_library_exports_the_gather():
    from face_vijnana_yolov3_amd.build import build_library
    txt = open(os.path.join(ROOT, 'include', 'fv_hotpath.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+fv_gather_u8_f32\s*\(\s*fv_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*store\s*,\s*int64_t\s+n_slots\s*,'
                     r'\s*int64_t\s+elems\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+n\s*,\s*float\s*\*\s*dst\s*\)\s*;', code)
    L = ctypes.CDLL(build_library())
    assert hasattr(L, 'fv_gather_u8_f32')
    L.fv_abi_version.restype = ctypes.c_int
    assert L.fv_abi_version() == 4
    # the chunk the wrapper exposes is the header's
    assert int(re.search(r'#define\s+FV_GATHER_CHUNK\s+(\d+)', code).group(1)) == fi.GATHER_CHUNK


def test_plan_store_boundary():
    n, S = 7, 32
    need = n * S * S * 3
    assert cs.plan_store(n, S, need) == cs.RESIDENT
    assert cs.plan_store(n, S, need - 1) == cs.PER_BATCH
    assert cs.plan_store(n, S, need + 1) == cs.RESIDENT
    assert cs.plan_store(n, S, 0) == cs.PER_BATCH
    # 416: 519 168 bytes per crop
    assert cs.plan_store(8274, 416, 8274 * 519168) == cs.RESIDENT and cs.plan_store(8274, 416, 8274 * 519168 - 1) == cs.PER_BATCH


def _check_slots(rows):
    unique, ia, ip, in_ = cs.batch_slots(rows)
    assert len(set(unique)) == len(unique) and set(unique) == {v for t in rows for v in t}
    for col, idx in enumerate((ia, ip, in_)):
        assert idx.dtype == np.int32 and idx.shape == (len(rows),)
        assert [unique[k] for k in idx] == [t[col] for t in rows]
    return unique


def test_batch_slots_repeats_within_and_across_columns():
    rows = [(3, 4, 9), (4, 3, 9), (3, 5, 4), (5, 3, 3), (3, 4, 9)]
    unique = _check_slots(rows)
    assert sorted(unique) == [3, 4, 5, 9]
    assert _check_slots([]) == []


def test_batch_slots_on_a_non_contiguous_index():
    import pandas as pd
    db = pd.DataFrame(dict(subject_id=[0, 0, 0, 1, 1, 2, 2], face_file=['f%d.jpg' % k for k in range(7)]),
                      index=[1000, 17, 5, 2 ** 40, 42, 7, 300])
    rows = fi.make_triplets(db, np.random.RandomState(0))
    assert len(rows) == 5
    unique = _check_slots(rows)
    assert set(unique) <= set(db.index) and all(db.loc[u, 'face_file'] for u in unique)


def _lib():
    from face_vijnana_yolov3_amd.build import build_library
    L = ctypes.CDLL(build_library())
    L.fv_gather_u8_f32.restype = ctypes.c_int
    L.fv_gather_u8_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.c_int, ctypes.c_void_p]
    L.fv_last_error.restype = ctypes.c_char_p
    L.fv_last_error.argtypes = [ctypes.c_void_p]
    return L


# (n_slots, elems, idx, n, store address, dst address) -> a word of the reason.  The addresses are never dereferenced: the
# call returns before it would look at the context, which is NULL here.
REFUSALS = [
    ('index == n_slots', 5, 32, [0, 5], None, 4096, 8192, 'index 1 is 5'),
    ('index -1', 5, 32, [-1], None, 4096, 8192, 'index 0 is -1'),
    ('elems 24', 5, 24, [0], None, 4096, 8192, 'elems 24'),
    ('elems 0', 5, 0, [0], None, 4096, 8192, 'elems 0'),
    ('dst off by 4', 5, 32, [0], None, 4096, 8196, '16-byte aligned'),
    ('store off by 8', 5, 32, [0], None, 4104, 8192, '16-byte aligned'),
    ('negative n', 5, 32, [0], -1, 4096, 8192, 'n -1'),
    ('null store', 5, 32, [0], None, None, 8192, 'null pointer'),
    ('null dst', 5, 32, [0], None, 4096, None, 'null pointer'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_gather_refuses_before_it_needs_a_device(case):
    _name, n_slots, elems, idx, n, store, dst, word = case
    L = _lib()
    arr = (ctypes.c_int32 * len(idx))(*idx)
    rc = L.fv_gather_u8_f32(None, store, n_slots, elems, arr, len(idx) if n is None else n, dst)
    assert rc == FV_ERR_INVALID
    assert word in L.fv_last_error(None).decode()
