"""The device-resident crop store on the GPU: fv_gather_u8_f32 against the numpy restatement of its contract
(tests/crop_gather_ref.py; float32, exact equality) -- every byte value, repeats, chunking, offsets beyond 4 GiB, refusals --,
CropStore.load against Pillow for every kind of file a faces directory can hold, the inputs of a training step from both tiers
against the sequence's own load(), and FaceIdentifier.train() / make_facial_ids_db() with and without the store."""
import ctypes
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import crop_store as cs
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError, lib, ptr
from crop_gather_ref import gather_u8_f32

pytestmark = pytest.mark.gpu

FV_ERR_INVALID = -1
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _raw_gather(store, n_slots, elems, idx, dst_ptr):
    arr = (ctypes.c_int32 * max(1, len(idx)))(*idx)
    return lib().fv_gather_u8_f32(_ctx().handle, ptr(store), n_slots, elems, arr, len(idx), ctypes.c_void_p(dst_ptr))


# ----------------------------------------------------------------------------- 1. all byte values, duplicates, order
def test_gather_every_byte_value_with_repeats():
    S = 32
    rng = np.random.default_rng(0)
    store = rng.integers(0, 256, (5, S, S, 3), dtype=np.uint8)
    store[3].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)          # whatever the generator drew: all 256 values are there,
    store[4].reshape(-1)[-256:] = np.arange(256, dtype=np.uint8)[::-1]   # in a slot that is gathered (4) and one that is not (3)
    idx = [4, 0, 4, 2, 2, 1]
    assert len(np.unique(store[idx])) == 256
    got = fi.gather_crops_f32(_ctx(), torch.from_numpy(store).cuda(), idx)
    assert got.shape == (6, S, S, 3) and got.dtype == torch.float32
    want = gather_u8_f32(store, idx)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ----------------------------------------------------------------------------- 2. chunking
@pytest.mark.parametrize('extra', [0, 1])
def test_gather_at_the_launch_chunk_and_one_beyond(extra):
    n = fi.GATHER_CHUNK + extra
    rng = np.random.default_rng(1 + extra)
    store = rng.integers(0, 256, (7, 16), dtype=np.uint8)
    idx = rng.integers(0, 7, n)
    assert len(np.unique(idx)) == 7 and len(idx) > 7                      # a permutation with repeats
    got = fi.gather_crops_f32(_ctx(), torch.from_numpy(store).cuda(), idx)
    assert np.array_equal(got.cpu().numpy(), gather_u8_f32(store, idx))


def test_gather_across_a_workgroup_boundary():
    """A workgroup converts 8 KiB of a slot: one whole workgroup and a tail of 16 bytes, and a slot one 16-byte unit short of two."""
    rng = np.random.default_rng(3)
    for elems in (8192 + 16, 2 * 8192 - 16):
        store = rng.integers(0, 256, (3, elems), dtype=np.uint8)
        got = fi.gather_crops_f32(_ctx(), torch.from_numpy(store).cuda(), [2, 0, 2, 1])
        assert np.array_equal(got.cpu().numpy(), gather_u8_f32(store, [2, 0, 2, 1])), elems


def test_gather_of_nothing_writes_nothing():
    store = torch.zeros((7, 16), dtype=torch.uint8, device='cuda')
    dst = torch.full((4, 16), 7.5, dtype=torch.float32, device='cuda')
    assert _raw_gather(store, 7, 16, [], dst.data_ptr()) == 0
    assert fi.gather_crops_f32(_ctx(), store, []).shape == (0, 16)
    torch.cuda.synchronize()
    assert bool((dst == 7.5).all())


# ----------------------------------------------------------------------------- 3. 64-bit offsets
def test_gather_beyond_4_gib():
    elems, n_slots = 519168, 8274                                        # 416 x 416 x 3; slot 4 137 passes 2 GiB, 8 273 passes 4 GiB
    free = torch.cuda.mem_get_info()[0]
    if free < 6e9:
        pytest.skip('a %.1f GB store needs 6 GB free, %.1f GB are' % (elems * n_slots / 1e9, free / 1e9))
    store = torch.empty((n_slots, elems), dtype=torch.uint8, device='cuda')
    assert store.numel() > 2 ** 32
    pats = {}
    for seed, slot in enumerate((0, 4137, 8273)):
        pats[slot] = np.random.default_rng(100 + seed).integers(0, 256, elems, dtype=np.uint8)
        store[slot].copy_(torch.from_numpy(pats[slot]))
    idx = [8273, 0, 4137]
    got = fi.gather_crops_f32(_ctx(), store, idx).cpu().numpy()
    del store
    for j, slot in enumerate(idx):
        assert np.array_equal(got[j], pats[slot].astype(np.float32) / np.float32(255.0)), slot


# ----------------------------------------------------------------------------- 4. refusals
def test_gather_refusals_leave_dst_untouched():
    store = torch.zeros((5, 32), dtype=torch.uint8, device='cuda')
    dst = torch.full((4, 32), -3.25, dtype=torch.float32, device='cuda')
    assert _raw_gather(store, 5, 32, [0, 5], dst.data_ptr()) == FV_ERR_INVALID              # an index of n_slots
    assert _raw_gather(store, 5, 32, [-1], dst.data_ptr()) == FV_ERR_INVALID                # an index of -1
    assert _raw_gather(store, 5, 24, [0], dst.data_ptr()) == FV_ERR_INVALID                 # elems = 24
    assert _raw_gather(store, 5, 32, [0], dst.data_ptr() + 4) == FV_ERR_INVALID             # dst off by 4 bytes
    with pytest.raises(FvError, match='outside'):
        fi.gather_crops_f32(_ctx(), store, [1, 7], out=dst[:2])
    torch.cuda.synchronize()
    assert bool((dst == -3.25).all())


# ----------------------------------------------------------------------------- 5. store == Pillow
def _smooth(rng, h, w):
    """A picture with structure (noise alone makes every JPEG block alike): gradients plus noise."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(1, w - 1)), (y * 255 // max(1, h - 1)), ((x + y) * 255 // max(1, h + w - 2))], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def test_store_equals_pillow_for_every_kind_of_file(tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    S = 32
    rng = np.random.default_rng(5)
    kinds = [('base420.jpg', {}), ('full444.jpg', dict(subsampling=0)), ('gray.jpg', None), ('progressive.jpg', dict(progressive=True)),
             ('lossless.png', {})]
    paths = []
    for name, opts in kinds:
        img = Image.fromarray(_smooth(rng, S, S))
        if opts is None:
            img, opts = img.convert('L'), {}
        img.save(tmp_path / name, **opts)
        paths.append(str(tmp_path / name))
    slots = [3, 0, 5, 1, 4]                                              # any slots, in any order
    store = cs.CropStore(_ctx(), 6, S, torch.device('cuda', 0))
    store.data.fill_(99)
    with ThreadPoolExecutor(max_workers=2) as pool:
        store.load(paths, slots, pool)
        got = store.data.cpu().numpy()
        for p, s in zip(paths, slots):
            assert np.array_equal(got[s], fi._imread(p)), p
        assert (got[2] == 99).all()                                      # the slot nobody named
        # a scan the Huffman decoder gives up on, found only while decoding: Pillow takes that file, the chunk's others stay
        data = bytearray(open(paths[0], 'rb').read())
        sos = data.rindex(b'\xff\xda')
        at = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], 'big') + 20
        data[at:at + 40] = b'\xff\x00' * 20                             # sixteen 1-bits and more: no code of the tables
        (tmp_path / 'damaged.jpg').write_bytes(bytes(data))
        from face_vijnana_yolov3_amd import jpeg
        with pytest.raises(ValueError):
            jpeg.entropy_decode(bytes(data), jpeg.parse(bytes(data)))
        store.data.fill_(99)
        trio = [paths[1], str(tmp_path / 'damaged.jpg'), paths[0]]
        store.load(trio, [0, 1, 2], pool)
        got = store.data.cpu().numpy()
        for s, p in enumerate(trio):
            assert np.array_equal(got[s], fi._imread(p)), p
        # a file of another size: refused by name, whichever decoder would have taken it
        for name in ('wide.jpg', 'wide.png'):
            Image.fromarray(_smooth(rng, S, 48)).save(tmp_path / name)
            with pytest.raises(ValueError, match=name):
                store.load([paths[0], str(tmp_path / name)], [0, 1], pool)


# ----------------------------------------------------------------------------- 6-8. a db of 3 subjects x 2 crops
S6 = 64


def _make_tree(root):
    """As test_face_identifier_train_end_to_end's, but JPEG crops and one PNG."""
    import pandas as pd
    from PIL import Image
    rng = np.random.RandomState(1)
    os.makedirs(os.path.join(root, 'subject_faces'))
    rows = []
    for sid in range(3):
        base = _smooth(np.random.default_rng(sid), S6, S6).astype(np.int64)
        for j in range(2):
            img = np.clip(base + rng.randint(-20, 21, (S6, S6, 3)), 0, 255).astype(np.uint8)
            name = 'f%d_%d.%s' % (sid, j, 'png' if (sid, j) == (1, 1) else 'jpg')
            Image.fromarray(img).save(os.path.join(root, 'subject_faces', name))
            rows.append(dict(subject_id=sid, face_file=name))
    pd.DataFrame(rows).to_csv(os.path.join(root, 'subject_image_db.csv'))


def _conf(root, **hps):
    h = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2, loader_threads=2)
    h.update(hps)
    return {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(root), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S6, dense1_dim=64), hps=h),
            'fd_conf': {}}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('crop_store_db')
    _make_tree(str(root))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        ident = fi.FaceIdentifier(_conf(root))           # synthetic weights; tests 6 and 8 do not train it
    finally:
        os.chdir(cwd)
    return root, ident


@pytest.mark.parametrize('tier', [cs.RESIDENT, cs.PER_BATCH])
def test_inputs_of_a_step_equal_the_sequence_load(tree, monkeypatch, tier):
    root, ident = tree
    monkeypatch.chdir(root)
    monkeypatch.setattr(ident, 'hps', dict(ident.hps, **({'crop_store_mb': 0} if tier == cs.PER_BATCH else {})))
    tr_gen = fi.TrainingSequence(str(root), dict(ident.hps), ident.nn_arch, load_flag=False)
    assert len(tr_gen) == 2 and [len(tr_gen.rows(k)) for k in range(2)] == [2, 1]
    inputs = ident._triplet_inputs(tr_gen)
    try:
        assert inputs.tier == tier
        batches = [tr_gen.rows(k) for k in (0, 1, 0, 1, 1)]              # five in a row: both transient stores are written twice
        fed = 0
        for rows, xs in zip(batches, inputs.batches(batches)):
            want, _ = tr_gen.load(rows)
            assert xs[0].data_ptr() + xs[0].numel() * 4 == xs[1].data_ptr() and xs[1].data_ptr() + xs[1].numel() * 4 == xs[2].data_ptr()
            for x, key in zip(xs, ('input_a', 'input_p', 'input_n')):
                assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
                assert ident.model._as_input(x) is x                     # handed to the step untouched
                assert np.array_equal(x.cpu().numpy(), want[key]), (tier, fed, key)
            fed += 1
        assert fed == 5
    finally:
        inputs.close()


def _counted_imread(monkeypatch):
    seen, real = [], fi._imread

    def counted(path):
        seen.append(os.path.basename(path))
        return real(path)
    monkeypatch.setattr(fi, '_imread', counted)
    return seen


def test_train_end_to_end_reads_each_crop_once(tmp_path, monkeypatch):
    _make_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    seen = _counted_imread(monkeypatch)
    conf = _conf(tmp_path)
    assert 'crop_store' not in conf['fi_conf']['hps']                    # the default
    ident = fi.FaceIdentifier(conf)
    ident.train()
    assert ident.model.iterations == 2 and os.path.exists('face_identifier.h5')
    assert seen == ['f1_1.png']                                          # Pillow saw the one file the parser refuses, once
    # the sequence's own path: every image of every triplet, each time it appears
    del seen[:]
    os.remove('face_identifier.h5')
    ident = fi.FaceIdentifier(_conf(tmp_path, crop_store=False))
    ident.train()
    assert ident.model.iterations == 2 and os.path.exists('face_identifier.h5')
    assert len(seen) == 9


def test_facial_ids_db_with_and_without_the_store(tree, monkeypatch):
    root, ident = tree
    monkeypatch.chdir(root)
    ident.model.save(ident.MODEL_PATH)
    conf = _conf(root)
    conf['fi_conf']['model_loading'] = True
    again = fi.FaceIdentifier(conf)                                      # a saved model
    seen = _counted_imread(monkeypatch)
    out = {}
    for key, hps in (('store', {}), ('per_chunk', dict(crop_store_mb=0)), ('host', dict(crop_store=False))):
        again.hps = dict(conf['fi_conf']['hps'], **hps)
        del seen[:]
        again.make_facial_ids_db()
        names, sids, ids = again._db_cache
        out[key] = (list(names), [int(s) for s in sids], np.asarray(ids), fi.read_facial_ids_h5('subject_facial_ids.h5'), list(seen))
    want = out['host']
    assert len(want[4]) == 6 and want[2].shape == (6, 64) and np.isfinite(want[2]).all()
    for key in ('store', 'per_chunk'):
        got = out[key]
        assert got[0] == want[0] and got[1] == want[1]
        assert np.array_equal(got[2], want[2]), key
        assert got[4] == ['f1_1.png']
        assert sorted(got[3]) == sorted(want[3])
        for name in want[3]:
            assert np.array_equal(got[3][name][0], want[3][name][0]) and got[3][name][1] == want[3][name][1]
