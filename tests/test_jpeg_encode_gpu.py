"""The device JPEG encoder on the GPU (csrc/jpeg_enc.hip): its front end's coefficients against the numpy restatement and against
Pillow's files, encode_batch's files against Pillow's byte for byte, batch counts, refusals, the bytes around the output, and the
two FaceIdentifier paths that write files with device_encode on against the Pillow path.  Exact equality everywhere."""
import ctypes
import io
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image, features

import jpeg_encode_ref as ref
from face_vijnana_yolov3_amd import data, jpeg
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd._lib import Context, FvError, ptr
from oracle import jpeg_oracle

pytestmark = pytest.mark.gpu

INPUTS = ref.input_set()
_CTX = []


def _ctx():
    if not _CTX:
        _CTX.append(Context(0))
    return _CTX[0]


def _turbo():
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('this Pillow is not built on libjpeg-turbo: IJG libjpeg 9 scales its DCT differently')


def _pillow(rgb):
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, 'JPEG')
    return f.getvalue()


def _upload(raws, order=None, gap=0):
    """The images packed into one device buffer in `order` (gap bytes of 0xEE between them) -> (buffer, offsets, hw) in the
    images' own order."""
    order = list(range(len(raws))) if order is None else order
    offs, parts, o = [0] * len(raws), [], 0
    for i in order:
        offs[i] = o
        parts += [raws[i].reshape(-1), np.full(gap, 0xEE, np.uint8)]
        o += raws[i].size + gap
    hw = [v for r in raws for v in r.shape[:2]]
    return torch.from_numpy(np.concatenate(parts)).cuda(), offs, hw


@pytest.fixture(scope='module')
def batch():
    """The whole input set in one buffer, in shuffled buffer order; Pillow's files and the restatement's coefficients, once."""
    raws = [a for _, a in INPUTS]
    order = [int(i) for i in np.random.default_rng(5).permutation(len(raws))]
    return raws, _upload(raws, order, gap=5), [_pillow(a) for a in raws], [ref.coefficients(a) for a in raws]


def test_front_end_coefficients_equal_the_restatement_and_pillow(batch):
    _turbo()
    raws, (buf, offs, hw), files, want = batch
    got = jpeg.encode_coefs(_ctx(), buf, offs, hw, buf.device)
    for i, (name, _) in enumerate(INPUTS):
        pil = jpeg_oracle.entropy_decode(jpeg_oracle.parse(files[i]))
        for c in range(3):
            assert got[i][c].shape == want[i][c].shape, (name, c)
            assert np.array_equal(got[i][c], want[i][c]), (name, c)           # dummy blocks included: the grids are whole MCUs
            assert np.array_equal(got[i][c], pil[c]), (name, c)


def test_files_equal_pillows_in_one_shuffled_call(batch):
    _turbo()
    raws, (buf, offs, hw), files, _ = batch
    got = jpeg.encode_batch(_ctx(), buf, offs, hw, buf.device)
    assert len(got) == len(files)
    for (name, _), g, w in zip(INPUTS, got, files):
        assert g == w, name
    assert bool((buf.cpu().numpy()[np.array(offs[:3]) + np.array([r.size for r in raws[:3]])] == 0xEE).all())   # the input is only read


@pytest.mark.parametrize('n', [0, 1, 65])
def test_batch_counts(n):
    _turbo()
    rng = np.random.default_rng(n)
    raws = [rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), 3), dtype=np.uint8) for _ in range(n)]
    if n == 0:
        assert jpeg.encode_batch(_ctx(), torch.zeros(16, dtype=torch.uint8, device='cuda'), [], [], torch.device('cuda', 0)) == []
        return
    buf, offs, hw = _upload(raws, [int(i) for i in rng.permutation(n)])
    got = jpeg.encode_batch(_ctx(), buf, offs, hw, buf.device)
    for k in range(n):
        assert got[k] == _pillow(raws[k]), (k, raws[k].shape)


def _raw_calls(buf, offs, hw, ws, counts_dev, counts_host, out, packed_bytes=None, ws_bytes=None, out_bytes=None):
    L = jpeg._fn()
    n = len(offs)
    o, s = (ctypes.c_int64 * max(1, n))(*offs), (ctypes.c_int32 * max(2, 2 * n))(*hw)
    rc1 = L.fv_jpeg_encode_measure(_ctx().handle, ptr(buf), buf.numel() if packed_bytes is None else packed_bytes, o, s, n, ptr(ws),
                                   ws.numel() if ws_bytes is None else ws_bytes, ptr(counts_dev))
    rc2 = None
    if counts_host is not None:
        rc2 = L.fv_jpeg_encode_emit(_ctx().handle, s, n, ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                    (ctypes.c_int64 * max(1, n))(*counts_host), ptr(out), out.numel() if out_bytes is None else out_bytes)
    return rc1, rc2


def test_refusals_leave_output_and_workspace_untouched_and_the_canaries_stand():
    _turbo()
    FV_ERR_INVALID = -1
    rng = np.random.default_rng(3)
    raws = [rng.integers(0, 256, (20, 31, 3), dtype=np.uint8), rng.integers(0, 256, (9, 50, 3), dtype=np.uint8)]
    buf, offs, hw = _upload(raws)
    want = [_pillow(r) for r in raws]
    scans = [w[len(jpeg.encode_header(*r.shape[:2])):-2] for w, r in zip(want, raws)]
    total = sum(len(s) for s in scans)
    need = jpeg._fn().fv_jpeg_encode_workspace_bytes((ctypes.c_int32 * 4)(*hw), 2)
    assert need > 0
    assert jpeg._fn().fv_jpeg_encode_workspace_bytes((ctypes.c_int32 * 2)(0, 5), 1) == -1
    assert jpeg._fn().fv_jpeg_encode_workspace_bytes((ctypes.c_int32 * 2)(5, 65536), 1) == -1
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
    counts_dev = torch.full((2,), -7, dtype=torch.int64, device='cuda')
    out = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    inner = out[32:32 + total]

    def untouched():
        torch.cuda.synchronize()
        return bool((ws == 0xA5).all()) and bool((counts_dev == -7).all()) and bool((out == 0x5A).all())
    good_counts = [len(s) for s in scans]
    for bad_hw in ([0, 31, 9, 50], [20, 0, 9, 50], [20, 31, 65536, 50], [20, 31, 9, 65536], [-1, 31, 9, 50]):     # a zero size, one above 65535
        assert _raw_calls(buf, offs, bad_hw, ws, counts_dev, good_counts, inner) == (FV_ERR_INVALID, FV_ERR_INVALID)
        assert untouched(), bad_hw
    for bad_offs in ([0, buf.numel() - 10], [-1, offs[1]], [0, buf.numel() + 1]):                                 # an offset outside the buffer
        assert _raw_calls(buf, bad_offs, hw, ws, counts_dev, None, inner)[0] == FV_ERR_INVALID
        assert untouched(), bad_offs
    assert _raw_calls(buf, offs, hw, ws, counts_dev, None, inner, packed_bytes=buf.numel() - 1)[0] == FV_ERR_INVALID
    assert _raw_calls(buf, offs, hw, ws, counts_dev, good_counts, inner, ws_bytes=need - 1) == (FV_ERR_INVALID, FV_ERR_INVALID)   # a short workspace
    assert untouched()
    with pytest.raises(FvError):
        _ctx().check(FV_ERR_INVALID, 'fv_jpeg_encode_measure')
    # the good call: counts, then a short output refused, then the exact one -- and not a byte around it
    rc1, _ = _raw_calls(buf, offs, hw, ws, counts_dev, None, inner)
    assert rc1 == 0 and counts_dev.cpu().tolist() == good_counts
    snap = ws.clone()
    L = jpeg._fn()
    s = (ctypes.c_int32 * 4)(*hw)
    c = (ctypes.c_int64 * 2)(*good_counts)
    assert L.fv_jpeg_encode_emit(_ctx().handle, s, 2, ptr(ws), need, c, ptr(inner), total - 1) == FV_ERR_INVALID          # a short output
    assert L.fv_jpeg_encode_emit(_ctx().handle, s, 2, ptr(ws), need, (ctypes.c_int64 * 2)(0, good_counts[1]), ptr(inner), total) == FV_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == snap).all())
    assert L.fv_jpeg_encode_emit(_ctx().handle, s, 2, ptr(ws), need, c, ptr(inner), total) == 0
    got = out.cpu().numpy()
    assert bool((got[:32] == 0x5A).all()) and bool((got[32 + total:] == 0x5A).all())                                     # canaries, both sides
    assert got[32:32 + total].tobytes() == b''.join(scans)


# ----------------------------------------------------------------------------- the two paths that write files
def _conf(raw, S, **hps):
    h = dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2, sim_th=0.2)
    h.update(hps)
    return {'fi_conf': dict(mode='data', resource_type='uccs', raw_data_path=str(raw), test_path=str(raw / 'frames'),
                            output_file_path=str(raw / 'solution_fi.csv'), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64), hps=h),
            'fd_conf': {}}


def _read_dir(d):
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def test_create_db_fi_writes_the_same_files_either_way(tmp_path, monkeypatch):
    _turbo()
    monkeypatch.chdir(tmp_path)
    S = 96
    data.make_synthetic_uccs(str(tmp_path / 'training'), n_images=6, seed=3)
    got = {}
    for on in (True, False):
        res = fi.create_db_fi(_conf(tmp_path, S, device_encode=on))
        got[on] = (res, _read_dir(tmp_path / 'subject_faces'), open('subject_image_db.csv').read())
    assert got[True][0] == got[False][0] and got[True][0]['written'] >= 6
    assert list(got[True][1]) == list(got[False][1]) and len(got[True][1]) == got[True][0]['written']
    for name in got[True][1]:
        assert got[True][1][name] == got[False][1][name], name
    assert got[True][2] == got[False][2]


def test_evaluate_writes_the_same_frames_either_way(tmp_path, monkeypatch):
    _turbo()
    from test_fi_evaluate_gpu import _fd_conf, _fi_conf, _tune_head
    monkeypatch.chdir(tmp_path)
    S = 96
    rng = np.random.default_rng(7)
    os.makedirs(tmp_path / 'frames')
    import pandas as pd
    rows = []
    for k, (h, w) in enumerate([(120, 200), (150, 90)]):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
        Image.fromarray(np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]).save(tmp_path / 'frames' / ('frame_%02d.jpg' % k), quality=92)
        rows.append(dict(FACE_ID=k, FILE='frame_%02d.jpg' % k, SUBJECT_ID=3, FACE_X=10.5, FACE_Y=12.5, FACE_WIDTH=40.0, FACE_HEIGHT=30.0))
    pd.DataFrame(rows, columns=['FACE_ID', 'FILE', 'SUBJECT_ID', 'FACE_X', 'FACE_Y', 'FACE_WIDTH', 'FACE_HEIGHT']).to_csv(
        tmp_path / 'frames' / 'validation.csv', index=False)
    reg = rng.normal(size=(2, 64)).astype(np.float32)
    with open('ref_facial_id_db.pickle', 'wb') as f:
        pickle.dump({3: reg[0], 11: reg[1]}, f)
    ident = fi.FaceIdentifier({'fi_conf': _fi_conf(tmp_path, S), 'fd_conf': _fd_conf(tmp_path, S)})
    _tune_head(ident.fd, S)
    ident.hps['sim_th'] = 10.0
    got = {}
    for on in (True, False):
        ident.evaluate(device_encode=on)
        got[on] = (_read_dir(tmp_path / 'frames' / 'results_fi'), open(tmp_path / 'solution_fi.csv', 'rb').read())
    assert len(got[True][0]) == 2 and list(got[True][0]) == list(got[False][0])
    for name in got[True][0]:
        assert got[True][0][name] == got[False][0][name], name
    assert got[True][1] == got[False][1]
