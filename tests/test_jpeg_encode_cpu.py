"""The device JPEG encoder's contract without a GPU: the numpy restatement (tests/jpeg_encode_ref.py) against Pillow's own files --
quantised coefficients and whole files, exact --, the host-built header, and the wiring's refusals and fallbacks.

Conditions on Pillow's files (test_the_input_set_reaches_every_path) keep the set honest.  One of them departs from the figure
its specification named: "a DC difference of 10 or more bits" cannot occur at quality 75 -- the DC divisors are 8 << 3 (luma) and
9 << 3 (chroma) and the transform's DC is 64 (mean - 128), so a quantised DC lies in [-128, 127] and a difference has at most 8
bits.  The test asks for that maximum, 8 bits, which the 0 / 255 tiles produce."""
import io

import numpy as np
import pytest
from PIL import Image, features

import jpeg_encode_ref as ref
from face_vijnana_yolov3_amd import _lib, jpeg
from face_vijnana_yolov3_amd import face_identification as fi
from oracle import jpeg_oracle

INPUTS = ref.input_set()
_CACHE = {}


def _turbo():
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('this Pillow is not built on libjpeg-turbo: IJG libjpeg 9 scales its DCT differently')


def pillow_file(name):
    """Pillow's file for the input, its parsed header and its quantised coefficients (computed once)."""
    if name not in _CACHE:
        f = io.BytesIO()
        Image.fromarray(dict(INPUTS)[name]).save(f, 'JPEG')
        info = jpeg_oracle.parse(f.getvalue())
        _CACHE[name] = (f.getvalue(), info, jpeg_oracle.entropy_decode(info))
    return _CACHE[name]


def _mcu_order(Y):
    my, mx = Y.shape[0] // 2, Y.shape[1] // 2
    return Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)


def test_the_input_set_reaches_every_path():
    _turbo()
    stuffed = padded = zrl = no_eob = False
    dc_bits, dummy = 0, set()
    zz = np.array(jpeg.ZIGZAG)
    for name, rgb in INPUTS:
        data, info, coefs = pillow_file(name)
        scan = info['scan'][:-2]
        assert info['scan'][-2:] == b'\xff\xd9'
        stuffed |= b'\xff\x00' in scan
        padded |= int(ref.scan_symbols(coefs)[1].sum()) % 8 != 0
        for c, plane in enumerate(coefs):
            blocks = (_mcu_order(plane) if c == 0 else plane.reshape(-1, 64))[:, zz]
            dc_bits = max(dc_bits, int(np.abs(np.diff(blocks[:, 0], prepend=0)).max()).bit_length())
            no_eob |= bool((blocks[:, 63] != 0).any())
            for b in blocks:
                nz = np.nonzero(b[1:])[0] + 1
                zrl |= bool(len(nz) and np.diff(nz, prepend=0).max() > 16)
        h, w = info['height'], info['width']
        cols, rows = -(-w // 8) < 2 * -(-w // 16), -(-h // 8) < 2 * -(-h // 16)
        dummy |= {'column'} if cols else set()
        dummy |= {'row'} if rows else set()
        dummy |= {'both'} if cols and rows else set()
    assert stuffed, 'no scan holds FF 00'
    assert padded, 'no scan ends inside a byte'
    assert zrl, 'no run of 16 or more zeros in front of a coefficient'
    assert dc_bits >= 8, 'largest DC difference has %d bits' % dc_bits
    assert no_eob, 'no block ends on coefficient 63'
    assert dummy == {'column', 'row', 'both'}, dummy


@pytest.mark.parametrize('name', [n for n, _ in INPUTS])
def test_restated_coefficients_equal_pillows(name):
    _turbo()
    _data, _info, want = pillow_file(name)
    got = ref.coefficients(dict(INPUTS)[name])
    for c in range(3):
        assert got[c].shape == want[c].shape and np.array_equal(got[c], want[c]), (name, c)


@pytest.mark.parametrize('name', [n for n, _ in INPUTS])
def test_restated_file_equals_pillows(name):
    _turbo()
    assert ref.encode(dict(INPUTS)[name]) == pillow_file(name)[0]


@pytest.mark.parametrize('hw', [(1, 1), (416, 416), (3456, 5184)])
def test_header_equals_pillows(hw):
    _turbo()
    f = io.BytesIO()
    Image.fromarray(np.zeros(hw + (3,), np.uint8)).save(f, 'JPEG')
    data = f.getvalue()
    head = jpeg.encode_header(*hw)
    assert head[-14:-12] == b'\xff\xda' and data[:len(head)] == head
    assert jpeg.quant_table(0) == tuple(jpeg_oracle.parse(data)['qt'][0]) and jpeg.quant_table(1) == tuple(jpeg_oracle.parse(data)['qt'][1])


def test_without_the_library_the_encoder_raises(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'libfv_hotpath.so'))
    with pytest.raises(_lib.FvError):
        jpeg.encode_batch(None, None, [0], [8, 8], 'cuda')
    with pytest.raises(_lib.FvError):
        jpeg.encode_coefs(None, None, [0], [8, 8], 'cuda')


def test_only_sizes_a_jpeg_holds_go_to_the_device():
    assert fi.encode_on_device(True, 1, 1) and fi.encode_on_device(True, 65535, 65535)
    assert not fi.encode_on_device(True, 65536, 10) and not fi.encode_on_device(True, 10, 65536)
    assert not fi.encode_on_device(True, 0, 10) and not fi.encode_on_device(False, 416, 416)
    with pytest.raises(ValueError):
        jpeg.encode_header(65536, 8)


def test_cut_and_write_without_device_encode_never_reaches_the_encoder(monkeypatch, tmp_path):
    """The device stages stubbed (no GPU here): with device_encode off the crops go through write_crop and the encoder, a stub
    that raises, is never called; with it on, the same call reaches the stub."""
    import torch
    S = 32
    crops = np.random.default_rng(1).integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    records = [fi.CropRecord('a.jpg', (0, 0, 5, 5), 'c%d.jpg' % i, (1, 'c%d.jpg' % i, 5, 5)) for i in range(3)]

    class Stream(object):
        def synchronize(self):
            pass

    def refuse(*a, **k):
        raise AssertionError('the encoder was reached')
    monkeypatch.setattr(fi, 'load_batch', lambda *a, **k: None)
    monkeypatch.setattr(fi, 'stage_batch', lambda *a, **k: None)
    monkeypatch.setattr(fi, 'crop_nearest_u8', lambda *a, **k: torch.from_numpy(crops))
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda t: t)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: Stream())
    monkeypatch.setattr(jpeg, 'encode_batch', refuse)

    class Ctx(object):
        device = 0
    fi.cut_and_write(Ctx(), records, S, str(tmp_path), 2, hw_of=lambda p: (10, 10), device_encode=False)
    for i in range(3):
        f = io.BytesIO()
        Image.fromarray(crops[i]).save(f, 'JPEG')
        assert (tmp_path / ('c%d.jpg' % i)).read_bytes() == f.getvalue()
    with pytest.raises(AssertionError, match='the encoder was reached'):
        fi.cut_and_write(Ctx(), records, S, str(tmp_path), 2, hw_of=lambda p: (10, 10), device_encode=True)
