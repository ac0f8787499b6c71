"""JPEG decode split host / device (reference `imread`, face_detection.py:112, 656, 798), CPU half:
  * oracle/jpeg_oracle.py (numpy restatement of libjpeg's default decode) == Pillow, bit for bit -- Pillow is the reference's
    actual reader (scikit-image's imread goes through it) and is importable here and on the GPU box, so it pins the oracle;
  * the product's host entropy decoder (fv_jpeg_parse / fv_jpeg_entropy_decode, C++ in libfv_hotpath.so, no GPU needed) produces
    exactly the oracle's coefficients, and oracle-reconstruct(product coefficients) == Pillow at sizes the Python Huffman loop
    would take minutes for;
  * what the decoder does not take (progressive, CMYK) is refused by parse() -> the loaders fall back to Pillow;
  * the differential contract: for ANY byte string the host half either refuses it or the restatement run
    on its coefficients yields exactly Pillow's pixels -- every size 1..24 x 1..24 in every sampling mode, the files of
    tests/jpeg_stream_ref.py (streams Pillow's encoder never writes), damaged files, and blocks at the edge of the accepted
    coefficient range.  tests/test_jpeg_gpu.py sends the same files through the device kernels."""
import functools
import io
import warnings

import numpy as np
import pytest
from PIL import Image

from oracle import jpeg_oracle as jo


def _jpeg(rng, h, w, sub, q, gray=False, ri=0, progressive=False, mode=None):
    lo = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(lo).resize((w, h), Image.BICUBIC)).astype(int) + rng.integers(-25, 25, (h, w, 3))
    im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
    if gray:
        im = im.convert('L')
    if mode:
        im = im.convert(mode)
    kw = {'restart_marker_blocks': ri} if ri else {}
    b = io.BytesIO()
    im.save(b, 'JPEG', quality=q, subsampling=sub, progressive=progressive, **kw)
    return b.getvalue()


CASES = [(45, 67, 0, 90, False, 0), (45, 67, 1, 75, False, 0), (45, 67, 2, 50, False, 0), (64, 64, 2, 95, False, 0), (33, 17, 2, 80, False, 0),
         (40, 56, 0, 85, True, 0), (50, 70, 2, 85, False, 3), (9, 9, 2, 90, False, 0), (1, 1, 2, 90, False, 0), (8, 31, 1, 100, False, 0),
         (100, 130, 1, 30, False, 2), (17, 200, 2, 5, False, 0)]


@pytest.mark.parametrize('h,w,sub,q,gray,ri', CASES)
def test_oracle_equals_pillow(h, w, sub, q, gray, ri):
    data = _jpeg(np.random.default_rng(h * 1000 + w), h, w, sub, q, gray, ri)
    want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    assert np.array_equal(jo.decode(data), want)


@pytest.mark.parametrize('h,w,sub,q,gray,ri', CASES + [(480, 640, 2, 90, False, 0), (601, 333, 1, 75, False, 7), (768, 1024, 2, 85, False, 0)])
def test_host_entropy_decoder_matches_oracle_and_pillow(h, w, sub, q, gray, ri):
    from face_vijnana_yolov3_amd import jpeg
    data = _jpeg(np.random.default_rng(h * 1000 + w + 1), h, w, sub, q, gray, ri)
    info = jpeg.parse(data)
    oi = jo.parse(data)
    assert info is not None and (info.width, info.height, info.ncomp, info.restart_interval) == (w, h, 1 if gray else 3, oi['ri'])
    coefs = jpeg.entropy_decode(data, info)
    blocks = jpeg.blocks_of(info, coefs)
    for c, comp in enumerate(oi['comps']):
        assert np.array_equal(np.asarray(info.qt[c][:], np.int32), oi['qt'][comp['tq']])
    if h * w <= 20000:                                      # the oracle's Python Huffman loop, coefficient by coefficient
        for mine, theirs in zip(blocks, jo.entropy_decode(oi)):
            assert np.array_equal(mine.astype(np.int32), theirs)
    rgb = jo.reconstruct(oi, [b.astype(np.int32) for b in blocks])
    assert np.array_equal(rgb, np.asarray(Image.open(io.BytesIO(data)).convert('RGB')))


def test_unsupported_files_are_refused():
    from face_vijnana_yolov3_amd import jpeg
    rng = np.random.default_rng(3)
    assert jpeg.parse(_jpeg(rng, 40, 40, 2, 90, progressive=True)) is None
    assert jpeg.parse(_jpeg(rng, 40, 40, 0, 90, mode='CMYK')) is None
    assert jpeg.parse(b'\x89PNG\r\n\x1a\n' + b'\0' * 64) is None
    good = _jpeg(rng, 40, 40, 2, 90)
    assert jpeg.parse(good[:100]) is None                   # truncated inside the headers
    info = jpeg.parse(good)
    with pytest.raises(AssertionError):
        jpeg.entropy_decode(good, info, np.empty(10, np.int16))
    with pytest.raises(jo.Unsupported):
        jo.parse(_jpeg(rng, 40, 40, 2, 90, progressive=True))


def _mutations(rng):
    """150 damaged files: truncated anywhere, up to seven bytes overwritten anywhere, sixteen bytes of the second half overwritten."""
    for trial in range(150):
        d = bytearray(_jpeg(rng, int(rng.integers(16, 120)), int(rng.integers(16, 120)), int(rng.integers(0, 3)), 85, ri=int(rng.integers(0, 2)) * 4))
        if trial % 3 == 0:
            d = d[:int(rng.integers(2, len(d)))]
        elif trial % 3 == 1:
            for _ in range(int(rng.integers(1, 8))):
                d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
        else:
            i = int(rng.integers(len(d) // 2, len(d)))
            d[i:i + 16] = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        yield d


def test_damaged_files_never_crash_the_host_decoder():
    """Truncated files, flipped bytes anywhere, overwritten scan data: parse() refuses, entropy_decode() raises or returns
    (garbage) coefficients -- never a crash or a read past the buffer; a header claiming an absurd size is refused before any
    buffer is sized from it."""
    from face_vijnana_yolov3_amd import jpeg
    rng = np.random.default_rng(5)
    seen = {'decoded': 0, 'refused': 0, 'raised': 0}
    for d in _mutations(rng):
        info = jpeg.parse(bytes(d))
        if info is None:
            seen['refused'] += 1
            continue
        assert info.width * info.height <= jpeg.MAX_PIXELS
        try:
            jpeg.entropy_decode(bytes(d), info, np.zeros(int(info.total_coefs), np.int16))
            seen['decoded'] += 1
        except ValueError:
            seen['raised'] += 1
    assert seen['refused'] > 0 and seen['decoded'] + seen['raised'] > 0, seen
    # SOF0 with 65535 x 65535: 4.3 Gpixel
    good = bytearray(_jpeg(rng, 32, 32, 2, 85))
    k = good.find(b'\xff\xc0')
    good[k + 5:k + 9] = b'\xff\xff\xff\xff'
    assert jpeg.parse(bytes(good)) is None


def _flush_against_guard_page(data):
    """-> (pointer, keepalive): `data` copied so that its last byte is the last byte of a readable page and the next page is
    PROT_NONE -- a read one byte past the buffer faults instead of passing unnoticed (the CPU build's stand-in for ASan)."""
    import ctypes
    import mmap
    page = mmap.PAGESIZE
    npages = (len(data) + page - 1) // page + 1
    mm = mmap.mmap(-1, npages * page, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + (npages - 1) * page, page, 0) == 0          # PROT_NONE
    start = (npages - 1) * page - len(data)
    mm[start:start + len(data)] = data
    return base + start, mm


def test_parser_never_reads_past_the_buffer():
    """the fill-byte loop of parse() could read b[n] when a file ends in a run of 0xFF.  Every prefix of a real header
    and every tail of fill bytes is parsed flush against a PROT_NONE page."""
    import ctypes
    from face_vijnana_yolov3_amd import jpeg
    L = jpeg._fn()
    good = _jpeg(np.random.default_rng(11), 40, 56, 2, 90, ri=2)
    sos = good.find(b'\xff\xda')
    cases = [good[:k] for k in range(0, sos + 16)]
    cases += [b'\xff\xd8' + b'\xff' * k for k in range(0, 12)]
    cases += [good[:k] + b'\xff' * t for k in (2, 4, 20, 21, sos, sos + 2) for t in (1, 2, 3, 7)]
    for d in cases:
        if not d:
            continue
        p, keep = _flush_against_guard_page(d)
        info = jpeg.JpegInfo()
        rc = L.fv_jpeg_parse(ctypes.c_void_p(p), len(d), ctypes.byref(info))
        assert rc != 0 or len(d) > sos, (len(d), rc)
        del keep
    p, keep = _flush_against_guard_page(good)                      # the whole file, headers + scan, both entry points
    info = jpeg.JpegInfo()
    assert L.fv_jpeg_parse(ctypes.c_void_p(p), len(good), ctypes.byref(info)) == 0
    out = np.zeros(int(info.total_coefs), np.int16)
    assert L.fv_jpeg_entropy_decode(ctypes.c_void_p(p), len(good), ctypes.c_void_p(out.ctypes.data), out.size) == 0
    assert np.array_equal(out, jpeg.entropy_decode(good, jpeg.parse(good)))


def test_loader_falls_back_to_pillow_on_damaged_scan_data(tmp_path):
    """a scan-level failure of the host Huffman decoder (bad code, run past the block) used to raise out of the
    loader thread and abort train() / test(); libjpeg -- the reference's reader behind imread (fd.py:112, 798) -- only warns and
    still returns an image.  The batch must go through Pillow instead."""
    import pandas as pd
    from face_vijnana_yolov3_amd import data, jpeg
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder
    rng = np.random.default_rng(21)
    good = _jpeg(rng, 96, 128, 2, 90)
    sos = good.find(b'\xff\xda')
    bad = None
    for trial in range(400):                                        # a corruption the product refuses and Pillow still decodes
        d = bytearray(good)
        i = int(rng.integers(sos + 14, len(d) - 2))
        d[i] = int(rng.integers(0, 255))
        d = bytes(d)
        info = jpeg.parse(d)
        if info is None:
            continue
        try:
            jpeg.entropy_decode(d, info)
            continue
        except ValueError:
            pass
        try:
            Image.open(io.BytesIO(d)).convert('RGB')
        except OSError:
            continue
        bad = d
        break
    assert bad is not None, 'no single-byte corruption found that the host decoder refuses and Pillow decodes'
    root = str(tmp_path)
    open(tmp_path / 'a.jpg', 'wb').write(good)
    open(tmp_path / 'b.jpg', 'wb').write(bad)
    rows = [[0, 'a.jpg', 1, 10.0, 12.0, 30.0, 30.0], [1, 'b.jpg', 1, 20.0, 22.0, 25.0, 35.0]]
    pd.DataFrame(rows, columns=data.CSV_COLUMNS).to_csv(tmp_path / 'training.csv', index=False)
    hps = dict(batch_size=2, step=1, lr=1e-4, beta_1=0.9, beta_2=0.99, decay=0.0)
    seq = data.TrainingSequence(root, hps, {'image_size': 96, 'bb_info_c_size': 6})
    f = BatchFeeder(seq, 1, 0, threads=2)
    try:
        packed, yt, weight, _ = f.load(0)
    finally:
        f.close()
    assert not isinstance(packed[0], str), 'the damaged batch must not arrive as JPEG coefficients'
    buf, offs, hw = packed
    assert list(hw) == [96, 128, 96, 128] and tuple(yt.shape) == (2, 3, 3, 6)
    want = np.asarray(Image.open(io.BytesIO(bad)).convert('RGB')).reshape(-1)
    assert np.array_equal(buf.numpy()[offs[1]:offs[1] + want.size], want)


# ================================================================= the differential contract: refused, or exactly Pillow's pixels
def _pillow(data):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def _product(data):
    """The product's host half on `data` -> (JpegInfo, coefficient blocks per component), or None when it refuses the file
    (parse() or the scan)."""
    from face_vijnana_yolov3_amd import jpeg
    info = jpeg.parse(data)
    if info is None:
        return None
    try:
        coefs = jpeg.entropy_decode(data, info)
    except ValueError:
        return None
    return info, jpeg.blocks_of(info, coefs)


def _restate(info, blocks):
    """The restatement's pixels from the PRODUCT's header fields and coefficients (jo.parse never sees the file: damaged headers
    are the product's to judge)."""
    oi = dict(width=info.width, height=info.height, comps=[dict(h=info.h[c], v=info.v[c], tq=c) for c in range(info.ncomp)],
              qt={c: np.asarray(info.qt[c][:], np.int32) for c in range(info.ncomp)})
    return jo.reconstruct(oi, [b.astype(np.int32) for b in blocks])


def _refused_or_equal(data):
    """-> 'refused', 'equal', or a description of the breach: accepted, and Pillow raises or decodes other pixels."""
    p = _product(data)
    if p is None:
        return 'refused'
    try:
        want = _pillow(data)
    except Exception as e:                                   # noqa: BLE001 -- whatever Pillow raises, the product took the file
        return 'accepted, Pillow raises %s' % type(e).__name__
    got = _restate(*p)
    if got.shape != want.shape:
        return 'accepted, %r against Pillow %r' % (got.shape, want.shape)
    if not np.array_equal(got, want):
        return 'accepted, %d pixels differ by up to %d' % (int((got != want).any(-1).sum()), int(np.abs(got.astype(int) - want).max()))
    return 'equal'


@functools.lru_cache(maxsize=1)
def sweep_files():
    """[((h, w, mode), file)]: every size 1..24 x 1..24 as 4:4:4, 4:2:2, 4:2:0 and grey, written by Pillow at quality 90."""
    rng = np.random.default_rng(24)
    return [((h, w, mode), _jpeg(rng, h, w, 0 if mode == 'gray' else mode, 90, gray=mode == 'gray'))
            for h in range(1, 25) for w in range(1, 25) for mode in (0, 1, 2, 'gray')]


def test_size_sweep_restatement_and_product_equal_pillow():
    """Narrow subsampled images (at most two chroma columns) take libjpeg's replicating upsamplers, not the fancy ones: 4:2:2 at
    w = 3, 4 and 4:2:0 at w = 1..4 used to come out up to 43 grey levels off, in the product and in the restatement alike."""
    bad = []
    for case, data in sweep_files():
        want = _pillow(data)
        if not np.array_equal(jo.decode(data), want):
            bad.append((case, 'restatement'))
        p = _product(data)
        if p is None:
            bad.append((case, 'refused'))
        elif not np.array_equal(_restate(*p), want):
            bad.append((case, 'restatement of the product coefficients'))
    assert not bad, (len(bad), bad[:20])


def test_writer_is_read_back_by_pillow_and_the_oracle():
    """tests/jpeg_stream_ref.py against two readers: Pillow decodes every file it writes, and the oracle's Huffman decoder returns
    the coefficients that were put in."""
    import jpeg_stream_ref as sr
    for name, data, planes, expect in sr.corpus():
        _pillow(data)
        if expect is False:                                  # RGB by its component ids: the oracle refuses it like the product
            with pytest.raises(jo.Unsupported):
                jo.parse(data)
            continue
        back = jo.entropy_decode(jo.parse(data))
        assert len(back) == len(planes) and all(np.array_equal(a, b) for a, b in zip(back, planes)), name
    zz = np.zeros(64, np.int64)
    zz[47] = 3                                               # zigzag order: 16 zeros behind it -> one ZRL, and no EOB, with zrl_tail
    assert [s for k, s, _b, _n in sr.block_symbols(zz, 0, zrl_tail=True) if k][-2:] == [(14 << 4) | 2, 0xF0]
    assert [s for k, s, _b, _n in sr.block_symbols(zz, 0)][-1] == 0


def test_writer_equals_the_encoder_restatement():
    """The writer's scan for 4:2:0 with the Annex K tables is, bit for bit, jpeg_encode_ref's (itself pinned to Pillow's files)."""
    import jpeg_encode_ref as ref
    import jpeg_stream_ref as sr
    from face_vijnana_yolov3_amd.jpeg import quant_table
    rgb = np.random.default_rng(2).integers(0, 256, (21, 35, 3), dtype=np.uint8)
    planes = ref.coefficients(rgb)
    mine = sr.write(planes, 21, 35, '420', [quant_table(0), quant_table(1)], dht_combined=False)
    assert mine.endswith(ref.encode_scan(rgb) + b'\xff\xd9')
    assert np.array_equal(_pillow(mine), _pillow(ref.encode(rgb)))


def test_stream_corpus_is_refused_or_equals_pillow():
    """Every writer-made file: refused, or restatement(product coefficients) == Pillow.  Plain YCbCr, grey, restart, optimised-table
    and fill-byte variants must be accepted; 'R','G','B' ids without JFIF / Adobe marker (RGB to libjpeg, not converted; up to 242
    grey levels off when it was taken for YCbCr) must be refused."""
    import jpeg_stream_ref as sr
    bad = []
    for name, data, _planes, expect in sr.corpus():
        outcome = _refused_or_equal(data)
        if outcome not in ('refused', 'equal') or (expect is True and outcome != 'equal') or (expect is False and outcome != 'refused'):
            bad.append((name, expect, outcome))
    assert not bad, bad


def _restart_markers(data):
    """Positions of the RSTn markers of the scan (inside entropy-coded data FF is always followed by 00)."""
    sos = data.find(b'\xff\xda')
    at = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], 'big')
    return at, [i for i in range(at, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


@functools.lru_cache(maxsize=1)
def damaged_corpus():
    """[(name, bytes)]: the 150 random mutations, then damage aimed at the scan's structure."""
    out = [('mutation_%d' % i, bytes(d)) for i, d in enumerate(_mutations(np.random.default_rng(5)))]
    rng = np.random.default_rng(55)
    for tag, args in (('420', (40, 56, 2, 90, False, 0)), ('422_ri2', (40, 56, 1, 85, False, 2)), ('gray_ri1', (24, 40, 0, 85, True, 1))):
        good = _jpeg(rng, *args)
        scan, rst = _restart_markers(good)
        out += [('%s_cut_at_%d' % (tag, k), good[:k]) for k in range(scan, len(good), 7)]
        out.append((tag + '_no_eoi', good[:-2]))
        out.append((tag + '_eoi_byte_missing', good[:-1]))
        out.append((tag + '_trailing_bytes', good + b'\x00\x01\xff\xd9trailer' * 3))
        out.append((tag + '_two_files', good + good))
        for j, r in enumerate(rst):
            out.append(('%s_rst%d_removed' % (tag, j), good[:r] + good[r + 2:]))
            out.append(('%s_rst%d_duplicated' % (tag, j), good[:r] + good[r:r + 2] + good[r:]))
            out.append(('%s_rst%d_renumbered' % (tag, j), good[:r + 1] + bytes((0xD0 | ((good[r + 1] + 1) & 7),)) + good[r + 2:]))
            out.append(('%s_rst%d_garbage_in_front' % (tag, j), good[:r] + b'\x5a\xa5' + good[r:]))
    return out


def test_damaged_corpus_acceptance_implies_pillows_pixels():
    """Acceptance implies that Pillow decodes the file without an exception and to the same pixels.  A scan cut anywhere, a
    missing EOI and a missing, doubled or renumbered RSTn used to be accepted: zeros were fed behind the end of the data, and
    the decoder resynchronised on whatever RSTn came next (Pillow: an exception, or other pixels in most of the image)."""
    outcomes = {}
    bad = []
    for name, data in damaged_corpus():
        outcome = _refused_or_equal(data)
        outcomes[outcome] = outcomes.get(outcome, 0) + 1
        if outcome not in ('refused', 'equal'):
            bad.append((name, outcome))
    print(outcomes)
    assert not bad, (outcomes, bad[:20])
    # intact files with bytes behind EOI decode, as in Pillow
    tails = [n for n, d in damaged_corpus() if n.endswith(('_trailing_bytes', '_two_files'))]
    assert tails and all(_refused_or_equal(d) == 'equal' for n, d in damaged_corpus() if n in tails)


def test_strict_scan_refuses_what_libjpeg_would_patch_up():
    """The three rules of the strict scan, one file each: a bit taken from behind the end of the data or a marker; RSTn not the
    next marker at the end of an interval, or not the expected n (fill bytes allowed); no EOI behind the last MCU."""
    from face_vijnana_yolov3_amd import jpeg
    good = _jpeg(np.random.default_rng(56), 40, 56, 2, 90, ri=2)
    scan, rst = _restart_markers(good)
    assert len(rst) >= 3 and _refused_or_equal(good) == 'equal'
    r = rst[1]
    for name, d, ok in (('cut inside an interval', good[:r - 3] + good[r:], False), ('cut at the end', good[:-9], False),
                        ('no EOI', good[:-2], False), ('EOI replaced', good[:-1] + b'\xd8', False),
                        ('RSTn removed', good[:r] + good[r + 2:], False), ('RSTn renumbered', good[:r + 1] + b'\xd7' + good[r + 2:], False),
                        ('a byte in front of RSTn', good[:r] + b'\x00' + good[r:], False),
                        ('fill bytes in front of RSTn and EOI', good[:r] + b'\xff\xff\xff' + good[r:-2] + b'\xff\xff\xd9', True)):
        info = jpeg.parse(d)
        assert info is not None, name
        if ok:
            assert np.array_equal(jpeg.entropy_decode(d, info), jpeg.entropy_decode(good, jpeg.parse(good))), name
        else:
            with pytest.raises(ValueError):
                jpeg.entropy_decode(d, info)


def _encoder_files():
    """Pillow's encoder at quality 1, 5, 50, 95 and 100 on uniform noise, two-level noise, a one-pixel checkerboard and a smooth
    image, every sampling mode, `optimize` on and off."""
    rng = np.random.default_rng(57)
    smooth = np.asarray(Image.fromarray(rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)).resize((72, 64), Image.BICUBIC))
    images = [('noise', rng.integers(0, 256, (64, 72, 3), dtype=np.uint8)), ('two_level', (rng.integers(0, 2, (64, 72, 3)) * 255).astype(np.uint8)),
              ('checker', np.repeat((np.add.outer(np.arange(64), np.arange(72)) % 2 * 255).astype(np.uint8)[..., None], 3, 2)), ('smooth', smooth)]
    for q in (1, 5, 50, 95, 100):
        for kind, a in images:
            for sub in (0, 1, 2):
                for opt in (False, True):
                    f = io.BytesIO()
                    Image.fromarray(a).save(f, 'JPEG', quality=q, subsampling=sub, optimize=opt)
                    yield (q, kind, sub, opt), f.getvalue()


def test_coefficient_range_condition_a_encoder_files_are_accepted():
    """Condition (a) of DESIGN.md section 12: no block an encoder makes from 8-bit samples, at any quantiser 1..255, leaves the
    accepted range.  (The size sweep's 2304 files are the other half of this check.)"""
    bad = [(case, o) for case, o in ((case, _refused_or_equal(data)) for case, data in _encoder_files()) if o != 'equal']
    assert not bad, bad


@pytest.mark.parametrize('kind', ['aligned', 'random'])
def test_coefficient_range_condition_b_pillow_agrees_up_to_the_bound(kind):
    """Condition (b): AT the bound and just inside it, restatement == Pillow (whose libjpeg-turbo keeps the IDCT's first-pass
    outputs in 16 bits) -- aligned-sign worst cases for each of the 64 output positions, and 2000 random blocks.  One step
    outside, the product refuses the file."""
    import jpeg_stream_ref as sr
    for offset in (0, -1):
        blocks = sr.bound_blocks(kind, offset)
        assert sr.in_range(blocks * np.array(sr.BOUND_QT[0])).all()
        data, _planes = sr.blocks_file(blocks)
        assert _refused_or_equal(data) == 'equal', offset
    outside = sr.bound_blocks(kind, 1)
    assert not sr.in_range(outside * np.array(sr.BOUND_QT[0])).any()
    for blk in outside[::97]:                                 # every block of that file is outside: one per file, a few of them
        assert _refused_or_equal(sr.blocks_file(blk[None])[0]) == 'refused'


def _outcome(fn):
    try:
        return 'returned', fn()
    except Exception as e:                                   # noqa: BLE001 -- the exception's type IS the outcome compared
        return 'raised', type(e)


def truncated_file(rng, h, w):
    """A baseline file cut in the middle of its scan: Pillow raises OSError('image file is truncated')."""
    good = _jpeg(rng, h, w, 2, 90)
    bad = good[:good.find(b'\xff\xda') + (len(good) - good.find(b'\xff\xda')) // 2]
    with pytest.raises(OSError):
        _pillow(bad)
    return good, bad


def test_training_feeder_treats_a_truncated_file_as_pillow_does(tmp_path):
    """A truncated file in a BatchFeeder batch: the same outcome with hps.device_jpeg on and off -- the reference's reader raises,
    so both raise; the device path used to train on rows the bit reader invented."""
    import pandas as pd
    from face_vijnana_yolov3_amd import data
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder
    good, bad = truncated_file(np.random.default_rng(58), 96, 128)
    open(tmp_path / 'a.jpg', 'wb').write(good)
    open(tmp_path / 'b.jpg', 'wb').write(bad)
    rows = [[0, 'a.jpg', 1, 10.0, 12.0, 30.0, 30.0], [1, 'b.jpg', 1, 20.0, 22.0, 25.0, 35.0]]
    pd.DataFrame(rows, columns=data.CSV_COLUMNS).to_csv(tmp_path / 'training.csv', index=False)
    outcomes = []
    for dj in (True, False):
        hps = dict(batch_size=2, step=1, lr=1e-4, beta_1=0.9, beta_2=0.99, decay=0.0, device_jpeg=dj)
        f = BatchFeeder(data.TrainingSequence(str(tmp_path), hps, {'image_size': 96, 'bb_info_c_size': 6}), 1, 0, threads=2)
        try:
            outcomes.append(_outcome(lambda: f.load(0)))
        finally:
            f.close()
    assert outcomes[0][0] == outcomes[1][0] == 'raised' and outcomes[0][1] is outcomes[1][1], outcomes
