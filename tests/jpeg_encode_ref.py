"""numpy restatement of the baseline JPEG encoder behind `PIL.Image.fromarray(rgb).save(f, 'JPEG')` (test aid): libjpeg-turbo with
its defaults -- quality 75, 4:2:0, the Annex K Huffman tables, no restart markers.  Front end and entropy coder, every stage integer:

    colour      jccolor.c rgb_ycc_convert, FIX(x) = int(x * 65536 + 0.5)
    edges       columns: the last real column replicated out to the MCU width; luma rows: the last real row replicated; chroma
                rows: the source padded to an even row count, downsampled, then the last DOWNSAMPLED row replicated
    downsample  jcsample.c h2v2_downsample: (a + b + c + d + bias) >> 2, bias 1 for even output columns and 2 for odd ones
    DCT         samples - 128, jfdctint.c jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2), rows first, output scaled by 8
    quantise    d = q << 3; sign(c) * ((|c| + (d >> 1)) // d)
    dummies     a luma block beyond ceil(w/8) x ceil(h/8): AC 0, DC of the block before it in the MCU (Y00 Y01 Y10 Y11)
    entropy     jchuff.c: MCUs row-major, blocks Y00 Y01 Y10 Y11 Cb Cr, last_dc per component from 0; DC code of nbits(|diff|) then
                the low bits of diff (diff - 1 when negative); AC in zigzag order, F0 per 16 zeros, (run << 4 | nbits) then the
                value bits, 00 when zeros trail; the last byte padded with 1-bits; 00 behind every FF

The tables (data of the JPEG standard) are the package's; tests/test_jpeg_encode_cpu.py pins them, and every function here,
against Pillow's own files."""
import numpy as np

from face_vijnana_yolov3_amd.jpeg import STD_AC, STD_DC, ZIGZAG, encode_header, quant_table

_ZZ = np.array(ZIGZAG)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    """uint8 [h][w][3] -> int64 Y, Cb, Cr planes."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode='edge')


def _downsample(plane, mx, my):
    h = plane.shape[0]
    p = _pad(plane, h + (h & 1), 16 * mx)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    s = (s + 1 + (np.arange(s.shape[1]) & 1)[None, :]) >> 2
    return _pad(s, 8 * my, 8 * mx)


def _fdct_1d(d, first):
    """one pass of jpeg_fdct_islow along the last axis."""
    F = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)
    sh = 13 - 2 if first else 13 + 2
    ds = lambda x, n: (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else ds(t10 - t11, 2)
    z1 = (t12 + t13) * F['c']
    o[2] = ds(z1 + t13 * F['d'], sh)
    o[6] = ds(z1 - t12 * F['h'], sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f']
    a4, a5, a6, a7 = t4 * F['a'], t5 * F['j'], t6 * F['l'], t7 * F['g']
    z1, z2, z3, z4 = -z1 * F['e'], -z2 * F['k'], -z3 * F['i'] + z5, -z4 * F['b'] + z5
    o[7], o[5], o[3], o[1] = ds(a4 + z1 + z3, sh), ds(a5 + z2 + z4, sh), ds(a6 + z2 + z3, sh), ds(a7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def _blocks(plane, q):
    """padded plane -> quantised [bh][bw][64], natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    x = _fdct_1d(x, True)                                             # rows
    x = np.swapaxes(_fdct_1d(np.swapaxes(x, -1, -2), False), -1, -2)  # columns
    d = (np.asarray(q, np.int64) << 3).reshape(8, 8)
    return (np.sign(x) * ((np.abs(x) + (d >> 1)) // d)).reshape(bh, bw, 64)


def coefficients(rgb):
    """-> [Y, Cb, Cr]: quantised coefficients [blocks_h][blocks_w][64] in natural order, the grids padded to whole MCUs, the dummy
    luma blocks as libjpeg makes them: what oracle.jpeg_oracle.entropy_decode returns for Pillow's file."""
    h, w = rgb.shape[:2]
    mx, my = -(-w // 16), -(-h // 16)
    y, cb, cr = ycc(rgb)
    Y = _blocks(_pad(y, 16 * my, 16 * mx), quant_table(0))
    wb, hb = -(-w // 8), -(-h // 8)
    m = Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64).copy()
    by = 2 * np.arange(my)[:, None, None] + np.array([0, 0, 1, 1])[None, None, :]
    bx = 2 * np.arange(mx)[None, :, None] + np.array([0, 1, 0, 1])[None, None, :]
    dummy = (by >= hb) | (bx >= wb)
    for k in (1, 2, 3):
        d = dummy[:, :, k]
        m[:, :, k][d] = 0
        m[:, :, k, 0][d] = m[:, :, k - 1, 0][d]
    Y = m.reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
    return [Y, _blocks(_downsample(cb, mx, my), quant_table(1)), _blocks(_downsample(cr, mx, my), quant_table(1))]


def _codes(spec):
    """(counts, symbols) -> {symbol: (code, length)} (jchuff.c jpeg_make_c_derived_tbl)."""
    counts, symbols = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1; k += 1
        code <<= 1
    return out


def _nbits(a):
    a = np.abs(a).astype(np.int64)
    n = np.zeros(a.shape, np.int64)
    for k in range(16):
        n += (a >> k) > 0
    return n


def scan_symbols(coefs):
    """[Y, Cb, Cr] of coefficients() -> (codes, lengths): every Huffman code with its value bits appended, in stream order."""
    Y, Cb, Cr = coefs
    my, mx = Cb.shape[:2]
    nat = np.concatenate([Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64), Cb[:, :, None], Cr[:, :, None]], 2)
    zz = nat.reshape(-1, 64)[:, _ZZ].astype(np.int64)                  # scan order, zigzag
    nb = zz.shape[0]
    comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), nb // 6)
    diff = zz[:, 0].copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        diff[idx] = np.diff(zz[idx, 0], prepend=0)
    tbl = (comp > 0).astype(np.int64)
    dc = [_codes(s) for s in STD_DC]
    ac = [_codes(s) for s in STD_AC]
    dc_code = np.array([[dc[t][s][0] for s in range(12)] for t in (0, 1)])
    dc_len = np.array([[dc[t][s][1] for s in range(12)] for t in (0, 1)])
    ac_code = np.zeros((2, 256), np.int64); ac_len = np.zeros((2, 256), np.int64)
    for t in (0, 1):
        for s, (c, l) in ac[t].items():
            ac_code[t, s], ac_len[t, s] = c, l

    def with_value(code, length, v):
        n = _nbits(v)
        bits = np.where(v < 0, v - 1, v) & ((1 << n) - 1)
        return (code << n) | bits, length + n

    keys, codes, lens = [], [], []
    n = _nbits(diff)
    c, l = with_value(dc_code[tbl, n], dc_len[tbl, n], diff)
    keys.append(np.arange(nb) * 65 * 4); codes.append(c); lens.append(l)
    b, p = np.nonzero(zz[:, 1:])
    p = p + 1
    prev = np.zeros(len(p), np.int64)                                  # the non-zero coefficient before, 0 (the DC) for a block's first
    prev[1:] = np.where(b[1:] != b[:-1], 0, p[:-1])
    run = p - prev - 1
    v = zz[b, p]
    n = _nbits(v)
    c, l = with_value(ac_code[tbl[b], ((run & 15) << 4) | n], ac_len[tbl[b], ((run & 15) << 4) | n], v)
    keys.append((b * 65 + p) * 4 + 3); codes.append(c); lens.append(l)
    for j in range(3):                                                 # up to three F0 (16 zeros each) in front of a coefficient
        sel = (run >> 4) > j
        keys.append((b[sel] * 65 + p[sel]) * 4 + j); codes.append(ac_code[tbl[b[sel]], 0xF0]); lens.append(ac_len[tbl[b[sel]], 0xF0])
    last = np.zeros(nb, np.int64)
    np.maximum.at(last, b, p)
    eob = np.nonzero(last < 63)[0]
    keys.append((eob * 65 + 64) * 4); codes.append(ac_code[tbl[eob], 0]); lens.append(ac_len[tbl[eob], 0])
    keys, codes, lens = np.concatenate(keys), np.concatenate(codes), np.concatenate(lens)
    order = np.argsort(keys, kind='stable')
    return codes[order], lens[order]


def pack_scan(codes, lens):
    """codes of lens bits each, most significant bit first -> the scan's bytes: 1-bits up to the byte boundary, 00 behind every FF."""
    width = 27                                                         # 16 bits of code + 11 of value at the most
    bits = ((codes[:, None] >> (width - 1 - np.arange(width))[None, :]) & 1).astype(np.uint8)
    keep = np.arange(width)[None, :] >= (width - lens)[:, None]
    stream = bits[keep]
    stream = np.concatenate([stream, np.ones(-len(stream) % 8, np.uint8)])
    raw = np.packbits(stream)
    out = np.zeros(len(raw) + int((raw == 0xFF).sum()), np.uint8)
    out[np.arange(len(raw)) + np.concatenate([[0], np.cumsum(raw == 0xFF)[:-1]])] = raw
    return out.tobytes()


def encode_scan(rgb):
    return pack_scan(*scan_symbols(coefficients(rgb)))


def encode(rgb):
    """uint8 [h][w][3] -> the whole file."""
    return encode_header(rgb.shape[0], rgb.shape[1]) + encode_scan(rgb) + b'\xff\xd9'


# ----------------------------------------------------------------------------- the inputs both encoder test files use
SMALL = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (24, 9), (40, 56), (3, 100), (100, 3), (101, 77)]     # rows, columns


def input_set():
    """[(name, uint8 [h][w][3])]: uniform noise at the small sizes, 250 x 190 and 416 x 416; a constant image (every block DC +
    EOB); 16 x 16 tiles alternating 0 and 255 (the largest DC differences); a smooth 1080 x 1920 gradient; a grey image whose
    every 8 x 8 block is 128 + 100 cos((2x+1) 7 pi / 16) cos((2y+1) 7 pi / 16) (only the last zigzag coefficient survives)."""
    rng = np.random.default_rng(2024)
    out = [('noise_%dx%d' % hw, rng.integers(0, 256, hw + (3,), dtype=np.uint8)) for hw in SMALL + [(250, 190), (416, 416)]]
    out.append(('constant_40x56', np.full((40, 56, 3), (200, 30, 90), np.uint8)))
    yy, xx = np.mgrid[0:64, 0:96]
    out.append(('tiles_64x96', np.repeat(((((yy >> 4) + (xx >> 4)) & 1) * 255).astype(np.uint8)[..., None], 3, 2)))
    yy, xx = np.mgrid[0:1080, 0:1920]
    out.append(('gradient_1080x1920', np.stack([xx * 255 // 1919, yy * 255 // 1079, (xx + yy) * 255 // 2998], -1).astype(np.uint8)))
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    out.append(('cosine_32x48', np.repeat(np.tile(np.rint(128 + 100 * np.outer(c, c)), (4, 6)).astype(np.uint8)[..., None], 3, 2)))
    return out
