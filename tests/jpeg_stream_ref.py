"""A baseline JPEG stream WRITER for tests: quantised coefficient arrays -> whole files, over the range of streams that
fv_jpeg_parse / fv_jpeg_entropy_decode accept and Pillow's own encoder never writes (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py).
Built on tests/jpeg_encode_ref.py (`_codes`, `pack_scan`; its `scan_symbols` is the 4:2:0 / Annex K special case and pins this
file's symbol order in test_writer_equals_the_encoder_restatement).

    write(planes, height, width, fmt, qts, **options) -> bytes

    planes   per component an int array [blocks_h][blocks_w][64], NATURAL order, the block grid padded to whole MCUs (grid())
    fmt      'gray' | '444' | '422' | '420'
    qts      [luma] or [luma, chroma]: 64 quantiser values each, natural order
    options  huff      'std' (Annex K), 'opt' (built from the symbol statistics of the data, Annex K.2 as jchuff.c
                       jpeg_gen_optimal_table does it), 'long' (every code 10..16 bits long, DC and AC)
             ri        restart interval in MCUs (0: none)
             ids       the component ids of SOF / SOS
             jfif      a JFIF APP0 in front;  adobe: None or the transform byte of an Adobe APP14
             sof       0xC0 | 0xC1
             dqt_combined / dht_combined   all tables of a kind in ONE segment instead of one segment each
             redefine  a wrong DQT and a wrong DHT first, both defined again (correctly) before SOS
             big       [(marker, payload bytes)]: COM / APPn segments of any size in front of the tables
             fill      FF FF in front of every marker and in front of every RSTn
             gray_sampling  the sampling-factor byte of a grey file's SOF (0x22: still one block per MCU)
             sos_tail  the three bytes Ss, Se, Ah/Al (sequential decoders ignore them)
             zrl_tail  trailing zeros that fill whole groups of 16 are coded as ZRLs up to coefficient 63, without EOB

Checked against two readers on the CPU: Pillow decodes every file, and oracle.jpeg_oracle.entropy_decode returns the coefficients
that were put in."""
import functools

import numpy as np

from face_vijnana_yolov3_amd.jpeg import STD_AC, STD_DC, ZIGZAG
from jpeg_encode_ref import _codes, pack_scan

_ZZ = np.array(ZIGZAG)
SAMPLING = {'gray': [(1, 1)], '444': [(1, 1)] * 3, '422': [(2, 1), (1, 1), (1, 1)], '420': [(2, 2), (1, 1), (1, 1)]}


def grid(height, width, fmt):
    """-> [(blocks_h, blocks_w)] per component."""
    hv = SAMPLING[fmt]
    hmax, vmax = hv[0]
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * v, mx * h) for h, v in hv]


def _nbits(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, n):
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


def block_symbols(zz, diff, zrl_tail=False):
    """One block in zigzag order -> [(class, symbol, value bits, number of value bits)], class 0 = DC, 1 = AC."""
    n = _nbits(diff)
    out = [(0, n, _value_bits(diff, n), n)]
    nz = np.nonzero(zz[1:])[0] + 1
    prev = 0
    for k in nz:
        run = int(k) - prev - 1
        out += [(1, 0xF0, 0, 0)] * (run >> 4)
        v = int(zz[k])
        n = _nbits(v)
        out.append((1, ((run & 15) << 4) | n, _value_bits(v, n), n))
        prev = int(k)
    if prev < 63:
        if zrl_tail and (63 - prev) % 16 == 0:
            out += [(1, 0xF0, 0, 0)] * ((63 - prev) // 16)
        else:
            out.append((1, 0, 0, 0))
    return out


def scan_intervals(planes, fmt, ri=0, zrl_tail=False):
    """-> one list per restart interval of (class, table, symbol, value bits, number of value bits), in stream order."""
    hv = SAMPLING[fmt]
    hmax, vmax = hv[0]
    my, mx = planes[0].shape[0] // vmax, planes[0].shape[1] // hmax
    pred = [0] * len(hv)
    out, cur = [], []
    for m in range(mx * my):
        if ri and m and m % ri == 0:
            out.append(cur)
            cur, pred = [], [0] * len(hv)
        y, x = divmod(m, mx)
        for c, (h, v) in enumerate(hv):
            for by in range(v):
                for bx in range(h):
                    zz = np.asarray(planes[c][y * v + by, x * h + bx])[_ZZ]
                    dc = int(zz[0])
                    cur += [(k, min(c, 1), s, b, n) for k, s, b, n in block_symbols(zz, dc - pred[c], zrl_tail)]
                    pred[c] = dc
    out.append(cur)
    return out


def optimal_table(freq):
    """{symbol: count} -> (counts per length 1..16, symbols): Annex K.2 with the all-ones code reserved, code lengths limited to 16
    (jchuff.c jpeg_gen_optimal_table)."""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    f[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]; f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * 40
    for s in size:
        if s:
            bits[s] += 1
    for i in range(39, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    symbols = [s for n in range(1, 40) for s in range(256) if size[s] == n]
    return tuple(bits[1:17]), tuple(symbols)


def long_table(symbols):
    """Every code 10..16 bits long: 1, 2, 4, ... symbols at lengths 10, 11, 12, ... and the rest at 16."""
    symbols = list(symbols)
    counts, left = [0] * 16, len(symbols)
    for length in range(10, 16):
        counts[length - 1] = min(left, 1 << (length - 10))
        left -= counts[length - 1]
    counts[15] = left
    return tuple(counts), tuple(symbols)


def _seg(marker, body, fill=False):
    return (b'\xff' if fill else b'') + bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)


def write(planes, height, width, fmt, qts, huff='std', ri=0, ids=(1, 2, 3), jfif=True, adobe=None, sof=0xC0, dqt_combined=False,
          dht_combined=False, redefine=False, big=(), fill=False, gray_sampling=0x11, sos_tail=(0, 63, 0), zrl_tail=False, eoi=True):
    hv = SAMPLING[fmt]
    nc = len(hv)
    assert [tuple(p.shape) for p in planes] == [g + (64,) for g in grid(height, width, fmt)]
    intervals = scan_intervals(planes, fmt, ri, zrl_tail)
    ntab = 1 if nc == 1 else 2
    # ---- Huffman tables: [class][table] -> (counts, symbols)
    if huff == 'std':
        specs = [[STD_DC[t] for t in range(ntab)], [STD_AC[t] for t in range(ntab)]]
    else:
        freq = [[{} for _ in range(ntab)] for _ in (0, 1)]
        for iv in intervals:
            for k, t, s, _b, _n in iv:
                freq[k][t][s] = freq[k][t].get(s, 0) + 1
        make = optimal_table if huff == 'opt' else (lambda fr: long_table(sorted(fr)))
        specs = [[make(freq[k][t]) for t in range(ntab)] for k in (0, 1)]
    codes = [[_codes(specs[k][t]) for t in range(ntab)] for k in (0, 1)]
    # ---- the scan: code and value bits as separate entries (16 + 15 bits would not fit pack_scan's 27)
    scan = b''
    for i, iv in enumerate(intervals):
        cs, ls = [], []
        for k, t, s, b, n in iv:
            c, l = codes[k][t][s]
            cs.append(c); ls.append(l)
            if n:
                cs.append(b); ls.append(n)
        if i:
            scan += (b'\xff' if fill else b'') + bytes((0xFF, 0xD0 + (i - 1) % 8))
        scan += pack_scan(np.array(cs, np.int64), np.array(ls, np.int64))
    # ---- the headers
    out = b'\xff\xd8'
    if jfif:
        out += _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00', fill)
    if adobe is not None:
        out += _seg(0xEE, b'Adobe\x00\x64\x00\x00\x00\x00' + bytes((adobe,)), fill)
    for marker, payload in big:
        out += _seg(marker, payload, fill)
    dqt = [bytes((t,)) + bytes(int(qts[t][k]) for k in ZIGZAG) for t in range(len(qts))]
    dht = [bytes((k << 4 | t,)) + bytes(specs[k][t][0]) + bytes(specs[k][t][1]) for t in range(ntab) for k in (0, 1)]
    if redefine:
        out += _seg(0xDB, bytes((0,)) + bytes([77] * 64), fill)
        out += _seg(0xC4, bytes((0x10,)) + bytes(STD_AC[1][0]) + bytes(STD_AC[1][1]), fill)
    out += _seg(0xDB, b''.join(dqt), fill) if dqt_combined else b''.join(_seg(0xDB, d, fill) for d in dqt)
    samp = [gray_sampling] if nc == 1 else [h << 4 | v for h, v in hv]
    out += _seg(sof, b'\x08' + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + bytes((nc,)) +
                b''.join(bytes((ids[c], samp[c], min(c, len(qts) - 1, 1))) for c in range(nc)), fill)
    out += _seg(0xC4, b''.join(dht), fill) if dht_combined else b''.join(_seg(0xC4, d, fill) for d in dht)
    if ri:
        out += _seg(0xDD, ri.to_bytes(2, 'big'), fill)
    out += _seg(0xDA, bytes((nc,)) + b''.join(bytes((ids[c], 0x11 * min(c, 1))) for c in range(nc)) + bytes(sos_tail), fill)
    return out + scan + ((b'\xff' if fill else b'') + b'\xff\xd9' if eoi else b'')


# ----------------------------------------------------------------------------- coefficient content
def natural_planes(rng, height, width, fmt, qts):
    """Photo-like content: DC anywhere in the 8-bit range, sparse AC that falls off with frequency -- quantised by qts."""
    out = []
    for c, (bh, bw) in enumerate(grid(height, width, fmt)):
        q = np.asarray(qts[min(c, len(qts) - 1)], np.float64)
        d = rng.laplace(0, 1, (bh, bw, 64)) * (90.0 / (1 + np.arange(64) // 8 + np.arange(64) % 8)) * (rng.random((bh, bw, 64)) < 0.4)
        d[..., 0] = rng.uniform(-900, 900, (bh, bw))
        out.append(np.rint(d / q).astype(np.int64))
    return out


# the range of dequantised blocks the product accepts, restated from DESIGN.md section 12: with W_k = 1 (k = 0, 4), 1.38704 (k odd),
# 1.30656 (k = 2, 6) in units of 1/1024 rounded up and U_c = sum_k W_k |d[k][c]|, the two largest U_c add up to at most 8190
RANGE_W = np.array([1024, 1421, 1338, 1421, 1024, 1421, 1338, 1421], np.int64)
RANGE_B = 8190


def in_range(d):
    """d: dequantised coefficients [..., 64] natural order -> bool [...]."""
    u = (np.abs(np.asarray(d, np.int64)).reshape(np.shape(d)[:-1] + (8, 8)) * RANGE_W[:, None]).sum(-2)
    u = np.sort(u, -1)
    return u[..., -1] + u[..., -2] <= RANGE_B * 1024


def aligned_signs(y, x):
    """[64] of +-1: the signs that make every term of the inverse DCT at output row y, column x positive."""
    k = np.arange(8)
    a = np.where(np.cos((2 * y + 1) * k * np.pi / 16) >= 0, 1, -1)
    b = np.where(np.cos((2 * x + 1) * k * np.pi / 16) >= 0, 1, -1)
    return np.outer(a, b).reshape(64)


def scale_to_range(shape, offset=0):
    """blk(s) = rint(s * shape / 1000) for the real-valued pattern `shape` [64], its DC rounded to a multiple of 8 (BOUND_QT: a DC
    of +-1024 x 8 stays within difference category 11) -> blk(s + offset) for the largest s with in_range(blk(s)).  offset 0: AT
    the bound; -1: just inside; a large one: outside."""
    lo, hi = 0, 1 << 40

    def blk(s):
        b = np.rint(s * np.asarray(shape, np.float64) / 1000.0).astype(np.int64)
        b[0] = 8 * int(np.rint(b[0] / 8.0))
        return b
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_range(blk(mid)) else (lo, mid)
    return blk(lo + offset)


# ----------------------------------------------------------------------------- the corpus both JPEG test files use
def _quant(quality):
    from face_vijnana_yolov3_amd.jpeg import quant_table
    return [quant_table(0, quality), quant_table(1, quality)]


ONES = [(1,) * 64]
BOUND_QT = [(8,) + (1,) * 63]


def bound_blocks(kind, offset=0):
    """Blocks [n][64], quantised by BOUND_QT, whose dequantised values sit AT the range bound (offset 0), just inside it (-1) or outside (large offset):
    'aligned': for each of the 64 output positions the aligned-sign pattern with equal magnitudes everywhere, the same confined
    to each pair of columns that libjpeg's 16-bit code adds (0,4), (1,5), (3,7), to one column, and to the first row;
    'random': 2000 blocks of random signs and magnitudes, a random subset of the coefficients."""
    out = []
    if kind == 'aligned':
        masks = [np.ones((8, 8))]
        for cols in ((0, 4), (1, 5), (3, 7), (2,), (7,)):
            m = np.zeros((8, 8)); m[:, list(cols)] = 1
            masks.append(m)
        m = np.zeros((8, 8)); m[0, :] = 1
        masks.append(m)
        for y in range(8):
            for x in range(8):
                for m in masks:
                    out.append(scale_to_range(aligned_signs(y, x) * m.reshape(64), offset))
    else:
        rng = np.random.default_rng(64)
        for _ in range(2000):
            shape = rng.uniform(0.05, 1, 64) * rng.choice([-1, 1], 64) * (rng.random(64) < rng.choice([0.1, 0.5, 1.0]))
            shape[int(rng.integers(0, 64))] = 1.0
            out.append(scale_to_range(shape, offset))
    out = np.array(out)
    out[:, 0] //= 8
    return out


def blocks_file(blocks, qt=BOUND_QT, huff='opt'):
    """[n][64] quantised blocks -> (grey file 8 blocks wide, planes)."""
    n = len(blocks)
    rows = -(-n // 8)
    pl = np.zeros((rows * 8, 64), np.int64)
    pl[:n] = blocks
    pl = [pl.reshape(rows, 8, 64)]
    return write(pl, rows * 8, 64, 'gray', qt, huff=huff), pl


@functools.lru_cache(maxsize=1)
def corpus():
    """-> [(name, file bytes, planes that were put in, expectation)], expectation True: the product must accept the file, False: it
    must refuse it, None: either -- and whatever it accepts must come out as Pillow's pixels."""
    rng = np.random.default_rng(12)
    q90, q50 = _quant(90), _quant(50)
    out = []

    def add(name, expect, planes, height, width, fmt, qts, **kw):
        qts = qts[:1] if fmt == 'gray' else qts
        out.append((name, write(planes, height, width, fmt, qts, **kw), planes, expect))

    def nat(height, width, fmt, qts):
        return natural_planes(rng, height, width, fmt, qts[:1] if fmt == 'gray' else qts)
    # formats x Huffman tables x restart intervals: 1, one that does not divide the MCU count (4), one that ends at the last MCU
    for fmt in ('gray', '444', '422', '420'):
        g = grid(19, 37, fmt)[-1]
        for huff in ('std', 'opt', 'long'):
            for ri in (0, 1, 4, g[0] * g[1] // 3):
                add('%s_%s_ri%d' % (fmt, huff, ri), True, nat(19, 37, fmt, q90), 19, 37, fmt, q90, huff=huff, ri=ri)
    # narrow images: the replicating upsamplers
    for fmt in ('422', '420'):
        for h, w in ((5, 1), (1, 3), (7, 4), (3, 5), (40, 3), (3, 40)):
            add('%s_%dx%d' % (fmt, h, w), True, nat(h, w, fmt, q50), h, w, fmt, q50)
    # component ids, JFIF, Adobe
    for ids in ((1, 2, 3), (0, 1, 2), (4, 5, 6), (82, 71, 66)):
        for jf in (True, False):
            for ad in (None, 1):
                rgb = ids[0] == 82 and not jf and ad is None
                add('ids%d_jfif%d_adobe%s' % (ids[0], jf, ad), False if rgb else True, nat(16, 24, '420', q90), 16, 24, '420', q90,
                    ids=ids, jfif=jf, adobe=ad)
    # header layout
    for name, fmt, kw in (('tables_combined', '420', dict(dqt_combined=True, dht_combined=True)),
                          ('tables_combined_opt', '444', dict(dqt_combined=True, dht_combined=True, huff='opt')),
                          ('table_redefined', '422', dict(redefine=True)), ('sof1', '420', dict(sof=0xC1)),
                          ('big_segments', '420', dict(big=((0xFE, b'c' * 65533), (0xE5, b'\xff\xd9' * 32766 + b'z'), (0xEF, b'')))),
                          ('fill_bytes', '420', dict(fill=True)), ('fill_bytes_rst', '422', dict(fill=True, ri=2, huff='opt')),
                          ('gray_2x2', 'gray', dict(gray_sampling=0x22)), ('gray_2x1_ri', 'gray', dict(gray_sampling=0x21, ri=2)),
                          ('sos_ss_se', '420', dict(sos_tail=(5, 40, 0x21))), ('sos_ss_se_gray', 'gray', dict(sos_tail=(1, 0, 0xFF)))):
        add(name, True, nat(24, 40, fmt, q90), 24, 40, fmt, q90, **kw)
    # coefficient content (grey, quantiser 1 unless said): DC differences of category 11, up and down
    dc = np.zeros((2, 8, 64), np.int64)
    dc[..., 0] = np.where(np.arange(16).reshape(2, 8) % 2 == 0, 1023, -1024)
    add('dc_category_11', True, [dc], 16, 64, 'gray', ONES)
    add('dc_category_11_opt_ri', True, [dc], 16, 64, 'gray', ONES, huff='long', ri=3)
    # a single coefficient of every AC size 1..15, largest and smallest magnitude of the size, both signs, at four positions
    for n in range(1, 16):
        blk = np.zeros((2, 8, 64), np.int64)
        vals = [(1 << n) - 1, -((1 << n) - 1), 1 << (n - 1), -(1 << (n - 1))]
        for i, pos in enumerate((1, 8, 36, 63)):
            for j, v in enumerate(vals):
                blk[i // 2, (i % 2) * 4 + j, pos] = v
        add('ac_size_%d' % n, True if n <= 10 else None, [blk], 16, 64, 'gray', ONES, huff='opt')
        if n <= 10:
            add('ac_size_%d_std' % n, True, [blk], 16, 64, 'gray', ONES)
    # the same magnitudes reached through the quantiser: coefficient 1..4 times 255
    blk = np.zeros((1, 8, 64), np.int64)
    for i in range(8):
        blk[0, i, (0, 1, 8, 9, 27, 62, 63, 7)[i]] = (4, -4, 3, -3, 2, -2, 1, -1)[i]
    add('single_times_255', True, [blk], 8, 64, 'gray', [(255,) * 64])
    # zero runs (_ZZ[k]: the natural index of zigzag position k): only coefficient 63; 15 and 63; the last coefficient at zigzag
    # 15, 31, 47, so that zrl_tail codes ZRL runs that END at coefficient 63 (no EOB); DC alone; runs of exactly 15 zeros
    zz = np.zeros((1, 8, 64), np.int64)
    zz[0, 0, _ZZ[63]] = 5
    zz[0, 1, _ZZ[15]] = -3; zz[0, 1, _ZZ[63]] = 2
    for i, last in enumerate((15, 31, 47)):
        zz[0, 2 + i, _ZZ[last]] = 7 - i
    zz[0, 5, 0] = 40
    zz[0, 6, _ZZ[1]] = 1; zz[0, 6, _ZZ[17]] = -1; zz[0, 6, _ZZ[33]] = 1; zz[0, 6, _ZZ[49]] = -1
    zz[0, 7, _ZZ[47]] = 9; zz[0, 7, 0] = -40
    zz = zz * 4
    for huff in ('std', 'opt', 'long'):
        add('zero_runs_%s' % huff, True, [zz], 8, 64, 'gray', q90, huff=huff)
        add('zrl_to_63_%s' % huff, True, [zz], 8, 64, 'gray', q90, huff=huff, zrl_tail=True)
    # the range bound: aligned-sign worst cases for all 64 output positions and random blocks, AT the bound
    for kind in ('aligned', 'random'):
        data, pl = blocks_file(bound_blocks(kind))
        out.append(('%s_at_bound' % kind, data, pl, True))
    return out
