"""JPEG input without a host-side image: Huffman decoding on host threads, everything after it on the device
(csrc/jpeg.hip; replaces `imread` of the reference's loaders, face_detection.py:112, 656, 798, for baseline JPEGs).

    info = parse(data)                       # None: not a file this decoder takes -> the caller uses Pillow for it
    entropy_decode(data, info, out_int16)    # quantised coefficients into a (pinned) host buffer; releases the GIL
    rgb = reconstruct_batch(ctx, ...)        # dequantise + IDCT + chroma upsampling + YCbCr->RGB for a whole batch

For every stream that parse() and entropy_decode() ACCEPT, the pixels are bit-identical to Pillow's; whatever cannot be held to
that is refused -- parse() returns None, entropy_decode() raises ValueError -- and the caller decodes the file with Pillow, which
then decides (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py; DESIGN.md section 12 lists what is refused and why).

JPEG output without a host-side image either (csrc/jpeg_enc.hip):

    files = encode_batch(ctx, packed, offsets, hw, device)   # whole files, byte-identical to Image.fromarray(rgb).save(f)

for packed RGB images that already lie on the device; only the compressed bytes cross to the host."""
import ctypes
import functools

import numpy as np

from ._lib import lib, ptr


class JpegInfo(ctypes.Structure):
    """fv_jpeg_info of include/fv_hotpath.h."""
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('ncomp', ctypes.c_int32), ('hmax', ctypes.c_int32),
                ('vmax', ctypes.c_int32), ('restart_interval', ctypes.c_int32),
                ('h', ctypes.c_int32 * 3), ('v', ctypes.c_int32 * 3), ('blocks_w', ctypes.c_int32 * 3), ('blocks_h', ctypes.c_int32 * 3),
                ('coef_off', ctypes.c_int64 * 3), ('total_coefs', ctypes.c_int64), ('qt', (ctypes.c_uint16 * 64) * 3)]


class JpegDesc(ctypes.Structure):
    """fv_jpeg_desc of include/fv_hotpath.h."""
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('ncomp', ctypes.c_int32), ('hmax', ctypes.c_int32),
                ('vmax', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('blocks_w', ctypes.c_int32 * 3), ('blocks_h', ctypes.c_int32 * 3),
                ('coef_off', ctypes.c_int64 * 3), ('plane_off', ctypes.c_int64 * 3), ('rgb_off', ctypes.c_int64),
                ('qt', (ctypes.c_uint16 * 64) * 3)]


assert ctypes.sizeof(JpegInfo) == 488 and ctypes.sizeof(JpegDesc) == 488


def _fn():
    L = lib()
    if not getattr(L, '_jpeg_declared', False):
        L.fv_jpeg_parse.restype = ctypes.c_int
        L.fv_jpeg_parse.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(JpegInfo)]
        L.fv_jpeg_entropy_decode.restype = ctypes.c_int
        L.fv_jpeg_entropy_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64]
        L.fv_jpeg_plane_bytes.restype = ctypes.c_int64
        L.fv_jpeg_plane_bytes.argtypes = [ctypes.POINTER(JpegInfo)]
        L.fv_jpeg_reconstruct_batch.restype = ctypes.c_int
        L.fv_jpeg_reconstruct_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        L.fv_jpeg_encode_workspace_bytes.restype = ctypes.c_int64
        L.fv_jpeg_encode_workspace_bytes.argtypes = [i32p, ctypes.c_int]
        L.fv_jpeg_encode_coefs.restype = ctypes.c_int
        L.fv_jpeg_encode_coefs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, i64p, i32p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_size_t, i64p]
        L.fv_jpeg_encode_measure.restype = ctypes.c_int
        L.fv_jpeg_encode_measure.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, i64p, i32p, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]
        L.fv_jpeg_encode_emit.restype = ctypes.c_int
        L.fv_jpeg_encode_emit.argtypes = [ctypes.c_void_p, i32p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, i64p, ctypes.c_void_p,
                                          ctypes.c_int64]
        L._jpeg_declared = True
    return L


# Pillow refuses images of more than 2 x Image.MAX_IMAGE_PIXELS pixels; a header claiming more is damaged or hostile, and the
# coefficient buffer for it would be page-locked before anything could notice
MAX_PIXELS = 178956970


def parse(data):
    """JPEG bytes -> JpegInfo, or None when the file is not one this decoder takes (progressive, arithmetic-coded, CMYK, 12-bit,
    unusual sampling, three components that libjpeg would not take for YCbCr, damaged header)."""
    info = JpegInfo()
    data = data if isinstance(data, bytes) else bytes(data)
    rc = _fn().fv_jpeg_parse(ctypes.c_char_p(data), len(data), ctypes.byref(info))
    if rc != 0 or info.width * info.height > MAX_PIXELS:
        return None          # implausible size (damaged header): left to Pillow, whose decompression-bomb check raises
    return info


def entropy_decode(data, info, out=None):
    """Huffman-decode the scan into `out` (int16 numpy array / memory of at least info.total_coefs elements; allocated when
    None).  ctypes releases the GIL for the duration of the call: a thread pool decodes in parallel.  -> the int16 array.
    ValueError for a scan the decoder does not take: a bad code, a scan that is cut or lacks its EOI, an RSTn that is missing,
    misplaced or misnumbered, a block outside the coefficient range in which libjpeg's inverse DCTs agree."""
    n = int(info.total_coefs)
    if out is None:
        out = np.empty(n, np.int16)
    assert out.dtype == np.int16 and out.size >= n and out.flags['C_CONTIGUOUS']
    data = data if isinstance(data, bytes) else bytes(data)
    rc = _fn().fv_jpeg_entropy_decode(ctypes.c_char_p(data), len(data), ctypes.c_void_p(out.ctypes.data), out.size)
    if rc != 0:
        raise ValueError('fv_jpeg_entropy_decode failed (%d): damaged, incomplete or out-of-range scan data' % rc)
    return out


def blocks_of(info, coefs):
    """(test aid) the flat coefficient array -> one [blocks_h][blocks_w][64] view per component."""
    return [np.asarray(coefs[int(info.coef_off[c]):int(info.coef_off[c]) + info.blocks_w[c] * info.blocks_h[c] * 64]).reshape(
        info.blocks_h[c], info.blocks_w[c], 64) for c in range(info.ncomp)]


class BatchPlan(object):
    """Host-side layout of one batch: where each image's coefficients, component planes and RGB pixels live."""

    def __init__(self, infos):
        self.infos = infos
        self.n = len(infos)
        self.descs = (JpegDesc * self.n)()
        coef = plane = rgb = 0
        self.coef_off, self.rgb_off, self.hw = [], [], []
        self.max_blocks = self.max_pixels = 1
        for i, I in enumerate(infos):
            d = self.descs[i]
            d.width, d.height, d.ncomp, d.hmax, d.vmax = I.width, I.height, I.ncomp, I.hmax, I.vmax
            nb = 0
            for c in range(I.ncomp):
                d.blocks_w[c], d.blocks_h[c] = I.blocks_w[c], I.blocks_h[c]
                d.coef_off[c] = coef + I.coef_off[c]
                d.plane_off[c] = plane
                plane += I.blocks_w[c] * I.blocks_h[c] * 64
                nb += I.blocks_w[c] * I.blocks_h[c]
                for k in range(64):
                    d.qt[c][k] = I.qt[c][k]
            plane = (plane + 15) & ~15
            d.rgb_off = rgb
            self.coef_off.append(coef); self.rgb_off.append(rgb); self.hw += [I.height, I.width]
            coef += int(I.total_coefs)
            rgb += I.height * I.width * 3
            self.max_blocks = max(self.max_blocks, nb); self.max_pixels = max(self.max_pixels, I.height * I.width)
        self.total_coefs, self.plane_bytes, self.rgb_bytes = coef, plane, rgb


def reconstruct_batch(ctx, plan, coefs_dev, device, rgb=None):
    """coefficients of the batch (int16 CUDA tensor laid out by `plan`) -> packed RGB uint8 CUDA tensor (image i at
    plan.rgb_off[i], hw plan.hw[2i:2i+2]): what fv_letterbox_batch takes as `packed`.  rgb: a flat uint8 CUDA tensor to write
    into instead of a new one -- image i then lands at plan.descs[i].rgb_off, which the caller has set (crop_store.CropStore)."""
    import torch
    descs = torch.frombuffer(bytearray(bytes(plan.descs)), dtype=torch.uint8).to(device, non_blocking=True)
    planes = torch.empty(max(plan.plane_bytes, 16), dtype=torch.uint8, device=device)
    if rgb is None:
        rgb = torch.empty(max(plan.rgb_bytes, 16), dtype=torch.uint8, device=device)
    rc = _fn().fv_jpeg_reconstruct_batch(ctx.handle, ptr(coefs_dev), ptr(descs), plan.n, ptr(planes), ptr(rgb), plan.max_blocks, plan.max_pixels)
    ctx.check(rc, 'fv_jpeg_reconstruct_batch')
    return rgb


# ----------------------------------------------------------------------------- encode (csrc/jpeg_enc.hip)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K of the JPEG standard: quantisation tables (natural order), Huffman code counts per length and symbols; [0] luma, [1] chroma
STD_QUANT = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
              100, 103, 99),
             (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66) + (99,) * 38)
STD_DC = (((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
          ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))))
STD_AC = (((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), tuple(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748'
    '494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3'
    'c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'))),
          ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), tuple(bytes.fromhex(
    '0001020311040521310612415107617113223281081442'
    '91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a73747576'
    '7778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6'
    'e7e8e9eaf2f3f4f5f6f7f8f9fa'))))
ENCODE_MAX_SIDE = 65535          # a JPEG's size fields are 16 bits


def quant_table(c, quality=75):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline): Annex K table c at `quality`, natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(min(max((q * scale + 50) // 100, 1), 255) for q in STD_QUANT[c])


def can_encode(h, w):
    """The sizes fv_jpeg_encode_* takes; the callers hand any other image to Pillow."""
    return 1 <= int(h) <= ENCODE_MAX_SIDE and 1 <= int(w) <= ENCODE_MAX_SIDE


@functools.lru_cache(maxsize=256)
def encode_header(h, w):
    """Everything `Image.fromarray(rgb).save(f, 'JPEG')` writes in front of the scan of an h x w RGB image: SOI, APP0 (JFIF 1.01),
    two DQT, SOF0 (4:2:0), four DHT (DC0, AC0, DC1, AC1), SOS."""
    if not can_encode(h, w):
        raise ValueError('a JPEG holds 1..65535 rows and columns, not %r x %r' % (h, w))

    def seg(marker, body):
        return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, 'big') + body
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for c in (0, 1):
        q = quant_table(c)
        out += seg(0xDB, bytes((c,)) + bytes(q[k] for k in ZIGZAG))
    out += seg(0xC0, b'\x08' + int(h).to_bytes(2, 'big') + int(w).to_bytes(2, 'big') + b'\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01')
    for c in (0, 1):
        out += seg(0xC4, bytes((c,)) + bytes(STD_DC[c][0]) + bytes(STD_DC[c][1]))
        out += seg(0xC4, bytes((0x10 | c,)) + bytes(STD_AC[c][0]) + bytes(STD_AC[c][1]))
    return out + seg(0xDA, b'\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00')


def _encode_args(packed, offsets, hw):
    import torch
    n = len(offsets)
    if len(hw) != 2 * n:
        raise ValueError('hw holds (rows, columns) per image: %d values for %d images' % (len(hw), n))
    if packed.dtype != torch.uint8 or not packed.is_cuda:
        raise ValueError('the encoder takes a uint8 CUDA buffer')
    return n, (ctypes.c_int64 * max(1, n))(*[int(o) for o in offsets]), (ctypes.c_int32 * max(2, 2 * n))(*[int(v) for v in hw])


def encode_workspace(hw, device):
    """uint8 CUDA tensor of fv_jpeg_encode_workspace_bytes(hw) bytes."""
    import torch
    n = len(hw) // 2
    need = _fn().fv_jpeg_encode_workspace_bytes((ctypes.c_int32 * max(2, 2 * n))(*[int(v) for v in hw]), n)
    if need < 0:
        raise ValueError('the encoder takes images of 1..65535 rows and columns')
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def encode_batch(ctx, packed, offsets, hw, device, pinned=None):
    """The packed RGB images (device uint8 buffer, byte offsets, [rows, columns] per image -- what reconstruct_batch,
    fv_crop_nearest_u8 and fv_draw_prims_u8 work on) -> one `bytes` per image: the whole JPEG file, byte-identical to
    `Image.fromarray(rgb).save(f, 'JPEG')` of Pillow on libjpeg-turbo.  fv_jpeg_encode_measure, one synchronising copy of the n
    scan lengths, fv_jpeg_encode_emit into a buffer of exactly that size, ONE device-to-host copy of the scans into pinned memory;
    header (cached per size) and EOI are added on the host.  pinned: callable(nbytes) -> pinned uint8 tensor to receive the copy
    (the callers' double-buffered slots); None: a fresh pinned buffer."""
    import torch
    L = _fn()
    n, offs, sizes = _encode_args(packed, offsets, hw)
    if n == 0:
        return []
    ws = encode_workspace(hw, device)
    counts_dev = torch.empty(n, dtype=torch.int64, device=device)
    rc = L.fv_jpeg_encode_measure(ctx.handle, ptr(packed), packed.numel(), offs, sizes, n, ptr(ws), ws.numel(), ptr(counts_dev))
    ctx.check(rc, 'fv_jpeg_encode_measure')
    counts = [int(c) for c in counts_dev.cpu().tolist()]            # the one synchronising copy: n numbers
    total = sum(counts)
    out = torch.empty(total, dtype=torch.uint8, device=device)
    rc = L.fv_jpeg_encode_emit(ctx.handle, sizes, n, ptr(ws), ws.numel(), (ctypes.c_int64 * n)(*counts), ptr(out), total)
    ctx.check(rc, 'fv_jpeg_encode_emit')
    host = (pinned(total) if pinned is not None else torch.empty(total, dtype=torch.uint8).pin_memory())[:total]
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    view = memoryview(host.numpy())
    files, at = [], 0
    for i, c in enumerate(counts):
        files.append(b''.join((encode_header(int(hw[2 * i]), int(hw[2 * i + 1])), view[at:at + c], b'\xff\xd9')))
        at += c
    return files


def encode_coefs(ctx, packed, offsets, hw, device):
    """(test aid) the encoder's front end alone -> per image, one int16 [blocks_h][blocks_w][64] array per component in NATURAL
    order, the block grid padded to whole MCUs: what oracle.jpeg_oracle.entropy_decode returns for the file."""
    L = _fn()
    n, offs, sizes = _encode_args(packed, offsets, hw)
    if n == 0:
        return []
    ws = encode_workspace(hw, device)
    where = ctypes.c_int64(0)
    rc = L.fv_jpeg_encode_coefs(ctx.handle, ptr(packed), packed.numel(), offs, sizes, n, ptr(ws), ws.numel(), ctypes.byref(where))
    ctx.check(rc, 'fv_jpeg_encode_coefs')
    nblk = [6 * ((int(hw[2 * i + 1]) + 15) // 16) * ((int(hw[2 * i]) + 15) // 16) for i in range(n)]
    flat = ws[where.value:where.value + 128 * sum(nblk)].cpu().numpy().view(np.int16).reshape(-1, 64)
    out, at = [], 0
    for i in range(n):
        out.append(mcu_blocks_to_planes(flat[at:at + nblk[i]], int(hw[2 * i]), int(hw[2 * i + 1])))
        at += nblk[i]
    return out


def mcu_blocks_to_planes(blocks, h, w):
    """[6 * MCUs][64] zigzag-ordered blocks in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU) -> [Y, Cb, Cr] as
    [blocks_h][blocks_w][64] in natural order."""
    mx, my = (w + 15) // 16, (h + 15) // 16
    nat = np.empty_like(blocks)
    nat[:, list(ZIGZAG)] = blocks
    m = nat.reshape(my, mx, 6, 64)
    y = m[:, :, :4].reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
    return [y, m[:, :, 4].copy(), m[:, :, 5].copy()]
