"""Host side of the detect post-processing: device tensors in, device tensors / BoundBox out.

Mirrors the tail of FaceDetector.detect (reference face_detection.py:900-949) and the BoundBox
record (reference yolov3_detect.py:126-163)."""
import numpy as np

from ._lib import lib, packed_args, ptr


class BoundBox(object):
    """Mutable detection record; same attribute surface as the reference's BoundBox
    (yolov3_detect.py:126-163): callers mutate xmin..ymax in place (face_detection.py:700-710)."""

    def __init__(self, xmin, ymin, xmax, ymax, objness=None, classes=None, anchor=None, subject_id=-1):
        self.xmin = xmin
        self.ymin = ymin
        self.xmax = xmax
        self.ymax = ymax
        self.objness = objness
        self.classes = classes
        self.anchor = anchor
        self.subject_id = subject_id
        self.label = -1
        self.score = -1

    def get_label(self):
        if self.label == -1:
            self.label = int(np.argmax(self.classes))
        return self.label

    def get_score(self):
        if self.score == -1:
            self.score = self.classes[self.get_label()]
        return np.min([self.score, 1.0])

    def get_relative_bb(self, width, height):
        return (int(self.xmin / width * 100.), int(self.ymin / height * 100.),
                int((self.xmax - self.xmin) / width * 100.), int((self.ymax - self.ymin) / height * 100.))


def decode_nms_buffers(n, num_cands, device):
    """The five result tensors of decode_nms for n images, uninitialised."""
    import torch
    k = int(num_cands)
    return dict(boxes=torch.empty((n, k, 4), dtype=torch.int32, device=device),
                cell=torch.empty((n, k), dtype=torch.int32, device=device),
                obj=torch.empty((n, k), dtype=torch.float32, device=device),
                score=torch.empty((n, k), dtype=torch.float32, device=device),
                count=torch.empty((n,), dtype=torch.int32, device=device))


def decode_nms(ctx, head, image_size, conf_th, iou_th, num_cands, out=None):
    """head: (n, G, G, 6) float32 CUDA tensor -> dict of CUDA tensors
    boxes (n,K,4) i32, cell (n,K) i32, obj (n,K) f32, score (n,K) f32, count (n,) i32.  out: such a dict to write into (slices
    along the first axis of decode_nms_buffers' tensors: the tiled path collects several calls in one result)."""
    import torch
    assert head.is_cuda and head.dtype == torch.float32 and head.dim() == 4 and head.shape[3] == 6
    head = head.contiguous()
    n, g = head.shape[0], head.shape[1]
    k = int(num_cands)
    dev = head.device
    if out is None:
        out = decode_nms_buffers(n, k, dev)
    boxes, cell, obj, score, count = out['boxes'], out['cell'], out['obj'], out['score'], out['count']
    assert tuple(boxes.shape) == (n, k, 4) and tuple(score.shape) == (n, k) and tuple(count.shape) == (n,)
    rc = lib().fv_decode_nms(ctx.handle, ptr(head), n, g, int(image_size), float(conf_th), float(iou_th), k,
                             ptr(boxes), ptr(cell), ptr(obj), ptr(score), ptr(count))
    ctx.check(rc, 'fv_decode_nms')
    return dict(boxes=boxes, cell=cell, obj=obj, score=score, count=count)


def to_boundboxes(res, img=0):
    """Device result of decode_nms -> list[BoundBox] for one image, reference order (ascending
    score).  Coordinates are np.int64 and scores np.float32 as in the reference."""
    c = int(res['count'][img])
    b = res['boxes'][img, :c].cpu().numpy().astype(np.int64)
    o = res['obj'][img, :c].cpu().numpy()
    s = res['score'][img, :c].cpu().numpy()
    return [BoundBox(b[k, 0], b[k, 1], b[k, 2], b[k, 3], objness=o[k], classes=[s[k]]) for k in range(c)]


def letterbox_device(ctx, raw_u8, image_size, out=None):
    """uint8 HxWx3 (numpy or CUDA tensor) -> (float32 CUDA tensor (S,S,3), geometry tuple
    (h, w, pad_t, pad_b, pad_l, pad_r)) -- the device form of data.letterbox
    (reference face_detection.py:112-147)."""
    import ctypes
    import torch
    t = raw_u8 if torch.is_tensor(raw_u8) else torch.from_numpy(np.array(raw_u8, dtype=np.uint8, copy=True))
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
    t = t.cuda().contiguous()
    h, w = int(t.shape[0]), int(t.shape[1])
    S = int(image_size)
    if out is None:
        out = torch.empty((S, S, 3), dtype=torch.float32, device=t.device)
    geom = (ctypes.c_int32 * 6)()
    ctx.check(lib().fv_letterbox(ctx.handle, ptr(t), h, w, S, ptr(out), geom), 'fv_letterbox')
    return out, (h, w, geom[2], geom[3], geom[4], geom[5])


class PinnedRing(object):
    """A few pinned host buffers reused round-robin.  Page-locking a fresh 35-100 MB buffer costs 50-160 ms on this stack whenever
    torch's pinned-memory cache holds no block of that size (tools/eval_load_probe.py: batches differ in size, so every second or
    third batch missed) -- more than decoding the batch -- so the loaders write into these instead.  take() hands out the next
    buffer (grown with 25 % slack when too small) once the H2D copy that last read it has completed; the consumer calls
    copied(buffer) right after it enqueued that copy."""

    def __init__(self, n=3):
        self._pins = [None] * n
        self._events = [None] * n
        self._next = 0

    def take(self, nbytes):
        """-> uint8 pinned tensor of nbytes (a view of the slot's buffer)."""
        import torch
        i = self._next
        self._next = (i + 1) % len(self._pins)
        if self._events[i] is not None:
            self._events[i].synchronize()
            self._events[i] = None
        if self._pins[i] is None or self._pins[i].numel() < nbytes:
            self._pins[i] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
        return self._pins[i][:nbytes]

    def untake(self):
        """The buffer of the last take() will not be used after all: the next take() hands out the same slot again."""
        self._next = (self._next - 1) % len(self._pins)

    def copied(self, buf):
        """An event on the current stream guards the slot `buf` (any view of it) came from."""
        import torch
        p = buf.data_ptr()
        for i, b in enumerate(self._pins):
            if b is not None and b.data_ptr() <= p < b.data_ptr() + max(b.numel(), 1):
                ev = torch.cuda.Event()
                ev.record()
                self._events[i] = ev
                return


def pack_images(raws, pin=True, ring=None):
    """Host side of fv_letterbox_batch: the decoded uint8 images back to back in ONE (pinned) host
    buffer -> (uint8 tensor, offsets int64 list, hw list).  ring: a PinnedRing to take the buffer from."""
    import torch
    sizes = [int(r.shape[0]) * int(r.shape[1]) * 3 for r in raws]
    if ring is not None and pin and torch.cuda.is_available():
        buf = ring.take(sum(sizes))
    else:
        buf = torch.empty(sum(sizes), dtype=torch.uint8)
        if pin and torch.cuda.is_available():
            buf = buf.pin_memory()
    view = buf.numpy()
    offs, hw, o = [], [], 0
    for r, n in zip(raws, sizes):
        a = np.asarray(r, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 3
        view[o:o + n] = a.reshape(-1)
        offs.append(o); hw += [int(a.shape[0]), int(a.shape[1])]
        o += n
    return buf, offs, hw


def letterbox_batch_device(ctx, raws, image_size, device, out=None, packed=None, keep=None, aug=None, mosaic=None):
    """list of uint8 HxWx3 arrays -> ((n,S,S,3) float32 CUDA tensor, [geometry tuples]) in ONE launch
    (fv_letterbox_batch); `packed` = the result of pack_images when a loader thread prepared it.  keep: a list that receives
    (device uint8 buffer, offsets, hw) -- the batch's decoded images on the device, for a later fv_letterbox_crops.
    aug: (place, colour) -- n x 8 int placements and n x 3 float colour parameters (or None) as data.draw_augment draws them: the
    launch is then fv_letterbox_augment_batch (crop, placement, flip and colour distortion in the same single pass) and the second
    result is None (the placements ARE the geometry).
    mosaic: (tiles, colour, n_out) -- n_tiles x 14 int tile records, n_tiles x 3 float colour parameters (or None) and the number
    of canvases, as data.draw_mosaic draws them: the launch is then fv_letterbox_mosaic_batch, the result holds n_out canvases made
    of the n images, and the second result is None.  Not together with aug (draw_mosaic carries the augmentation per tile)."""
    import ctypes
    import torch
    if packed is not None and isinstance(packed[0], str) and packed[0] == 'jpeg':
        # ('jpeg', int16 host tensor of quantised coefficients, jpeg.BatchPlan): the images are reconstructed on the device
        # (fv_jpeg_reconstruct_batch) straight into the packed RGB buffer this launch reads -- no RGB image on the host
        from . import jpeg
        _tag, coefs, plan = packed
        dbuf = jpeg.reconstruct_batch(ctx, plan, coefs.to(device, non_blocking=True), device)
        offs, hw = plan.rgb_off, plan.hw
    else:
        buf, offs, hw = packed if packed is not None else pack_images(raws)
        dbuf = buf.to(device, non_blocking=True)
    n, S = len(offs), int(image_size)
    if mosaic is not None and aug is not None:
        raise ValueError('letterbox_batch_device: aug and mosaic are given together (the mosaic tables carry the augmentation)')
    # the records of the launch (`per` ints each), their colour parameters (3 floats each, or None) and the number of canvases
    if mosaic is not None:
        (recs, colour, n_out), per, what = mosaic, 14, 'tiles'
    else:
        (recs, colour), n_out, per, what = (aug if aug is not None else (None, None)), n, 8, 'images'
    n_out, rp, cp = int(n_out), None, None
    if recs is not None:
        recs = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
        n_rec = max(1, recs.size // per) if mosaic is not None else n
        if recs.size != per * n_rec:
            raise ValueError('letterbox_batch_device: %d record values for %d %s (%d each)' % (recs.size, n_rec, what, per))
        rp = recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if colour is not None:
            colour = np.ascontiguousarray(np.asarray(colour, np.float32).reshape(-1))
            if colour.size != 3 * n_rec:
                raise ValueError('letterbox_batch_device: %d colour values for %d %s (3 each)' % (colour.size, n_rec, what))
            cp = colour.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    if out is None:
        out = torch.empty((n_out, S, S, 3), dtype=torch.float32, device=device)
    head = (ctx.handle,) + packed_args(dbuf, offs, hw)
    geom = None
    if mosaic is not None:
        name, rc = 'fv_letterbox_mosaic_batch', lib().fv_letterbox_mosaic_batch(*head, S, n_out, rp, cp, n_rec, ptr(out))
    elif aug is not None:
        name, rc = 'fv_letterbox_augment_batch', lib().fv_letterbox_augment_batch(*head, S, rp, cp, ptr(out))
    else:
        geom = (ctypes.c_int32 * (6 * n))()
        name, rc = 'fv_letterbox_batch', lib().fv_letterbox_batch(*head, S, ptr(out), geom)
    ctx.check(rc, name)
    if keep is not None:
        keep.append((dbuf, list(offs), list(hw)))
    return out, None if geom is None else [(hw[2 * i], hw[2 * i + 1]) + tuple(geom[6 * i + 2:6 * i + 6]) for i in range(n)]


def letterbox_crops(ctx, images, crops, image_size, out=None):
    """fv_letterbox_crops: images = (device uint8 buffer, offsets, hw) of a batch (letterbox_batch_device's `keep`), crops = list
    of (image index, y0, x0, rows, cols) -> (n, S, S, 3) float32 CUDA tensor."""
    import ctypes
    import torch
    n, S = len(crops), int(image_size)
    if out is None:
        out = torch.empty((n, S, S, 3), dtype=torch.float32, device=images[0].device)
    if n == 0:
        return out
    flat = [int(v) for c in crops for v in c]
    rc = lib().fv_letterbox_crops(ctx.handle, *packed_args(*images), (ctypes.c_int32 * (5 * n))(*flat), n, S, ptr(out))
    ctx.check(rc, 'fv_letterbox_crops')
    return out


TILE_ROWS = 60                # FV_DET_ROWS
TILE_MAX_CANDS = 4096         # FV_TILE_MAX_CANDS of csrc/tile_merge.h
TILE_METRICS = {'ios': 0, 'iou': 1}


def tile_merge_workspace(n_frames, device):
    """A CUDA tensor of fv_tile_merge_workspace_bytes(n_frames) bytes (float64, so 8-byte aligned); contents do not matter."""
    import torch
    need = int(lib().fv_tile_merge_workspace_bytes(int(n_frames)))
    return torch.empty(max(need // 8, 1), dtype=torch.float64, device=device)


def tile_merge(ctx, res, tiles, frame_off, image_size, metric, merge_th, workspace=None, out=None):
    """fv_tile_merge: decode_nms' device dict for T tile views, tiles (T, 5) int32 CUDA tensor (frame, y0, x0, th, tw) and frame_off
    (F + 1,) int32 CUDA tensor (frame f owns the views frame_off[f] .. frame_off[f + 1]) -> dict of CUDA tensors corners
    (F, 60, 4) float64 xmin, ymin, xmax, ymax in frame pixels, rows (F, 60, 5) float64 x, y, w, h, conf (what det_metric.match_rows
    reads), nrows (F,) int32 (-1: the frame held more than 4096 candidates) and src (F, 60) int32 (view * K + slot, -1 past nrows).
    metric 'ios' or 'iou'.  workspace: a CUDA tensor of at least fv_tile_merge_workspace_bytes(F) bytes (its contents are ignored);
    out: a dict of the four tensors to write into (views of a longer buffer are fine).  No host sync."""
    import torch
    boxes, score, count = res['boxes'], res['score'], res['count']
    T, K = int(boxes.shape[0]), int(boxes.shape[1])
    F = int(frame_off.numel()) - 1
    dev = boxes.device
    assert boxes.dtype == torch.int32 and score.dtype == torch.float32 and count.dtype == torch.int32
    assert tuple(score.shape) == (T, K) and tuple(count.shape) == (T,)
    assert tiles.dtype == torch.int32 and tuple(tiles.shape) == (T, 5) and frame_off.dtype == torch.int32 and frame_off.dim() == 1
    if metric not in TILE_METRICS:
        raise ValueError("tile_merge: metric %r is not valid ('ios' or 'iou')" % (metric,))
    ws = workspace if workspace is not None else tile_merge_workspace(F, dev)
    if out is None:
        out = dict(corners=torch.empty((F, TILE_ROWS, 4), dtype=torch.float64, device=dev),
                   rows=torch.empty((F, TILE_ROWS, 5), dtype=torch.float64, device=dev),
                   nrows=torch.empty((F,), dtype=torch.int32, device=dev),
                   src=torch.empty((F, TILE_ROWS), dtype=torch.int32, device=dev))
    assert tuple(out['corners'].shape) == (F, TILE_ROWS, 4) and tuple(out['rows'].shape) == (F, TILE_ROWS, 5)
    assert tuple(out['nrows'].shape) == (F,) and tuple(out['src'].shape) == (F, TILE_ROWS)
    rc = lib().fv_tile_merge(ctx.handle, ptr(boxes), ptr(score), ptr(count), ptr(tiles), ptr(frame_off), T, F, K, int(image_size),
                             TILE_METRICS[metric], float(merge_th), ptr(ws), ws.numel() * ws.element_size(), ptr(out['corners']),
                             ptr(out['rows']), ptr(out['nrows']), ptr(out['src']))
    ctx.check(rc, 'fv_tile_merge')
    return out
