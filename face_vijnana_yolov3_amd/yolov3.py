"""Secondary path: the full three-scale YOLOv3 model of the reference (make_yolov3_model,
yolov3_detect.py:217-311) and its decode / NMS chain (yolov3_detect.py:335-444, driver
yolov3_detect.py:_main_ :545-610), on the device.  FaceDetector does not use this; it exists
because SURVEY 8a-17/18 list it as part of the reference's hot-path files."""
import ctypes

import numpy as np
import torch

from . import model
from ._lib import Context, FvError, lib, ptr

COCO_ANCHORS = [[116, 90, 156, 198, 373, 326], [30, 61, 62, 45, 59, 119], [10, 13, 16, 30, 33, 23]]  # yd.py:560


def yolov3_layer_table(out_channels=255):
    L = lib()
    return model.layer_table(L.fv_yolov3_num_layers, lambda i, d: L.fv_yolov3_layer(i, out_channels, d))


class Yolov3(model.Model):
    def __init__(self, device=0, out_channels=255, ctx=None):
        self.out_channels = int(out_channels)
        self.nclass = self.out_channels // 3 - 5
        # data.det_loss_conf's dict: forward_backward then runs fv_yolov3_train_step_det (the YOLOv3 detection loss) and
        # keeps its statistics in det_stats (12 float64 on the device, the last step's); None: fv_yolov3_train_step
        self.det_loss = None
        self.det_stats = None
        self._det_key = None
        super(Yolov3, self).__init__(ctx or Context(device), yolov3_layer_table(self.out_channels),
                                     lib().fv_yolov3_param_count(self.out_channels), lib().fv_yolov3_state_count(self.out_channels))

    def _workspace_bytes(self, batch, image_size, training):
        if training:
            return lib().fv_yolov3_train_workspace_bytes(batch, image_size, self.out_channels)
        return lib().fv_yolov3_workspace_bytes(batch, image_size, self.out_channels)

    def _workspace_tensor(self, batch, image_size, layer, code, off, cnt):
        return lib().fv_yolov3_train_workspace_tensor(batch, image_size, self.out_channels, layer, code, off, cnt)

    def train_flops_per_image(self, S):
        """forward + weight-gradient of every conv + data-gradient of every conv but the first (2 FLOPs per MAC)."""
        f = [2.0 * d['ksize'] ** 2 * d['cin'] * d['cout'] * (S // d['out_div']) ** 2 for d in self.layers]
        return 3.0 * sum(f) - f[0]

    def load_darknet(self, path_or_bytes):
        """Full Darknet yolov3.weights (conv index order 0..105; yd.py:90-121)."""
        from .weights import header_len
        buf = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, 'rb').read()
        data = np.frombuffer(buf, dtype='<f4', offset=header_len(buf))
        p = np.zeros(self.n_params, np.float32); s = np.zeros(self.n_state, np.float32)
        off = 0
        for d in sorted(self.layers, key=lambda d: d['darknet_index']):
            k, cin, cout = d['ksize'], d['cin'], d['cout']
            n = cout * cin * k * k
            if d['has_bn']:
                for dst, o in ((p, d['beta_off']), (p, d['gamma_off']), (s, d['mean_off']), (s, d['var_off'])):
                    dst[o:o + cout] = data[off:off + cout]; off += cout
            else:
                p[d['beta_off']:d['beta_off'] + cout] = data[off:off + cout]; off += cout
            p[d['w_off']:d['w_off'] + n] = data[off:off + n].reshape(cout, cin, k, k).transpose(0, 2, 3, 1).reshape(-1); off += n
        self.set_params(p, s)
        return off

    def predict_device(self, x):
        """x (B,S,S,3) -> the three outputs [(B,S/32,S/32,out_channels), S/16, S/8], float32 CUDA tensors."""
        return self._in_parts(self._predict, torch.as_tensor(x).to(device=self.dev, dtype=torch.float32).contiguous())

    def _predict(self, x):
        B, S = x.shape[0], x.shape[1]
        ws = self._workspace(B, S, False)
        ys = [torch.empty((B, S // d, S // d, self.out_channels), dtype=torch.float32, device=self.dev) for d in (32, 16, 8)]
        rc = lib().fv_yolov3_forward(self.ctx.handle, ptr(self.params), ptr(self.state), ptr(x), B, S, self.out_channels, ptr(ws),
                                     ws.numel(), ptr(ys[0]), ptr(ys[1]), ptr(ys[2]))
        self.ctx.check(rc, 'fv_yolov3_forward')
        return ys

    # ------------------------------------------------------------------ training (fv_yolov3_train_step)
    def forward_backward(self, x, targets, on_bucket=None, loss_weight=1.0):
        """x (B,S,S,3); targets: three tensors shaped like the outputs, (B,g,g,3*(5+classes)).  Gradients land in
        self.grads; returns the loss (1-element CUDA tensor).  on_bucket(offset, count): called as gradient ranges complete
        (descending offsets), the protocol of Engine.forward_backward -- parallel.DataParallelTrainer drives either."""
        self.ensure_optimizer()
        x = torch.as_tensor(x).to(device=self.dev, dtype=torch.float32).contiguous()
        B, S = x.shape[0], x.shape[1]
        t = [torch.as_tensor(y).to(device=self.dev, dtype=torch.float32).contiguous() for y in targets]
        for y, dv in zip(t, (32, 16, 8)):
            assert y.numel() == B * (S // dv) ** 2 * self.out_channels, tuple(y.shape)
        ws = self._workspace(B, S, True)
        cb, errors = self._bucket_fn(on_bucket)
        if self.det_loss is None:
            return self._train_call('fv_yolov3_train_step', ptr(x), ptr(t[0]), ptr(t[1]), ptr(t[2]), B, S, self.out_channels, ptr(ws),
                                    ws.numel(), ptr(self.grads), ptr(self._loss), float(loss_weight), cb, None, errors=errors)
        conf, scratch = self._det_buffers(B, S)
        loss = self._train_call('fv_yolov3_train_step_det', ptr(x), ptr(t[0]), ptr(t[1]), ptr(t[2]), B, S, self.out_channels, ptr(ws),
                                ws.numel(), ptr(self.grads), ptr(self._loss), float(loss_weight), cb, None, ctypes.byref(conf),
                                ptr(scratch), scratch.numel() * 8, ptr(self.det_stats), errors=errors)
        # the epoch's running totals stay on the device (no host sync in the step): sums, and the maximum for entry 9
        self._det_sum.add_(self.det_stats)
        torch.maximum(self._det_max, self.det_stats, out=self._det_max)
        self._det_steps += 1
        self._det_slots += B * 63 * (S // 32) ** 2
        return loss

    def head_tensor(self, batch, image_size, scale, grad=False):
        """The raw output (batch*g^2, out_channels) of scale `scale` the last training call left in its workspace, or with grad
        its gradient (batch*g^2, c_pad); a view."""
        off, cnt = ctypes.c_size_t(0), ctypes.c_int64(0)
        rc = lib().fv_yolov3_train_workspace_head(batch, image_size, self.out_channels, scale, 1 if grad else 0, ctypes.byref(off),
                                                  ctypes.byref(cnt))
        if rc != 0:
            raise FvError('no head tensor of scale %d at batch %d, image size %d' % (scale, batch, image_size))
        rows = batch * ((image_size // 32) << scale) ** 2
        ws = self._workspace(batch, image_size, True)
        return ws[off.value:off.value + 4 * cnt.value].view(torch.float32).view(rows, -1)

    def _det_buffers(self, B, S):
        """-> (fv_yolo_det_conf, scratch) of self.det_loss at this batch / image size; det_stats and the epoch totals on first use."""
        from . import ops
        key = (B, S, tuple(sorted((k, str(v)) for k, v in self.det_loss.items())))
        if self._det_key != key:
            self._det_conf = ops.yolo_det_conf(self.det_loss)
            self._det_scratch = ops.yolo_det_scratch(B, S, int(self.det_loss['max_boxes']), self.dev)
            self._det_key = key
        if self.det_stats is None:
            self.det_stats = torch.zeros(12, dtype=torch.float64, device=self.dev)
            self.reset_det_epoch()
        return self._det_conf, self._det_scratch

    def reset_det_epoch(self):
        self._det_sum = torch.zeros(12, dtype=torch.float64, device=self.dev)
        self._det_max = torch.zeros(12, dtype=torch.float64, device=self.dev)
        self._det_steps = self._det_slots = 0

    def take_det_epoch(self):
        """-> (the 12 stats of the steps since the last call: sums, entry 9 their maximum; steps; slots) or None when no step ran
        with det_loss; host sync.  Resets the totals."""
        if self.det_stats is None or self._det_steps == 0:
            return None
        sums = self._det_sum.cpu().numpy()
        sums[9] = float(self._det_max[9].item())
        out = (sums, self._det_steps, self._det_slots)
        self.reset_det_epoch()
        return out

    def train_on_batch(self, x, targets, lr, beta_1, beta_2, decay=0.0):
        loss = self.forward_backward(x, targets)
        self.adam_step(lr, beta_1, beta_2, decay)
        return loss

    def save(self, path):
        """As Engine.save: `*.h5` = HDF5 in Keras' weight layout, one group per layer as `make_yolov3_model().save_weights` names
        them (conv_i / bnorm_i; the detection convs conv_81 / conv_93 / conv_105 carry a bias), Adam state under /fv."""
        self._save(path, None, out_channels=np.int64(self.out_channels))

    def load(self, path):
        self._load(path, error=ValueError, check=self._check_out_channels)

    def _check_out_channels(self, path, fv):
        if 'out_channels' in fv and int(fv['out_channels']) != self.out_channels:
            raise ValueError('%s holds a model with %d output channels, this one has %d' % (path, int(fv['out_channels']), self.out_channels))


MAX_CANDIDATES = 8192   # fv_yolo_decode_nms: the per-class sort of one image runs in the LDS of one workgroup


def candidate_slots(g):
    """Candidate slots of one image at grid g: kept anchors 1 @g, 2 @2g, 1 @4g (the reference's skip list) = 25 g^2."""
    return g * g + 2 * (2 * g) * (2 * g) + (4 * g) * (4 * g)


def check_candidate_count(count, capacity, g):
    """The wrappers pass capacity = min(slots, MAX_CANDIDATES).  From grid 19 (608 input, 9025 slots) on an image can hold
    more candidates than the kernel sorts; it then reports count == capacity < slots and the list is cut short.  That is an
    error here, never a shortened result (a frame with exactly MAX_CANDIDATES candidates is refused with it)."""
    if count >= capacity and capacity < candidate_slots(g):
        raise FvError('three-scale decode: an image holds at least %d candidates above the objectness threshold, the kernel handles '
                      '%d (grid %d has %d slots): raise the threshold' % (count, MAX_CANDIDATES, g, candidate_slots(g)))


def decode_nms(ctx, y13, y26, y52, image_hw, net_hw=(416, 416), anchors=COCO_ANCHORS, obj_thresh=0.5, nms_thresh=0.45):
    """One image: three (g,g,3*(5+nclass)) float32 CUDA tensors -> dict(boxes (n,4) int32 image
    pixels, objness (n,), classes (n,nclass) with suppressed entries zeroed), reference list order.
    Any grid: up to MAX_CANDIDATES candidates per image; more raise FvError (check_candidate_count)."""
    g = int(y13.shape[-3])
    nclass = int(y13.shape[-1]) // 3 - 5
    cap = min(candidate_slots(g), MAX_CANDIDATES)
    dev = y13.device
    boxes = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    obj = torch.empty((cap,), dtype=torch.float32, device=dev)
    cls = torch.empty((cap, nclass), dtype=torch.float32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    anc = (ctypes.c_float * 18)(*[float(v) for row in anchors for v in row])
    rc = lib().fv_yolo_decode_nms(ctx.handle, ptr(y13.contiguous()), ptr(y26.contiguous()), ptr(y52.contiguous()), g, nclass, anc,
                                  float(obj_thresh), float(nms_thresh), int(net_hw[0]), int(net_hw[1]), int(image_hw[0]),
                                  int(image_hw[1]), cap, ptr(boxes), ptr(obj), ptr(cls), ptr(cnt))
    ctx.check(rc, 'fv_yolo_decode_nms')
    n = int(cnt.item())
    check_candidate_count(n, cap, g)
    return dict(boxes=boxes[:n], objness=obj[:n], classes=cls[:n])


def decode_nms_batch(ctx, y13, y26, y52, image_hw, net_hw=(416, 416), anchors=COCO_ANCHORS, obj_thresh=0.5, nms_thresh=0.45):
    """A batch of images of one size: three (B,g,g,3*(5+nclass)) float32 CUDA tensors -> dict of CUDA tensors boxes (B,cap,4)
    int32, objness (B,cap), classes (B,cap,nclass), count (B,) -- ONE launch pair for the batch, no host sync (the caller
    copies the tensors out and reads count[b] entries of image b).  cap = min(slots, MAX_CANDIDATES): where the caller reads
    count on the host it passes each count[b] to check_candidate_count(count[b], cap, g), which refuses a saturated image."""
    B, g = int(y13.shape[0]), int(y13.shape[-3])
    nclass = int(y13.shape[-1]) // 3 - 5
    cap = min(candidate_slots(g), MAX_CANDIDATES)
    dev = y13.device
    boxes = torch.empty((B, cap, 4), dtype=torch.int32, device=dev)
    obj = torch.empty((B, cap), dtype=torch.float32, device=dev)
    cls = torch.empty((B, cap, nclass), dtype=torch.float32, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    anc = (ctypes.c_float * 18)(*[float(v) for row in anchors for v in row])
    rc = lib().fv_yolo_decode_nms_batch(ctx.handle, ptr(y13.contiguous()), ptr(y26.contiguous()), ptr(y52.contiguous()), B, g, nclass, anc,
                                        float(obj_thresh), float(nms_thresh), int(net_hw[0]), int(net_hw[1]), int(image_hw[0]),
                                        int(image_hw[1]), cap, ptr(boxes), ptr(obj), ptr(cls), ptr(cnt))
    ctx.check(rc, 'fv_yolo_decode_nms_batch')
    return dict(boxes=boxes, objness=obj, classes=cls, count=cnt)


INT_MAX = 2 ** 31 - 1


def select_refuse_at(capacity, g):
    """The count from which fv_yolo_select_cands refuses an image: capacity where the list may have been cut short (what
    check_candidate_count decides on the host), never (INT_MAX) where the capacity holds every slot of grid g."""
    return int(capacity) if int(capacity) < candidate_slots(g) else INT_MAX


def select_cands_buffers(n, num_cands, nclass, device):
    """The six result tensors of select_cands for n images, uninitialised."""
    from .postproc import decode_nms_buffers
    out = decode_nms_buffers(n, num_cands, device)
    out['classes'] = torch.empty((n, int(num_cands), int(nclass)), dtype=torch.float32, device=device)
    return out


def select_cands(ctx, res, num_cands, grid, out=None):
    """fv_yolo_select_cands: decode_nms_batch's dict -> the tail of detect() (score > 0, ascending stable argsort, the first
    num_cands) per image, as a dict of CUDA tensors under fv_decode_nms' key names: boxes (B,K,4) int32, cell (B,K) int32 (the row's
    index in the candidate list), obj (B,K), score (B,K) (the arg-max class probability capped at 1), count (B,) int32, and classes
    (B,K,nclass).  det_metric.rows_from_nms and the pinned-copy code of the single-scale path take it as is.  grid: the coarsest
    grid (image_size // 32); an image whose list may have been cut short (check_candidate_count) gets count -1, which
    check_selected_count turns into the error where the count is read on the host.  out: such a dict to write into (views along
    the first axis of a longer buffer are fine).  No host sync."""
    boxes, obj, cls, cnt = res['boxes'], res['objness'], res['classes'], res['count']
    B, cap, nclass = int(boxes.shape[0]), int(boxes.shape[1]), int(cls.shape[2])
    K = int(num_cands)
    assert boxes.dtype == torch.int32 and obj.dtype == torch.float32 and cls.dtype == torch.float32 and cnt.dtype == torch.int32
    assert tuple(boxes.shape) == (B, cap, 4) and tuple(obj.shape) == (B, cap) and tuple(cls.shape) == (B, cap, nclass)
    assert tuple(cnt.shape) == (B,)
    if out is None:
        out = select_cands_buffers(B, K, nclass, boxes.device)
    assert tuple(out['boxes'].shape) == (B, K, 4) and tuple(out['cell'].shape) == (B, K) and tuple(out['obj'].shape) == (B, K)
    assert tuple(out['score'].shape) == (B, K) and tuple(out['classes'].shape) == (B, K, nclass) and tuple(out['count'].shape) == (B,)
    rc = lib().fv_yolo_select_cands(ctx.handle, ptr(boxes), ptr(obj), ptr(cls), ptr(cnt), B, cap, nclass, select_refuse_at(cap, grid), K,
                                    ptr(out['boxes']), ptr(out['cell']), ptr(out['obj']), ptr(out['score']), ptr(out['classes']),
                                    ptr(out['count']))
    ctx.check(rc, 'fv_yolo_select_cands')
    return dict(boxes=out['boxes'], cell=out['cell'], obj=out['obj'], score=out['score'], classes=out['classes'], count=out['count'])


def check_selected_count(count, g):
    """select_cands' count of one image, read on the host: -1 is the image check_candidate_count refuses (its list may have been
    cut short at the kernel's capacity); the same error."""
    if count < 0:
        cap = min(candidate_slots(g), MAX_CANDIDATES)
        check_candidate_count(cap, cap, g)
