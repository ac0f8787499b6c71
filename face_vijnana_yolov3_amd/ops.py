"""Thin Python wrappers over the operator-level C ABI (device tensors in / out).

Used by the parity tests and by anyone composing the kernels differently from engine.py.
All tensors are contiguous float32 CUDA (ROCm) tensors in NHWC / OHWI layout."""
import ctypes

import numpy as np
import torch

from ._lib import lib, ptr, c_void_p

NULL = c_void_p(None)


def _p(t):
    return NULL if t is None else ptr(t)


def pack_first_layer(ctx, w_ohwi):
    cout = w_ohwi.shape[0]
    k = w_ohwi[0].numel()
    out = torch.empty((cout, 32), dtype=torch.float32, device=w_ohwi.device)
    ctx.check(lib().fv_pack_first_layer(ctx.handle, ptr(w_ohwi.contiguous()), cout, k, ptr(out)), 'fv_pack_first_layer')
    return out


def conv2d_forward(ctx, x, w, stride=1, scale=None, shift=None, leaky=-1.0, addend=None, stats=False):
    """x (B,H,W,Cin), w OHWI (Cout,k,k,Cin) -> out (B,H/s,W/s,Cout) [, psum, psq]."""
    B, H, W, cin = x.shape
    cout, k = w.shape[0], w.shape[1]
    wd = pack_first_layer(ctx, w) if cin % 32 else w.contiguous()
    out = torch.empty((B, H // stride, W // stride, cout), dtype=torch.float32, device=x.device)
    psum = psq = None
    if stats:
        rows = lib().fv_conv2d_stat_rows(B * (H // stride) * (W // stride))
        psum = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
        psq = torch.empty_like(psum)
    rc = lib().fv_conv2d_forward(ctx.handle, ptr(x.contiguous()), ptr(wd), B, H, W, cin, cout, k, stride, _p(scale),
                                 _p(shift), float(leaky), _p(addend), ptr(out), _p(psum), _p(psq))
    ctx.check(rc, 'fv_conv2d_forward')
    return (out, psum, psq) if stats else out


def transpose_weights(ctx, w, cout_pad=None):
    cout, k, _, cin = w.shape
    cp = cout_pad or cout
    wt = torch.empty((cin, k * k, cp), dtype=torch.float32, device=w.device)
    ctx.check(lib().fv_transpose_weights(ctx.handle, ptr(w.contiguous()), cout, k * k, cin, cp, ptr(wt)), 'fv_transpose_weights')
    return wt


def conv2d_dgrad(ctx, dy, w, in_hw, stride=1, addend=None):
    """dy (B,Ho,Wo,CoutPad), w OHWI -> dx (B,H,W,Cin)."""
    B = dy.shape[0]
    H, W = in_hw
    cout, k, _, cin = w.shape
    wt = transpose_weights(ctx, w, dy.shape[3])
    dx = torch.empty((B, H, W, cin), dtype=torch.float32, device=dy.device)
    rc = lib().fv_conv2d_dgrad(ctx.handle, ptr(dy.contiguous()), ptr(wt), B, H, W, cin, dy.shape[3], k, stride, _p(addend), ptr(dx))
    ctx.check(rc, 'fv_conv2d_dgrad')
    return dx


def conv2d_wgrad(ctx, x, dy, cout, ksize, stride=1):
    """x (B,H,W,Cin), dy (B,Ho,Wo,Ndy>=cout) -> dw OHWI (cout,k,k,Cin)."""
    B, H, W, cin = x.shape
    dw = torch.zeros((cout, ksize, ksize, cin), dtype=torch.float32, device=x.device)
    rc = lib().fv_conv2d_wgrad(ctx.handle, ptr(x.contiguous()), ptr(dy.contiguous()), B, H, W, cin, cout, dy.shape[3], ksize, stride, ptr(dw))
    ctx.check(rc, 'fv_conv2d_wgrad')
    return dw


def bn_finalize(ctx, psum, psq, count, gamma, beta, eps=1e-3, momentum=0.99, moving_mean=None, moving_var=None):
    C = gamma.numel()
    mk = lambda: torch.empty(C, dtype=torch.float32, device=gamma.device)
    mean, invstd, scale, shift = mk(), mk(), mk(), mk()
    rc = lib().fv_bn_finalize(ctx.handle, ptr(psum), ptr(psq), psum.shape[0], C, int(count), ptr(gamma), ptr(beta), eps, momentum,
                              ptr(mean), ptr(invstd), ptr(scale), ptr(shift), _p(moving_mean), _p(moving_var))
    ctx.check(rc, 'fv_bn_finalize')
    return mean, invstd, scale, shift


def bn_act(ctx, z, scale, shift, skip=None, leaky=0.1):
    out = torch.empty_like(z)
    C = z.shape[-1]
    ctx.check(lib().fv_bn_act(ctx.handle, ptr(z), ptr(scale), ptr(shift), _p(skip), ptr(out), z.numel() // C, C, leaky), 'fv_bn_act')
    return out


def bn_bwd(ctx, g, z, scale, shift, mean, invstd, leaky=0.1):
    C = z.shape[-1]
    rows = z.numel() // C
    n = lib().fv_bn_bwd_scratch_floats(rows, C)
    scratch = torch.empty(2 * n, dtype=torch.float32, device=z.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=z.device)
    dgamma = torch.empty_like(dbeta)
    dz = torch.empty_like(z)
    rc = lib().fv_bn_bwd(ctx.handle, ptr(g.contiguous()), ptr(z), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), rows, C, leaky,
                         ptr(scratch), ptr(dbeta), ptr(dgamma), ptr(dz))
    ctx.check(rc, 'fv_bn_bwd')
    return dz, dgamma, dbeta


# ------------------------------------------------------------------ the fused slot forms fv_train_step runs
def stat_slots(C, device):
    """Zeroed [nslot][2][C] float64 accumulators."""
    return torch.zeros((lib().fv_bn_stat_slots(C), 2, C), dtype=torch.float64, device=device)


def conv2d_forward_slots(ctx, x, w, stride, slots):
    B, H, W, cin = x.shape
    cout, k = w.shape[0], w.shape[1]
    wd = pack_first_layer(ctx, w) if cin % 32 else w.contiguous()
    z = torch.empty((B, H // stride, W // stride, cout), dtype=torch.float32, device=x.device)
    rc = lib().fv_conv2d_forward_slots(ctx.handle, ptr(x.contiguous()), ptr(wd), B, H, W, cin, cout, k, stride, ptr(z), ptr(slots),
                                       slots.shape[0])
    ctx.check(rc, 'fv_conv2d_forward_slots')
    return z


def bn_act_slots(ctx, z, slots, gamma, beta, eps=1e-3, momentum=0.99, moving_mean=None, moving_var=None, skip=None, leaky=0.1):
    C = z.shape[-1]
    rows = z.numel() // C
    mk = lambda: torch.empty(C, dtype=torch.float32, device=z.device)
    mean, invstd, scale, shift = mk(), mk(), mk(), mk()
    out = torch.empty_like(z)
    rc = lib().fv_bn_act_slots(ctx.handle, ptr(z), ptr(slots), slots.shape[0], rows, C, ptr(gamma), ptr(beta), eps, momentum, ptr(mean),
                               ptr(invstd), ptr(scale), ptr(shift), _p(moving_mean), _p(moving_var), _p(skip), ptr(out), leaky)
    ctx.check(rc, 'fv_bn_act_slots')
    return out, mean, invstd, scale, shift


def conv2d_dgrad_bnred(ctx, dy, w, in_hw, stride, bn_z, scale, shift, mean, invstd, slots, addend=None, leaky=0.1):
    """dgrad + fused d-beta/d-gamma reduction of the layer that produced the conv input (adds into `slots`)."""
    B = dy.shape[0]
    H, W = in_hw
    cout, k, _, cin = w.shape
    wt = transpose_weights(ctx, w, dy.shape[3])
    dx = torch.empty((B, H, W, cin), dtype=torch.float32, device=dy.device)
    rc = lib().fv_conv2d_dgrad_bnred(ctx.handle, ptr(dy.contiguous()), ptr(wt), B, H, W, cin, dy.shape[3], k, stride, _p(addend), ptr(dx),
                                     ptr(bn_z), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), leaky, ptr(slots), slots.shape[0])
    ctx.check(rc, 'fv_conv2d_dgrad_bnred')
    return dx


def bn_bwd_slots(ctx, g, z, scale, shift, mean, invstd, slots, reduced, leaky=0.1):
    C = z.shape[-1]
    rows = z.numel() // C
    dbeta = torch.empty(C, dtype=torch.float32, device=z.device)
    dgamma = torch.empty_like(dbeta)
    dz = torch.empty_like(z)
    rc = lib().fv_bn_bwd_slots(ctx.handle, ptr(g.contiguous()), ptr(z), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), rows, C, leaky,
                               ptr(slots), slots.shape[0], 1 if reduced else 0, ptr(dbeta), ptr(dgamma), ptr(dz))
    ctx.check(rc, 'fv_bn_bwd_slots')
    return dz, dgamma, dbeta


# ------------------------------------------------------------------ the BN passes folded into halo kernels (option early_bn_fused)
def conv2d_forward_slots_bn_in(ctx, z_in, in_scale, in_shift, w, stride, slots, leaky=0.1):
    """conv2d_forward_slots of leaky(z_in*in_scale+in_shift), formed while the halo kernel stages z_in (3x3, 32 -> 64 channels)."""
    B, H, W, cin = z_in.shape
    cout, k = w.shape[0], w.shape[1]
    z = torch.empty((B, H // stride, W // stride, cout), dtype=torch.float32, device=z_in.device)
    rc = lib().fv_conv2d_forward_slots_bn_in(ctx.handle, ptr(z_in.contiguous()), ptr(in_scale), ptr(in_shift), leaky, ptr(w.contiguous()),
                                             B, H, W, cin, cout, k, stride, ptr(z), ptr(slots), slots.shape[0])
    ctx.check(rc, 'fv_conv2d_forward_slots_bn_in')
    return z


def conv2d_forward_slots_bn_stats_in(ctx, z_in, in_slots, gamma, beta, w, slots, eps=1e-3, momentum=0.99, moving_mean=None, moving_var=None,
                                     skip=None, leaky=0.1, a_out=None):
    """bn_act_slots of the producing layer + conv2d_forward_slots of a 1x1 conv in one kernel (option bn_in_1x1).
    Returns z, a, mean, invstd, scale, shift; a_out: the buffer the activation is written to (default: a new one)."""
    B, H, W, cin = z_in.shape
    cout = w.shape[0]
    mk = lambda: torch.empty(cin, dtype=torch.float32, device=z_in.device)
    mean, invstd, scale, shift = mk(), mk(), mk(), mk()
    a = torch.empty_like(z_in) if a_out is None else a_out
    z = torch.empty((B, H, W, cout), dtype=torch.float32, device=z_in.device)
    rc = lib().fv_conv2d_forward_slots_bn_stats_in(ctx.handle, ptr(z_in), ptr(in_slots), in_slots.shape[0], ptr(gamma), ptr(beta), eps, momentum,
                                                   ptr(mean), ptr(invstd), ptr(scale), ptr(shift), _p(moving_mean), _p(moving_var), _p(skip),
                                                   ptr(a), leaky, ptr(w.contiguous()), B, H, W, cin, cout, ptr(z), ptr(slots), slots.shape[0])
    ctx.check(rc, 'fv_conv2d_forward_slots_bn_stats_in')
    return z, a, mean, invstd, scale, shift


def conv2d_wgrad_bn_in(ctx, z_in, in_scale, in_shift, dy, cout, ksize, stride=1, leaky=0.1):
    """conv2d_wgrad with x = leaky(z_in*in_scale+in_shift) formed on load (3x3, 32 -> 64 channels)."""
    B, H, W, cin = z_in.shape
    dw = torch.zeros((cout, ksize, ksize, cin), dtype=torch.float32, device=z_in.device)
    rc = lib().fv_conv2d_wgrad_bn_in(ctx.handle, ptr(z_in.contiguous()), ptr(in_scale), ptr(in_shift), leaky, ptr(dy.contiguous()), B, H, W,
                                     cin, cout, dy.shape[3], ksize, stride, ptr(dw))
    ctx.check(rc, 'fv_conv2d_wgrad_bn_in')
    return dw


def conv2d_wgrad_bn_bwd(ctx, x, g, z, scale, shift, mean, invstd, slots, dbeta=None, dgamma=None, leaky=0.1):
    """First layer: bn_bwd_slots(reduced) + conv2d_wgrad in one kernel.  dbeta / dgamma given: the slot sums are ADDED to them.
    Returns dw, dgamma, dbeta."""
    B, H, W, cin = x.shape
    C = z.shape[-1]
    accumulate = dbeta is not None
    if not accumulate:
        dbeta = torch.empty(C, dtype=torch.float32, device=z.device)
        dgamma = torch.empty_like(dbeta)
    dw = torch.zeros((C, 3, 3, cin), dtype=torch.float32, device=z.device)
    rc = lib().fv_conv2d_wgrad_bn_bwd(ctx.handle, ptr(x.contiguous()), ptr(g.contiguous()), ptr(z), ptr(scale), ptr(shift), ptr(mean),
                                      ptr(invstd), leaky, ptr(slots), slots.shape[0], B, H, W, cin, C, 3, 1, 1 if accumulate else 0,
                                      ptr(dbeta), ptr(dgamma), ptr(dw))
    ctx.check(rc, 'fv_conv2d_wgrad_bn_bwd')
    return dw, dgamma, dbeta


def mse_loss_grad(ctx, yp, yt, c_pad=32):
    C = yp.shape[-1]
    rows = yp.numel() // C
    loss = torch.empty(1, dtype=torch.float32, device=yp.device)
    dy = torch.empty((rows, c_pad), dtype=torch.float32, device=yp.device)
    db = torch.empty(C, dtype=torch.float32, device=yp.device)
    rc = lib().fv_mse_loss_grad(ctx.handle, ptr(yp.contiguous()), ptr(yt.contiguous()), rows, C, c_pad, ptr(loss), ptr(dy), ptr(db))
    ctx.check(rc, 'fv_mse_loss_grad')
    return loss, dy, db


def fd_loss_grad(ctx, yp, yt, c_pad=32):
    """The reference's unused fd_loss (face_detection.py:59-64) and its gradient."""
    cells = yp.numel() // 6
    loss = torch.empty(1, dtype=torch.float32, device=yp.device)
    dy = torch.empty((cells, c_pad), dtype=torch.float32, device=yp.device)
    ctx.check(lib().fv_fd_loss_grad(ctx.handle, ptr(yp.contiguous()), ptr(yt.contiguous()), cells, c_pad, ptr(loss), ptr(dy)), 'fv_fd_loss_grad')
    return loss, dy


def adam_step(ctx, p, g, m, v, iteration, lr, beta_1, beta_2, eps=1e-7, decay=0.0):
    rc = lib().fv_adam_step(ctx.handle, ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), int(iteration), float(lr), float(beta_1),
                            float(beta_2), float(eps), float(decay))
    ctx.check(rc, 'fv_adam_step')


# ------------------------------------------------------------------ three-scale helpers / FaceIdentifier head, one call per kernel family
# Output tensors may be passed in (`out=` ...): the parity tests pre-fill them with NaN so that an element the kernel skips shows.
def _new(shape, like, out=None):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == tuple(shape), (tuple(out.shape), tuple(shape))
    return out


def upsample_concat(ctx, src, skip, out=None):
    """src (B,Hs,Ws,C1), skip (B,2Hs,2Ws,C2) -> (B,2Hs,2Ws,C1+C2)."""
    B, Hs, Ws, C1 = src.shape
    C2 = skip.shape[3]
    assert tuple(skip.shape[:3]) == (B, 2 * Hs, 2 * Ws)
    out = _new((B, 2 * Hs, 2 * Ws, C1 + C2), src, out)
    ctx.check(lib().fv_upsample_concat(ctx.handle, ptr(src), ptr(skip), ptr(out), B, Hs, Ws, C1, C2), 'fv_upsample_concat')
    return out


def upsample_concat_bwd(ctx, g, C1, g_up=None, g_skip=None):
    """g (B,2Hs,2Ws,C1+C2) -> g_up (B,Hs,Ws,C1), g_skip (B,2Hs,2Ws,C2)."""
    B, H2, W2, C = g.shape
    g_up = _new((B, H2 // 2, W2 // 2, C1), g, g_up)
    g_skip = _new((B, H2, W2, C - C1), g, g_skip)
    ctx.check(lib().fv_upsample_concat_bwd(ctx.handle, ptr(g), ptr(g_up), ptr(g_skip), B, H2 // 2, W2 // 2, C1, C - C1),
              'fv_upsample_concat_bwd')
    return g_up, g_skip


def colsum(ctx, dy, C, out=None):
    """dy (rows, c_pad) -> (C,): sums of the first C columns."""
    rows, c_pad = dy.shape
    part = torch.full((max(1, lib().fv_colsum_partial_doubles(rows, C)),), float('nan'), dtype=torch.float64, device=dy.device)
    out = _new((C,), dy, out)
    ctx.check(lib().fv_colsum(ctx.handle, ptr(dy), rows, C, c_pad, ptr(part), ptr(out)), 'fv_colsum')
    return out


def yolo_loss_grad(ctx, yp3, yt3, ncls, c_pad, grad_weight=1.0, A=3, dy3=None):
    """Three scales' logits / targets (cells_s, A*(5+ncls)) -> loss (1,), [dy_s (cells_s, c_pad)]."""
    import ctypes
    cells = [int(y.shape[0]) for y in yp3]
    c3 = (ctypes.c_int64 * 3)(*cells)
    n = lib().fv_yolo_loss_partial_doubles(c3, A)
    part = torch.full((max(1, n),), float('nan'), dtype=torch.float64, device=yp3[0].device)
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=yp3[0].device)
    dy3 = [_new((c, c_pad), yp3[0], None if dy3 is None else dy3[s]) for s, c in enumerate(cells)]
    arr = lambda ts: (c_void_p * 3)(*[t.data_ptr() for t in ts])
    for t in list(yp3) + list(yt3):
        assert t.is_contiguous() and t.dtype == torch.float32
    rc = lib().fv_yolo_loss_grad(ctx.handle, arr(yp3), arr(yt3), c3, ncls, A, c_pad, float(grad_weight), ptr(part), ptr(loss), arr(dy3))
    ctx.check(rc, 'fv_yolo_loss_grad')
    return loss, dy3


def yolo_det_conf(conf):
    """data.det_loss_conf's dict -> the fv_yolo_det_conf struct (floats are rounded to float32 there)."""
    from ._lib import YoloDetConf
    from .data import DET_BOX_LOSSES
    anchors = [float(v) for row in conf['anchors'] for v in row]
    assert len(anchors) == 18
    box_loss = conf['box_loss']
    return YoloDetConf(DET_BOX_LOSSES.index(box_loss) if box_loss in DET_BOX_LOSSES else int(box_loss), conf['ignore_thresh'],
                       conf['box_weight'], conf['noobj_weight'], int(conf['max_boxes']), (ctypes.c_float * 18)(*anchors))


def yolo_det_scratch(batch, image_size, max_boxes, device):
    """The caller-owned scratch of fv_yolo_det_loss_grad / fv_yolov3_train_step_det as a float64 tensor."""
    n = lib().fv_yolo_det_scratch_bytes(batch, image_size, max_boxes)
    if n == 0:
        raise ValueError('fv_yolo_det_scratch_bytes: bad batch %r, image_size %r or max_boxes %r' % (batch, image_size, max_boxes))
    return torch.empty(((n + 7) // 8,), dtype=torch.float64, device=device)


def yolo_det_loss_grad(ctx, yp3, yt3, batch, image_size, ncls, c_pad, conf, loss_weight=1.0, dy3=None, scratch=None):
    """The YOLOv3 detection loss on its own: three scales' logits / targets (batch*g_s^2, 3*(5+ncls)), conf = data.det_loss_conf's
    dict -> loss (1,), [dy_s (batch*g_s^2, c_pad)], stats (12,) float64."""
    dev = yp3[0].device
    cells = [batch * ((image_size // 32) << s) ** 2 for s in range(3)]
    for t in list(yp3) + list(yt3):
        assert t.is_contiguous() and t.dtype == torch.float32
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    stats = torch.full((12,), float('nan'), dtype=torch.float64, device=dev)
    dy3 = [_new((c, c_pad), yp3[0], None if dy3 is None else dy3[s]) for s, c in enumerate(cells)]
    if scratch is None:
        scratch = yolo_det_scratch(batch, image_size, int(conf['max_boxes']), dev)
    arr = lambda ts: (c_void_p * 3)(*[t.data_ptr() for t in ts])
    c = yolo_det_conf(conf)
    rc = lib().fv_yolo_det_loss_grad(ctx.handle, arr(yp3), arr(yt3), batch, image_size, ncls, c_pad, ctypes.byref(c), float(loss_weight),
                                     ptr(scratch), scratch.numel() * 8, ptr(loss), arr(dy3), ptr(stats))
    ctx.check(rc, 'fv_yolo_det_loss_grad')
    return loss, dy3, stats


def _towers(ts):
    """Up to three (per, F) tower buffers -> (three pointers, per)."""
    ts = list(ts) + [None] * (3 - len(ts))
    return [_p(t) for t in ts], int(ts[0].shape[0])


def fid_towers_dense_l2(ctx, towers, M, w, bias, pre=None, out=None):
    """towers: up to three (per, F) buffers holding rows m -> towers[m // per][m % per]; -> pre, u (M, 64)."""
    (x0, x1, x2), per = _towers(towers)
    F = int(w.shape[0])
    part = torch.full((max(1, lib().fv_fid_dense_partial_floats(max(M, 1), F)),), float('nan'), dtype=torch.float32, device=w.device)
    pre = _new((M, 64), w, pre)
    out = _new((M, 64), w, out)
    rc = lib().fv_fid_towers_dense_l2(ctx.handle, x0, x1, x2, per, M, F, ptr(w), ptr(bias), ptr(part), ptr(pre), ptr(out))
    ctx.check(rc, 'fv_fid_towers_dense_l2')
    return pre, out


def fid_triplet_loss_grad(ctx, pre, u, grad_weight=1.0, dE=None, dbias=None):
    """pre, u (3B, 64) -> loss (1,), dE (3B, 64), dbias (64,)."""
    B = pre.shape[0] // 3
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=pre.device)
    dE = _new((3 * B, 64), pre, dE)
    dbias = _new((64,), pre, dbias)
    rc = lib().fv_fid_triplet_loss_grad(ctx.handle, ptr(pre), ptr(u), B, float(grad_weight), ptr(loss), ptr(dE), ptr(dbias))
    ctx.check(rc, 'fv_fid_triplet_loss_grad')
    return loss, dE, dbias


def fid_batch_triplet_loss_grad(ctx, pre, u, subjects, margin=0.2, mode=0, grad_weight=1.0, out=None):
    """pre, u (M, 64) float32, subjects (M,) int32; mode 0 batch hard, 1 batch semi-hard -> dict(loss (1,), dE (M, 64), dbias (64,),
    pos_index, neg_index, kind (M,) int32, d_ap, d_an (M,) float64).  out: buffers to write into, by those names."""
    M = pre.shape[0]
    out = dict(out or {})
    new = lambda name, shape, dtype: out[name] if name in out else torch.empty(shape, dtype=dtype, device=pre.device)
    o = dict(loss=new('loss', (1,), torch.float32), dE=new('dE', (M, 64), torch.float32), dbias=new('dbias', (64,), torch.float32),
             pos_index=new('pos_index', (M,), torch.int32), neg_index=new('neg_index', (M,), torch.int32),
             kind=new('kind', (M,), torch.int32), d_ap=new('d_ap', (M,), torch.float64), d_an=new('d_an', (M,), torch.float64))
    rc = lib().fv_fid_batch_triplet_loss_grad(ctx.handle, ptr(pre), ptr(u), ptr(subjects), M, float(margin), int(mode), float(grad_weight),
                                              ptr(o['loss']), ptr(o['dE']), ptr(o['dbias']), ptr(o['pos_index']), ptr(o['neg_index']),
                                              ptr(o['kind']), ptr(o['d_ap']), ptr(o['d_an']))
    ctx.check(rc, 'fv_fid_batch_triplet_loss_grad')
    return o


def fid_margin_softmax_loss_grad(ctx, pre, u, labels, W, kind=0, scale=30.0, margin=0.35, grad_weight=1.0, out=None, workspace=None):
    """pre, u (M, 64) float32, labels (M,) int32 (< 0: an unknown identity), W (C, 64) float32, the class kernel; kind 0 CosFace,
    1 ArcFace -> dict(loss (1,), dE (M, 64), dbias (64,), dW (C, 64), pred (M,) int32, cos_t (M,) float64).  out: buffers to write
    into, by those names.  Labels handed over as a host array are checked against C here; on the device a label >= C makes the
    row one of an unknown identity with pred -2."""
    M, C = int(pre.shape[0]), int(W.shape[0])
    if not torch.is_tensor(labels):
        host = np.asarray(labels)
        if host.shape != (M,) or (host.size and int(host.max()) >= C):
            raise ValueError('fid_margin_softmax_loss_grad expects %d labels below %d' % (M, C))
        labels = torch.from_numpy(host.astype(np.int32)).to(pre.device)
    out = dict(out or {})
    new = lambda name, shape, dtype: out[name] if name in out else torch.empty(shape, dtype=dtype, device=pre.device)
    o = dict(loss=new('loss', (1,), torch.float32), dE=new('dE', (M, 64), torch.float32), dbias=new('dbias', (64,), torch.float32),
             dW=new('dW', (C, 64), torch.float32), pred=new('pred', (M,), torch.int32), cos_t=new('cos_t', (M,), torch.float64))
    if workspace is None:
        workspace = torch.empty(max(16, int(lib().fv_fid_margin_workspace_bytes(M, C))), dtype=torch.uint8, device=pre.device)
    rc = lib().fv_fid_margin_softmax_loss_grad(ctx.handle, ptr(pre), ptr(u), ptr(labels), M, ptr(W), C, int(kind), float(scale),
                                               float(margin), float(grad_weight), ptr(workspace), workspace.numel(), ptr(o['loss']),
                                               ptr(o['dE']), ptr(o['dbias']), ptr(o['dW']), ptr(o['pred']), ptr(o['cos_t']))
    ctx.check(rc, 'fv_fid_margin_softmax_loss_grad')
    return o


def fid_towers_dense_dgrad(ctx, dE, w, towers, M):
    """dE (M, 64), w (F, 64): writes rows m of dE . w^T into towers[m // per][m % per]."""
    (d0, d1, d2), per = _towers(towers)
    rc = lib().fv_fid_towers_dense_dgrad(ctx.handle, ptr(dE), M, int(w.shape[0]), ptr(w), d0, d1, d2, per)
    ctx.check(rc, 'fv_fid_towers_dense_dgrad')


def fid_towers_dense_wgrad(ctx, towers, dE, M, F, dw=None):
    """-> dw (F, 64) = X^T . dE over the M rows of the towers."""
    (x0, x1, x2), per = _towers(towers)
    dw = _new((F, 64), dE, dw)
    rc = lib().fv_fid_towers_dense_wgrad(ctx.handle, x0, x1, x2, per, ptr(dE), M, F, ptr(dw))
    ctx.check(rc, 'fv_fid_towers_dense_wgrad')
    return dw


def recon_dense_head(ctx, ids, w, bias):
    """ids (N,64), w (F,64), bias (F,) -> (u (N,64) = relu(l2_normalize(ids)), x (N,F) = u . w^T + bias)."""
    N, F = ids.shape[0], w.shape[0]
    u = torch.empty((N, 64), dtype=torch.float32, device=ids.device)
    x = torch.empty((N, F), dtype=torch.float32, device=ids.device)
    ctx.check(lib().fv_recon_dense_head(ctx.handle, ptr(ids.contiguous()), N, F, ptr(w.contiguous()), ptr(bias.contiguous()), ptr(u), ptr(x)),
              'fv_recon_dense_head')
    return u, x


def l2norm_affine(ctx, x, scale, shift, skip=None, leaky=0.1, keep_d=True):
    """x (rows,C) [, skip (rows,C)] -> (y, d): d = x - skip (None without skip or with keep_d=False), y = BN-folded l2-normalised
    leaky_relu(d) (fv_l2norm_affine)."""
    rows, C = x.shape
    y = torch.empty_like(x)
    d = torch.empty_like(x) if (skip is not None and keep_d) else None
    ctx.check(lib().fv_l2norm_affine(ctx.handle, ptr(x), _p(skip), _p(d), ptr(scale), ptr(shift), ptr(y), rows, C, float(leaky)),
              'fv_l2norm_affine')
    return y, d


def conv2d_transpose(ctx, x, w, stride=1):
    """x (B,Hin,Win,Cout), w OHWI (Cout,k,k,Cin) of the conv layer whose kernel the transposed conv carries
    -> (B,Hin*stride,Win*stride,Cin): Keras' Conv2DTranspose(Cin, k, strides=stride, padding='same', use_bias=False)."""
    B, Hin, Win, cout = x.shape
    k, cin = w.shape[1], w.shape[3]
    wt = transpose_weights(ctx, w)
    out = torch.empty((B, Hin * stride, Win * stride, cin), dtype=torch.float32, device=x.device)
    rc = lib().fv_conv2d_transpose(ctx.handle, ptr(x.contiguous()), ptr(wt), B, Hin, Win, cin, cout, k, stride, ptr(out))
    ctx.check(rc, 'fv_conv2d_transpose')
    return out
