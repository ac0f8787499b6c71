"""GPU parity of every operator-level kernel (through the C ABI) against a float64 torch-CPU
restatement of the same Keras op (oracle/net_oracle.py conventions).

Tolerance: the kernels compute in exact fp32 (v_mfma_f32_32x32x2_f32 = fmaf chain); against the
float64 reference the error is bounded by ~K * 2^-24 * sum|a||b|, so we assert
|got - ref| <= 2e-6 * (|a| conv |b|) + 1e-6 -- i.e. a few fp32 ulps of the absolute-value
convolution -- much tighter than a blanket rtol."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _ref_conv(x, w, k, s):
    """NHWC x, OHWI w, float64: ZeroPadding2D(1)+Conv2D valid (k=3) or 1x1."""
    xn = x.permute(0, 3, 1, 2)
    if k == 3:
        xn = F.pad(xn, (1, 1, 1, 1))
    return F.conv2d(xn, w.permute(0, 3, 1, 2), stride=s).permute(0, 2, 3, 1).contiguous()


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    tol = 2e-6 * bound + 1e-6
    bad = err > tol
    assert not bad.any(), '%s: max err %.3e, tol there %.3e, %d bad' % (what, err.max().item(), tol[bad].min().item() if bad.any() else 0, int(bad.sum()))


FWD_CASES = [
    # B, H, cin, cout, k, s
    (2, 16, 32, 64, 3, 2),
    (2, 16, 64, 32, 1, 1),
    (3, 13, 32, 64, 3, 1),      # M = 507: tail tile
    (2, 8, 128, 256, 3, 1),     # BN = 128 tiles
    (1, 26, 256, 128, 1, 1),
    (2, 12, 3, 32, 3, 1),       # first layer, gathered K = 27
    (2, 13, 1024, 6, 3, 1),     # head: N = 6 guard
    (1, 4, 512, 1024, 3, 2),
    # the three detection convs of the three-scale graph at their real widths (1x1, linear + bias): N = 255 and 27 guards
    (2, 13, 1024, 255, 1, 1),
    (1, 26, 512, 255, 1, 1),
    (1, 52, 256, 255, 1, 1),
    (2, 13, 1024, 27, 1, 1),
    (1, 52, 256, 27, 1, 1),
]


@pytest.mark.parametrize('B,H,cin,cout,k,s', FWD_CASES)
def test_conv_forward_raw_and_stats(ctx, B, H, cin, cout, k, s):
    from face_vijnana_yolov3_amd import ops
    x = _rand((B, H, H, cin), 1); w = _rand((cout, k, k, cin), 2)
    ref = _ref_conv(x.double(), w.double(), k, s)
    bound = _ref_conv(x.double().abs(), w.double().abs(), k, s)
    out, psum, psq = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), stride=s, stats=True)
    _check(out, ref, bound, 'conv fwd')
    rows = ref.numel() // cout
    _check(psum.sum(0), ref.view(rows, cout).sum(0), bound.view(rows, cout).sum(0), 'psum')
    _check(psq.sum(0), (ref.view(rows, cout) ** 2).sum(0), (bound.view(rows, cout) ** 2).sum(0) * 2, 'psq')
    # the plain (no epilogue, no statistics) call: right by the same bound; and bit-identical to the statistics form whenever both run the
    # tile kernels (a small-M inference launch may take conv_small_kernel, which adds the K steps up in another order)
    out2 = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), stride=s)
    _check(out2, ref, bound, 'conv fwd, plain call')
    ctx.set_option('conv_small', 0)
    try:
        out3 = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), stride=s)
    finally:
        ctx.set_option('conv_small', 1)
    assert torch.equal(out, out3)


def test_conv_forward_fused_inference_epilogue(ctx):
    from face_vijnana_yolov3_amd import ops
    B, H, cin, cout = 2, 13, 64, 128
    x = _rand((B, H, H, cin), 3); w = _rand((cout, 3, 3, cin), 4)
    scale = _rand((cout,), 5, 0.5, 1.5); shift = _rand((cout,), 6); skip = _rand((B, H, H, cout), 7)
    ref = _ref_conv(x.double(), w.double(), 3, 1) * scale.double() + shift.double()
    ref = F.leaky_relu(ref, 0.1) + skip.double()
    bound = _ref_conv(x.double().abs(), w.double().abs(), 3, 1) * scale.double().abs() + 2.0
    out = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), 1, scale.cuda(), shift.cuda(), 0.1, skip.cuda())
    _check(out, ref, bound, 'fused epilogue')
    # head form: bias only, linear
    out = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), 1, None, shift.cuda(), -1.0, None)
    _check(out, _ref_conv(x.double(), w.double(), 3, 1) + shift.double(), bound, 'bias epilogue')
    # the three-scale detection convs as fv_yolov3_train_step runs them: 1x1, bias only, linear, 255 / 27 output channels
    for (B, H, cin, cout) in [(1, 52, 256, 255), (2, 13, 1024, 255), (1, 26, 512, 255), (1, 52, 256, 27), (2, 13, 1024, 27)]:
        x = _rand((B, H, H, cin), 8); w = _rand((cout, 1, 1, cin), 9); bias = _rand((cout,), 10)
        out = ops.conv2d_forward(ctx, x.cuda(), w.cuda(), 1, None, bias.cuda(), -1.0, None)
        _check(out, _ref_conv(x.double(), w.double(), 1, 1) + bias.double(), _ref_conv(x.double().abs(), w.double().abs(), 1, 1) + 1.0,
               'detection conv %r' % ((B, H, cin, cout),))


DGRAD_CASES = [
    (2, 16, 32, 64, 3, 1, 64),
    (2, 16, 32, 64, 3, 2, 64),
    (2, 13, 128, 64, 1, 1, 64),
    (3, 12, 64, 128, 3, 2, 128),
    (2, 13, 1024, 6, 3, 1, 32),   # head: dy padded to 32 channels
    (1, 26, 256, 512, 3, 2, 512),
    # detection convs: dy padded from 255 to 256 / from 27 to 32 channels
    (2, 13, 1024, 255, 1, 1, 256),
    (1, 26, 512, 255, 1, 1, 256),
    (1, 52, 256, 255, 1, 1, 256),
    (2, 13, 1024, 27, 1, 1, 32),
    (1, 52, 256, 27, 1, 1, 32),
]


@pytest.mark.parametrize('B,H,cin,cout,k,s,cpad', DGRAD_CASES)
def test_conv_dgrad(ctx, B, H, cin, cout, k, s, cpad):
    from face_vijnana_yolov3_amd import ops
    Ho = H // s
    w = _rand((cout, k, k, cin), 11)
    dy = torch.zeros((B, Ho, Ho, cpad)); dy[..., :cout] = _rand((B, Ho, Ho, cout), 12)
    add = _rand((B, H, H, cin), 13)
    x = torch.zeros((B, H, H, cin), dtype=torch.float64, requires_grad=True)
    y = _ref_conv(x, w.double(), k, s)
    (ref,) = torch.autograd.grad(y, x, dy[..., :cout].double())
    xa = torch.zeros((B, H, H, cin), dtype=torch.float64, requires_grad=True)
    (bound,) = torch.autograd.grad(_ref_conv(xa, w.double().abs(), k, s), xa, dy[..., :cout].double().abs())
    got = ops.conv2d_dgrad(ctx, dy.cuda(), w.cuda(), (H, H), s)
    _check(got, ref, bound, 'dgrad')
    got = ops.conv2d_dgrad(ctx, dy.cuda(), w.cuda(), (H, H), s, addend=add.cuda())
    _check(got, ref + add.double(), bound + 1.0, 'dgrad+add')


WGRAD_CASES = [
    (2, 16, 128, 128, 3, 1, 128),   # QUAD 128x128
    (2, 16, 64, 64, 3, 1, 64),
    (2, 16, 32, 64, 3, 2, 64),      # 64x32 tiles, stride 2
    (2, 16, 64, 32, 1, 1, 32),      # 32x64
    (3, 13, 32, 32, 3, 1, 32),      # 32x32, odd pixel count
    (2, 20, 3, 32, 3, 1, 32),       # first layer, gathered
    (2, 13, 1024, 6, 3, 1, 32),     # head
    (1, 26, 256, 128, 1, 1, 128),
    (4, 26, 128, 256, 3, 1, 256),
    (2, 16, 256, 512, 3, 1, 512),   # >= 64 (tile, tap) workgroups per K-split: plain split order
    # lattices smaller than one 32-pixel chunk: the row table's image / row / column carries all fire within a chunk
    (5, 3, 128, 128, 3, 1, 128),    # 3x3 lattice: a chunk spans 3.6 images
    (7, 4, 128, 256, 3, 2, 256),    # stride 2 -> 2x2 lattice: 8 images per chunk
    (3, 5, 64, 64, 3, 1, 64),       # split form, 25-pixel images
    (9, 2, 256, 128, 1, 1, 128),    # 1x1 on a 2x2 lattice
    (2, 33, 32, 64, 3, 1, 64),      # row length 33: the column wraps at a different lane every chunk
    # the fused nine-tap kernel (32 -> 64 channels): whole units, ragged units in both directions, both strides, padded dy
    (2, 16, 32, 64, 3, 1, 64),
    (3, 13, 32, 64, 3, 1, 64),
    (2, 20, 32, 64, 3, 2, 64),
    (1, 38, 32, 64, 3, 2, 128),
    (5, 4, 32, 64, 3, 1, 64),
    # the first layer's halo kernel: whole / ragged units, padded dy, more units than workgroups, one-row images
    (2, 32, 3, 32, 3, 1, 32),
    (3, 13, 3, 32, 3, 1, 32),
    (1, 70, 3, 32, 3, 1, 64),
    (200, 8, 3, 32, 3, 1, 32),
    (4, 1, 3, 32, 3, 1, 32),
    # the streaming 1x1 kernel (64 -> 32 channels): whole units, a ragged last unit, padded dy, fewer pixels than one unit
    (2, 16, 64, 32, 1, 1, 64),
    (3, 13, 64, 32, 1, 1, 32),
    (1, 5, 64, 32, 1, 1, 32),
    (9, 40, 64, 32, 1, 1, 32),
    # detection convs: 255 of 256 / 27 of 32 dy channels
    (2, 13, 1024, 255, 1, 1, 256),
    (1, 26, 512, 255, 1, 1, 256),
    (1, 52, 256, 255, 1, 1, 256),
    (2, 13, 1024, 27, 1, 1, 32),
    (1, 52, 256, 27, 1, 1, 32),
]


def test_first_layer_wgrad_halo_equals_gather(ctx):
    """wgrad0_mfma.hip against the element-wise gather kernel (option "wgrad_fused_taps" = 0): same products, other summation order."""
    from face_vijnana_yolov3_amd import ops
    for (B, H) in [(3, 48), (2, 21)]:
        x = _rand((B, H, H, 3), 83).cuda(); dy = _rand((B, H, H, 32), 84).cuda()
        got = ops.conv2d_wgrad(ctx, x, dy, 32, 3, 1)
        ctx.set_wgrad_fused_taps(False)
        try:
            ref = ops.conv2d_wgrad(ctx, x, dy, 32, 3, 1)
        finally:
            ctx.set_wgrad_fused_taps(True)
        assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), (B, H)


def test_wgrad_fused_taps_equals_generic(ctx):
    """option "wgrad_fused_taps": the nine-tap kernel and the one-workgroup-per-tap kernel form the same products; only the
    order of the float additions differs."""
    from face_vijnana_yolov3_amd import ops
    for (B, H, s) in [(3, 40, 1), (2, 52, 2)]:
        x = _rand((B, H, H, 32), 81).cuda(); dy = _rand((B, H // s, H // s, 64), 82).cuda()
        got = ops.conv2d_wgrad(ctx, x, dy, 64, 3, s)
        ctx.set_wgrad_fused_taps(False)
        try:
            ref = ops.conv2d_wgrad(ctx, x, dy, 64, 3, s)
        finally:
            ctx.set_wgrad_fused_taps(True)
        scale = ref.abs().max().item()
        assert (got - ref).abs().max().item() <= 2e-5 * scale, (B, H, s)


@pytest.mark.parametrize('B,H,cin,cout,k,s,ndy', WGRAD_CASES)
def test_conv_wgrad(ctx, B, H, cin, cout, k, s, ndy):
    from face_vijnana_yolov3_amd import ops
    Ho = H // s
    x = _rand((B, H, H, cin), 21)
    dy = torch.zeros((B, Ho, Ho, ndy)); dy[..., :cout] = _rand((B, Ho, Ho, cout), 22)
    w = torch.zeros((cout, k, k, cin), dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(_ref_conv(x.double(), w, k, s), w, dy[..., :cout].double())
    wa = torch.zeros((cout, k, k, cin), dtype=torch.float64, requires_grad=True)
    (bound,) = torch.autograd.grad(_ref_conv(x.double().abs(), wa, k, s), wa, dy[..., :cout].double().abs())
    got = ops.conv2d_wgrad(ctx, x.cuda(), dy.cuda(), cout, k, s)
    _check(got, ref, bound, 'wgrad')


@pytest.mark.parametrize('H', [140, 100])
def test_conv_tail_split_with_lent_scratch(ctx, H):
    """fv_set_conv_scratch, both plans of fv_conv_tail_plan: H = 100 -> 157 output tiles of 72 K steps, every tile cut into K
    slices; H = 140 -> 307 tiles, 256 stay whole (one per CU) and the other 51 are cut into slices that fill the second slot of
    the CUs.  The fix-up kernel applies the epilogue.  Forward (raw + BN partial sums, fused affine/leaky/add) and stride-1
    data-gradient against float64; the unsplit launch differs only in rounding."""
    from face_vijnana_yolov3_amd import ops
    B, cin, cout = 2, 256, 128
    x = _rand((B, H, H, cin), 31); w = _rand((cout, 3, 3, cin), 32, -0.1, 0.1)
    scale = _rand((cout,), 33, 0.5, 1.5); shift = _rand((cout,), 34); skip = _rand((B, H, H, cout), 35)
    ref = _ref_conv(x.double(), w.double(), 3, 1)
    bound = _ref_conv(x.double().abs(), w.double().abs(), 3, 1)
    xd, wd = x.cuda(), w.cuda()
    plain, _, _ = ops.conv2d_forward(ctx, xd, wd, stride=1, stats=True)
    ctx.set_conv_scratch(torch.empty(64 << 20, dtype=torch.uint8, device='cuda'))
    try:
        out, psum, psq = ops.conv2d_forward(ctx, xd, wd, stride=1, stats=True)
        out_again, _, _ = ops.conv2d_forward(ctx, xd, wd, stride=1, stats=True)
        fused = ops.conv2d_forward(ctx, xd, wd, 1, scale.cuda(), shift.cuda(), 0.1, skip.cuda())
        # data-gradient of a 128 -> 256 conv: the same gather problem with mirrored taps
        w2 = _rand((cin, 3, 3, cout), 36, -0.1, 0.1); dy = _rand((B, H, H, cin), 37)
        dgrad = ops.conv2d_dgrad(ctx, dy.cuda(), w2.cuda(), (H, H), 1)
    finally:
        ctx.set_conv_scratch(None)
    dgrad_plain = ops.conv2d_dgrad(ctx, dy.cuda(), w2.cuda(), (H, H), 1)
    assert torch.equal(out, out_again)                      # deterministic
    assert not torch.equal(out, plain)                      # the split really ran (other summation order)
    _check(out, ref, bound, 'tail-split fwd')
    _check(plain, ref, bound, 'unsplit fwd')
    rows = ref.numel() // cout
    _check(psum.sum(0), ref.view(rows, cout).sum(0), bound.view(rows, cout).sum(0), 'psum')
    _check(psq.sum(0), (ref.view(rows, cout) ** 2).sum(0), (bound.view(rows, cout) ** 2).sum(0) * 2, 'psq')
    ref_f = F.leaky_relu(ref * scale.double() + shift.double(), 0.1) + skip.double()
    _check(fused, ref_f, bound * scale.double().abs() + 2.0, 'tail-split fused epilogue')
    xg = torch.zeros((B, H, H, cout), dtype=torch.float64, requires_grad=True)
    (ref_d,) = torch.autograd.grad(_ref_conv(xg, w2.double(), 3, 1), xg, dy.double())
    xa = torch.zeros((B, H, H, cout), dtype=torch.float64, requires_grad=True)
    (bound_d,) = torch.autograd.grad(_ref_conv(xa, w2.double().abs(), 3, 1), xa, dy.double().abs())
    _check(dgrad, ref_d, bound_d, 'tail-split dgrad')
    assert not torch.equal(dgrad, dgrad_plain)


@pytest.mark.parametrize('B,H,cin,cout,k', [(4, 3, 512, 1024, 3), (4, 6, 512, 256, 1), (2, 13, 1024, 6, 3), (3, 8, 64, 128, 3),
                                            (2, 140, 256, 128, 3)])
def test_k_split_slabs_are_reused_safely(ctx, B, H, cin, cout, k):
    """Two different problems of one shape alternate through the SAME lent scratch: each result must be
    bit-identical every time (a slab line left over from the previous launch -- per-XCD L2s are not
    coherent -- would show up here) and within rounding of the launch without scratch.  The last shape
    takes the tail split (307 tiles); the small ones document that lending scratch is harmless there."""
    from face_vijnana_yolov3_amd import ops
    xs = [_rand((B, H, H, cin), 40 + i).cuda() for i in range(2)]
    ws = [_rand((cout, k, k, cin), 50 + i, -0.1, 0.1).cuda() for i in range(2)]
    sc = _rand((cout,), 60, 0.5, 1.5).cuda(); sh = _rand((cout,), 61).cuda()
    skip = _rand((B, H, H, cout), 62).cuda()
    plain = [ops.conv2d_forward(ctx, xs[i], ws[i], 1, sc, sh, 0.1, skip) for i in range(2)]
    ctx.set_conv_scratch(torch.empty(96 << 20, dtype=torch.uint8, device='cuda'))
    try:
        first = [None, None]
        for rep in range(6):
            i = rep & 1
            out = ops.conv2d_forward(ctx, xs[i], ws[i], 1, sc, sh, 0.1, skip)
            if first[i] is None:
                first[i] = out
            else:
                assert torch.equal(out, first[i]), (rep, (out - first[i]).abs().max().item())
    finally:
        ctx.set_conv_scratch(None)
    for i in range(2):
        d = (first[i] - plain[i]).abs().max().item()
        assert d <= 2e-5 * plain[i].abs().max().item(), d


@pytest.mark.parametrize('rows,C', [(1000, 32), (4097, 64), (338, 1024), (70000, 128)])
def test_bn_forward_backward(ctx, rows, C):
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import lib
    z = (_rand((rows, C), 31) * 2 + 0.3)
    gamma = _rand((C,), 32, 0.5, 1.5); beta = _rand((C,), 33); g = _rand((rows, C), 34); skip = _rand((rows, C), 35)
    mm = _rand((C,), 36); mv = _rand((C,), 37, 0.5, 2.0)
    # partials as the conv epilogue would emit them (128-row tiles)
    nt = lib().fv_conv2d_stat_rows(rows)
    zp = torch.zeros((nt * 128, C)); zp[:rows] = z
    psum = zp.view(nt, 128, C).sum(1); psq = (zp.view(nt, 128, C) ** 2).sum(1)
    mmd, mvd = mm.cuda(), mv.cuda()
    mean, invstd, scale, shift = ops.bn_finalize(ctx, psum.cuda(), psq.cuda(), rows, gamma.cuda(), beta.cuda(), 1e-3, 0.99, mmd, mvd)
    zd = z.double()
    rmean = zd.mean(0); rvar = zd.var(0, unbiased=False)
    torch.testing.assert_close(mean.cpu().double(), rmean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(invstd.cpu().double(), 1 / torch.sqrt(rvar + 1e-3), rtol=2e-5, atol=0)
    torch.testing.assert_close(mmd.cpu().double(), 0.99 * mm.double() + 0.01 * rmean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mvd.cpu().double(), 0.99 * mv.double() + 0.01 * rvar * rows / (rows - 1.001), rtol=1e-5, atol=1e-6)
    # forward activation (+skip)
    zt = zd.clone().requires_grad_(True); gt = gamma.double().clone().requires_grad_(True); bt = beta.double().clone().requires_grad_(True)
    y = (zt - zt.mean(0)) / torch.sqrt(zt.var(0, unbiased=False) + 1e-3) * gt + bt
    a = F.leaky_relu(y, 0.1)
    out = ops.bn_act(ctx, z.cuda(), scale, shift, skip.cuda(), 0.1)
    torch.testing.assert_close(out.cpu().double(), (a + skip.double()).detach(), rtol=2e-5, atol=2e-5)
    # backward
    rdz, rdg, rdb = torch.autograd.grad(a, (zt, gt, bt), g.double())
    dz, dgamma, dbeta = ops.bn_bwd(ctx, g.cuda(), z.cuda(), scale, shift, mean, invstd, 0.1)
    sc = math.sqrt(rows)
    torch.testing.assert_close(dbeta.cpu().double(), rdb, rtol=1e-4, atol=1e-5 * sc)
    torch.testing.assert_close(dgamma.cpu().double(), rdg, rtol=1e-4, atol=1e-5 * sc)
    # elements whose pre-activation sits within float rounding of the LeakyReLU kink may pick the other slope
    near = (y.detach().abs() < 1e-5)
    err = (dz.cpu().double() - rdz).abs()
    assert (err[~near] <= 2e-5 + 1e-4 * rdz[~near].abs()).all(), err[~near].max()


def test_mse_loss_and_grad(ctx):
    from face_vijnana_yolov3_amd import ops
    yp = _rand((40 * 169, 6), 41, -2, 2); yt = _rand((40 * 169, 6), 42, 0, 1)
    loss, dy, db = ops.mse_loss_grad(ctx, yp.cuda(), yt.cuda(), 32)
    ref = ((yp.double() - yt.double()) ** 2).mean()
    assert abs(loss.item() - ref.item()) <= 1e-6 * ref.item()
    rdy = 2 * (yp.double() - yt.double()) / yp.numel()
    torch.testing.assert_close(dy.cpu()[:, :6].double(), rdy, rtol=1e-6, atol=1e-12)
    assert torch.count_nonzero(dy[:, 6:]) == 0
    torch.testing.assert_close(db.cpu().double(), rdy.sum(0), rtol=1e-5, atol=1e-9)


def test_adam_matches_keras_formula(ctx):
    from face_vijnana_yolov3_amd import ops
    from oracle import net_oracle as no
    n = 1000003  # not a multiple of 4: exercises the tail kernel
    p = _rand((n,), 51); g = _rand((n,), 52, -1e-2, 1e-2)
    m = torch.zeros(n); v = torch.zeros(n)
    pd, md, vd = p.cuda(), m.cuda(), v.cuda()
    rp, rm, rv = p.double(), m.double(), v.double()
    for it in range(3):
        ops.adam_step(ctx, pd, g.cuda(), md, vd, it, 1e-4, 0.99, 0.99, 1e-7, 0.01)
        rp, rm, rv = no.keras_adam(rp, g.double(), rm, rv, it, 1e-4, 0.99, 0.99, decay=0.01)
    torch.testing.assert_close(pd.cpu().double(), rp, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(md.cpu().double(), rm, rtol=1e-5, atol=1e-10)
    torch.testing.assert_close(vd.cpu().double(), rv, rtol=1e-5, atol=1e-12)


def test_fd_loss_and_grad(ctx):
    """fd_loss is defined but unused in the reference (fd.py:59-64); operator-level parity only."""
    from face_vijnana_yolov3_amd import ops
    from oracle import net_oracle as no
    yp = _rand((3 * 169, 6), 61, -0.3, 1.3)          # linear head: values outside [0,1] get clipped
    yt = (_rand((3 * 169, 6), 62, 0, 1) > 0.7).float(); yt[:, 1:5] = _rand((3 * 169, 4), 63, 0, 1)
    ypd = yp.double().clone().requires_grad_(True)
    ref = no.fd_loss(ypd, yt.double())
    (rg,) = torch.autograd.grad(ref, ypd)
    loss, dy = ops.fd_loss_grad(ctx, yp.cuda(), yt.cuda(), 32)
    assert abs(loss.item() - ref.item()) <= 2e-6 * abs(ref.item())
    torch.testing.assert_close(dy.cpu()[:, :6].double(), rg, rtol=2e-6, atol=1e-9)
    assert torch.count_nonzero(dy[:, 6:]) == 0


@pytest.mark.parametrize('B,H,cin,cout,k,s', [(2, 13, 128, 256, 3, 1), (2, 16, 32, 64, 3, 2), (3, 13, 64, 32, 1, 1), (2, 13, 1024, 6, 3, 1)])
def test_four_and_eight_wave_tiles_are_bit_identical(ctx, B, H, cin, cout, k, s):
    """option "conv_waves8": 2x4 waves of 64x32 (default) against 2x2 waves of 64x64 -- the same k-ordered fmaf chain per output
    element, so outputs (incl. zero padding at the borders) and data-gradients are bit-identical."""
    from face_vijnana_yolov3_amd import ops
    x = _rand((B, H, H, cin), 71).cuda(); w = _rand((cout, k, k, cin), 72).cuda()
    dy = _rand((B, H // s, H // s, max(32, cout)), 73).cuda()
    if cout < 32:
        dy[..., cout:] = 0
    ref = ops.conv2d_forward(ctx, x, w, stride=s)
    dg_ref = ops.conv2d_dgrad(ctx, dy, w, (H, H), s)
    ctx.set_conv_waves8(False)
    try:
        got = ops.conv2d_forward(ctx, x, w, stride=s)
        dg = ops.conv2d_dgrad(ctx, dy, w, (H, H), s)
    finally:
        ctx.set_conv_waves8(True)
    assert torch.equal(got, ref) and torch.equal(dg, dg_ref)


# ---------------------------------------------------------------------------------------------------------------------------
# Three-scale helpers (elementwise.hip) and the FaceIdentifier head (fid.hip), one operator at a time.  References: plain torch
# float64 on the CPU, evaluated on the same fp32 inputs the kernel gets.  Every output buffer is pre-filled with NaN: an element
# the kernel skips, or a padding column it leaves unwritten, fails the comparison.  Every bound is derived from the arithmetic
# (an fp64 accumulation rounded to float once: 2^-24 relative; a length-K fp32 chain: K 2^-24 sum|a||b|), none is fitted.
U24, U23 = 2.0 ** -24, 2.0 ** -23


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (float64 CPU tensors; a NaN in got fails); prints the worst ratio before it asserts."""
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= tol)
    ratio = (err / tol.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max().item() if err.numel() else 0.0
    print('%s: max err %.3e, worst err / tol %.3f' % (what, err.nan_to_num(nan=float('inf')).max().item(), ratio))
    assert not bad.any(), '%s: %d of %d outside the bound, worst err / tol %.3f' % (what, int(bad.sum()), bad.numel(), ratio)


UPSAMPLE_CASES = [
    # B, Hs, Ws, C1, C2
    (1, 1, 1, 4, 4),
    (2, 3, 5, 8, 12),            # rectangular
    (3, 13, 13, 256, 512),
    (40, 13, 13, 256, 512),      # 5.2 M float4 over 2048 workgroups of 256: ~10 grid-stride passes
    (40, 26, 26, 128, 256),
]


@pytest.mark.parametrize('B,Hs,Ws,C1,C2', UPSAMPLE_CASES)
def test_upsample_concat_forward_is_a_copy(ctx, B, Hs, Ws, C1, C2):
    from face_vijnana_yolov3_amd import ops
    src = _rand((B, Hs, Ws, C1), 101); skip = _rand((B, 2 * Hs, 2 * Ws, C2), 102)
    ref = torch.cat([src.repeat_interleave(2, 1).repeat_interleave(2, 2), skip], -1)
    out = ops.upsample_concat(ctx, src.cuda(), skip.cuda(), out=_nan((B, 2 * Hs, 2 * Ws, C1 + C2)))
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize('B,Hs,Ws,C1,C2', UPSAMPLE_CASES)
def test_upsample_concat_backward(ctx, B, Hs, Ws, C1, C2):
    """g_skip is a copy; g_up is bit-equal to (p + q) + (r + t) in fp32 (p, q the upper pixels of the 2x2 block, r, t the lower)
    and within 3 roundings of the float64 sum: 3 * 2^-24 * (|p| + |q| + |r| + |t|)."""
    from face_vijnana_yolov3_amd import ops
    g = _rand((B, 2 * Hs, 2 * Ws, C1 + C2), 103)
    g_up, g_skip = ops.upsample_concat_bwd(ctx, g.cuda(), C1, g_up=_nan((B, Hs, Ws, C1)), g_skip=_nan((B, 2 * Hs, 2 * Ws, C2)))
    assert torch.equal(g_skip.cpu(), g[..., C1:].contiguous())
    u = g[..., :C1]
    p, q, r, t = u[:, 0::2, 0::2], u[:, 0::2, 1::2], u[:, 1::2, 0::2], u[:, 1::2, 1::2]
    assert torch.equal(g_up.cpu(), (p + q) + (r + t))
    ref = p.double() + q.double() + r.double() + t.double()
    _within(g_up, ref, 3 * U24 * (p.double().abs() + q.double().abs() + r.double().abs() + t.double().abs()), 'g_up')


def test_upsample_concat_refuses_channels_not_divisible_by_four(ctx):
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import FvError
    for C1, C2 in [(6, 8), (8, 6)]:
        src = _rand((1, 2, 2, C1), 104).cuda(); skip = _rand((1, 4, 4, C2), 105).cuda()
        out = _nan((1, 4, 4, C1 + C2))
        with pytest.raises(FvError):
            ops.upsample_concat(ctx, src, skip, out=out)
        g_up, g_skip = _nan((1, 2, 2, C1)), _nan((1, 4, 4, C2))
        with pytest.raises(FvError):
            ops.upsample_concat_bwd(ctx, _rand((1, 4, 4, C1 + C2), 106).cuda(), C1, g_up=g_up, g_skip=g_skip)
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(g_up).all() and torch.isnan(g_skip).all()


@pytest.mark.parametrize('rows,C,cpad', [(1, 6, 32), (511, 27, 32), (513, 255, 256), (32768, 255, 256), (32769, 255, 256),
                                         (108160, 255, 256), (108160, 27, 32)])
def test_colsum_of_padded_rows(ctx, rows, C, cpad):
    """fv_ew_colsum_chunks: 1, 1, 2, 64 (exactly), 64 (capped), 64, 64 chunks; from 4097 rows on a thread takes more than one stride
    of 8 * chunks rows.  The padding columns hold 1e30 and must not reach the result.  Bound: an fp64 accumulation rounded to float
    once, 2^-24 |ref| + 1e-13 sum|column| (about 300 fp64 additions lie on the longest path of the two-stage sum: 3e-14)."""
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import lib
    assert lib().fv_colsum_partial_doubles(rows, C) == min(64, (rows + 511) // 512) * C
    dy = torch.full((rows, cpad), 1e30); dy[:, :C] = _rand((rows, C), 111, -1.0, 1.0) * _rand((1, C), 112, 0.0, 3.0)
    out = ops.colsum(ctx, dy.cuda(), C, out=_nan((C,)))
    d = dy[:, :C].double()
    ref = d.sum(0)
    _within(out, ref, U24 * ref.abs() + 1e-13 * d.abs().sum(0), 'colsum')


def _ref_yolo_loss(t, y, ncls, A):
    """The formula in elementwise.hip's comment, float64: per (cell, anchor) (bce(t4, y4) + mean_{k<4} |t_k - y_k| +
    mean_c bce(t_{5+c}, y_{5+c})) / 3 with bce(t, y) = max(t, 0) - t y + log1p(exp(-|t|)); mean over the boxes.  -> loss, its
    gradient d loss / d t.  sigmoid(t) - y is evaluated as (1 - y) - 1 / (1 + exp(t)) for t > 0 (no cancellation at y = 1)."""
    E = 5 + ncls
    t = t.double().view(-1, A, E); y = y.double().view(-1, A, E)
    nbox = t.shape[0] * A
    bce = t.clamp_min(0) - t * y + torch.log1p(torch.exp(-t.abs()))
    w = torch.full((E,), 1.0 / ncls, dtype=torch.float64); w[:4] = 0.25; w[4] = 1.0
    d = t[..., :4] - y[..., :4]
    per_box = (0.25 * d.abs().sum(-1) + bce[..., 4] + bce[..., 5:].sum(-1) / ncls) / 3.0
    sig_minus_y = torch.where(t > 0, (1.0 - y) - 1.0 / (1.0 + torch.exp(t.clamp_min(0))), 1.0 / (1.0 + torch.exp(-t.clamp_max(0))) - y)
    g = torch.cat([torch.sign(d), sig_minus_y[..., 4:]], -1) * w / (3.0 * nbox)
    return per_box.sum() / nbox, g.view(-1, A * E)


def _yolo_case(cells, ncls, A, seed):
    """Logits over a wide range with planted 0, +-1e-8, +-20, +-100, +-1e4; a tenth of the box entries equal their target;
    objectness / class targets exactly 0 or 1."""
    E = 5 + ncls
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand((cells, A, E), generator=g, dtype=torch.float64) * 16 - 8).float()
    y = torch.rand((cells, A, E), generator=g, dtype=torch.float64).float()
    y[..., 4:] = (torch.rand((cells, A, E - 4), generator=g) > 0.7).float()
    planted = torch.tensor([0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4])
    pick = torch.randint(0, 3 * len(planted), (cells, A, E), generator=g)
    t = torch.where(pick < len(planted), planted[pick.clamp_max(len(planted) - 1)], t)
    same = torch.rand((cells, A, 4), generator=g) < 0.1
    t[..., :4] = torch.where(same, y[..., :4], t[..., :4])
    return t.view(cells, A * E).contiguous(), y.view(cells, A * E).contiguous()


@pytest.mark.parametrize('cells3', [(1, 4, 16), (3 * 169, 3 * 676, 3 * 2704), (40 * 169, 40 * 676, 40 * 2704)])
@pytest.mark.parametrize('ncls,cpad', [(1, 32), (4, 32), (80, 256)])
def test_detection_loss_and_gradient(ctx, ncls, cpad, cells3):
    """yolo_loss_part x 3 + yolo_loss_finish.  E = 6, 9, 85 entries per box (85: a lane's second pass); at the production cell
    counts fv_ew_yolo_loss_blocks is capped at 1024 and a wave walks up to 80 boxes.  Loss within 2^-23 relative and dy within
    2^-23 |ref| + 1e-30 (fp64 throughout, one rounding to float); padding columns exactly 0; the gradient weight is a factor
    (a power of two scales every stored bit pattern exactly); two runs are bit-identical."""
    from face_vijnana_yolov3_amd import ops
    A, E = 3, 5 + ncls
    ts, ys = zip(*[_yolo_case(c, ncls, A, 120 + s) for s, c in enumerate(cells3)])
    td, yd = [t.cuda() for t in ts], [y.cuda() for y in ys]
    loss, dys = ops.yolo_loss_grad(ctx, td, yd, ncls, cpad, 1.0, A, dy3=[_nan((c, cpad)) for c in cells3])
    ref_loss = 0.0
    for s in range(3):
        l, g = _ref_yolo_loss(ts[s], ys[s], ncls, A)
        ref_loss += l.item()
        assert not torch.isnan(dys[s]).any()
        assert torch.count_nonzero(dys[s][:, A * E:]) == 0
        _within(dys[s][:, :A * E], g, U23 * g.abs() + 1e-30, 'dy, scale %d' % s)
    print('loss %.9g ref %.9g' % (loss.item(), ref_loss))
    assert abs(loss.item() - ref_loss) <= U23 * abs(ref_loss)
    loss2, dys2 = ops.yolo_loss_grad(ctx, td, yd, ncls, cpad, 1.0, A, dy3=[_nan((c, cpad)) for c in cells3])
    loss4, dys4 = ops.yolo_loss_grad(ctx, td, yd, ncls, cpad, 0.25, A, dy3=[_nan((c, cpad)) for c in cells3])
    assert torch.equal(loss, loss2) and torch.equal(loss, loss4)
    for s in range(3):
        assert torch.equal(dys[s], dys2[s])
        # exact in float's normal range; below it (sigmoid(-100) / (3 nbox) ~ 1e-45) a quarter of a subnormal is not representable
        a1, a4 = dys[s].cpu(), dys4[s].cpu()
        normal = a1.abs() >= 2.0 ** -100
        assert torch.equal(a1[normal] * 0.25, a4[normal]) and (a4[~normal].abs() <= 2.0 ** -100).all()


def _l2n_relu64(pre):
    """u = l2_normalize(relu(pre)) in float64 (TF 1.13: x * rsqrt(max(sum x^2, 1e-12)))."""
    r = pre.double().clamp_min(0)
    return r / torch.sqrt((r * r).sum(-1, keepdim=True).clamp_min(1e-12))


def _triplet_case(B, seed):
    """pre [3B][64] (rows b anchor, B + b positive, 2B + b negative) with triplet b built by kind b % 5; -> pre, kinds."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64) * 2 - 0.6     # ~30 % negative pre-activations
    pre = torch.zeros((3 * B, 64), dtype=torch.float64)
    lo, hi = slice(0, 32), slice(32, 64)
    for b in range(B):
        a = rnd(64)
        near = a + 0.02 * (torch.rand(64, generator=g, dtype=torch.float64) - 0.5)
        far_a, far_o = -torch.ones(64, dtype=torch.float64) * 0.3, -torch.ones(64, dtype=torch.float64) * 0.3
        k = b % 5
        if k == 3:      # disjoint supports: distance sqrt(2)
            far_a[lo] = a[lo].abs() + 0.1; far_o[hi] = rnd(32).abs() + 0.1
        else:           # supports [0, 48) and [16, 64): distance ~1.  They overlap, so that no gradient row is parallel to its own u:
                        # such a row is projected to exactly 0, and what fp64 leaves of it is rounding noise in reference and kernel alike
            far_a[:48] = a[:48].abs() + 0.1; far_o[16:] = rnd(48).abs() + 0.1
        if k == 0:      # hinge active: positive far, negative near
            pre[b], pre[B + b], pre[2 * B + b] = far_a, far_o, far_a + 0.02 * (torch.rand(64, generator=g, dtype=torch.float64) - 0.5) * (far_a > 0)
        elif k == 1:    # hinge inactive by a clear margin: positive near, negative far
            pre[b], pre[B + b], pre[2 * B + b] = far_a, far_a + 0.02 * (torch.rand(64, generator=g, dtype=torch.float64) - 0.5) * (far_a > 0), far_o
        elif k == 2:    # positive row EQUALS the anchor row: distance exactly 0; negative near -> hinge active through -|a - n| alone
            pre[b], pre[B + b], pre[2 * B + b] = a, a, near
        elif k == 3:    # dead negative row (every pre <= 0, one exactly 0): u = 0, |a - n| = 1; positive far -> active
            dead = -rnd(64).abs(); dead[7] = 0.0
            pre[b], pre[B + b], pre[2 * B + b] = far_a, far_o, dead
        else:           # positive row with entries ~1e-8: 0 < sum relu^2 <= 1e-12, the constant-factor branch; negative near
            pre[b], pre[B + b], pre[2 * B + b] = a, rnd(64) * 1e-8, near
    return pre.float(), [b % 5 for b in range(B)]


def _ref_triplet(pre, u, B, weight):
    """fid.hip's formulas in float64, written out (autograd through sqrt at 0 gives NaN): u is given, as the kernel's argument."""
    pre, u = pre.double(), u.double()
    ua, up, un = u[:B], u[B:2 * B], u[2 * B:]
    dap, dan = ua - up, ua - un
    dp, dn = dap.pow(2).sum(-1).sqrt(), dan.pow(2).sum(-1).sqrt()
    h = dp - dn + 0.2
    loss = h.clamp_min(0).sum() / B
    act = (h >= 0).double()
    cp = torch.where(dp > 0, 1.0 / (B * dp.clamp_min(1e-300)), torch.zeros_like(dp)) * act
    cn = torch.where(dn > 0, 1.0 / (B * dn.clamp_min(1e-300)), torch.zeros_like(dn)) * act
    du = torch.cat([cp[:, None] * dap - cn[:, None] * dan, -cp[:, None] * dap, cn[:, None] * dan])
    r = pre.clamp_min(0)
    ss = (r * r).sum(-1, keepdim=True)
    s = 1.0 / ss.clamp_min(1e-300).sqrt()
    uu = r * s
    dr = torch.where(ss > 1e-12, s * (du - uu * (uu * du).sum(-1, keepdim=True)), du * 1e6)
    dE = torch.where(pre > 0, dr * weight, torch.zeros_like(dr))
    return loss, dE, h, ss[:, 0]


@pytest.mark.parametrize('B', [1, 3, 4, 5, 8, 11, 43, 96])
def test_fid_triplet_loss_and_gradient(ctx, B):
    """fid_triplet_kernel + l2_relu_bwd on a `pre` array built directly; u = float32(l2_normalize(relu(pre))) computed in float64
    from the same pre and then treated as given, as the kernel treats its two arguments.  A wave takes the triplets w, w + 4, ...:
    B = 1, 3 leave waves idle, B >= 5 runs the loop more than once, 43 and 96 unevenly / evenly many times.  Triplet b is of kind
    b % 5 (B = 1 has kind 0 only, B >= 5 all five):
      0  hinge active (h > 0.05): all three rows get gradient
      1  hinge inactive (h < -0.05): its three dE rows are exactly 0 and it adds nothing to the loss
      2  positive row == anchor row: |a - p| is exactly 0, that term's gradient is 0 (not NaN); active through the negative alone
      3  negative row has every pre <= 0: a dead row, u = 0, its dE row is exactly 0; the triplet is active
      4  positive row has entries ~1e-8: 0 < sum relu(pre)^2 <= 1e-12, l2_relu_bwd's constant-factor branch (dr = du * 1e6)
    These are asserted on the CPU before the kernel runs.  Bounds: loss 2^-23 relative; dE 2^-23 |ref| + 1e-12 max|ref|; dbias
    3B 2^-24 sum|dE column| + 2^-23 |ref|.  The gradient weight is a factor: 0.25 scales every stored bit pattern exactly."""
    from face_vijnana_yolov3_amd import ops
    pre, kinds = _triplet_case(B, 130 + B)
    u = _l2n_relu64(pre).float()
    ref_loss, ref_dE, h, ss = _ref_triplet(pre, u, B, 1.0)
    dp = (u[:B].double() - u[B:2 * B].double()).pow(2).sum(-1).sqrt()
    for b, k in enumerate(kinds):
        if k == 1:
            assert h[b] < -0.05
        else:
            assert h[b] > 0.05
        if k == 2:
            assert torch.equal(pre[b], pre[B + b]) and dp[b] == 0.0
        else:
            assert dp[b] > 0.0
        if k == 3:
            assert (pre[2 * B + b] <= 0).all() and ss[2 * B + b] == 0.0
        if k == 4:
            assert 0.0 < ss[B + b] <= 1e-12 and (pre[B + b] > 0).any()
        assert ss[b] > 1e-3
    assert torch.isfinite(ref_dE).all()
    loss, dE, db = ops.fid_triplet_loss_grad(ctx, pre.cuda(), u.cuda(), 1.0, dE=_nan((3 * B, 64)), dbias=_nan((64,)))
    print('loss %.9g ref %.9g' % (loss.item(), ref_loss.item()))
    assert abs(loss.item() - ref_loss.item()) <= U23 * abs(ref_loss.item())
    _within(dE, ref_dE, U23 * ref_dE.abs() + 1e-12 * ref_dE.abs().max(), 'dE')
    dEc = dE.cpu()
    for b, k in enumerate(kinds):
        if k == 1:
            assert torch.count_nonzero(dEc[[b, B + b, 2 * B + b]]) == 0
        if k == 3:
            assert torch.count_nonzero(dEc[2 * B + b]) == 0
        if k == 2:   # the positive's only gradient would come from the zero distance
            assert torch.count_nonzero(dEc[B + b]) == 0
    ref_db = ref_dE.sum(0)
    _within(db, ref_db, 3 * B * U24 * ref_dE.abs().sum(0) + U23 * ref_db.abs(), 'dbias')
    loss4, dE4, db4 = ops.fid_triplet_loss_grad(ctx, pre.cuda(), u.cuda(), 0.25, dE=_nan((3 * B, 64)), dbias=_nan((64,)))
    assert torch.equal(loss4, loss) and torch.equal(dE4, dE * 0.25) and torch.equal(db4, db * 0.25)


def _dense_case(per, F, seed):
    """Three separately allocated tower buffers [per][F], the dense kernel [F][64], bias, dE [3 per][64]."""
    towers = [_rand((per, F), seed + i) for i in range(3)]
    w = _rand((F, 64), seed + 3, -0.05, 0.05); bias = _rand((64,), seed + 4, -0.5, 0.5); dE = _rand((3 * per, 64), seed + 5)
    return towers, w, bias, dE


DENSE_CASES = [(1, 4096), (5, 4096), (11, 4096), (22, 4096), (43, 4096), (96, 4096), (2, 173056), (96, 173056)]


@pytest.mark.parametrize('per,F', DENSE_CASES)
def test_fid_dense_forward_over_three_towers(ctx, per, F):
    """fid_dense_fwd_kernel + fid_dense_finish_kernel over the FidRows fv_fid_train_step builds: per not a multiple of 32 puts a
    32-row block across two (three) towers' buffers.  pre: each chunk's 256 products go through fp32 chains (four of 64, added in
    lane order), the chunks are summed in fp64, then one rounding and the fp32 bias add -- inside the worst-case bound of a
    length-256 chain, 256 2^-24 (|x| . |w| + |bias|) + 1e-30.  u against float64 l2_normalize(relu(.)) of the pre the kernel stored:
    fp64 arithmetic rounded once, 2^-24 |ref| + 1e-13.  Row independence (fid.hip's header): the same rows as ONE buffer of 3 per rows
    give the same bits, and a row on its own gives the same bits as inside the batch."""
    from face_vijnana_yolov3_amd import ops
    towers, w, bias, _ = _dense_case(per, F, 140)
    M = 3 * per
    td = [t.cuda() for t in towers]; wd, bd = w.cuda(), bias.cuda()
    pre, u = ops.fid_towers_dense_l2(ctx, td, M, wd, bd, pre=_nan((M, 64)), out=_nan((M, 64)))
    X = torch.cat(towers).double()
    ref = X @ w.double() + bias.double()
    bound = X.abs() @ w.double().abs() + bias.double().abs()
    _within(pre, ref, 256 * U24 * bound + 1e-30, 'pre')
    ref_u = _l2n_relu64(pre.cpu())
    _within(u, ref_u, U24 * ref_u.abs() + 1e-13, 'u')
    one = torch.cat(td)
    pre1, u1 = ops.fid_towers_dense_l2(ctx, [one], M, wd, bd, pre=_nan((M, 64)), out=_nan((M, 64)))
    assert torch.equal(pre1, pre) and torch.equal(u1, u)
    m = M - 1   # the last row of the third tower, alone
    pre_m, u_m = ops.fid_towers_dense_l2(ctx, [td[2][per - 1:].contiguous()], 1, wd, bd, pre=_nan((1, 64)), out=_nan((1, 64)))
    assert torch.equal(pre_m[0], pre[m]) and torch.equal(u_m[0], u[m])


@pytest.mark.parametrize('per,F', DENSE_CASES)
def test_fid_dense_data_gradient_over_three_towers(ctx, per, F):
    """fid_dense_dgrad_kernel: M = 66 ... 288 rows run the 64-row LDS tile loop more than once.  Each element is one fp32 chain over
    the 64 columns: 64 2^-24 (|dE| . |w|^T) + 1e-30.  Writing into three tower buffers or one buffer of 3 per rows: same bits."""
    from face_vijnana_yolov3_amd import ops
    _, w, _, dE = _dense_case(per, F, 150)
    M = 3 * per
    dx = [_nan((per, F)) for _ in range(3)]
    ops.fid_towers_dense_dgrad(ctx, dE.cuda(), w.cuda(), dx, M)
    one = _nan((M, F))
    ops.fid_towers_dense_dgrad(ctx, dE.cuda(), w.cuda(), [one], M)
    got = torch.cat(dx)
    assert torch.equal(got, one)
    del one
    ref = dE.double() @ w.double().t()
    bound = dE.double().abs() @ w.double().abs().t()
    _within(got, ref, 64 * U24 * bound + 1e-30, 'dX')


@pytest.mark.parametrize('per,F', DENSE_CASES)
def test_fid_dense_weight_gradient_over_three_towers(ctx, per, F):
    """fid_dense_wgrad_kernel: M = 33 has a ragged second 32-row tile, M = 288 nine whole ones; rows come from three buffers.  Each
    element is one fp32 chain over the M rows: M 2^-24 (|X|^T . |dE|) + 1e-30.  Three towers or one buffer: same bits."""
    from face_vijnana_yolov3_amd import ops
    towers, _, _, dE = _dense_case(per, F, 160)
    M = 3 * per
    td = [t.cuda() for t in towers]
    dw = ops.fid_towers_dense_wgrad(ctx, td, dE.cuda(), M, F, dw=_nan((F, 64)))
    dw1 = ops.fid_towers_dense_wgrad(ctx, [torch.cat(td)], dE.cuda(), M, F, dw=_nan((F, 64)))
    assert torch.equal(dw, dw1)
    X = torch.cat(towers).double()
    ref = X.t() @ dE.double()
    bound = X.abs().t() @ dE.double().abs()
    _within(dw, ref, M * U24 * bound + 1e-30, 'dW')


def test_fid_dense_operators_refuse_bad_rows(ctx):
    """F not a multiple of 256, M > 3 per, and a NULL tower that M reaches: an error, and nothing is written."""
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import FvError
    per, F = 2, 512
    towers, w, bias, dE = _dense_case(per, F, 170)
    td = [t.cuda() for t in towers]; wd, bd, dEd = w.cuda(), bias.cuda(), dE.cuda()
    bad_F = 300
    cases = [
        # towers, M, F-sized kernel
        ([t[:, :bad_F].contiguous() for t in td], 3 * per, wd[:bad_F].contiguous()),
        (td, 3 * per + 1, wd),
        ([td[0], None, td[2]], 2 * per + 1, wd),
        ([td[0], td[1]], 2 * per + 1, wd),
    ]
    for tw, M, wk in cases:
        Fk = wk.shape[0]
        pre, u = _nan((M, 64)), _nan((M, 64))
        with pytest.raises(FvError):
            ops.fid_towers_dense_l2(ctx, tw, M, wk, bd, pre=pre, out=u)
        dw = _nan((Fk, 64))
        with pytest.raises(FvError):
            ops.fid_towers_dense_wgrad(ctx, tw, torch.zeros((M, 64), device='cuda'), M, Fk, dw=dw)
        dx = [None if t is None else _nan(tuple(t.shape)) for t in tw]
        with pytest.raises(FvError):
            ops.fid_towers_dense_dgrad(ctx, torch.zeros((M, 64), device='cuda'), wk, dx, M)
        torch.cuda.synchronize()
        assert torch.isnan(pre).all() and torch.isnan(u).all() and torch.isnan(dw).all()
        assert all(torch.isnan(t).all() for t in dx if t is not None)
    # a tower that M does not reach may be NULL
    pre, u = ops.fid_towers_dense_l2(ctx, [td[0], td[1], None], 2 * per, wd, bd, pre=_nan((2 * per, 64)), out=_nan((2 * per, 64)))
    assert torch.isfinite(pre).all() and torch.isfinite(u).all()
