"""Option "early_bn_fused": the BN passes of the first layers folded into their halo-kernel consumers.

  * conv9_mfma.hip / wgrad9_mfma.hip (conv_1, conv_3: 3x3, 32 -> 64 channels) read the producer's raw conv output z and
    apply scale/shift + LeakyReLU while staging it, so a(0) / a(2) are never written;
  * wgrad0_mfma.hip (first layer) forms dz from g and z while staging them, so dz(0) is never written.

Each fused operator is compared with the two-launch form it replaces ON THE SAME DATA.  The per-element expressions are
shared device code (csrc/elementwise.h) and the library is built with -ffp-contract=off: the forward's z is bit-identical,
d-beta / d-gamma are bit-identical, weight-gradients agree to their float-atomic summation order (the bound the
wgrad-kernel pairs of test_ops_gpu.py use: 2e-5 of the largest entry).

The inputs have both signs of z*scale+shift well represented and |beta| >= 0.5: a padding slot that received
LeakyReLU(shift) instead of 0.0 changes every border output by >= 0.05 |w|, far above either bound.  No output side is a
multiple of the unit, and every case runs with more units than workgroups (the prefetch / stage loop) and with fewer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LEAKY = 0.1


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


_CACHE = {}


def _producer(ctx, B, s):
    """z_in of the producing layer (output of the consumer is 40 x 56), its activation through bn_act_slots (the pass the
    fused form drops) with the published scale / shift, the consumer's weights and an output gradient.  Made once per case."""
    key = (B, s)
    if key not in _CACHE:
        from face_vijnana_yolov3_amd import ops
        H, W = 40 * s, 56 * s
        z_in = _rand((B, H, W, 32), 11 + s, -2.0, 2.0).cuda()
        gamma = _rand((32,), 21, 0.5, 1.5).cuda()
        bsign = torch.where(_rand((32,), 22) > 0, 1.0, -1.0)
        beta = (bsign * _rand((32,), 23, 0.5, 1.0)).cuda()                    # |beta| >= 0.5, both signs
        slots = ops.stat_slots(32, 'cuda')
        zc = z_in.double().view(-1, 32)
        slots[0, 0] = zc.sum(0); slots[0, 1] = (zc * zc).sum(0)
        a, mean, invstd, scale, shift = ops.bn_act_slots(ctx, z_in, slots, gamma, beta)
        pre = z_in * scale + shift
        frac = (pre > 0).float().mean().item()
        assert 0.25 < frac < 0.75 and shift.abs().min().item() >= 0.4, (frac, shift.abs().min().item())
        w = _rand((64, 3, 3, 32), 31, -0.2, 0.2).cuda()
        dy = _rand((B, 40, 56, 64), 41).cuda()
        _CACHE[key] = (z_in, a, scale, shift, w, dy)
    return _CACHE[key]


CASES = [(14, 1), (14, 2), (1, 1), (1, 2)]   # B = 14: 280 units > 256 workgroups; B = 1: 20 units


@pytest.mark.parametrize('B,s', CASES)
def test_forward_from_z_is_bit_identical(ctx, B, s):
    from face_vijnana_yolov3_amd import ops
    z_in, a, scale, shift, w, _ = _producer(ctx, B, s)
    sl0 = ops.stat_slots(64, 'cuda')
    z0 = ops.conv2d_forward_slots(ctx, a, w, s, sl0)
    sl1 = ops.stat_slots(64, 'cuda')
    z1 = ops.conv2d_forward_slots_bn_in(ctx, z_in, scale, shift, w, s, sl1)
    assert z1.shape == (B, 40, 56, 64)
    assert torch.equal(z1, z0)
    # the slot totals: the comparison test_halo_forward_is_bit_identical_to_the_tile_kernel makes
    zc = z0.double().view(-1, 64)
    s1, s0 = sl1.sum(0).cpu(), sl0.sum(0).cpu()
    assert ((s1[0] - zc.sum(0).cpu()).abs() <= 1e-6 * zc.abs().sum(0).cpu() + 1e-9).all()
    assert ((s1[1] - (zc * zc).sum(0).cpu()).abs() <= 1e-6 * (zc * zc).sum(0).cpu() + 1e-9).all()
    assert ((s1 - s0).abs() <= 2e-5 * s0.abs() + 1e-5).all()


@pytest.mark.parametrize('B,s', CASES)
def test_wgrad_from_z_equals_wgrad_of_the_activation(ctx, B, s):
    from face_vijnana_yolov3_amd import ops
    z_in, a, scale, shift, _, dy = _producer(ctx, B, s)
    ref = ops.conv2d_wgrad(ctx, a, dy, 64, 3, s)
    got = ops.conv2d_wgrad_bn_in(ctx, z_in, scale, shift, dy, 64, 3, s)
    d, m = (got - ref).abs().max().item(), ref.abs().max().item()
    print('wgrad from z: max diff %.3e of %.3e' % (d, m))
    assert d <= 2e-5 * m, (B, s, d, m)


@pytest.mark.parametrize('B', [22, 1])   # 72 x 112: 36 units per image; B = 22: 792 units > 768 workgroups
def test_first_layer_wgrad_with_bn_backward(ctx, B):
    from face_vijnana_yolov3_amd import ops
    H, W, C = 72, 112, 32
    x = _rand((B, H, W, 3), 51, 0.0, 1.0).cuda()
    g = _rand((B, H, W, C), 52).cuda()
    z = _rand((B, H, W, C), 53, -2.0, 2.0).cuda()
    scale = _rand((C,), 54, 0.5, 1.5).cuda()
    shift = (torch.where(_rand((C,), 55) > 0, 1.0, -1.0) * _rand((C,), 56, 0.5, 1.0)).cuda()
    mean = _rand((C,), 57, -0.3, 0.3).cuda(); invstd = _rand((C,), 58, 0.5, 2.0).cuda()
    # slots as a finished reduction would leave them: d-beta / rows and d-gamma / rows of order 0.3, so that a pixel beyond the
    # lattice staged through the formula (instead of as 0.0) would carry -scale * 0.3 into the products
    rows = B * H * W
    slots = ops.stat_slots(C, 'cuda')
    gs = torch.Generator().manual_seed(59)
    slots.copy_((torch.rand(slots.shape, generator=gs, dtype=torch.float64) - 0.3) * 0.6 * rows / slots.shape[0])
    dz, dg0, db0 = ops.bn_bwd_slots(ctx, g, z, scale, shift, mean, invstd, slots, True)
    assert (db0.abs() / rows).max().item() > 0.05
    ref = ops.conv2d_wgrad(ctx, x, dz, C, 3, 1)
    got, dg1, db1 = ops.conv2d_wgrad_bn_bwd(ctx, x, g, z, scale, shift, mean, invstd, slots)
    assert torch.equal(db1, db0) and torch.equal(dg1, dg0)
    d, m = (got - ref).abs().max().item(), ref.abs().max().item()
    print('wgrad0 + BN backward: max diff %.3e of %.3e' % (d, m))
    assert d <= 2e-5 * m, (B, d, m)
    # accumulate: the slot sums are added to what the outputs hold (a BN layer shared by several towers of one step)
    pb, pg = _rand((C,), 60, -5.0, 5.0).cuda(), _rand((C,), 61, -5.0, 5.0).cuda()
    got2, dg2, db2 = ops.conv2d_wgrad_bn_bwd(ctx, x, g, z, scale, shift, mean, invstd, slots, dbeta=pb.clone(), dgamma=pg.clone())
    assert torch.equal(db2, pb + db0) and torch.equal(dg2, pg + dg0)
    assert (got2 - ref).abs().max().item() <= 2e-5 * m


def test_shapes_the_halo_kernels_do_not_take_are_refused(ctx):
    """There is no second implementation of the modes: another shape (or the halo kernel switched off) is an error."""
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import FvError
    z64 = _rand((1, 8, 16, 64), 71).cuda(); v64 = _rand((64,), 72).cuda()
    with pytest.raises(FvError):
        ops.conv2d_forward_slots_bn_in(ctx, z64, v64, v64, _rand((64, 3, 3, 64), 73).cuda(), 1, ops.stat_slots(64, 'cuda'))
    with pytest.raises(FvError):
        ops.conv2d_wgrad_bn_in(ctx, z64, v64, v64, _rand((1, 8, 16, 64), 74).cuda(), 64, 3, 1)
    z32 = _rand((1, 8, 16, 32), 75).cuda(); v32 = _rand((32,), 76).cuda()
    ctx.set_conv_halo(False)
    try:
        with pytest.raises(FvError):
            ops.conv2d_forward_slots_bn_in(ctx, z32, v32, v32, _rand((64, 3, 3, 32), 77).cuda(), 1, ops.stat_slots(64, 'cuda'))
    finally:
        ctx.set_conv_halo(True)
    ctx.set_wgrad_fused_taps(False)
    try:
        with pytest.raises(FvError):
            ops.conv2d_wgrad_bn_in(ctx, z32, v32, v32, _rand((1, 8, 16, 64), 78).cuda(), 64, 3, 1)
        with pytest.raises(FvError):
            ops.conv2d_wgrad_bn_bwd(ctx, _rand((1, 8, 32, 3), 79).cuda(), _rand((1, 8, 32, 32), 80).cuda(), _rand((1, 8, 32, 32), 81).cuda(),
                                    v32, v32, v32, v32, ops.stat_slots(32, 'cuda'))
    finally:
        ctx.set_wgrad_fused_taps(True)


def test_option_default_and_parts(ctx):
    from face_vijnana_yolov3_amd._lib import FvError
    assert ctx.get_option('early_bn_fused') == 1
    try:
        for v in (0, 2, 4, 8, 6, 1):
            ctx.set_option('early_bn_fused', v); assert ctx.get_option('early_bn_fused') == v
        ctx.set_option('early_bn_fused', 14); assert ctx.get_option('early_bn_fused') == 1     # all three parts = on
        for bad in (3, 16, -1):
            with pytest.raises(FvError):
                ctx.set_option('early_bn_fused', bad)
    finally:
        ctx.set_option('early_bn_fused', 1)


def test_train_step_with_and_without_the_option():
    """One fv_train_step at 2 x 96^2 from the same state, option 1 against option 0: the loss and z of layers 1 and 3 (the
    consumers of the two activations that are no longer written) agree to 1e-6 relative -- the fp64 slot atomics may move a
    statistic's last bit between any two runs -- and all gradients within the bound test_side_stream_overlap_equals_serial
    applies to two orders of the float atomics."""
    from face_vijnana_yolov3_amd.engine import Engine
    from oracle import net_oracle as no
    eng = Engine(0)
    assert eng.ctx.get_option('early_bn_fused') == 1
    B, S = 2, 96
    p, st = no.init_params(29, torch.float32)
    g = torch.Generator().manual_seed(30)
    ents, _, _ = no.param_layout()
    for e in ents:
        if e['has_bn']:
            c = e['cout']
            p[e['gamma_off']:e['gamma_off'] + c] = 0.8 + 0.4 * torch.rand(c, generator=g)
            p[e['beta_off']:e['beta_off'] + c] = torch.where(torch.rand(c, generator=g) > 0.5, 1.0, -1.0) * (0.5 + 0.3 * torch.rand(c, generator=g))
    x = torch.rand((B, S, S, 3), generator=g); yt = torch.rand((B, S // 32, S // 32, 6), generator=g)
    res = {}
    try:
        for on in (1, 0):
            eng.ctx.set_option('early_bn_fused', on)
            eng.set_params(p, st)
            eng.m = eng.v = eng.grads = None
            buckets = []
            loss = eng.forward_backward(x, yt, on_bucket=lambda o, c: buckets.append((o, c)))
            torch.cuda.synchronize()
            res[on] = (loss.item(), eng.grads.clone(), eng.train_tensor(B, S, 1, 'z').clone(), eng.train_tensor(B, S, 3, 'z').clone(),
                       eng.state.clone(), buckets)
    finally:
        eng.ctx.set_option('early_bn_fused', 1)
    assert abs(res[1][0] - res[0][0]) <= 1e-6 * abs(res[0][0]), (res[1][0], res[0][0])
    for i in (2, 3):
        m = res[0][i].abs().max().item()
        d = (res[1][i] - res[0][i]).abs().max().item()
        print('z: max diff %.3e of %.3e' % (d, m))
        assert d <= 1e-6 * m, (i, d, m)
    torch.testing.assert_close(res[1][4], res[0][4], rtol=1e-6, atol=1e-7)     # moving statistics: the publish launch updates them as the pass does
    assert res[1][5] == res[0][5]                                              # same ranges in the same order
    d = (res[1][1] - res[0][1]).abs().max().item()
    print('grads: max diff %.3e of %.3e' % (d, res[0][1].abs().max().item()))
    assert d <= 1e-5 * res[0][1].abs().max().item() + 1e-9, d
