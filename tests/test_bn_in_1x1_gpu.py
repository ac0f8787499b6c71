"""Option "bn_in_1x1": the normalise pass of the layer in front of a residual block's first 1x1 conv, inside that conv.

conv1x1_mfma.hip sums the producing layer's statistics slots, publishes mean / invstd / scale / shift and the moving statistics,
forms a = LeakyReLU(z * scale + shift) (+ skip) while it stages z as its A operand, writes a once (the workgroups of N tile 0)
and multiplies.  The prologue and the per-element expression are the device code of bn_act_stats_kernel (csrc/elementwise.h) and
the K step / epilogue are those of the plain kernel, so everything is compared for EQUALITY with fv_bn_act_slots followed by
fv_conv2d_forward_slots on the same slots -- except the consumer's own fp64 statistics slots, whose atomics may add in another
order (1e-12 relative).

Shapes: 169 rows = two M tiles with a ragged last one; Cin 32 / 64 / 96 = 1 / 2 / 3 K steps (both ends of the operand double
buffer); Cout 64 (64-wide tile), 128 and 256 (two N tiles, only the first writes a); with and without skip; and one launch with
515 tiles on 512 workgroups, in which a workgroup takes a second tile.  |beta| >= 0.5 with both signs: a row beyond M staged
through the formula instead of as 0.0 would put LeakyReLU(shift) into the consumer's statistics."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096           # floats behind a(l)
SENTINEL = -12345.5


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _case(ctx, B, H, W, cin, cout, with_skip):
    """Both paths on one set of slots.  Returns (fused, reference): dicts of tensors."""
    from face_vijnana_yolov3_amd import ops
    z_in = _rand((B, H, W, cin), 100 + cin, -2.0, 2.0).cuda()
    skip = _rand((B, H, W, cin), 200 + cin).cuda() if with_skip else None
    gamma = _rand((cin,), 21, 0.5, 1.5).cuda()
    beta = (torch.where(_rand((cin,), 22) > 0, 1.0, -1.0) * _rand((cin,), 23, 0.5, 1.0)).cuda()
    w = _rand((cout, 1, 1, cin), 31, -0.2, 0.2).cuda()
    # the slots as the producing conv's epilogue leaves them: the column sums spread over the slots
    in_slots = ops.stat_slots(cin, 'cuda')
    ns = in_slots.shape[0]
    zc = z_in.double().view(-1, cin)
    parts = zc.chunk(ns, 0)
    for k, part in enumerate(parts):
        in_slots[k, 0] = part.sum(0); in_slots[k, 1] = (part * part).sum(0)
    mm0, mv0 = _rand((cin,), 41, -0.2, 0.2).cuda(), _rand((cin,), 42, 0.5, 1.5).cuda()

    mm_r, mv_r = mm0.clone(), mv0.clone()
    a_r, mean_r, invstd_r, scale_r, shift_r = ops.bn_act_slots(ctx, z_in, in_slots, gamma, beta, 1e-3, 0.99, mm_r, mv_r, skip)
    sl_r = ops.stat_slots(cout, 'cuda')
    z_r = ops.conv2d_forward_slots(ctx, a_r, w, 1, sl_r)

    mm_f, mv_f = mm0.clone(), mv0.clone()
    buf = torch.full((z_in.numel() + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    a_f = buf[:z_in.numel()].view(z_in.shape)
    sl_f = ops.stat_slots(cout, 'cuda')
    z_f, _, mean_f, invstd_f, scale_f, shift_f = ops.conv2d_forward_slots_bn_stats_in(ctx, z_in, in_slots, gamma, beta, w, sl_f, 1e-3, 0.99,
                                                                                      mm_f, mv_f, skip, a_out=a_f)
    torch.cuda.synchronize()
    pre = z_in * scale_r + shift_r
    frac = (pre > 0).float().mean().item()
    assert 0.2 < frac < 0.8 and shift_r.abs().min().item() >= 0.05, (frac, shift_r.abs().min().item())
    fused = dict(a=a_f, z=z_f, mean=mean_f, invstd=invstd_f, scale=scale_f, shift=shift_f, mm=mm_f, mv=mv_f, slots=sl_f, guard=buf[z_in.numel():])
    ref = dict(a=a_r, z=z_r, mean=mean_r, invstd=invstd_r, scale=scale_r, shift=shift_r, mm=mm_r, mv=mv_r, slots=sl_r)
    return fused, ref


def _check(fused, ref):
    for k in ('mean', 'invstd', 'scale', 'shift', 'mm', 'mv', 'a', 'z'):
        assert torch.equal(fused[k], ref[k]), (k, (fused[k] - ref[k]).abs().max().item())
    s1, s0 = fused['slots'], ref['slots']
    d = (s1 - s0).abs()
    print('consumer slots: max relative difference %.3e' % (d / s0.abs().clamp_min(1e-300)).max().item())
    assert (d <= 1e-12 * s0.abs()).all()
    assert (fused['guard'] == SENTINEL).all()          # nothing is written behind row M - 1 of a(l)


@pytest.mark.parametrize('with_skip', [False, True])
@pytest.mark.parametrize('cout', [64, 128, 256])
@pytest.mark.parametrize('cin', [32, 64, 96])
def test_fused_launch_equals_pass_plus_conv(ctx, cin, cout, with_skip):
    _check(*_case(ctx, 1, 13, 13, cin, cout, with_skip))


@pytest.mark.parametrize('with_skip', [False, True])
def test_a_workgroup_takes_a_second_tile(ctx, with_skip):
    # 2 x 182 x 181 = 65 884 rows = 515 M tiles (the last one with 92 rows) of one N tile on 512 workgroups; 8 MB per tensor
    _check(*_case(ctx, 2, 182, 181, 32, 64, with_skip))


def test_shapes_the_kernel_does_not_take_are_refused(ctx):
    """The mode exists in one kernel: another shape, or that kernel switched off, is an error and never the two launches."""
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import FvError

    def call(cin, cout):
        z = _rand((1, 8, 8, cin), 71).cuda()
        return ops.conv2d_forward_slots_bn_stats_in(ctx, z, ops.stat_slots(cin, 'cuda'), _rand((cin,), 72).cuda(), _rand((cin,), 73).cuda(),
                                                    _rand((cout, 1, 1, cin), 74).cuda(), ops.stat_slots(cout, 'cuda'))
    with pytest.raises(FvError):
        call(64, 32)           # 32 output channels: the 32-wide tile kernel has no such mode
    with pytest.raises(FvError):
        call(1024, 512)        # scale / shift of 1024 channels do not fit next to two workgroups' operand buffers
    ctx.set_option('conv1x1_persist', 0)
    try:
        with pytest.raises(FvError):
            call(64, 64)
    finally:
        ctx.set_option('conv1x1_persist', 1)
    call(64, 64)


def test_option_default_and_values(ctx):
    from face_vijnana_yolov3_amd._lib import FvError
    assert ctx.get_option('bn_in_1x1') == 1
    try:
        for v in (0, 2, 1):
            ctx.set_option('bn_in_1x1', v); assert ctx.get_option('bn_in_1x1') == v
        for bad in (3, -1):
            with pytest.raises(FvError):
                ctx.set_option('bn_in_1x1', bad)
    finally:
        ctx.set_option('bn_in_1x1', 1)


def _bn_params(p, ents, seed):
    g = torch.Generator().manual_seed(seed)
    for e in ents:
        if e['has_bn']:
            c = e['cout']
            p[e['gamma_off']:e['gamma_off'] + c] = 0.8 + 0.4 * torch.rand(c, generator=g)
            p[e['beta_off']:e['beta_off'] + c] = torch.where(torch.rand(c, generator=g) > 0.5, 1.0, -1.0) * (0.5 + 0.3 * torch.rand(c, generator=g))


def _step_compare(model, run, layers, B, S):
    """run() -> loss after one forward_backward from the same state.  Option 0 twice (the spread of the float-atomic gradients),
    then 1 (the shape classes that measured faster: none of them occurs at this size, so the parent's launches) and 2 (every
    launch the kernel takes: here all residual blocks with at most 512 input channels)."""
    res = {}
    try:
        for key, opt in (('off', 0), ('off2', 0), ('on', 1), ('all', 2)):
            model.ctx.set_option('bn_in_1x1', opt)
            loss = run()
            torch.cuda.synchronize()
            # z, a, mean, invstd, scale, shift of every BN layer (a(0) and a(2) are never written under early_bn_fused)
            kept = [model._train_tensor(B, S, l, code).clone() for l in layers for code in range(6) if not (code == 1 and l in (0, 2))]
            res[key] = (loss.item(), kept, model.state.clone(), model.grads.clone())
    finally:
        model.ctx.set_option('bn_in_1x1', 1)
    g0 = res['off'][3]
    idx = torch.arange(0, g0.numel(), 97, device=g0.device)       # sampled gradients
    spread = (res['off2'][3][idx] - g0[idx]).abs().max().item()
    scale = g0[idx].abs().max().item()
    print('gradient spread of two runs with the option off: %.3e of %.3e' % (spread, scale))
    for key in ('on', 'all'):
        assert res[key][0] == res['off'][0], (key, res[key][0], res['off'][0])
        for i, (t1, t0) in enumerate(zip(res[key][1], res['off'][1])):
            assert torch.equal(t1, t0), (key, 'kept tensor', i, (t1 - t0).abs().max().item())
        assert torch.equal(res[key][2], res['off'][2]), key
        d = (res[key][3][idx] - g0[idx]).abs().max().item()
        print('%s: sampled gradient difference %.3e' % (key, d))
        # two orders of the same float atomics: within the spread two identical runs show, with the head-room of a sample of two
        assert d <= 4.0 * spread + 1e-7 * scale, (key, d, spread, scale)


def test_train_step_with_and_without_the_option():
    from face_vijnana_yolov3_amd._lib import lib
    from face_vijnana_yolov3_amd.engine import Engine
    from oracle import net_oracle as no
    import ctypes
    eng = Engine(0)
    B, S = 2, 64
    p, st = no.init_params(29, torch.float32)
    ents, _, _ = no.param_layout()
    _bn_params(p, ents, 30)
    g = torch.Generator().manual_seed(31)
    x = torch.rand((B, S, S, 3), generator=g); yt = torch.rand((B, S // 32, S // 32, 6), generator=g)
    n = lib().fv_num_layers()
    folded = (ctypes.c_int32 * n)()
    assert lib().fv_train_bn_in_1x1_plan(2, B, S, folded, n) == 0 and sum(folded) >= 10     # option 2 does fold passes at this size

    def run():
        eng.set_params(p, st)
        eng.m = eng.v = eng.grads = None
        return eng.forward_backward(x, yt)
    _step_compare(eng, run, [l for l in range(n - 1)], B, S)


def test_three_scale_step_with_and_without_the_option():
    from face_vijnana_yolov3_amd._lib import lib
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    from oracle import net_oracle as no
    OUT = 18
    m = Yolov3(0, out_channels=OUT)
    B, S = 2, 64
    p, st = no.yolov3_init(33, OUT, torch.float32)
    ents, _, _ = no.yolov3_layout(OUT)
    _bn_params(p, ents, 34)
    g = torch.Generator().manual_seed(35)
    x = torch.rand((B, S, S, 3), generator=g)
    targets = [torch.rand((B, S // d, S // d, OUT), generator=g) for d in (32, 16, 8)]

    def run():
        m.set_params(p, st)
        m.m = m.v = m.grads = None
        return m.forward_backward(x, targets)
    layers = [l for l, d in enumerate(m.layers) if d['has_bn']]
    _step_compare(m, run, layers, B, S)
