"""Every conv kernel against float64, bit for bit, on exact-grid data (tests/exact_grid.py): forward (raw, and with affine +
LeakyReLU(0.125) + addend), data-gradient (plain, + addend, + fused BN-backward reduction) and weight-gradient, through the operator
entry points.  On this data every fp32 product and partial sum is exact in any order, so each variant of a kernel -- tile shapes, wave
layouts, K splits inside a workgroup, tail split + fix-up, persistent tiles, halo kernels, float atomics over K-splits -- has the same
single right answer and the comparison is torch.equal against the float64 truth: a term that is dropped, doubled or read from a pad row
moves the result by at least one grid step.

Each case names the kernel it is meant for and asserts from the launch profile that this kernel ran; an on/off case asserts both names,
and that neither run used the other's kernel.  The tail split has no profile name of its own (its slices run in conv_kernel<128,...> and
the fix-up launch is not bracketed): there the witness is a second pair of launches of the same shape on general-position data, which
differ in rounding exactly when the split ran."""
import contextlib

import pytest
import torch

import exact_grid as eg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


@contextlib.contextmanager
def _options(ctx, **kv):
    """Set tuning switches for the block; all of them default to on and are put back to 1."""
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kv:
            ctx.set_option(k, 1)


def _profiled(ctx, fn):
    """-> fn(), the set of kernel names it launched."""
    ctx.profile(True)
    try:
        out = fn()
        names = set(ctx.profile_collect())
    finally:
        ctx.profile(False)
    return out, names


def _assert_ran(names, want, never=()):
    assert want in names, 'expected %s, ran %s' % (want, sorted(names))
    for n in never:
        assert n not in names, '%s must not run here, ran %s' % (n, sorted(names))


def _assert_bits(got, truth, what):
    want = eg.exact32(truth, what + ' truth')
    g = got.cpu()
    if not torch.equal(g, want):
        d = (g.double() - truth).abs()
        raise AssertionError('%s: %d of %d elements differ, largest difference %.10g (grid step 1/64 = %.6g), first at %r' % (
            what, int((d != 0).sum()), d.numel(), d.max().item(), 1 / 64, tuple(torch.nonzero(d)[0].tolist())))


def _tile(nout, gather=False):
    """The tile kernel fv_conv_launch picks by output width (default switches, no small-M inference tiling)."""
    if gather:
        return 'conv_kernel<32,4,1,true>'
    return 'conv_kernel<128,2,4,false>' if nout > 64 else 'conv_kernel<64,4,2,false>' if nout > 32 else 'conv_kernel<32,4,1,false>'


SMALL = ('conv_small_kernel<64,64,4>', 'conv_small_kernel<64,32,4>', 'conv_small_kernel<32,32,8>')
NO_INFER = dict(conv_small=0, conv_bm64=0)

# shape (B, H, W, cin, cout, k, s); epilogue: 'full' = affine + leaky + addend, 'noadd' = affine + leaky, 'bias' = shift only, linear;
# base: switches held for both runs; then (switch, kernel with it on, kernel with it off), switch None: one run
FWD_CASES = [
    ((2, 8, 8, 128, 256, 3, 1), 'full', NO_INFER, 'conv_waves8', 'conv_kernel<128,2,4,false>', 'conv_kernel<128,2,2,false>'),
    ((2, 16, 16, 64, 32, 1, 1), 'full', NO_INFER, None, _tile(32), None),
    ((2, 16, 16, 32, 64, 3, 2), 'full', NO_INFER, 'conv_waves8', 'conv_kernel<64,4,2,false>', 'conv_kernel<64,2,2,false>'),
    # the first layer: H = 12 is no multiple of the direct kernel's 8 x 32 tile and stays with the gather kernel; 8 x 32 reaches it
    # (the direct kernel has no addend epilogue)
    ((2, 12, 12, 3, 32, 3, 1), 'full', {}, None, _tile(32, True), None),
    ((3, 8, 32, 3, 32, 3, 1), 'noadd', {}, 'conv0_direct', 'conv0_direct_kernel', _tile(32, True)),
    ((2, 13, 13, 1024, 6, 3, 1), 'bias', {}, None, _tile(6), None),                    # the head: K = 9216, N = 6 guard
    ((2, 13, 13, 1024, 255, 1, 1), 'bias', {}, None, _tile(255), None),                # detection convs
    ((1, 52, 52, 256, 27, 1, 1), 'bias', {}, None, _tile(27), None),
    ((1, 13, 13, 1024, 512, 1, 1), 'full', {}, 'conv_small', SMALL[2], 'conv_kernel<128,2,4,false,64>'),
    ((1, 26, 26, 256, 512, 3, 2), 'full', {}, 'conv_small', SMALL[2], 'conv_kernel<128,2,4,false,64>'),
    ((1, 9, 9, 128, 512, 3, 1), 'full', {}, 'conv_small', SMALL[1], _tile(512)),
    ((1, 104, 104, 128, 64, 1, 1), 'full', {}, 'conv_small', SMALL[0], _tile(64)),
    ((1, 26, 26, 512, 256, 1, 1), 'full', {}, 'conv_small', SMALL[2], 'conv_kernel<32,4,1,false>'),   # off: the 128x32 "narrow" launch
    ((1, 13, 13, 512, 1024, 3, 1), 'full', {}, 'conv_bm64', 'conv_kernel<128,2,4,false,64>', _tile(1024)),
    ((9, 96, 96, 32, 128, 1, 1), 'full', {}, 'conv1x1_persist', 'conv1x1_persist_kernel<128>', _tile(128)),
    ((5, 84, 84, 96, 256, 1, 1), 'full', {}, 'conv1x1_persist', 'conv1x1_persist_kernel<128>', _tile(256)),
    ((9, 96, 96, 32, 64, 1, 1), 'full', {}, 'conv1x1_persist', 'conv1x1_persist_kernel<64>', _tile(64)),
]


def _dev(kw):
    return {k: v.cuda() if torch.is_tensor(v) else v for k, v in kw.items()}


def _runs(switch):
    return [(None, {})] if switch is None else [(True, {switch: 1}), (False, {switch: 0})]


def _fwd_forms(shape, epi, seed):
    """x, w, the epilogue calls [(label, kwargs (CPU tensors), truth)] of a forward case."""
    B, H, W, cin, cout, k, s = shape
    x, w = eg.conv_operands('fwd', B, H, W, cin, cout, k, s, seed)
    z = eg.conv_truth(x, w, k, s)
    forms = [('raw', {}, z)]
    scale, shift, addend = eg.epilogue_operands(tuple(z.shape), seed + 5, eg.conv_terms('fwd', B, H, W, cin, cout, k, s))
    if epi == 'bias':
        forms.append(('bias', dict(shift=shift), eg.epilogue_truth(z, None, shift, -1.0, None)))
    else:
        add = addend if epi == 'full' else None
        forms.append((epi, dict(scale=scale, shift=shift, leaky=eg.LEAKY, addend=add),
                      eg.epilogue_truth(z, scale, shift, eg.LEAKY, add)))
    return x, w, forms


@pytest.mark.parametrize('shape,epi,base,switch,on,off', FWD_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_forward_is_bit_equal_to_float64(ctx, shape, epi, base, switch, on, off):
    from face_vijnana_yolov3_amd import ops
    s = shape[6]
    x, w, forms = _fwd_forms(shape, epi, 1000 + shape[3])
    xd, wd = x.cuda(), w.cuda()
    for state, opt in _runs(switch):
        want, other = (on, off) if state is not False else (off, on)
        with _options(ctx, **dict(base, **opt)):
            for label, kw, truth in forms:
                got, names = _profiled(ctx, lambda: ops.conv2d_forward(ctx, xd, wd, s, **_dev(kw)))
                _assert_ran(names, want, [other] if other and other != want else [])
                _assert_bits(got, truth, '%s, %s (%s)' % (label, want, shape))


@pytest.mark.parametrize('shape,halo', [((2, 16, 16, 32, 64, 3, 2), 'conv9_fwd_kernel<2>'), ((3, 13, 13, 32, 64, 3, 1), 'conv9_fwd_kernel<1>'),
                                        ((1, 40, 24, 32, 64, 3, 1), 'conv9_fwd_kernel<1>')])
def test_halo_forward_and_its_column_sums(ctx, shape, halo):
    """conv2d_forward_slots of the 32 -> 64 channel 3x3 layer: conv9_fwd_kernel<1> / <2> (option conv_halo) against the tile kernel.
    z is bit-equal to float64; so is the first row of slots.sum(0), the column sums of z (|n| <= 64 x 288 per element, times the 128
    pixels of a tile or unit partial < 2^24).  The sums of squares leave the grid (z^2 needs up to 29 bits) and are not compared."""
    from face_vijnana_yolov3_amd import ops
    B, H, W, cin, cout, k, s = shape
    x, w = eg.conv_operands('fwd', B, H, W, cin, cout, k, s, 1100)
    eg.require_exact(64 * 9 * cin * 256, 'column sums of z over a partial of up to 256 pixels')
    z = eg.conv_truth(x, w, k, s)
    for state in (1, 0):
        want, other = (halo, _tile(64)) if state else (_tile(64), halo)
        with _options(ctx, conv_halo=state):
            slots = ops.stat_slots(cout, 'cuda')
            got, names = _profiled(ctx, lambda: ops.conv2d_forward_slots(ctx, x.cuda(), w.cuda(), s, slots))
        _assert_ran(names, want, [other])
        _assert_bits(got, z, 'z, %s' % want)
        assert torch.equal(slots.sum(0)[0].cpu(), z.view(-1, cout).sum(0)), 'column sums, %s' % want


@pytest.mark.parametrize('H', [100, 140])
def test_tail_split_forward_with_and_without_scratch(ctx, H):
    """Both plans of fv_conv_tail_plan (H = 100: all 157 tiles cut into K slices; H = 140: 256 of 307 tiles whole, 51 cut) + the fix-up
    kernel's epilogue, and the unsplit launch: raw and fused, all four bit-equal to float64.  That the split ran shows on general-position
    data of the same shape, where it rounds differently from the unsplit launch."""
    from face_vijnana_yolov3_amd import ops
    shape = (2, H, H, 256, 128, 3, 1)
    x, w, forms = _fwd_forms(shape, 'full', 1200)
    xd, wd = x.cuda(), w.cuda()
    g = torch.Generator().manual_seed(H)
    xr, wr = torch.rand(x.shape, generator=g).cuda(), (torch.rand(w.shape, generator=g) - 0.5).cuda()
    # (157 tiles are few enough for the 64-row tiles of small-M inference, which have no tail split: conv_bm64 off keeps H = 100 on
    # the 128-row tiles; the statistics form of the training step, which the split was built for, never takes 64-row tiles)
    with _options(ctx, conv_bm64=0):
        plain_r = ops.conv2d_forward(ctx, xr, wr, 1)
        for lend in (False, True):
            if lend:
                ctx.set_conv_scratch(torch.empty(64 << 20, dtype=torch.uint8, device='cuda'))
            try:
                if lend:
                    assert not torch.equal(ops.conv2d_forward(ctx, xr, wr, 1), plain_r), 'the tail split did not run'
                for label, kw, truth in forms:
                    got, names = _profiled(ctx, lambda: ops.conv2d_forward(ctx, xd, wd, 1, **_dev(kw)))
                    _assert_ran(names, _tile(128))
                    _assert_bits(got, truth, '%s, scratch %s, H = %d' % (label, lend, H))
            finally:
                ctx.set_conv_scratch(None)


# ---------------------------------------------------------------------------------------------------------------- data-gradient
# (B, H, cin, cout, k, s, cpad) of tests/test_ops_gpu.py DGRAD_CASES; switch, kernel on, kernel off (plain call; the + addend call of the
# stride-2 32 -> 64 layer stays with the tile kernel: the halo kernel has no addend epilogue)
DGRAD_CASES = [
    ((2, 16, 32, 64, 3, 1, 64), None, _tile(32), None),
    ((2, 16, 32, 64, 3, 2, 64), 'conv_halo', 'dgrad9s2_kernel', _tile(32)),
    ((2, 13, 128, 64, 1, 1, 64), None, _tile(128), None),
    ((3, 12, 64, 128, 3, 2, 128), None, _tile(64), None),
    ((2, 13, 1024, 6, 3, 1, 32), None, _tile(1024), None),
    ((1, 26, 256, 512, 3, 2, 512), None, _tile(256), None),
    ((2, 13, 1024, 255, 1, 1, 256), None, _tile(1024), None),
    ((1, 26, 512, 255, 1, 1, 256), None, _tile(512), None),
    ((1, 52, 256, 255, 1, 1, 256), None, _tile(256), None),
    ((2, 13, 1024, 27, 1, 1, 32), None, _tile(1024), None),
    ((1, 52, 256, 27, 1, 1, 32), None, _tile(256), None),
    ((9, 96, 128, 32, 1, 1, 32), 'conv1x1_persist', 'conv1x1_persist_kernel<128>', _tile(128)),      # 648 tiles: the persistent form
]


@pytest.mark.parametrize('case,switch,on,off', DGRAD_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_dgrad_is_bit_equal_to_float64(ctx, case, switch, on, off):
    from face_vijnana_yolov3_amd import ops
    B, H, cin, cout, k, s, cpad = case
    dy, w = eg.conv_operands('dgrad', B, H, H, cin, cout, k, s, 1300, pad_to=cpad)
    add = eg.dyadic((B, H, H, cin), 1310, 8, 8)
    eg.require_exact(64 * eg.conv_terms('dgrad', B, H, H, cin, cout, k, s) + 8, 'dgrad + addend')
    truth = eg.dgrad_truth(dy, w, (H, H), k, s)
    dyd, wd, addd = dy.cuda(), w.cuda(), add.cuda()
    for state, opt in _runs(switch):
        want, other = (on, off) if state is not False else (off, on)
        with _options(ctx, **opt):
            got, names = _profiled(ctx, lambda: ops.conv2d_dgrad(ctx, dyd, wd, (H, H), s))
            _assert_ran(names, want, [other] if other and other != want else [])
            _assert_bits(got, truth, 'dgrad, %s' % want)
            got, names = _profiled(ctx, lambda: ops.conv2d_dgrad(ctx, dyd, wd, (H, H), s, addend=addd))
            _assert_ran(names, off if on == 'dgrad9s2_kernel' else want)
            _assert_bits(got, truth + add.double(), 'dgrad + addend, %s' % want)


def test_tail_split_dgrad(ctx):
    """The data-gradient of a 128 -> 256 conv at 140 x 140 (307 tiles of 144 K steps): split with scratch lent, whole without."""
    from face_vijnana_yolov3_amd import ops
    B, H, cin, cout = 2, 140, 128, 256
    dy, w = eg.conv_operands('dgrad', B, H, H, cin, cout, 3, 1, 1400)
    truth = eg.dgrad_truth(dy, w, (H, H), 3, 1)
    g = torch.Generator().manual_seed(5)
    dyr, wr = (torch.rand(dy.shape, generator=g) - 0.5).cuda(), (torch.rand(w.shape, generator=g) - 0.5).cuda()
    plain_r = ops.conv2d_dgrad(ctx, dyr, wr, (H, H), 1)
    for lend in (False, True):
        if lend:
            ctx.set_conv_scratch(torch.empty(64 << 20, dtype=torch.uint8, device='cuda'))
        try:
            if lend:
                assert not torch.equal(ops.conv2d_dgrad(ctx, dyr, wr, (H, H), 1), plain_r), 'the tail split did not run'
            got, names = _profiled(ctx, lambda: ops.conv2d_dgrad(ctx, dy.cuda(), w.cuda(), (H, H), 1))
            _assert_ran(names, _tile(128))
            _assert_bits(got, truth, 'dgrad, scratch %s' % lend)
        finally:
            ctx.set_conv_scratch(None)


# tests/test_fused_slots_gpu.py BNRED_CASES; switch, kernel on, kernel off
BNRED_CASES = [
    ((2, 16, 64, 128, 3, 1, 128, False), None, _tile(64), None),
    ((2, 16, 128, 256, 3, 1, 256, True), None, _tile(128), None),
    ((2, 16, 32, 64, 3, 2, 64, False), 'conv_halo', 'dgrad9s2_kernel', _tile(32)),
    ((3, 12, 128, 128, 3, 2, 128, False), None, _tile(128), None),
    ((2, 13, 256, 128, 1, 1, 128, True), None, _tile(256), None),
    ((2, 13, 1024, 6, 3, 1, 32, False), None, _tile(1024), None),
]


def _bnred_case(case, partial_rows):
    """Operands and float64 truth of a conv2d_dgrad_bnred case.  The reduction forms fp32 partials of gy and gy xhat over a tile of dx
    pixels (128 rows; the halo kernel's unit: up to 512), so this data is coarser than the conv grid: dy in {-1, 0, 1}, w and the addend
    on the 1/4 grid (dx = n/4, |n| <= 4 T + 4), z in {15.5, 16, 16.5} with mean 16 and invstd 2 (xhat in {-1, 0, 1}), slope 0.125:
    gy xhat = n/32 with |n| <= 32 (T + 1), times 512 rows < 2^24 for T <= 1022 -- and times 128 rows for T <= 4094 (the 128 -> 256
    layer: T = 2304).  -> device operands of ops.conv2d_dgrad_bnred (without slots), addend, dx, sum gy, sum gy xhat."""
    B, H, cin, cout, k, s, cpad, with_add = case
    T = eg.conv_terms('dgrad', B, H, H, cin, cout, k, s)
    eg.require_exact(32 * (T + 1) * partial_rows, 'bnred partial, T = %d' % T)
    Ho = H // s
    dy = torch.zeros((B, Ho, Ho, cpad)); dy[..., :cout] = eg.dyadic((B, Ho, Ho, cout), 1500, 1, 1)
    w = eg.dyadic((cout, k, k, cin), 1501, 4, 4)
    add = eg.dyadic((B, H, H, cin), 1502, 4, 4) if with_add else None
    z = eg.dyadic((B, H, H, cin), 1503, 2, 1) + eg.BWD_MEAN
    scale = eg.pick((cin,), 1504, [0.5, 1.0, 2.0]); shift = eg.dyadic((cin,), 1505, 8, 4) - eg.BWD_MEAN * scale
    mean = torch.full((cin,), eg.BWD_MEAN); invstd = torch.full((cin,), eg.BWD_INVSTD)
    dx = eg.dgrad_truth(dy, w, (H, H), k, s)
    if add is not None:
        dx = dx + add.double()
    gy, xhat, dbeta, dgamma = eg.bn_bwd_truth(dx, z, scale, shift, mean, invstd)
    eg.exact32(gy); eg.exact32(gy * xhat)
    dev = (dy.cuda(), w.cuda(), (H, H), s, z.cuda(), scale.cuda(), shift.cuda(), mean.cuda(), invstd.cuda())
    return dev, None if add is None else add.cuda(), dx, dbeta, dgamma


def _assert_bnred(ctx, dev, add, dx, dbeta, dgamma, want, never):
    from face_vijnana_yolov3_amd import ops
    slots = ops.stat_slots(dx.shape[-1], 'cuda')
    got, names = _profiled(ctx, lambda: ops.conv2d_dgrad_bnred(ctx, *dev, slots, addend=add, leaky=eg.LEAKY))
    _assert_ran(names, want, never)
    _assert_bits(got, dx, 'dx, %s' % want)
    tot = slots.sum(0).cpu()
    assert torch.equal(tot[0], dbeta), 'sum gy, %s: off by at most %.6g' % (want, (tot[0] - dbeta).abs().max().item())
    assert torch.equal(tot[1], dgamma), 'sum gy xhat, %s: off by at most %.6g' % (want, (tot[1] - dgamma).abs().max().item())


@pytest.mark.parametrize('case,switch,on,off', BNRED_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_dgrad_bnred_slots_are_bit_equal_in_fp64(ctx, case, switch, on, off):
    """conv2d_dgrad_bnred: dx bit-equal, and slots.sum(0) bit-equal IN FP64 to the exact sum gy and sum gy xhat (_bnred_case)."""
    operands = _bnred_case(case, 512 if on == 'dgrad9s2_kernel' else 128)
    for state, opt in _runs(switch):
        want, other = (on, off) if state is not False else (off, on)
        with _options(ctx, **opt):
            _assert_bnred(ctx, *operands, want, [other] if other and other != want else [])


def test_dgrad_bnred_through_the_tail_split_fixup(ctx):
    """307 tiles of 144 K steps: with scratch lent conv_tail_fixup_kernel performs the epilogue of the cut tiles, the fused BN-backward
    reduction included; whole and split launches give the same dx and the same fp64 slot totals."""
    from face_vijnana_yolov3_amd import ops
    operands = _bnred_case((2, 140, 128, 256, 3, 1, 256, True), 128)
    g = torch.Generator().manual_seed(6)
    dyr, wr = (torch.rand((2, 140, 140, 256), generator=g) - 0.5).cuda(), (torch.rand((256, 3, 3, 128), generator=g) - 0.5).cuda()
    plain_r = ops.conv2d_dgrad(ctx, dyr, wr, (140, 140), 1)
    for lend in (False, True):
        if lend:
            ctx.set_conv_scratch(torch.empty(64 << 20, dtype=torch.uint8, device='cuda'))
        try:
            if lend:
                assert not torch.equal(ops.conv2d_dgrad(ctx, dyr, wr, (140, 140), 1), plain_r), 'the tail split did not run'
            _assert_bnred(ctx, *operands, _tile(128), [])
        finally:
            ctx.set_conv_scratch(None)


# ---------------------------------------------------------------------------------------------------------------- weight-gradient
Q = 'wgrad_kernel<128,128,quad>'
# (B, H, cin, cout, k, s, ndy); switch, kernel on, kernel off
WGRAD_CASES = [
    ((2, 16, 128, 128, 3, 1, 128), None, Q, None),
    ((2, 16, 64, 64, 3, 1, 64), None, 'wgrad_kernel<64,64>', None),
    ((3, 13, 32, 32, 3, 1, 32), None, 'wgrad_kernel<32,32>', None),
    ((2, 16, 32, 64, 3, 2, 64), 'wgrad_fused_taps', 'wgrad9_kernel<2>', 'wgrad_kernel<64,32>'),       # off: 64x32 tiles at stride 2
    ((1, 38, 32, 64, 3, 2, 128), 'wgrad_fused_taps', 'wgrad9_kernel<2>', 'wgrad_kernel<64,32>'),      # ragged units, padded dy
    ((3, 13, 32, 64, 3, 1, 64), 'wgrad_fused_taps', 'wgrad9_kernel<1>', 'wgrad_kernel<64,32>'),
    ((2, 16, 64, 32, 1, 1, 32), 'wgrad_fused_taps', 'wgrad1_kernel', 'wgrad_kernel<32,64>'),          # off: 32x64, 1x1
    ((3, 13, 64, 32, 1, 1, 32), 'wgrad_fused_taps', 'wgrad1_kernel', 'wgrad_kernel<32,64>'),          # a ragged last unit
    ((3, 13, 3, 32, 3, 1, 32), 'wgrad_fused_taps', 'wgrad0_kernel', 'wgrad_kernel<32,32,gather>'),
    ((1, 70, 3, 32, 3, 1, 64), 'wgrad_fused_taps', 'wgrad0_kernel', 'wgrad_kernel<32,32,gather>'),    # padded dy
    ((2, 13, 1024, 6, 3, 1, 32), None, 'wgrad_kernel<32,64>', None),                                  # the head
    ((2, 13, 1024, 255, 1, 1, 256), None, Q, None),
    ((1, 52, 256, 27, 1, 1, 32), None, 'wgrad_kernel<32,64>', None),
    ((5, 3, 128, 128, 3, 1, 128), None, Q, None),                                                     # 3x3 lattice
    ((7, 4, 128, 256, 3, 2, 256), None, Q, None),                                                     # stride 2 -> 2x2 lattice
    # long sums: float atomics over many K-splits
    ((2, 208, 32, 64, 3, 1, 64), 'wgrad_fused_taps', 'wgrad9_kernel<1>', 'wgrad_kernel<64,32>'),      # M = 86528
    ((2, 208, 64, 32, 1, 1, 32), 'wgrad_fused_taps', 'wgrad1_kernel', 'wgrad_kernel<32,64>'),
    ((2, 208, 3, 32, 3, 1, 32), 'wgrad_fused_taps', 'wgrad0_kernel', 'wgrad_kernel<32,32,gather>'),
    ((4, 52, 128, 128, 3, 1, 128), None, Q, None),                                                    # M = 10816
]


@pytest.mark.parametrize('case,switch,on,off', WGRAD_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_wgrad_is_bit_equal_to_float64(ctx, case, switch, on, off):
    from face_vijnana_yolov3_amd import ops
    B, H, cin, cout, k, s, ndy = case
    x, dy = eg.conv_operands('wgrad', B, H, H, cin, cout, k, s, 1600, pad_to=ndy)
    truth = eg.wgrad_truth(x, dy, cout, k, s)
    xd, dyd = x.cuda(), dy.cuda()
    for state, opt in _runs(switch):
        want, other = (on, off) if state is not False else (off, on)
        with _options(ctx, **opt):
            got, names = _profiled(ctx, lambda: ops.conv2d_wgrad(ctx, xd, dyd, cout, k, s))
        _assert_ran(names, want, [other] if other else [])
        _assert_bits(got, truth, 'wgrad, %s' % want)


@pytest.mark.parametrize('B,H,s', [(3, 13, 1), (2, 20, 2)])
def test_wgrad_bn_in(ctx, B, H, s):
    """conv2d_wgrad_bn_in (wgrad9_kernel, 32 -> 64): x = leaky(z_in scale + shift) formed on load.  z_in, shift on the 1/8 grid, scale in
    {0.5, 1, 2}: x = n/64 with |n| <= 192, dy = j/8: products n/512 with |n| <= 1536, times M <= 507 pixels < 2^24."""
    from face_vijnana_yolov3_amd import ops
    Ho = H // s
    eg.require_exact(1536 * B * Ho * Ho, 'wgrad_bn_in')
    z_in = eg.dyadic((B, H, H, 32), 1700, 8, 8); dy = eg.dyadic((B, Ho, Ho, 64), 1701, 8, 8)
    scale = eg.pick((32,), 1702, [0.5, 1.0, 2.0]); shift = eg.dyadic((32,), 1703, 8, 8)
    x = eg.epilogue_truth(z_in.double(), scale, shift, eg.LEAKY, None)
    truth = eg.wgrad_truth(eg.exact32(x, 'x'), dy, 64, 3, s)
    got, names = _profiled(ctx, lambda: ops.conv2d_wgrad_bn_in(ctx, z_in.cuda(), scale.cuda(), shift.cuda(), dy.cuda(), 64, 3, s, leaky=eg.LEAKY))
    _assert_ran(names, 'wgrad9_kernel<%d>' % s)
    _assert_bits(got, truth, 'wgrad_bn_in')


def test_wgrad_bn_bwd(ctx):
    """conv2d_wgrad_bn_bwd (wgrad0_kernel, the first layer): dz formed on load from g, z and the slots, then the weight-gradient.
    d-beta, d-gamma bit-equal to the exact sums; with M = 128 pixels (1 / M exact), g in {-1, 0, 1}, xhat on the 1/2 grid and the image
    in {0, 0.5, 1} every intermediate of dz and every product dz x stays on a grid of 2^-22 below 2^24 steps, so dw is bit-equal too
    (asserted of the float64 intermediates before the kernel runs)."""
    from face_vijnana_yolov3_amd import ops
    B, H, C = 2, 8, 32
    M = B * H * H
    x = eg.dyadic((B, H, H, 3), 1800, 2, 2, 0)
    g = eg.dyadic((B, H, H, C), 1801, 1, 1)
    z = eg.dyadic((B, H, H, C), 1802, 4, 2) + eg.BWD_MEAN
    scale = eg.pick((C,), 1803, [0.5, 1.0, 2.0]); shift = eg.dyadic((C,), 1804, 8, 4) - eg.BWD_MEAN * scale
    mean = torch.full((C,), eg.BWD_MEAN); invstd = torch.full((C,), eg.BWD_INVSTD)
    gy, xhat, dbeta, dgamma = eg.bn_bwd_truth(g, z, scale, shift, mean, invstd)
    t1 = eg.exact32(dbeta / M).double(); t2 = eg.exact32(dgamma / M).double()
    t3 = eg.exact32(xhat * t2).double(); s1 = eg.exact32(gy - t1).double()
    dz = eg.exact32(scale.double() * eg.exact32(s1 - t3).double(), 'dz')
    # dz = n 2^-13 with |dz| <= 2 (1 + 1 + 1), x = i/2: products on the 2^-14 grid, a sum over M pixels below M 6 2^14 steps
    assert torch.equal(dz.double() * 2 ** 13, (dz.double() * 2 ** 13).round())
    eg.require_exact(M * 6 * 2 ** 14, 'wgrad_bn_bwd products')
    truth = eg.wgrad_truth(x, dz, C, 3, 1)
    nt = (M + 127) // 128
    a = gy.view(nt, 128, C).sum(1); b = (gy * xhat).view(nt, 128, C).sum(1)
    slots = ops.stat_slots(C, 'cuda')
    slots.copy_(eg.spread_over_slots(a, b, slots.shape[0]))
    (dw, dgam, dbet), names = _profiled(ctx, lambda: ops.conv2d_wgrad_bn_bwd(ctx, x.cuda(), g.cuda(), z.cuda(), scale.cuda(), shift.cuda(),
                                                                           mean.cuda(), invstd.cuda(), slots, leaky=eg.LEAKY))
    _assert_ran(names, 'wgrad0_kernel')
    assert torch.equal(dbet.cpu(), eg.exact32(dbeta)) and torch.equal(dgam.cpu(), eg.exact32(dgamma))
    _assert_bits(dw, truth, 'wgrad_bn_bwd')
