"""The BatchNorm statistics and their backward sums on ill-conditioned channels, exactly (tests/exact_grid.py).

Forward: z = c0 + k/16 with c0 = 16 (|mean| >> std: (mean^2 + var) / var ~ 2700) or 0, some channels constant.  Every fp32 tile partial
of z and z^2 is exact, the fp64 slots beyond are exact, so the totals have one right value and mean / var / invstd follow from them by
the kernels' own few float64 operations.  A statistic summed in fp32 across tiles, a dropped row or a counted pad row is thousands of
ulp away (tests/test_exact_grid_cpu.py shows each of them failing these assertions on an emulation).  The statistics reach the
normalise pass through three producers -- host-made psum / psq into bn_finalize, a selection conv (z equals its input) into
conv2d_forward_slots into bn_act_slots, and conv2d_forward_slots_bn_stats_in -- and all are held to the same assertions.

Backward: g, z, mean, invstd, scale, shift dyadic, so gy, gy xhat and all their sums are exact: d-beta / d-gamma bit-equal to float64.

General position: the same paths on z = r + N(0, 1), r in {1, 30, 300}, against a bound derived from the contract (see the test)."""
import numpy as np
import pytest
import torch

import exact_grid as eg

pytestmark = pytest.mark.gpu

MOMENTUM = 0.99
# rows as a lattice (B, H, W) for the conv producers, C, eps: every row count of {4, 100, 128, 1000, 4097, 70000} (one ragged tile,
# whole tiles, ragged last tiles, more tiles than slots) and every C of {32, 64, 256, 1024} (C < 256 and C >= 256: the two branches of
# the slot summation)
SHAPES = [
    ((1, 2, 2), 32, 1e-3),
    ((1, 10, 10), 64, eg.EPS_POW2),
    ((2, 8, 8), 256, 1e-3),
    ((10, 10, 10), 1024, eg.EPS_POW2),
    ((1, 241, 17), 32, eg.EPS_POW2),
    ((1, 241, 17), 1024, 1e-3),
    ((7, 100, 100), 64, 1e-3),
    ((7, 100, 100), 256, eg.EPS_POW2),
]


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _profiled(ctx, fn):
    ctx.profile(True)
    try:
        out = fn()
        names = set(ctx.profile_collect())
    finally:
        ctx.profile(False)
    return out, names


def _vectors(C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: torch.rand(C, generator=g) * (hi - lo) + lo
    return r(0.5, 1.5), r(-1, 1), r(-1, 1), r(0.5, 2.0)          # gamma, beta, moving mean, moving variance


def _assert_published(z, eps, gamma, beta, mm0, mv0, mean, invstd, scale, shift, mm1, mv1, what):
    """mean / invstd / scale / shift / moving statistics as published by a kernel, against the exact totals of z [rows][C]."""
    rows, C = z.shape
    S, Q = (t.sum(0) for t in eg.tile_partials(z))
    mean64, var64, _ = eg.contract_stats(S, Q, rows, eps)
    mean, invstd, scale, shift = mean.cpu(), invstd.cpu(), scale.cpu(), shift.cpu()
    assert torch.equal(mean, mean64.float()), '%s: mean' % what
    e = float(np.float32(eps))
    _, var2 = eg.two_pass_stats(z)
    u = eg.ulps32(invstd, 1.0 / torch.sqrt(var2 + e))
    print('%s: invstd worst %.3f ulp from two-pass float64' % (what, u.max().item()))
    assert (u <= 1.0).all(), '%s: invstd %.1f ulp off' % (what, u.max().item())
    const = eg.constant_channels(C)
    assert (var2[const] == 0).all()
    assert (invstd[const] == np.float32(1.0 / np.sqrt(np.float64(e)))).all(), '%s: constant channels' % what
    if eps == eg.EPS_POW2:
        assert (invstd[const] == 32.0).all()
    # the kernels' fp32 expressions (built with -ffp-contract=off), from the published mean / invstd
    sc = gamma * invstd
    assert torch.equal(scale, sc) and torch.equal(shift, beta - mean * sc), '%s: scale / shift' % what
    m = torch.tensor(MOMENTUM, dtype=torch.float32)
    old, new = m, torch.ones((), dtype=torch.float32) - m
    corr = rows / (rows - (1.0 + e))
    assert torch.equal(mm1.cpu(), old * mm0 + new * mean), '%s: moving mean' % what
    assert torch.equal(mv1.cpu(), old * mv0 + new * (var64 * corr).float()), '%s: moving variance' % what
    return scale, shift


def _assert_activation(out, z, scale, shift, skip, what):
    pre = z * scale + shift
    want = torch.where(pre > 0, pre, pre * eg.LEAKY)
    if skip is not None:
        want = want + skip
    assert torch.equal(out.cpu().view(z.shape), want), '%s: activation' % what


def _assert_slots(slots, z, what):
    S, Q = (t.sum(0) for t in eg.tile_partials(z))
    tot = slots.sum(0).cpu()
    assert torch.equal(tot[0], S), '%s: sum z in the slots off by up to %.6g' % (what, (tot[0] - S).abs().max().item())
    assert torch.equal(tot[1], Q), '%s: sum z^2 in the slots off by up to %.6g' % (what, (tot[1] - Q).abs().max().item())


def _selection_conv(ctx, x_rows, lattice, C, k):
    """x_rows [rows][cin] through a selection conv (output channel c = input channel c % cin) with the statistics epilogue
    -> z (device, B H W C), its slots, z as rows on the CPU, kernel names."""
    from face_vijnana_yolov3_amd import ops
    B, H, W = lattice
    cin = x_rows.shape[1]
    x = x_rows.view(B, H, W, cin)
    slots = ops.stat_slots(C, 'cuda')
    z, names = _profiled(ctx, lambda: ops.conv2d_forward_slots(ctx, x.cuda(), eg.selection_weights(C, cin, k).cuda(), 1, slots))
    z_rows = x_rows.repeat(1, C // cin)
    assert torch.equal(z.cpu().view(-1, C), z_rows), 'the selection conv does not copy its input'
    return z, slots, z_rows, names


@pytest.mark.parametrize('lattice,C,eps', SHAPES)
def test_statistics_from_host_partials_through_bn_finalize(ctx, lattice, C, eps):
    from face_vijnana_yolov3_amd import ops
    from face_vijnana_yolov3_amd._lib import lib
    rows = lattice[0] * lattice[1] * lattice[2]
    z = eg.bn_stat_rows(rows, C, 2000 + rows)
    psum, psq = eg.tile_partials(z)
    assert psum.shape[0] == lib().fv_conv2d_stat_rows(rows)
    gamma, beta, mm0, mv0 = _vectors(C, 2001)
    mm1, mv1 = mm0.cuda(), mv0.cuda()
    (mean, invstd, scale, shift), names = _profiled(ctx, lambda: ops.bn_finalize(
        ctx, eg.exact32(psum).cuda(), eg.exact32(psq).cuda(), rows, gamma.cuda(), beta.cuda(), eps, MOMENTUM, mm1, mv1))
    assert 'bn_finalize_kernel' in names, sorted(names)
    sc, sh = _assert_published(z, eps, gamma, beta, mm0, mv0, mean, invstd, scale, shift, mm1, mv1, 'bn_finalize')
    skip = eg.dyadic((rows, C), 2002, 8, 8)
    out, names = _profiled(ctx, lambda: ops.bn_act(ctx, z.cuda(), scale, shift, skip.cuda(), eg.LEAKY))
    assert 'bn_act_kernel' in names, sorted(names)
    _assert_activation(out, z, sc, sh, skip, 'bn_act')


@pytest.mark.parametrize('lattice,C,eps', SHAPES)
def test_statistics_from_a_conv_through_the_slots(ctx, lattice, C, eps):
    """Selection conv (1x1; 3x3 centre tap for C = 64, where 32 -> 64 channels is the halo kernel's layer) -> slots -> bn_act_slots, and
    the same z and slots into conv2d_forward_slots_bn_stats_in where its kernel takes the layer (C <= 512)."""
    from face_vijnana_yolov3_amd import ops
    rows = lattice[0] * lattice[1] * lattice[2]
    k = 3 if C == 64 else 1
    x_rows = eg.bn_stat_rows(rows, 32, 2100 + rows)
    z, slots, z_rows, names = _selection_conv(ctx, x_rows, lattice, C, k)
    conv_names = [n for n in names if n.startswith(('conv_kernel', 'conv9_fwd_kernel', 'conv1x1_persist_kernel'))]
    assert len(conv_names) == 1, sorted(names)
    print('producer: %s' % conv_names[0])
    if C == 64:
        assert conv_names[0] == 'conv9_fwd_kernel<1>'
    _assert_slots(slots, z_rows, conv_names[0])
    gamma, beta, mm0, mv0 = _vectors(C, 2101)
    skip = eg.dyadic((rows, C), 2102, 8, 8)
    mm1, mv1 = mm0.cuda(), mv0.cuda()
    (out, mean, invstd, scale, shift), names = _profiled(ctx, lambda: ops.bn_act_slots(
        ctx, z, slots, gamma.cuda(), beta.cuda(), eps, MOMENTUM, mm1, mv1, skip.cuda().view(z.shape), eg.LEAKY))
    assert 'bn_act_stats_kernel' in names, sorted(names)
    sc, sh = _assert_published(z_rows, eps, gamma, beta, mm0, mv0, mean, invstd, scale, shift, mm1, mv1, 'bn_act_slots')
    _assert_activation(out, z_rows, sc, sh, skip, 'bn_act_slots')
    if C <= 512:
        cout = 64
        mm2, mv2 = mm0.cuda(), mv0.cuda()
        slots2 = ops.stat_slots(cout, 'cuda')
        (z2, a, mean, invstd, scale, shift), names = _profiled(ctx, lambda: ops.conv2d_forward_slots_bn_stats_in(
            ctx, z, slots, gamma.cuda(), beta.cuda(), eg.selection_weights(cout, C, 1).cuda(), slots2, eps, MOMENTUM, mm2, mv2,
            skip.cuda().view(z.shape), eg.LEAKY))
        assert 'conv1x1_persist_kernel<64>' in names, sorted(names)
        sc, sh = _assert_published(z_rows, eps, gamma, beta, mm0, mv0, mean, invstd, scale, shift, mm2, mv2, 'bn_stats_in')
        _assert_activation(a, z_rows, sc, sh, skip, 'bn_stats_in')
        a_rows = a.cpu().view(rows, C)
        assert torch.equal(z2.cpu().view(rows, cout), a_rows.repeat(1, (cout + C - 1) // C)[:, :cout]), 'the conv of the activation'


BWD_SHAPES = [(4, 32), (100, 64), (128, 256), (1000, 1024), (4097, 32), (4097, 1024), (70000, 64), (70000, 256), (4096, 64), (4096, 256)]
_bwd_last = {}


def _backward_runs(ctx, rows, C):
    """bn_bwd (fp32 chunk partials of at least 64 rows, fp64 beyond), bn_bwd_slots with its own reduction pass (reduced = 0) and with
    slots filled beforehand as the data-gradient epilogue leaves them (reduced = 1: exact per-128-row sums spread over the slots), once
    per shape: the two tests of a shape follow each other and share the truth and the three results (only the last shape is kept).
    -> scale, gy, xhat, sum gy, sum gy xhat (float64), {variant: (dz, dgamma, dbeta) on the CPU}."""
    from face_vijnana_yolov3_amd import ops
    if _bwd_last.get('key') == (rows, C):
        return _bwd_last['value']
    _bwd_last.clear()
    chunk = max(64, (rows + 2047) // 2048, eg.TILE)
    g, z, scale, shift, mean, invstd = eg.bn_bwd_operands(rows, C, 2200 + rows, chunk, coarse=rows == 4096)
    gy, xhat, db64, dg64 = eg.bn_bwd_truth(g, z, scale, shift, mean, invstd)
    dev = [t.cuda() for t in (g, z, scale, shift, mean, invstd)]
    res = {}
    out, names = _profiled(ctx, lambda: ops.bn_bwd(ctx, *dev, leaky=eg.LEAKY))
    assert {'bn_bwd_reduce_kernel', 'bn_bwd_apply_kernel'} <= names, sorted(names)
    res['bn_bwd'] = tuple(t.cpu() for t in out)
    nt = (rows + eg.TILE - 1) // eg.TILE
    pad = torch.zeros((nt * eg.TILE, C), dtype=torch.float64)
    a = pad.clone(); a[:rows] = gy
    b = pad.clone(); b[:rows] = gy * xhat
    for reduced in (0, 1):
        slots = ops.stat_slots(C, 'cuda')
        if reduced:
            slots.copy_(eg.spread_over_slots(a.view(nt, eg.TILE, C).sum(1), b.view(nt, eg.TILE, C).sum(1), slots.shape[0]))
        out, names = _profiled(ctx, lambda: ops.bn_bwd_slots(ctx, *dev, slots, reduced, leaky=eg.LEAKY))
        assert 'bn_bwd_apply_slots_kernel' in names and ('bn_bwd_reduce_kernel' in names) == (not reduced), sorted(names)
        if not reduced:
            tot = slots.sum(0).cpu()
            assert torch.equal(tot[0], db64) and torch.equal(tot[1], dg64), 'slots of the reduction pass'
        res['bn_bwd_slots(reduced=%d)' % reduced] = tuple(t.cpu() for t in out)
    _bwd_last.update(key=(rows, C), value=(scale, gy, xhat, db64, dg64, res))
    return _bwd_last['value']


@pytest.mark.parametrize('rows,C,part', [(r, c, p) for r, c in BWD_SHAPES for p in ('sums', 'dz')])
def test_backward(ctx, rows, C, part):
    """part 'sums': d-beta, d-gamma of the three variants bit-equal to the float64 sums rounded once (and, at reduced = 0, the fp64 slot
    totals bit-equal to the float64 sums themselves).

    part 'dz': bit-equal at rows = 4096 (1 / rows exact, the coarse grid: every intermediate is asserted to be a float before the
    comparison); elsewhere within 2 float ulp of the float64 expression scale (gy - dbeta / rows - xhat dgamma / rows) evaluated from the
    kernel's own d-beta / d-gamma.  The ulp is taken at mag = |scale| (|gy| + |dbeta / rows| + |xhat dgamma / rows|), the sum of the
    magnitudes of the terms: dz is a difference of three terms, and a float difference is no more accurate than the ulp of its
    operands, however small the result.  The kernel rounds dbeta / rows, dgamma / rows, xhat (dgamma / rows) and the two differences
    once each (gy, xhat and the product with scale are exact on this data): with u = 2^-24 the error is at most
    u (|gy| + 2 |dbeta / rows| + 2 |xhat dgamma / rows| + mag) <= 3 u mag < 3 ulp(mag) if every rounding is extreme and aligned; the
    bound asserted is the 2 ulp the contract states.

    This test found the kernels forming dbeta / rows as dbeta float(1 / rows): float(1 / 1000) is 0.80 u above 1 / 1000, the error
    entered both terms of every element with one sign, and at rows = 1000, C = 1024 two of 1 024 000 elements stood at 2.016 ulp in
    all three variants.  They now divide once per channel (fv_bn_mean_of, elementwise.h): the same fp32 expression in torch on the CPU gives 1.64 ulp there, at most 1.58 elsewhere."""
    scale, gy, xhat, db64, dg64, res = _backward_runs(ctx, rows, C)
    worst = {}
    for what, (dz, dgamma, dbeta) in res.items():
        if part == 'sums':
            assert torch.equal(dbeta, db64.float()), '%s: d-beta off by up to %.6g' % (what, (dbeta.double() - db64).abs().max().item())
            assert torch.equal(dgamma, dg64.float()), '%s: d-gamma off by up to %.6g' % (what, (dgamma.double() - dg64).abs().max().item())
            continue
        want, mag = eg.bn_bwd_dz(gy, xhat, scale, dbeta, dgamma, rows, check_exact=rows == 4096)
        if rows == 4096:
            assert torch.equal(dz, want.float()), '%s: dz' % what
        else:
            ulp = torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - 23)
            err = (dz.double() - want).abs() / ulp
            print('%s: dz worst %.3f ulp, %d of %d elements above 2' % (what, err.max().item(), int((err > 2).sum()), err.numel()))
            worst[what] = err.max().item()
    assert all(w <= 2 for w in worst.values()), 'dz, ulp off: %r' % worst


@pytest.mark.parametrize('lattice,C', [((1, 241, 17), 64), ((10, 10, 10), 256)])
@pytest.mark.parametrize('r', [1.0, 30.0, 300.0])
def test_general_position_variance_within_the_contract_bound(ctx, r, lattice, C):
    """z = r + N(0, 1), off the grid, through the three producers.  Bound on the variance the kernel used (recovered from the published
    invstd as 1 / invstd^2 - eps) against two-pass float64:

        |var - var64| <= 2^-17 (mean^2 + var) + 2^-16 mean^2

    Derivation: a tile partial is at most 127 fp32 additions of 128 terms, so its error is at most 127 x 2^-24 < 2^-17 of the sum of the
    terms' magnitudes; everything beyond the partials (fp64 slots and totals, mean, var) adds errors of order 2^-53.  For Q = sum z^2
    that is 2^-17 sum z^2, and Q / n = mean^2 + var, which gives the first term.  For S = sum z it is 2^-17 sum |z|, an error of
    2^-17 |mean| in the mean (|z| ~ |mean| in these channels) and of 2 |mean| 2^-17 |mean| = 2^-16 mean^2 in mean^2: the second term.
    (Recovering var from the float invstd adds 2^-23 (var + eps), not allowed for in the bound and small against it.)  The CPU emulation
    of the contract stays below 1 % of this bound (tests/test_exact_grid_cpu.py); the kernels measured at most 0.72 % of it."""
    from face_vijnana_yolov3_amd import ops
    rows = lattice[0] * lattice[1] * lattice[2]
    eps = 1e-3
    e = float(np.float32(eps))
    gen = torch.Generator().manual_seed(int(r) + C)
    x_rows = (r + torch.randn((rows, 32), generator=gen, dtype=torch.float64)).float()
    z, slots, z_rows, _ = _selection_conv(ctx, x_rows, lattice, C, 1)
    mean64, var64 = eg.two_pass_stats(z_rows)
    bound = 2.0 ** -17 * (mean64 ** 2 + var64) + 2.0 ** -16 * mean64 ** 2
    gamma, beta, _, _ = _vectors(C, 2301)

    def check(invstd, what):
        var = 1.0 / invstd.cpu().double() ** 2 - e
        ratio = ((var - var64).abs() / bound).max().item()
        print('%s, r = %g: worst |var - var64| / bound = %.4f' % (what, r, ratio))
        assert ratio <= 1.0, '%s: |var - var64| is %.3f of the bound' % (what, ratio)

    nt = (rows + eg.TILE - 1) // eg.TILE
    zp = torch.zeros((nt * eg.TILE, C)); zp[:rows] = z_rows
    zp = zp.view(nt, eg.TILE, C)
    psum, psq = zp.sum(1), (zp * zp).sum(1)                       # fp32 partials in torch's order
    check(ops.bn_finalize(ctx, psum.cuda(), psq.cuda(), rows, gamma.cuda(), beta.cuda(), eps, MOMENTUM)[1], 'bn_finalize')
    check(ops.bn_act_slots(ctx, z, slots, gamma.cuda(), beta.cuda(), eps, MOMENTUM)[2], 'bn_act_slots')
    slots2 = ops.stat_slots(64, 'cuda')
    check(ops.conv2d_forward_slots_bn_stats_in(ctx, z, slots, gamma.cuda(), beta.cuda(), eg.selection_weights(64, C, 1).cuda(), slots2,
                                               eps, MOMENTUM)[3], 'bn_stats_in')
