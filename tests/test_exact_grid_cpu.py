"""The exact-grid reference on its own (tests/exact_grid.py): on the CPU, without a kernel, the generators meet their condition --
fp32 accumulation in three different orders gives the float64 sum, bit for bit -- and the assertions of the GPU files discriminate:
three emulated defects of the statistics contract (fp32 across tiles, a dropped row, a counted pad row) each fail the assertion the
contract itself passes.  Nothing is mutated in a kernel and nothing runs on the GPU."""
import numpy as np
import pytest
import torch

import exact_grid as eg


def _three_orders(terms):
    """terms: float64 numpy [T][...] of exactly representable values -> the three fp32 running sums over axis 0."""
    t32 = terms.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), terms)
    perm = np.random.RandomState(7).permutation(len(t32))
    return [np.cumsum(o, axis=0, dtype=np.float32)[-1] for o in (t32, t32[::-1], t32[perm])]


def _assert_orders_exact(terms, what):
    want = terms.sum(axis=0)                    # float64: exact, the numerators stay far below 2^53
    for i, got in enumerate(_three_orders(terms)):
        assert np.array_equal(got.astype(np.float64), want), '%s, order %d' % (what, i)


@pytest.mark.parametrize('kind,B,H,cin,cout,k,s', [
    ('fwd', 2, 13, 1024, 6, 3, 1),             # the head: K = 9216, the longest forward chain
    ('fwd', 2, 12, 3, 32, 3, 1),               # the first layer's image in [0, 1]
    ('dgrad', 1, 26, 256, 512, 3, 2),
    ('wgrad', 2, 208, 32, 64, 3, 1),           # M = 86528 output pixels
])
def test_conv_products_sum_exactly_in_any_order(kind, B, H, cin, cout, k, s):
    a, b = eg.conv_operands(kind, B, H, H, cin, cout, k, s, 11)
    T = eg.conv_terms(kind, B, H, H, cin, cout, k, s)
    g = np.random.RandomState(3)
    # T products of operand values drawn from the case's own tensors, eight columns of them, plus the extreme column (every product 1)
    av = a.numpy().ravel()[g.randint(0, a.numel(), (T, 8))].astype(np.float64)
    bv = b.numpy().ravel()[g.randint(0, b.numel(), (T, 8))].astype(np.float64)
    terms = np.concatenate([av * bv, np.ones((T, 1))], axis=1)
    _assert_orders_exact(terms, kind)
    if kind == 'fwd':
        scale, shift, addend = eg.epilogue_operands((4, cout), 12, T)
        z = torch.from_numpy(np.resize(terms.sum(0), (4, cout)))          # the nine sums, one of them the extreme T
        eg.exact32(eg.epilogue_truth(z, scale, shift, eg.LEAKY, addend), 'fused epilogue')


def test_helper_refuses_a_case_that_can_round():
    with pytest.raises(ValueError):
        eg.conv_operands('wgrad', 4, 256, 256, 32, 64, 3, 1, 1)            # M = 262144: 64 M = 2^24
    with pytest.raises(ValueError):
        eg.conv_operands('fwd', 1, 8, 8, 32768, 32, 3, 1, 1)
    eg.conv_operands('wgrad', 1, 8, 8, 32, 64, 3, 1, 1)
    with pytest.raises(ValueError):
        eg.bn_bwd_operands(8, 4, 1, chunk_rows=16384)
    with pytest.raises(AssertionError):
        eg.exact32(torch.tensor([0.1], dtype=torch.float64))


def test_selection_weights_copy_the_input():
    x = eg.bn_stat_rows(37, 32, 5).view(1, 37, 1, 32)
    for k in (1, 3):
        z = eg.conv_truth(x, eg.selection_weights(64, 32, k), k, 1)
        assert torch.equal(z.view(37, 64), x.view(37, 32).double().repeat(1, 2))


@pytest.mark.parametrize('rows,C', [(128, 32), (1000, 64), (4097, 32)])
def test_bn_tile_partials_are_exact_in_any_order(rows, C):
    z = eg.bn_stat_rows(rows, C, 21)
    zd = z.double().numpy()
    for t0 in range(0, rows, eg.TILE):
        blk = zd[t0:t0 + eg.TILE]
        _assert_orders_exact(blk, 'sum z')
        _assert_orders_exact(blk * blk, 'sum z^2')
    # the extreme tile: every row at the largest magnitude
    _assert_orders_exact(np.full((eg.TILE, 1), 16.5), 'extreme z')
    _assert_orders_exact(np.full((eg.TILE, 1), 16.5 ** 2), 'extreme z^2')
    psum, psq = eg.tile_partials(z)
    eg.exact32(psum); eg.exact32(psq)
    const = eg.constant_channels(C)
    assert const.any() and (~const).any() and (z[:, const].std(0) == 0).all()
    assert (z[0, const] == 0).any() and (z[0, const] == 16).any()


@pytest.mark.parametrize('rows', [1000, 4097, 70000])
def test_bn_backward_partials_are_exact_in_any_order(rows):
    C = 8
    chunk = max(64, (rows + 2047) // 2048)
    g, z, scale, shift, mean, invstd = eg.bn_bwd_operands(rows, C, 31, max(chunk, eg.TILE))
    gy, xhat, dbeta, dgamma = eg.bn_bwd_truth(g, z, scale, shift, mean, invstd)
    pre = z.double() * scale.double() + shift.double()
    assert (pre > 0).any() and (pre <= 0).any()
    eg.exact32(pre); eg.exact32(gy); eg.exact32(xhat); eg.exact32(gy * xhat); eg.exact32(dbeta); eg.exact32(dgamma)
    for t0 in range(0, min(rows, 1024), eg.TILE):
        _assert_orders_exact(gy[t0:t0 + eg.TILE].numpy(), 'sum gy')
        _assert_orders_exact((gy * xhat)[t0:t0 + eg.TILE].numpy(), 'sum gy xhat')
    _assert_orders_exact(np.full((eg.TILE, 1), 1.0), 'extreme gy xhat')


def _ill_conditioned(rows, seed):
    """z = 16 + k/16 in every channel (mean 16, std ~0.3: (mean^2 + var) / var ~ 2700), one constant channel."""
    z = eg.dyadic((rows, 8), seed, 16, 8) + 16.0
    z[:, 3] = 16.0
    return z


def _assert_contract(z, got, eps):
    """The assertion of the GPU tests on mean / invstd, on an emulation's output."""
    mean, var, invstd = got
    S, Q = (t.sum(0) for t in eg.tile_partials(z))
    assert torch.equal(mean.float(), (S / z.shape[0]).float()), 'mean'
    m2, v2 = eg.two_pass_stats(z)
    e = float(np.float32(eps))
    u = eg.ulps32(invstd, 1.0 / torch.sqrt(v2 + e))
    assert (u <= 1.0).all(), 'invstd %.1f ulp off' % u.max().item()


@pytest.mark.parametrize('rows', [1000, 70000, 346112])
def test_contract_emulation_is_within_one_ulp_and_the_defects_are_not(rows):
    eps = 1e-3
    z = _ill_conditioned(rows, 41)
    _assert_contract(z, eg.emulate_contract(z, eps), eps)
    # the same from exact totals: the emulation's partials were exact
    S, Q = (t.sum(0) for t in eg.tile_partials(z))
    m, v, i = eg.contract_stats(S, Q, rows, eps)
    m_e, v_e, i_e = eg.emulate_contract(z, eps)
    assert torch.equal(m, m_e) and torch.equal(v, v_e) and torch.equal(i, i_e)
    for name, defect in (('fp32 across tiles', dict(across=np.float32)), ('one dropped row', dict(drop_row=rows // 2)),
                         ('one pad row counted', dict(pad_value=1.0))):
        with pytest.raises(AssertionError):
            _assert_contract(z, eg.emulate_contract(z, eps, **defect), eps)


def test_constant_channel_has_zero_variance_and_invstd_32():
    z = _ill_conditioned(4097, 43)
    mean, var, invstd = eg.emulate_contract(z, eg.EPS_POW2)
    assert var[3].item() == 0.0 and mean[3].item() == 16.0
    assert invstd[3].item() == 32.0
    mean, var, invstd = eg.emulate_contract(z, 1e-3)
    assert var[3].item() == 0.0
    assert invstd[3].item() == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-3))))
    assert (var[[0, 1, 2, 4]] > 0).all()


@pytest.mark.parametrize('r', [1.0, 30.0, 300.0])
def test_general_position_bound_holds_for_the_emulation(r):
    """z = r + N(0, 1), off the grid: the emulation's variance against two-pass float64 within the derived bound of
    tests/test_exact_bn_gpu.py, and far inside it."""
    g = torch.Generator().manual_seed(int(r))
    z = (r + torch.randn((4097, 16), generator=g, dtype=torch.float64)).float()
    mean, var, _ = eg.emulate_contract(z, 1e-3)
    m2, v2 = eg.two_pass_stats(z)
    bound = 2.0 ** -17 * (m2 * m2 + v2) + 2.0 ** -16 * m2 * m2
    ratio = ((var - v2).abs() / bound).max().item()
    print('r = %g: worst |var - var64| / bound = %.4f' % (r, ratio))
    assert ratio <= 1.0
