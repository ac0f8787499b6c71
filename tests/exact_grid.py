"""Exact-grid data for the reduction kernels, and their float64 truth (no GPU).

Every generator puts its values on a dyadic grid (integers over a power of two) coarse enough that every fp32 product and every partial
sum of those products, in ANY order, is an integer below 2^24 over one common power of two -- exactly representable in fp32.  A kernel
that sums in fp32 (MFMA chains, float atomics, 128-row tile partials) or in fp64 (the slots) then has exactly one right answer, whatever
its tiling, split or atomic order: the float64 result of the CPU, and the tests compare with torch.equal.  A term that is dropped,
doubled or read from a pad row changes the sum by at least one grid step and cannot hide in a tolerance.

Each generator states its grid; `require_exact` refuses a case whose largest possible numerator reaches 2^24, and `exact32` asserts of a
float64 truth that a float holds it (the tests call it on everything they compare against).

Conv data        x = i/8, |i| <= 8 (the first layer's image: 0 <= i <= 8), w = j/8, |j| <= 8: products are n/64 with |n| <= 64, a sum
                 of T products has |n| <= 64 T, exact while 64 T < 2^24, T < 262144.
Epilogue data    scale in {0.5, 1, 2}, shift / bias / addend on the 1/8 grid, LeakyReLU slope 0.125 (0.1 is not dyadic).
BN statistics    z = c0 + k/16, c0 = 16 or 0, |k| <= 8, some channels constant: |z| 16ths <= 264, z^2 256ths < 2^17, times 128 rows of a
                 tile partial still < 2^24.
BN backward      g = k/16 with |k| <= 16, mean 16, invstd 2 (xhat = (z - 16) 2 on the 1/8 grid, |xhat| <= 1), scale in {0.5, 1, 2},
                 shift on the 1/8 grid (so the LeakyReLU mask is decided exactly): gy, gy xhat are n/1024 with |n| <= 1024.
"""
import numpy as np
import torch
import torch.nn.functional as F

LEAKY = 0.125
LIMIT = 1 << 24
TILE = 128                      # rows of one fp32 statistics partial (the conv kernels' output tile, fv_conv2d_stat_rows)
EPS_POW2 = 2.0 ** -10           # an eps at which a constant channel's invstd is exactly 32


def require_exact(max_numerator, what):
    """Refuse a case whose largest possible partial-sum numerator is not below 2^24."""
    if not max_numerator < LIMIT:
        raise ValueError('%s: numerators up to %d reach 2^24, an fp32 partial sum may round' % (what, max_numerator))
    return max_numerator


def exact32(t, what='truth'):
    """Assert that a float holds every element of the float64 tensor exactly; -> the float tensor."""
    f = t.float()
    assert torch.equal(f.double(), t), '%s is not exactly representable in fp32' % what
    return f


def dyadic(shape, seed, den, hi, lo=None):
    """Integers in [lo, hi] (lo defaults to -hi) over den, float32 (exact: |numerator| and den are small)."""
    g = torch.Generator().manual_seed(seed)
    lo = -hi if lo is None else lo
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).float() / float(den)


def pick(shape, seed, values):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


# ------------------------------------------------------------------------------------------------------------------- convolution
def conv_terms(kind, B, H, W, cin, cout, k, s):
    """T: the largest number of products summed into one result element."""
    if kind == 'fwd':
        return k * k * cin
    if kind == 'dgrad':             # stride 2: a dx pixel receives from at most 2 x 2 of the 3 x 3 taps
        return (k * k if s == 1 else 4) * cout
    if kind == 'wgrad':
        return B * (H // s) * (W // s)
    raise ValueError(kind)


def conv_operands(kind, B, H, W, cin, cout, k, s, seed, num=8, den=8, pad_to=None):
    """The two operands of a forward ('fwd': x, w), data-gradient ('dgrad': dy, w) or weight-gradient ('wgrad': x, dy) case on the
    num/den grid; cin == 3 makes x an image in [0, 1].  dy is padded with zero channels up to pad_to.  Refuses an inexact case."""
    T = conv_terms(kind, B, H, W, cin, cout, k, s)
    require_exact(num * num * T, '%s %r' % (kind, (B, H, W, cin, cout, k, s)))
    Ho, Wo = H // s, W // s
    x = dyadic((B, H, W, cin), seed, den, num, 0 if cin == 3 else None)
    w = dyadic((cout, k, k, cin), seed + 1, den, num)
    dy = torch.zeros((B, Ho, Wo, pad_to or cout))
    dy[..., :cout] = dyadic((B, Ho, Wo, cout), seed + 2, den, num)
    return {'fwd': (x, w), 'dgrad': (dy, w), 'wgrad': (x, dy)}[kind]


def epilogue_operands(out_shape, seed, T, num=8):
    """scale in {0.5, 1, 2}, shift and addend on the 1/8 grid; checks leaky(z scale + shift) + addend on the 1/512 grid (z = n/64,
    |n| <= num^2 T): |numerator| <= 2 num^2 T + 64 + 512."""
    require_exact(2 * num * num * T + 64 + 512, 'fused epilogue, T = %d' % T)
    C = out_shape[-1]
    return pick((C,), seed, [0.5, 1.0, 2.0]), dyadic((C,), seed + 1, 8, 8), dyadic(out_shape, seed + 2, 8, 8)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv_truth(x, w, k, s):
    """NHWC x, OHWI w -> float64 ZeroPadding2D(1) + Conv2D valid (k = 3) or 1x1, NHWC."""
    return F.conv2d(_nchw(x.double()), _nchw(w.double()), stride=s, padding=1 if k == 3 else 0).permute(0, 2, 3, 1).contiguous()


def epilogue_truth(z, scale, shift, leaky, addend):
    v = z
    if scale is not None:
        v = v * scale.double()
    if shift is not None:
        v = v + shift.double()
    if leaky >= 0:
        v = torch.where(v > 0, v, v * leaky)
    if addend is not None:
        v = v + addend.double()
    return v


def dgrad_truth(dy, w, in_hw, k, s):
    """float64 gradient of conv_truth with respect to x (autograd's own backward formula, without running the forward)."""
    cout, cin = w.shape[0], w.shape[3]
    B = dy.shape[0]
    g = torch.nn.grad.conv2d_input((B, cin, in_hw[0], in_hw[1]), _nchw(w.double()), _nchw(dy[..., :cout].double()).contiguous(),
                                   stride=s, padding=1 if k == 3 else 0)
    return g.permute(0, 2, 3, 1).contiguous()


def wgrad_truth(x, dy, cout, k, s):
    """float64 gradient of conv_truth with respect to w, OHWI."""
    cin = x.shape[3]
    g = torch.nn.grad.conv2d_weight(_nchw(x.double()).contiguous(), (cout, cin, k, k), _nchw(dy[..., :cout].double()).contiguous(),
                                    stride=s, padding=1 if k == 3 else 0)
    return g.permute(0, 2, 3, 1).contiguous()


def selection_weights(cout, cin, k):
    """Output channel c copies input channel c % cin (1x1, or the centre tap of a 3x3): the conv's result equals its input exactly."""
    w = torch.zeros((cout, k, k, cin))
    w[torch.arange(cout), k // 2, k // 2, torch.arange(cout) % cin] = 1.0
    return w


# ------------------------------------------------------------------------------------------------------------------- BN statistics
def bn_stat_rows(rows, C, seed):
    """z [rows][C] = c0 + k/16: channel c has c0 = 0 when c % 4 == 3 (else 16) and is constant (k = 0) when c % 8 in (1, 7) -- both
    kinds of offset have constant channels.  -> z (float32)."""
    require_exact(264 * 264 * TILE, 'BN statistics tile partial')
    k = dyadic((rows, C), seed, 16, 8)
    c0 = torch.where(torch.arange(C) % 4 == 3, 0.0, 16.0)
    return torch.where(constant_channels(C), torch.zeros(()), k) + c0


def constant_channels(C):
    c = torch.arange(C)
    return (c % 8 == 1) | (c % 8 == 7)


def tile_partials(z):
    """Exact per-128-row-tile sums of z and z^2 (what the conv epilogue leaves in psum / psq): float64 [tiles][C] each."""
    rows, C = z.shape
    nt = (rows + TILE - 1) // TILE
    zp = torch.zeros((nt * TILE, C), dtype=torch.float64)
    zp[:rows] = z.double()
    zp = zp.view(nt, TILE, C)
    return zp.sum(1), (zp * zp).sum(1)


def two_pass_stats(z):
    """float64 mean, biased variance by the two-pass formula."""
    zd = z.double()
    mean = zd.mean(0)
    return mean, ((zd - mean) ** 2).mean(0)


def contract_stats(S, Q, n, eps):
    """The kernels' expressions from exact totals S, Q (float64 tensors): mean = S / n, var = max(Q / n - mean^2, 0),
    invstd = float32(1 / sqrt(var + eps)) with eps the float the kernel is given.  -> mean64, var64, invstd32."""
    mean = S / float(n)
    var = (Q / float(n) - mean * mean).clamp_min(0.0)
    e = float(np.float32(eps))
    return mean, var, (1.0 / torch.sqrt(var + e)).float()


def emulate_contract(z, eps, across=np.float64, drop_row=None, pad_value=None):
    """The statistics contract on the CPU, literally: fp32 running sums of z and z z within each 128-row tile, `across` (float64 by
    contract) over the tiles, then contract_stats.  Defects for the mutation checks: across=np.float32, drop_row=r (row r never
    added), pad_value=v (one pad row of the ragged last tile counted with value v).  -> mean64, var64, invstd32."""
    a = z.numpy().astype(np.float32)
    rows, C = a.shape
    keep = np.ones(rows, dtype=bool)
    if drop_row is not None:
        keep[drop_row] = False
    S = np.zeros(C, dtype=across)
    Q = np.zeros(C, dtype=across)
    for t0 in range(0, rows, TILE):
        blk = a[t0:t0 + TILE][keep[t0:t0 + TILE]]
        if pad_value is not None and t0 + TILE >= rows:
            blk = np.concatenate([blk, np.full((1, C), pad_value, dtype=np.float32)])
        S = S + np.cumsum(blk, axis=0, dtype=np.float32)[-1].astype(across)
        Q = Q + np.cumsum(blk * blk, axis=0, dtype=np.float32)[-1].astype(across)
    return contract_stats(torch.from_numpy(S.astype(np.float64)), torch.from_numpy(Q.astype(np.float64)), rows, eps)


def ulps32(got, want64):
    """|got - want| in units of the float ulp at |want| (got float32, want float64) -> float64 tensor."""
    w = want64.abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(w)) - 23)
    return (got.double() - want64).abs() / ulp


# ------------------------------------------------------------------------------------------------------------------- BN backward
BWD_MEAN, BWD_INVSTD = 16.0, 2.0


def bn_bwd_operands(rows, C, seed, chunk_rows, coarse=False):
    """g = k/16 (|k| <= 16), z = 16 + k/16 (|k| <= 8), mean 16, invstd 2, scale in {0.5, 1, 2}, shift = -16 scale + j/8: the
    pre-activation z scale + shift = (z - 16) scale + j/8 is exact and changes sign within the data.  chunk_rows: the longest fp32
    partial the kernel under test forms.  coarse: g = k/4 (|k| <= 4), z = 16 + j/4 (|j| <= 2, xhat = j/2) -- still on the 1/16 grid,
    and coarse enough that with rows = 2^m <= 4096 every intermediate of dz = scale (gy - dbeta / rows - xhat dgamma / rows) is exact
    too: gy = n/32, dbeta / rows on the 2^-(5+m) grid, xhat dgamma / rows on the 2^-(7+m) grid, all below 3 in magnitude: < 2^21 steps.
    -> g, z, scale, shift, mean, invstd (float32)."""
    require_exact(1024 * chunk_rows, 'BN backward partial over %d rows' % chunk_rows)
    if coarse:
        if rows & (rows - 1) or rows > 4096:
            raise ValueError('the coarse grid makes dz exact for rows a power of two up to 4096, not %d' % rows)
        g = dyadic((rows, C), seed, 4, 4)
        z = dyadic((rows, C), seed + 1, 4, 2) + BWD_MEAN
    else:
        g = dyadic((rows, C), seed, 16, 16)
        z = dyadic((rows, C), seed + 1, 16, 8) + BWD_MEAN
    scale = pick((C,), seed + 2, [0.5, 1.0, 2.0])
    shift = dyadic((C,), seed + 3, 8, 4) - BWD_MEAN * scale
    return g, z, scale, shift, torch.full((C,), BWD_MEAN), torch.full((C,), BWD_INVSTD)


def bn_bwd_truth(g, z, scale, shift, mean, invstd, leaky=LEAKY):
    """float64 gy = g LeakyReLU'(z scale + shift), xhat = (z - mean) invstd, and their column sums d-beta, d-gamma."""
    pre = z.double() * scale.double() + shift.double()
    gy = torch.where(pre > 0, g.double(), g.double() * leaky)
    xhat = (z.double() - mean.double()) * invstd.double()
    C = z.shape[-1]
    return gy, xhat, gy.reshape(-1, C).sum(0), (gy * xhat).reshape(-1, C).sum(0)


def bn_bwd_dz(gy, xhat, scale, dbeta, dgamma, rows, check_exact=False):
    """float64 dz = scale (gy - dbeta / rows - xhat dgamma / rows) from given d-beta, d-gamma, evaluated in the kernels' order
    -> dz, mag = |scale| (|gy| + |dbeta / rows| + |xhat dgamma / rows|): the sum of the terms' magnitudes, the scale of the rounding
    error of a float sum.  check_exact: assert of every intermediate that a float holds it."""
    t1 = dbeta.double() / rows
    t3 = xhat * (dgamma.double() / rows)
    s1 = gy - t1
    s2 = s1 - t3
    dz = scale.double() * s2
    if check_exact:
        for name, t in (('dbeta / rows', t1), ('dgamma / rows', dgamma.double() / rows), ('xhat dgamma / rows', t3), ('gy - .', s1),
                        ('gy - . - .', s2), ('dz', dz)):
            exact32(t, name)
    mag = scale.double().abs() * (gy.abs() + t1.abs() + t3.abs())
    return dz, mag


def spread_over_slots(a, b, nslot):
    """Exact per-tile sums a, b [tiles][C] (float64) -> [nslot][2][C] accumulator slots, tile t in slot t % nslot."""
    nt, C = a.shape
    host = torch.zeros((nslot, 2, C), dtype=torch.float64)
    for t in range(nt):
        host[t % nslot, 0] += a[t]
        host[t % nslot, 1] += b[t]
    return host
