"""The reconstruction model on the GPU (fv_recon_forward and its kernels as single operators) against the float64 restatement of
tests/recon_oracle.py.  Tolerance as tests/test_fid_gpu.py's `_within`: 4x the error the same restatement makes in float32 on the
CPU plus 1e-6 of the largest value."""
import numpy as np
import pytest
import torch

import recon_oracle as ro
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd import ops

pytestmark = pytest.mark.gpu

CHANNELS = (32, 64, 128, 256, 512, 1024)
_CTX = []
_MODELS = {}


def _ctx():
    if not _CTX:
        from face_vijnana_yolov3_amd._lib import Context
        _CTX.append(Context(0))
    return _CTX[0]


def _model(S):
    if S not in _MODELS:
        _MODELS[S] = fi.ReconModel(S, ctx=_ctx())
    return _MODELS[S]


def _within(got, ref64, ref32, what, factor=4.0, floor=1e-6):
    e_gpu = (got.double().cpu() - ref64).abs().max().item()
    e_cpu = (ref32.double() - ref64).abs().max().item()
    lim = factor * e_cpu + floor * max(ref64.abs().max().item(), 1.0)
    print('%s: gpu err %.3e, cpu fp32 err %.3e, limit %.3e, max |ref| %.3e' % (what, e_gpu, e_cpu, lim, ref64.abs().max().item()))
    assert e_gpu <= lim, '%s: gpu err %.3e > limit %.3e (cpu fp32 err %.3e)' % (what, e_gpu, lim, e_cpu)


# ----------------------------------------------------------------------------- 1. the normalise stage
def _norm_ref(d, scale, shift, dtype):
    d, scale, shift = d.to(dtype), scale.to(dtype), shift.to(dtype)
    l = torch.where(d > 0, d, d * 0.1)
    return l * torch.rsqrt(torch.clamp((l * l).sum(-1, keepdim=True), min=1e-12)) * scale + shift


def _norm_case(rows, C, with_skip, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=g)
    skip = torch.randn((rows, C), generator=g) if with_skip else None
    if rows >= 7:
        x[2] = skip[2] if with_skip else 0.0                       # d is a row of zeros: stays zero, y = shift
        x[5] = 1e-8 * torch.sign(torch.randn(C, generator=g))       # sum of squares < 1e-12: the clamp decides
        if with_skip:
            skip[5] = 0.0
    scale = 0.5 + torch.rand(C, generator=g)
    shift = 0.1 * torch.randn(C, generator=g)
    return x, skip, scale, shift


@pytest.mark.parametrize('with_skip', [False, True])
@pytest.mark.parametrize('C', CHANNELS)
def test_l2norm_affine(C, with_skip):
    ctx = _ctx()
    for rows in (1, 7, 67, 2 * 13 * 13):
        x, skip, scale, shift = _norm_case(rows, C, with_skip, 1000 * C + rows)
        d32 = x - skip if with_skip else x
        y, d = ops.l2norm_affine(ctx, x.cuda(), scale.cuda(), shift.cuda(), skip.cuda() if with_skip else None)
        if with_skip:
            assert torch.equal(d.cpu(), d32), 'stored d, rows %d' % rows
        else:
            assert d is None
        assert (x < 0).any()
        _within(y, _norm_ref(d32.double(), scale, shift, torch.float64), _norm_ref(d32, scale, shift, torch.float32),
                'l2norm_affine C=%d rows=%d skip=%d' % (C, rows, with_skip))
        if rows >= 7:
            assert torch.equal(y[2].cpu(), shift), 'an all-zero pixel stays zero before the affine'
        if rows == 67:
            # a pixel's bits do not depend on the row count: first row, one inside, the last (partial wave / workgroup)
            for r in (0, 33, 66):
                y1, _ = ops.l2norm_affine(ctx, x[r:r + 1].cuda(), scale.cuda(), shift.cuda(), skip[r:r + 1].cuda() if with_skip else None)
                assert torch.equal(y1[0], y[r]), 'row %d alone differs' % r
    # in place: d over x, and d not kept
    x, skip, scale, shift = _norm_case(67, C, True, C)
    from face_vijnana_yolov3_amd._lib import lib, ptr
    xd, sk, sc, sh = x.cuda(), skip.cuda(), scale.cuda(), shift.cuda()          # named: the pointers must outlive the call
    y2 = torch.empty_like(xd)
    ctx.check(lib().fv_l2norm_affine(ctx.handle, ptr(xd), ptr(sk), ptr(xd), ptr(sc), ptr(sh), ptr(y2), 67, C, 0.1), 'fv_l2norm_affine')
    y3, none = ops.l2norm_affine(ctx, x.cuda(), sc, sh, sk, keep_d=False)
    assert none is None and torch.equal(xd.cpu(), x - skip) and torch.equal(y2, y3)


def test_l2norm_affine_refusals():
    from face_vijnana_yolov3_amd._lib import FvError, lib, ptr
    ctx = _ctx()
    L = lib()
    x = torch.ones((4, 48), device='cuda'); y = torch.full((4, 48), 7.0, device='cuda'); v = torch.ones(1024, device='cuda')
    for C in (48, 16, 2048, 0):
        with pytest.raises(FvError, match='not one of 32, 64, 128, 256, 512, 1024'):
            ctx.check(L.fv_l2norm_affine(ctx.handle, ptr(x), None, None, ptr(v), ptr(v), ptr(y), 4, C, 0.1), 'fv_l2norm_affine')
    with pytest.raises(FvError, match='NULL buffer'):
        ctx.check(L.fv_l2norm_affine(ctx.handle, ptr(x), None, None, None, ptr(v), ptr(y), 4, 32, 0.1), 'fv_l2norm_affine')
    with pytest.raises(FvError, match='NULL buffer'):
        ctx.check(L.fv_l2norm_affine(ctx.handle, None, None, None, ptr(v), ptr(v), ptr(y), 4, 32, 0.1), 'fv_l2norm_affine')
    with pytest.raises(FvError, match='buffer of its own'):
        ctx.check(L.fv_l2norm_affine(ctx.handle, ptr(x), None, None, ptr(v), ptr(v), ptr(x), 4, 32, 0.1), 'fv_l2norm_affine')
    torch.cuda.synchronize()
    assert (y == 7.0).all()                                         # a refused call writes nothing


# ----------------------------------------------------------------------------- 2. transposed convs on the matrix-core tiles
@pytest.mark.parametrize('B,H,W,cout,cin', [(2, 3, 5, 64, 32), (1, 1, 1, 1024, 512), (3, 2, 3, 256, 128)])
def test_stride2_transposed_conv_and_the_untouched_data_gradient(B, H, W, cout, cin):
    ctx = _ctx()
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x = torch.randn((B, H, W, cout), generator=g)
    w = torch.randn((cout, 3, 3, cin), generator=g) * float(np.sqrt(2.0 / (9 * cin)))
    got = ops.conv2d_transpose(ctx, x.cuda(), w.cuda(), stride=2)
    assert got.shape == (B, 2 * H, 2 * W, cin)
    _within(got, ro.conv_transpose(x.double(), w.double(), 2), ro.conv_transpose(x, w, 2), 'conv2d_transpose s2 %r' % ((B, H, W, cout, cin),))
    # the existing data-gradient on the same data is still the (1, 1)-padded one
    own = ops.conv2d_dgrad(ctx, x.cuda(), w.cuda(), (2 * H, 2 * W), stride=2)
    ref64 = ro.conv_s2_grad(x.double(), w.double(), (2 * H, 2 * W), (1, 1))
    _within(own, ref64, ro.conv_s2_grad(x, w, (2 * H, 2 * W), (1, 1)), 'conv2d_dgrad s2 %r' % ((B, H, W, cout, cin),))
    assert (got.double().cpu() - ref64).abs().max().item() > 0.5     # and the two are different things


@pytest.mark.parametrize('B,H,W,cout,cin,k', [(2, 3, 5, 64, 32, 3), (1, 13, 13, 64, 128, 1), (2, 1, 1, 1024, 512, 3)])
def test_stride1_transposed_conv(B, H, W, cout, cin, k):
    ctx = _ctx()
    g = torch.Generator().manual_seed(B + H + cout)
    x = torch.randn((B, H, W, cout), generator=g)
    w = torch.randn((cout, k, k, cin), generator=g) * float(np.sqrt(2.0 / (k * k * cin)))
    got = ops.conv2d_transpose(ctx, x.cuda(), w.cuda(), stride=1)
    _within(got, ro.conv_transpose(x.double(), w.double(), 1), ro.conv_transpose(x, w, 1), 'conv2d_transpose s1 k%d' % k)


# ----------------------------------------------------------------------------- 3. the last layer, 32 -> 3 channels
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S', [32, 64, 96])
def test_last_layer_direct_kernel(S, B):
    ctx = _ctx()
    g = torch.Generator().manual_seed(S + B)
    x = torch.randn((B, S, S, 32), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) * float(np.sqrt(2.0 / 27))
    ctx.profile(True)
    got = ops.conv2d_transpose(ctx, x.cuda(), w.cuda(), stride=1)
    prof = ctx.profile_collect()
    ctx.profile(False)
    assert any(k.startswith('convt_last_kernel') for k in prof), sorted(prof)      # cin == 3 selects the direct kernel
    assert got.shape == (B, S, S, 3)
    _within(got, ro.conv_transpose(x.double(), w.double(), 1), ro.conv_transpose(x, w, 1), 'last layer S=%d B=%d' % (S, B))


def test_conv2d_transpose_refusals():
    from face_vijnana_yolov3_amd._lib import FvError, lib, ptr
    ctx = _ctx()
    L = lib()
    x = torch.ones((1, 8, 32, 32), device='cuda'); w = torch.ones((3 * 9 * 32,), device='cuda'); o = torch.full((1, 8, 32, 3), 7.0, device='cuda')
    with pytest.raises(FvError, match='NULL buffer'):
        ctx.check(L.fv_conv2d_transpose(ctx.handle, ptr(x), None, 1, 8, 32, 3, 32, 3, 1, ptr(o)), 'fv_conv2d_transpose')
    with pytest.raises(FvError, match='H % 8 == 0 and W % 32 == 0'):
        ctx.check(L.fv_conv2d_transpose(ctx.handle, ptr(x), ptr(w), 1, 4, 32, 3, 32, 3, 1, ptr(o)), 'fv_conv2d_transpose')
    with pytest.raises(FvError, match='32 -> 3 channel'):
        ctx.check(L.fv_conv2d_transpose(ctx.handle, ptr(x), ptr(w), 1, 8, 32, 3, 64, 3, 1, ptr(o)), 'fv_conv2d_transpose')
    with pytest.raises(FvError, match='unsupported k=3 s=3'):
        ctx.check(L.fv_conv2d_transpose(ctx.handle, ptr(x), ptr(w), 1, 8, 32, 32, 32, 3, 3, ptr(o)), 'fv_conv2d_transpose')
    torch.cuda.synchronize()
    assert (o == 7.0).all()


# ----------------------------------------------------------------------------- 4. the dense head
@pytest.mark.parametrize('F', [1024, 9216])
@pytest.mark.parametrize('N', [1, 5, 33])
def test_dense_head(N, F):
    ctx = _ctx()
    g = torch.Generator().manual_seed(N * 7 + F)
    K = (torch.rand((F, 64), generator=g) * 2 - 1) * float(np.sqrt(6.0 / (F + 64)))
    b = torch.rand(F, generator=g)
    ids = torch.randn((N, 64), generator=g)
    assert (ids < 0).any()                                          # the ReLU has something to cut
    if N > 1:
        ids[1] = 0.0
    u, x = ops.recon_dense_head(ctx, ids.cuda(), K.cuda(), b.cuda())
    u64 = torch.relu(ro.l2_normalize(ids.double()))
    _within(u, u64, torch.relu(ro.l2_normalize(ids)), 'head u N=%d' % N)
    assert (u.cpu()[ids < 0] == 0).all()
    _within(x, ro.head(ids.double(), K.double(), b.double()), ro.head(ids, K, b), 'head x N=%d F=%d' % (N, F))
    zero = x[1] if N > 1 else ops.recon_dense_head(ctx, torch.zeros((1, 64), device='cuda'), K.cuda(), b.cuda())[1][0]
    assert torch.equal(zero.cpu(), b), 'an all-zero id row gives the bias'


# ----------------------------------------------------------------------------- 5. end to end
_BASES = {}


def _base(random_bn):
    """The kernels and BN vectors, drawn once per BN kind and shared by the sizes: (float64, float32, the kernel prefix of the
    flat vector)."""
    if random_bn not in _BASES:
        layers = fi.base_layers()
        b64 = ro.make_base(layers, 11 + random_bn, random_bn)
        b32 = dict(kernels=[k.float() for k in b64['kernels']], bn=[tuple(v.float() for v in q) for q in b64['bn']])
        prefix = torch.zeros(fi.recon_offsets(32)['dense'], dtype=torch.float32)
        for d, k in zip(layers, b32['kernels']):
            prefix[d['w_off']:d['w_off'] + k.numel()] = k.reshape(-1)
        _BASES[random_bn] = (b64, b32, prefix)
    return _BASES[random_bn]


def _load_oracle_params(m, P, prefix):
    m.params[:prefix.numel()].copy_(prefix)
    tail = torch.zeros(m.n_params - m.off['dense'], dtype=torch.float32)
    o = m.off['dense']
    tail[:m.off['bias'] - o] = P['K'].float().reshape(-1)
    tail[m.off['bias'] - o:m.off['bn'] - o] = P['b'].float()
    for l in range(len(m.layers)):
        for which in range(4):
            sl = m.bn_slice(l, which)
            tail[sl.start - o:sl.stop - o] = P['bn'][l][which].float()
    m.params[o:].copy_(tail)


@pytest.mark.parametrize('random_bn', [False, True])
@pytest.mark.parametrize('S,N', [(32, 3), (64, 2), (96, 2)])
def test_predict_matches_the_oracle(S, N, random_bn):
    layers = fi.base_layers()
    b64, b32, prefix = _base(random_bn)
    P = ro.make_params(b64, layers, S, 11 + S)
    ids = ro.make_ids(N, S + N)
    ref64, min_norm = ro.forward(P, ids, layers, S)
    ref32, _ = ro.forward(dict(b32, K=P['K'].float(), b=P['b'].float()), ids.float(), layers, S)
    # no pixel that enters a normalise is anywhere near the max(sum, 1e-12) corner (that corner is test_l2norm_affine's)
    assert min_norm >= 0.1, min_norm
    m = _model(S)
    _load_oracle_params(m, P, prefix)
    got = m.predict(ids.float().numpy())
    assert got.shape == (N, S, S, 3) and got.dtype == np.float32
    _within(torch.from_numpy(got), ref64, ref32, 'predict S=%d N=%d random_bn=%d (min norm %.2f)' % (S, N, random_bn, min_norm))
    # the same call gives the same bits, and a row alone is within the same tolerance
    assert np.array_equal(m.predict(ids.float().numpy()), got)
    _within(m.predict_device(ids[1:2].float()), ref64[1:2], ref32[1:2], 'predict row 1 alone')


def test_forward_refusals():
    from face_vijnana_yolov3_amd._lib import FvError, lib, ptr
    m = _model(32)
    L = lib()
    ids = torch.zeros((1, 64), device='cuda'); out = torch.full((1, 32, 32, 3), 7.0, device='cuda')
    ws = torch.empty(int(L.fv_recon_workspace_bytes(1, 32)), dtype=torch.uint8, device='cuda')
    with pytest.raises(FvError, match='multiple of 32'):
        m.ctx.check(L.fv_recon_forward(m.ctx.handle, ptr(m.params), ptr(ids), 1, 48, ptr(ws), ws.numel(), ptr(out)), 'fv_recon_forward')
    with pytest.raises(FvError, match='NULL buffer'):
        m.ctx.check(L.fv_recon_forward(m.ctx.handle, ptr(m.params), None, 1, 32, ptr(ws), ws.numel(), ptr(out)), 'fv_recon_forward')
    with pytest.raises(FvError, match='workspace'):
        m.ctx.check(L.fv_recon_forward(m.ctx.handle, ptr(m.params), ptr(ids), 1, 32, ptr(ws), ws.numel() - 4096, ptr(out)), 'fv_recon_forward')
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(ValueError, match=r'\(N, 64\)'):
        m.predict(np.zeros((2, 63), np.float32))
    with pytest.raises(ValueError, match='multiple of 32'):
        fi.ReconModel(48, ctx=m.ctx)


# ----------------------------------------------------------------------------- 6. the host class
def test_from_identifier_is_a_snapshot_and_save_load_round_trips(tmp_path):
    S = 32
    fid = fi.FidModel(S, 0)
    fid.init_synthetic(seed=7); fid.init_dense(seed=1)
    rec = fi.ReconModel.from_identifier(fid, seed=3)
    for l in (0, 1, 30, 51):
        assert torch.equal(rec.params[rec.kernel_slice(l)], fid.params[rec.kernel_slice(l)])
        assert (rec.params[rec.bn_slice(l, 0)] == 1).all() and (rec.params[rec.bn_slice(l, 1)] == 0).all()
        assert (rec.params[rec.bn_slice(l, 2)] == 0).all() and (rec.params[rec.bn_slice(l, 3)] == 1).all()
    assert torch.equal(rec.dense_kernel(), fid.dense_kernel())
    assert np.array_equal(rec.dense_bias().cpu().numpy(), np.random.RandomState(3).rand(rec.F).astype(np.float32))
    before = rec.params.clone()
    fid.params.normal_()                                            # "training" the identifier afterwards
    assert torch.equal(rec.params, before)
    # non-trivial BN, then the file
    g = torch.Generator().manual_seed(4)
    for l in range(52):
        for which in range(4):
            sl = rec.bn_slice(l, which)
            rec.params[sl] = (0.5 + torch.rand(sl.stop - sl.start, generator=g)).cuda()
    path = str(tmp_path / 'recon.h5')
    rec.save(path)
    from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5
    datasets, attrs = read_hdf5(path)
    assert {k: v.shape for k, v in datasets.items()} == dict(fi.recon_h5_layout(S))
    assert [n.decode() for n in attrs['/model_weights']['layer_names']][:3] == ['dense1', 'bnorm_73', 'conv_73']
    K = rec.dense_kernel().cpu().numpy()
    assert np.array_equal(datasets['/model_weights/dense1/dense1/kernel:0'], K.T)
    again = fi.ReconModel(S, ctx=rec.ctx)
    again.load(path)
    assert torch.equal(again.params, rec.params)


def test_create_face_reconst_model_writes_and_reads_its_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    S = 32
    conf = dict(mode='train', resource_type='uccs', raw_data_path=str(tmp_path), multi_gpu=False, num_gpus=1, yolov3_base_model_load=False,
                model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64),
                hps=dict(lr=1e-3, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=1))
    ident = fi.FaceIdentifier({'fi_conf': dict(conf), 'fd_conf': {}})          # no face_vijana_recon_load key: false
    ident.create_face_reconst_model(seed=3)
    assert (tmp_path / 'face_vijnana_recon.h5').exists()
    assert np.array_equal(ident.recon_model.dense_bias().cpu().numpy(), np.random.RandomState(3).rand(1024).astype(np.float32))
    ids = ro.make_ids(3, 2).float().numpy()
    want = ident.recon_model.predict(ids)
    assert want.shape == (3, S, S, 3) and np.isfinite(want).all() and np.abs(want).max() > 0
    other = fi.FaceIdentifier({'fi_conf': dict(conf, face_vijana_recon_load=True), 'fd_conf': {}})
    other.model.params.normal_()                                     # the loaded model does not depend on this identifier's weights
    other.create_face_reconst_model()
    assert torch.equal(other.recon_model.params.cpu(), ident.recon_model.params.cpu())
    got = other.recon_model.predict(ids)
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
