"""The reconstruction model without a GPU: the float64 restatement (tests/recon_oracle.py) against autograd and a hand case, the
stage order, the flat layout and the names / shapes of face_vijnana_recon.h5."""
import numpy as np
import pytest
import torch

import recon_oracle as ro
from face_vijnana_yolov3_amd import face_identification as fi

# issue text: the order of the stages in Darknet conv indices
ORDER = [73, 72, 70, 69, 67, 66, 64, 63, 62] + [i for b in range(60, 37, -3) for i in (b, b - 1)] + [37] + \
        [i for b in range(35, 12, -3) for i in (b, b - 1)] + [12, 10, 9, 7, 6, 5, 3, 2, 1, 0]


@pytest.mark.parametrize('B,H,W,cout,cin', [(2, 3, 5, 64, 32), (1, 1, 1, 16, 8)])
def test_stride2_transposed_conv_is_the_gradient_of_the_same_padded_conv(B, H, W, cout, cin):
    g = torch.Generator().manual_seed(H * W + cout)
    x = torch.randn((B, H, W, cout), generator=g, dtype=torch.float64)
    w = torch.randn((cout, 3, 3, cin), generator=g, dtype=torch.float64)
    got = ro.conv_transpose(x, w, 2)
    assert got.shape == (B, 2 * H, 2 * W, cin)
    same = ro.conv_s2_grad(x, w, (2 * H, 2 * W), (0, 1))
    assert (got - same).abs().max().item() <= 1e-12 * max(1.0, same.abs().max().item())
    # ... and NOT the data-gradient of this network's own stride-2 layers (ZeroPadding2D(1) + 'valid'): one pixel off
    own = ro.conv_s2_grad(x, w, (2 * H, 2 * W), (1, 1))
    assert (got - own).abs().max().item() > 1.0
    # parity classes: output row 2a takes r = 0 from in[a] and r = 2 from in[a - 1]; row 2a + 1 takes r = 1 from in[a]
    a, c = H - 1, W - 1
    ev = torch.einsum('bo,oi->bi', x[:, a, c], w[:, 0, 0]) if a == 0 and c == 0 else None
    odd = torch.einsum('bo,oi->bi', x[:, a, c], w[:, 1, 1])
    assert torch.allclose(got[:, 2 * a + 1, 2 * c + 1], odd, rtol=0, atol=1e-12)
    if ev is not None:
        assert torch.allclose(got[:, 0, 0], ev, rtol=0, atol=1e-12)


def test_stride1_transposed_conv_is_the_data_gradient():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 5, 8), generator=g, dtype=torch.float64)
    for k in (1, 3):
        w = torch.randn((8, k, k, 6), generator=g, dtype=torch.float64)
        xin = torch.zeros((2, 6, 4, 5), dtype=torch.float64, requires_grad=True)
        z = torch.nn.functional.conv2d(xin, w.permute(0, 3, 1, 2), padding=k // 2)
        (z * x.permute(0, 3, 1, 2)).sum().backward()
        assert (ro.conv_transpose(x, w, 1) - xin.grad.permute(0, 2, 3, 1)).abs().max().item() <= 1e-12


def test_stage_order_is_the_references():
    layers = fi.base_layers()
    assert ro.stage_conv_indices(layers) == ORDER and len(ORDER) == 52
    ops = ro.schedule(layers)
    assert sum(o[0] == 'subtract' for o in ops) == 23 and sum(o[0] == 'skip' for o in ops) == 4
    assert ops[-2:] == [('stage', 1), ('stage', 0)] and ops[-3] == ('subtract',)
    assert fi.recon_stage_order() == [o[1] for o in ops if o[0] == 'stage']


def test_output_shape_and_hand_case_on_the_1x1_grid():
    layers = fi.base_layers()
    S, F = 32, 1024
    P = ro.make_params(ro.make_base(layers, 5, random_bn=False), layers, S, 5)
    ids = torch.zeros((1, 64), dtype=torch.float64); ids[0, 0] = 1.0           # e_0
    out, min_norm = ro.forward(P, ids, layers, S)
    assert out.shape == (1, S, S, 3) and torch.isfinite(out).all() and min_norm > 0
    # head: u = e_0, x = K[:, 0] + b
    x0 = P['K'][:, 0] + P['b']
    assert torch.equal(ro.forward(P, ids, layers, S, n_stages=0)[0].reshape(-1), x0)
    # first stage on the 1x1 grid: fresh BN is a scale by 1 / sqrt(1.001); of the 3x3 kernel of layer 51 only the centre tap
    # meets the single pixel
    l = torch.where(x0 > 0, x0, 0.1 * x0)
    y = l / l.norm() / np.sqrt(1.001)
    want = y @ P['kernels'][51][:, 1, 1, :]
    got = ro.forward(P, ids, layers, S, n_stages=1)[0]
    assert got.shape == (1, 1, 1, 512)
    assert (got.reshape(-1) - want).abs().max().item() <= 1e-12
    # batch rows are independent
    two = ro.forward(P, torch.cat([ids, ro.make_ids(1, 9)]), layers, S)[0]
    assert two.shape == (2, S, S, 3) and (two[0] - out[0]).abs().max().item() <= 1e-9


def test_all_zero_pixel_stays_zero_in_the_normalise():
    x = torch.zeros((1, 1, 2, 8), dtype=torch.float64); x[0, 0, 1] = torch.arange(8.0) - 3
    bn = (torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64))
    y, nrm = ro.stage_input(x, bn)
    assert nrm == 0.0 and torch.equal(y[0, 0, 0], torch.zeros(8, dtype=torch.float64))
    assert abs((y[0, 0, 1] ** 2).sum().item() * 1.001 - 1.0) < 1e-12


def test_param_layout_and_h5_names_need_no_device():
    from face_vijnana_yolov3_amd._lib import lib
    L = lib()
    layers = fi.base_layers()
    chans = sum(d['cout'] for d in layers)
    for S in (32, 416):
        F = fi.feature_size(S)
        o = fi.recon_offsets(S)
        assert o['dense'] == 40584928 and o['bias'] == o['dense'] + F * 64 and o['bn'] == o['bias'] + F
        assert o['count'] == o['bn'] + 4 * chans == L.fv_recon_param_count(S)
    assert L.fv_recon_param_count(100) == 0 and L.fv_recon_param_count(0) == 0
    assert L.fv_recon_workspace_bytes(0, 32) == 0 and L.fv_recon_workspace_bytes(1, 33) == 0
    # the workspace holds the transposed kernels, three activation buffers of batch * S * S * 32 floats and little else
    kern = sum(d['cout'] * d['ksize'] ** 2 * d['cin'] for d in layers)
    assert 4 * (kern + 3 * 2 * 64 * 64 * 32) <= L.fv_recon_workspace_bytes(2, 64) < 4 * (kern + 3 * 2 * 64 * 64 * 32) + (64 << 20)

    lay = fi.recon_h5_layout(32)
    names = [n for n, _ in lay]
    assert len(set(names)) == len(names) == 2 + 52 * 5
    shapes = dict(lay)
    assert shapes['/model_weights/dense1/dense1/kernel:0'] == (64, 1024)           # the transpose of dense1's [F][64]
    assert shapes['/model_weights/dense1/dense1/bias:0'] == (1024,)
    assert shapes['/model_weights/output/output/kernel:0'] == (3, 3, 3, 32)
    assert shapes['/model_weights/conv_1/conv_1/kernel:0'] == (3, 3, 32, 64)
    assert shapes['/model_weights/conv_73/conv_73/kernel:0'] == (3, 3, 512, 1024)
    assert shapes['/model_weights/conv_72/conv_72/kernel:0'] == (1, 1, 1024, 512)
    assert '/model_weights/conv_0/conv_0/kernel:0' not in shapes
    for i, c in ((0, 32), (1, 64), (73, 1024)):
        for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
            assert shapes['/model_weights/bnorm_%d/bnorm_%d/%s:0' % (i, i, w)] == (c,)
    # in the order the model runs: dense1, then bnorm_73, conv_73, bnorm_72, ...
    assert names[2].startswith('/model_weights/bnorm_73/') and names[6] == '/model_weights/conv_73/conv_73/kernel:0'
    assert names[-1] == '/model_weights/output/output/kernel:0'
    assert fi.recon_h5_layout(416)[0][1] == (64, 173056)


def test_create_face_reconst_model_raises_without_a_model():
    f = fi.FaceIdentifier.__new__(fi.FaceIdentifier)
    with pytest.raises(ValueError, match='valid model'):
        f.create_face_reconst_model()
    f.model = object()
    with pytest.raises(ValueError, match='valid model'):
        f.create_face_reconst_model(seed=1)
