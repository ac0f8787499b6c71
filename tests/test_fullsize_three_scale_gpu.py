"""Full-size checks of the three-scale step (416x416, 255 output channels, batch 16 -- bench.py's secondary configuration) where
the CPU oracle cannot run in seconds: size-independent properties, as tests/test_fullsize_gpu.py has them for the single head."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, OUT = 16, 416, 255


@pytest.fixture(scope='module')
def net():
    from face_vijnana_yolov3_amd.yolov3 import Yolov3
    m = Yolov3(0, out_channels=OUT)
    m.init_synthetic(seed=3)
    return m


@pytest.fixture(scope='module')
def batch(net):
    """Images and targets as bench.py's three-scale measurement draws them, with one amendment.  The box term |t - y| has a kink
    where a logit equals its target: two summation orders of the same step (a permuted batch) move the logits by ~1e-6 relative,
    and of the 6.2 M box entries a few lie that close to their uniform target -- there the gradient entry flips sign, one
    2 * 0.25 / (3 nbox) step in one dy entry, which is no property of the kernels (measured before the amendment: the conv_105
    kernel gradients of a permuted batch differed by 2.4e-4 of their max in ONE output channel, a box entry, its bias gradient
    by exactly one such step; every other channel agreed to 7e-7).  So the training-mode logits are recomputed from the kept
    input of each detection conv, and a box target within 1e-3 (1 + |t|) of its logit is moved a whole unit away.  The logits
    do not depend on the targets, so every box entry then has a margin a thousand times the rounding between two orders."""
    from face_vijnana_yolov3_amd import ops
    g = torch.Generator().manual_seed(4321)
    x = torch.rand((B, S, S, 3), generator=g).cuda()
    tg = []
    for d in (32, 16, 8):
        t = torch.rand((B, S // d, S // d, OUT), generator=g)
        t5 = t.view(B, S // d, S // d, 3, OUT // 3)
        t5[..., 4] = (t5[..., 4] > 0.9).float(); t5[..., 5:] = (t5[..., 5:] > 0.98).float()
        tg.append(t.cuda())
    p0, s0 = net.params.clone(), net.state.clone()
    net.forward_backward(x, tg)
    moved = 0
    for li, d in enumerate(net.layers):
        if d['has_bn']:
            continue
        assert net.layers[li - 1]['darknet_index'] == d['darknet_index'] - 1 and d['ksize'] == 1
        gs = S // d['in_div']
        a = net._train_tensor(B, S, li - 1, 1).view(B, gs, gs, d['cin'])
        w = net.params[d['w_off']:d['w_off'] + d['cout'] * d['cin']].view(d['cout'], 1, 1, d['cin'])
        y = ops.conv2d_forward(net.ctx, a, w, 1, None, net.params[d['beta_off']:d['beta_off'] + d['cout']].contiguous(), -1.0, None)
        yb = y.view(B, gs, gs, 3, OUT // 3)[..., :4]
        tb = tg[{32: 0, 16: 1, 8: 2}[d['in_div']]].view(B, gs, gs, 3, OUT // 3)[..., :4]
        near = (yb - tb).abs() < 1e-3 * (1.0 + yb.abs())
        moved += int(near.sum())
        tb.copy_(torch.where(near, yb + 1.0 + 0.01 * yb.abs(), tb))
    print('box targets moved off the kink: %d' % moved)
    net.set_params(p0, s0)
    net.grads = net.m = net.v = None
    net.iterations = 0; net.bn_updates = 0
    torch.cuda.synchronize()
    return x, tg


def test_inference_is_per_image_and_deterministic(net, batch):
    """Inference-mode BN is per sample: the three outputs of a batch predicted in two parts (7 + 9: other tile counts and tails)
    reproduce the full batch to fp32 rounding, and repeated calls are bit-identical."""
    x, _ = batch
    ys = [y.clone() for y in net.predict_device(x)]
    ys2 = [y.clone() for y in net.predict_device(x)]
    ya = [y.clone() for y in net.predict_device(x[:7].contiguous())]
    yb = [y.clone() for y in net.predict_device(x[7:].contiguous())]
    for s, g in enumerate((13, 26, 52)):
        assert tuple(ys[s].shape) == (B, g, g, OUT) and torch.isfinite(ys[s]).all()
        assert torch.equal(ys[s], ys2[s]), s
        d = (torch.cat([ya[s], yb[s]]) - ys[s]).abs().max().item()
        assert d <= 2e-5 * ys[s].abs().max().item(), (s, d)


def test_train_step_batch_permutation_invariance(net, batch):
    """Batch statistics, the loss and every gradient are symmetric in the batch order.  The three detection convs have no BN or
    LeakyReLU behind them: kernel and bias gradients within 1e-4 of their max; every BN layer at the measured conditioning of the
    randomly initialised network (tests/test_fullsize_gpu.py: 6e-2)."""
    x, tg = batch
    p0, s0 = net.params.clone(), net.state.clone()
    net.grads = net.m = net.v = None
    l1 = net.forward_backward(x, tg).clone(); g1 = net.grads.clone(); st1 = net.state.clone()
    net.set_params(p0, s0)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    l2 = net.forward_backward(x[perm].contiguous(), [t[perm].contiguous() for t in tg]).clone(); g2 = net.grads.clone()
    torch.cuda.synchronize()
    print('loss %.9g permuted %.9g' % (l1.item(), l2.item()))
    assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
    torch.testing.assert_close(net.state, st1, rtol=1e-5, atol=1e-7)
    ndet = 0
    for li, d in enumerate(net.layers):
        n = d['cout'] * d['ksize'] ** 2 * d['cin']
        a, b = g1[d['w_off']:d['w_off'] + n], g2[d['w_off']:d['w_off'] + n]
        tol = 6e-2 if d['has_bn'] else 1e-4
        assert (a - b).abs().max().item() <= tol * a.abs().max().item() + 1e-12, (d['darknet_index'], li)
        if not d['has_bn']:
            ndet += 1
            a, b = g1[d['beta_off']:d['beta_off'] + d['cout']], g2[d['beta_off']:d['beta_off'] + d['cout']]
            assert (a - b).abs().max().item() <= 1e-4 * a.abs().max().item() + 1e-12, (d['darknet_index'], li, 'bias')
    assert ndet == 3
    net.set_params(p0, s0)


def test_gradient_matches_directional_derivative(net, batch):
    """Forward and backward kernels agree at full size: along the normalised gradient direction d,
    (L(p + e d) - L(p - e d)) / 2e  ==  <g, d> = |g|  (training-mode forward, fp32), within 5 % for one of two step sizes."""
    x, tg = batch
    p0, s0 = net.params.clone(), net.state.clone()
    net.grads = net.m = net.v = None
    net.forward_backward(x, tg)
    g = net.grads.clone().double()
    gn = g.norm().item()
    d = (g / gn).float()
    ratios = []
    for e in (2e-3, 5e-3):
        net.set_params(p0 + e * d, s0); lp = net.forward_backward(x, tg).item()
        net.set_params(p0 - e * d, s0); lm = net.forward_backward(x, tg).item()
        ratios.append((lp - lm) / (2 * e) / gn)
    net.set_params(p0, s0)
    print('directional derivative / |g| at e = 2e-3, 5e-3:', ratios, '|g| = %.6g' % gn)
    assert min(abs(r - 1.0) for r in ratios) < 0.05, ratios
