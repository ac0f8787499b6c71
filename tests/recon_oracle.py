"""The reconstruction model of the reference (face_identification.py:1155-1488, create_face_reconst_model) restated in torch on the
CPU, in float64 or float32 -- Keras is not importable here, so this restatement is what the device path is pinned against:

  head   u = relu(l2_normalize(ids));  x = u . K^T + b, reshaped to (N, g, g, 1024);  skip = x
  stage  y = BN_l(l2_normalize_channels(leaky_relu(x, 0.1)));  x = conv_transpose_l(y)
  order  layers 51 .. 2 of the layer table: a stride-2 layer is one stage, then skip = x; every other layer comes as a residual
         block's 3x3 then its 1x1: two stages, then x = x - skip, skip = x.  Then stage(1), stage(0).

l2_normalize is TF 1.13's x * rsqrt(max(sum x^2, 1e-12)); BN is inference-mode with eps 1e-3; conv_transpose is TF's
conv2d_transpose with 'SAME' padding: for stride 2, conv_transpose2d(x, w, stride=2)[:, :, :2H, :2W].
Kernels are OHWI (cout, k, k, cin) as in the flat parameter vector."""
import numpy as np
import torch
import torch.nn.functional as F_

BN_EPS = 1e-3
LEAKY = 0.1


def l2_normalize(x, dim=-1):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim, keepdim=True), min=1e-12))


def head(ids, K, b):
    """ids (N,64), K (F,64) the dense1 kernel, b (F,) -> (N,F)."""
    return torch.relu(l2_normalize(ids)) @ K.t() + b


def conv_transpose(x, w, stride):
    """x (N,H,W,cout) NHWC, w OHWI (cout,k,k,cin) -> (N,H*stride,W*stride,cin): Conv2DTranspose(cin, k, stride, 'same', no bias)."""
    k = w.shape[1]
    wt = w.permute(0, 3, 1, 2)                       # torch: (in_channels = cout, out_channels = cin, kH, kW)
    xn = x.permute(0, 3, 1, 2)
    if stride == 1:
        y = F_.conv_transpose2d(xn, wt, stride=1, padding=(k - 1) // 2)
    else:
        H, W = x.shape[1], x.shape[2]
        y = F_.conv_transpose2d(xn, wt, stride=2)[:, :, :2 * H, :2 * W]
    return y.permute(0, 2, 3, 1).contiguous()


def conv_s2_grad(g, w, in_hw, pad):
    """Gradient, by autograd, w.r.t. the input x (N,H,W,cin) of conv2d(zero_pad(x, pad), w, stride=2) for the output gradient g
    (N,H/2,W/2,cout), H and W even.  pad = (0, 1): a 'SAME' stride-2 conv; pad = (1, 1): ZeroPadding2D(1) + 'valid', as this
    network's stride-2 layers."""
    N, (H, W), cin = g.shape[0], in_hw, w.shape[3]
    x = torch.zeros((N, cin, H, W), dtype=g.dtype, requires_grad=True)
    z = F_.conv2d(F_.pad(x, (pad[0], pad[1], pad[0], pad[1])), w.permute(0, 3, 1, 2), stride=2)
    assert z.shape[2:] == (H // 2, W // 2)
    (z * g.permute(0, 3, 1, 2)).sum().backward()
    return x.grad.permute(0, 2, 3, 1).contiguous()


def stage_input(x, bn):
    """LeakyReLU -> per-pixel l2_normalize over channels -> inference BN (gamma, beta, mean, var).  Also the smallest pixel norm
    that entered the normalise."""
    l = torch.where(x > 0, x, x * LEAKY)
    nrm = torch.sqrt((l * l).sum(-1)).min().item()
    gamma, beta, mean, var = bn
    return (l2_normalize(l) - mean) / torch.sqrt(var + BN_EPS) * gamma + beta, nrm


def schedule(layers):
    """[('stage', l) | ('skip',) | ('subtract',)] in run order, from the layer table alone."""
    ops = []
    l = len(layers) - 1
    while l >= 2:
        if layers[l]['stride'] == 2:
            ops += [('stage', l), ('skip',)]
            l -= 1
        else:
            assert layers[l]['ksize'] == 3 and layers[l - 1]['ksize'] == 1, l
            ops += [('stage', l), ('stage', l - 1), ('subtract',)]
            l -= 2
    assert l == 1
    return ops + [('stage', 1), ('stage', 0)]


def stage_conv_indices(layers):
    return [layers[op[1]]['darknet_index'] for op in schedule(layers) if op[0] == 'stage']


def forward(P, ids, layers, S, n_stages=None):
    """P: dict(kernels=[OHWI per layer], K (F,64), b (F,), bn=[(gamma, beta, mean, var) per layer]) in one dtype; ids (N,64).
    -> (out (N,S,S,3), smallest pixel norm that entered any normalise).  n_stages: stop after that many stages (x so far)."""
    g = S // 32
    x = head(ids, P['K'], P['b']).reshape(ids.shape[0], g, g, layers[-1]['cout'])
    skip = x
    min_norm, done = float('inf'), 0
    for op in schedule(layers):
        if n_stages is not None and done == n_stages:
            break
        if op[0] == 'stage':
            l = op[1]
            y, nrm = stage_input(x, P['bn'][l])
            min_norm = min(min_norm, nrm)
            x = conv_transpose(y, P['kernels'][l], layers[l]['stride'])
            done += 1
        elif op[0] == 'skip':
            skip = x
        else:
            x = x - skip
            skip = x
    return x, min_norm


def make_base(layers, seed, random_bn):
    """The part of the parameters that does not depend on the image size, in float64: He-scaled random kernels; BN fresh (gamma 1,
    beta 0, mean 0, var 1) or random (gamma in [0.8, 1.2], beta and mean ~ 0.1 N(0,1), var in [0.5, 1.5]).  Every value is a
    float32 number (the device holds float32), so both precisions of the oracle start from the same parameters."""
    gen = torch.Generator().manual_seed(seed)
    kernels, bn = [], []
    for d in layers:
        k, cin, cout = d['ksize'], d['cin'], d['cout']
        kernels.append((torch.randn((cout, k, k, cin), generator=gen) * float(np.sqrt(2.0 / (k * k * cin)))).double())
        if random_bn:
            q = (0.8 + 0.4 * torch.rand(cout, generator=gen), 0.1 * torch.randn(cout, generator=gen), 0.1 * torch.randn(cout, generator=gen),
                 0.5 + torch.rand(cout, generator=gen))
        else:
            q = (torch.ones(cout), torch.zeros(cout), torch.zeros(cout), torch.ones(cout))
        bn.append(tuple(v.double() for v in q))
    return dict(kernels=kernels, bn=bn)


def make_params(base, layers, S, seed):
    """base (make_base) + a glorot-uniform dense kernel and the bias np.random.RandomState(seed).rand(F) as float32."""
    gen = torch.Generator().manual_seed(seed)
    Fs = (S // 32) ** 2 * layers[-1]['cout']
    K = ((torch.rand((Fs, 64), generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (Fs + 64)))).double()
    b = torch.from_numpy(np.random.RandomState(seed).rand(Fs).astype(np.float32)).double()
    return dict(kernels=base['kernels'], bn=base['bn'], K=K, b=b)


def make_ids(N, seed):
    g = torch.Generator().manual_seed(seed)
    return l2_normalize(torch.relu(torch.randn((N, 64), generator=g, dtype=torch.float64))).float().double()

