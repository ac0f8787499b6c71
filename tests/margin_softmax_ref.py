"""fv_fid_margin_softmax_loss_grad's contract (include/fv_hotpath.h) restated in numpy, float64 throughout,
the gradient written out; `autograd` is the same definition in torch float64 for autograd to differentiate (the CPU test compares
the two).  Test infrastructure: the product does not import it.  Also the cases the CPU and GPU tests share."""
import functools

import numpy as np

from batch_triplet_ref import l2_relu_bwd, l2n_relu

DIM = 64
KIND_COSFACE, KIND_ARCFACE = 0, 1
DEFAULT_MARGIN = {KIND_COSFACE: 0.35, KIND_ARCFACE: 0.5}


def l2n_relu64(pre):
    """The unrounded u of float64 pre-activations."""
    r = np.maximum(np.asarray(pre, np.float64), 0.0)
    return r / np.sqrt(np.maximum((r * r).sum(-1, keepdims=True), 1e-12))


def normalise_classes(W):
    """-> w^ (C, 64), inv (C,), live (C,) bool: the l2_normalize rule, the constant 1e6 where sum w^2 <= 1e-12."""
    W = np.asarray(W, np.float64)
    ss = (W * W).sum(-1)
    live = ss > 1e-12
    inv = np.where(live, 1.0 / np.sqrt(np.where(live, ss, 1.0)), 1e6)
    return W * inv[:, None], inv, live


def margin_of(t, kind, m):
    """psi(t), psi'(t) of a clamped target cosine t (arrays)."""
    if kind == KIND_COSFACE:
        return t - m, np.ones_like(t)
    q = 1.0 - t * t
    sn = np.sqrt(np.maximum(q, 1e-12))
    main = t > np.cos(np.pi - m)
    psi = np.where(main, t * np.cos(m) - sn * np.sin(m), t - m * np.sin(np.pi - m))
    dpsi = np.where(main, np.cos(m) + np.where(q > 1e-12, t * np.sin(m) / sn, 0.0), 1.0)
    return psi, dpsi


def margin_softmax(pre, u, labels, W, kind, scale, margin, weight=1.0):
    """-> dict(loss, dE (M, 64), dbias (64,), dW (C, 64), pred (M,), cos_t (M,), cos (M, C), V, dpre = dE / weight): float64.  pre
    may be float32 or float64; u is taken as given (float32 as the dense call hands it over, or the unrounded float64)."""
    pre = np.asarray(pre)
    u = np.asarray(u, np.float64)
    W = np.asarray(W, np.float64)
    labels = np.asarray(labels, np.int64)
    M, C = len(u), len(W)
    wh, inv, live = normalise_classes(W)
    cos = u @ wh.T
    pred = np.argmax(cos, axis=1).astype(np.int32)         # the first maximum: the lowest c among equals
    pred[labels >= C] = -2
    valid = (labels >= 0) & (labels < C)
    rows = np.flatnonzero(valid)
    V = len(rows)
    cos_t = np.full(M, np.nan)
    G = np.zeros((M, C))
    loss = 0.0
    if V:
        y = labels[rows]
        cy = cos[rows, y]
        cos_t[rows] = cy
        t = np.clip(cy, -1.0, 1.0)
        dclamp = ((cy >= -1.0) & (cy <= 1.0)).astype(np.float64)
        psi, dpsi = margin_of(t, kind, margin)
        z = scale * cos[rows]
        z[np.arange(V), y] = scale * psi
        mx = z.max(1, keepdims=True)
        e = np.exp(z - mx)
        se = e.sum(1, keepdims=True)
        loss = float(((mx[:, 0] + np.log(se[:, 0])) - z[np.arange(V), y]).sum() / V)
        g = e / se
        g[np.arange(V), y] -= 1.0
        g *= scale / V
        g[np.arange(V), y] *= dpsi * dclamp
        G[rows] = g
    dU = G @ wh
    dpre = l2_relu_bwd(pre, dU, 1.0)
    dE = l2_relu_bwd(pre, dU, weight)
    dWh = G.T @ u
    dW = np.where(live[:, None], inv[:, None] * (dWh - wh * (wh * dWh).sum(-1, keepdims=True)), dWh * 1e6) * weight
    return dict(loss=loss, dE=dE, dpre=dpre, dW=dW, pred=pred, cos_t=cos_t, cos=cos, V=V, G=G)


def stored(out):
    """What the device stores: dbias is the column sums of the dE rows AS STORED (float32)."""
    out = dict(out)
    out['dbias'] = out['dE'].astype(np.float32).astype(np.float64).sum(0)
    return out


def autograd(pre, labels, W, kind, scale, margin):
    """The definition in torch float64 -> (loss, d pre, dW) by autograd, u = l2_normalize(relu(pre)) unrounded."""
    import torch
    pre = torch.tensor(np.asarray(pre, np.float64), requires_grad=True)
    W = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    loss = torch_loss(pre, torch.as_tensor(np.asarray(labels, np.int64)), W, kind, scale, margin)
    if not loss.requires_grad:
        return 0.0, np.zeros(pre.shape), np.zeros(W.shape)
    gp, gw = torch.autograd.grad(loss, [pre, W], allow_unused=True)
    zero = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
    return float(loss.detach()), zero(gp, pre), zero(gw, W)


def torch_l2n(x):
    import torch
    ss = (x * x).sum(-1, keepdim=True)
    return x * torch.where(ss > 1e-12, torch.rsqrt(torch.clamp(ss, min=1e-12)), torch.full_like(ss, 1e6))


def torch_loss_of_u(u, labels, W, kind, scale, margin):
    """The loss of facial IDs u (M, 64) and the class kernel W in torch, any float dtype: differentiable."""
    import torch
    cos = u @ torch_l2n(W).T
    valid = (labels >= 0) & (labels < W.shape[0])
    rows = torch.nonzero(valid).reshape(-1)
    if len(rows) == 0:
        return torch.zeros((), dtype=u.dtype)
    y = labels[rows]
    idx = torch.arange(len(rows))
    t = torch.clamp(cos[rows, y], -1.0, 1.0)
    if kind == KIND_COSFACE:
        psi = t - margin
    else:
        q = 1.0 - t * t
        safe = torch.where(q > 1e-12, q, torch.ones_like(q))
        sn = torch.where(q > 1e-12, torch.sqrt(safe), torch.full_like(q, 1e-6))      # a constant where q <= 1e-12: gradient 0
        psi = torch.where(t > float(np.cos(np.pi - margin)), t * float(np.cos(margin)) - sn * float(np.sin(margin)),
                          t - margin * float(np.sin(np.pi - margin)))
    z = scale * cos[rows]
    z = z.clone()
    z[idx, y] = scale * psi
    return (torch.logsumexp(z, dim=1) - z[idx, y]).mean()


def torch_loss(pre, labels, W, kind, scale, margin):
    import torch
    return torch_loss_of_u(torch_l2n(torch.relu(pre)), labels, W, kind, scale, margin)


# ----------------------------------------------------------------------------- cases
def random_case(M, C, seed, unknown=1.0 / 7):
    """Random normal pre, W at 0.1 scale, about a seventh of the labels -1; with M >= 2 one dead row (every pre <= 0, labelled),
    with C >= 2 one zero class row that some row is labelled with -> pre (float32), labels (int32), W (float32)."""
    rng = np.random.RandomState(seed)
    pre = rng.standard_normal((M, DIM)).astype(np.float32)
    W = (0.1 * rng.standard_normal((C, DIM))).astype(np.float32)
    labels = rng.randint(0, C, M).astype(np.int32)
    labels[rng.rand(M) < unknown] = -1
    if M >= 2:
        pre[M // 2] = -np.abs(pre[M // 2])
        labels[M // 2] = C // 2
    if C >= 2:
        W[C - 1] = 0.0
        labels[0] = C - 1
    return pre, labels, W


@functools.lru_cache(maxsize=None)
def searched_case(M, C, kind, scale=30.0, first_seed=0):
    """random_case with the first seed at which the restatement's top-two cosines differ by more than 1e-9 in every row and every
    target cosine keeps 1e-6 from -1, 1 and cos(pi - m) -> (pre, u, labels, W, want, seed); want is computed on the float32 u."""
    m = DEFAULT_MARGIN[kind]
    for seed in range(first_seed + 1000 * M + C, first_seed + 1000 * M + C + 50):
        pre, labels, W = random_case(M, C, seed)
        u = l2n_relu(pre)
        want = stored(margin_softmax(pre, u, labels, W, kind, scale, m))
        if well_separated(want, m, C):
            return pre, u, labels, W, want, seed
    raise AssertionError('no seed found for M=%d C=%d' % (M, C))


def well_separated(want, m, C, gap=1e-9, branch=1e-6):
    if C >= 2:
        # a row whose u is exactly 0 has cosines of exactly 0 in any summation order: the tie rule (the lowest c) decides alike
        cos = want['cos'][want['cos'].any(axis=1)]
        top = np.sort(cos, axis=1)[:, -2:]
        if not (top[:, 1] - top[:, 0] > gap).all():
            return False
    ct = want['cos_t'][~np.isnan(want['cos_t'])]
    return all((np.abs(ct - p) > branch).all() for p in (-1.0, 1.0, np.cos(np.pi - m)))


def _e(k, s=1.0):
    v = np.zeros(DIM, np.float32)
    v[k] = s
    return v


def hand_cases():
    """name -> dict(pre, labels, W): float32 / int32.  u = l2n_relu(pre)."""
    rng = np.random.RandomState(4)
    rnd = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    cases = {}
    # one class: the softmax has one entry, p = 1 -- loss 0 and every gradient 0
    cases['one_class'] = dict(pre=rnd(3, DIM), labels=[0, 0, -1], W=rnd(1, DIM))
    cases['all_unknown'] = dict(pre=rnd(4, DIM), labels=[-1, -3, -1, -2], W=rnd(5, DIM))
    dead = rnd(3, DIM)
    dead[1] = -np.abs(dead[1])
    cases['dead_row'] = dict(pre=dead, labels=[0, 1, 2], W=rnd(3, DIM))
    tiny = rnd(4, DIM)
    tiny[2] = 1e-8 * tiny[2]                                   # 0 < sum w^2 <= 1e-12
    tiny[3] = 0.0
    cases['tiny_class_rows'] = dict(pre=rnd(5, DIM), labels=[2, 3, 0, 1, 2], W=tiny)
    # u = e0 exactly and w_y = 2 e0: the target cosine is exactly 1 in any summation order (q = 0 <= 1e-12)
    cases['target_cosine_one'] = dict(pre=np.stack([_e(0, 3.0), rnd(DIM)]), labels=[0, 1], W=np.stack([_e(0, 2.0), rnd(DIM), rnd(DIM)]))
    # u = e0, w_y = -e0: the target cosine is exactly -1, below cos(pi - m): ArcFace's fallback branch
    cases['target_cosine_minus_one'] = dict(pre=np.stack([_e(0, 3.0), rnd(DIM)]), labels=[0, 1], W=np.stack([_e(0, -1.0), rnd(DIM), rnd(DIM)]))
    for c in cases.values():
        c['pre'] = np.asarray(c['pre'], np.float32)
        c['labels'] = np.asarray(c['labels'], np.int32)
        c['W'] = np.asarray(c['W'], np.float32)
    return cases
