"""Workspace contract harness: no call may read what it has not written, and none may write outside what it was lent.

Every network-level entry point works in a caller-provided workspace that the host allocates once (torch.empty) and hands
to call after call.  Only a few small regions are cleared by the library; everything else is correct only if each kernel
reads what an earlier kernel OF THE SAME CALL wrote.  A reader that breaks this finds, in an ordinary test, the bits the
previous call with the same input left there -- the correct bits.  This module takes that luck away:

  guarded(model)        every workspace tensor of the model (model._ws, Yolov3._det_scratch) becomes a view [G : G + n] of
                        a fresh allocation of n + 2 G bytes whose two guards hold 0xA5; check_guards(model) asserts that
                        both are untouched.  G = 1 MiB, so the view keeps the alignment of the allocation.
  poison(model, how)    'zero': all bytes 0 -- the clean reference;  'nan': all bytes 0xFF -- a NaN as float32 / float64, -1
                        as int32 / int64.  'stale' is not a fill: the caller first runs one complete call of the same shape
                        with another input, other parameters and another target and leaves the result in place
                        (contract_runs lets that call start from 0xFF, so that the state does not depend on the run before).
  poison_outputs(model) the gradient vectors documented as "overwritten" (grads, class_grads) are set to NaN.
  contract_runs(...)    the four runs every test compares: zero, zero again (the clean-to-clean spread), nan, stale.

Plain torch on whatever device the tensors live on: tests/test_workspace_poison_cpu.py drives it with a fake model.
"""
import torch

G = 1 << 20
GUARD_BYTE = 0xA5
HOWS = ('zero', 'zero2', 'nan', 'stale')


def _slots(model):
    """(container, key) of every workspace tensor the model holds."""
    out = [(model._ws, k) for k in list(model._ws)]
    if getattr(model, '_det_scratch', None) is not None:
        out.append((model.__dict__, '_det_scratch'))
    return out


def workspaces(model):
    return [c[k] for c, k in _slots(model)]


def _bytes(t):
    assert t.is_contiguous()
    return t.view(-1).view(torch.uint8)


def release(model):
    """Forget every workspace (and its guards): the next call allocates afresh."""
    model._ws = {}
    model._ws_guards = {}
    if hasattr(model, '_det_scratch'):
        model._det_scratch = None
        model._det_key = None


def guarded(model):
    """Move every workspace tensor that is not guarded yet between two guards.  The contents are not carried over."""
    guards = model.__dict__.setdefault('_ws_guards', {})
    for c, k in _slots(model):
        t = c[k]
        full = guards.get((id(c), k))
        if full is not None and full.data_ptr() + G == t.data_ptr() and full.numel() == _bytes(t).numel() + 2 * G:
            continue
        n = _bytes(t).numel()
        full = torch.empty(n + 2 * G, dtype=torch.uint8, device=t.device)
        full[:G] = GUARD_BYTE
        full[G + n:] = GUARD_BYTE
        c[k] = full[G:G + n].view(t.dtype).view(t.shape)
        assert c[k].data_ptr() == full.data_ptr() + G
        guards[(id(c), k)] = full
    return model


def check_guards(model):
    guards = getattr(model, '_ws_guards', {})
    slots = _slots(model)
    assert slots and len(guards) >= len(slots), 'check_guards: the model has workspaces without guards'
    for c, k in slots:
        t, full = c[k], guards[(id(c), k)]
        n = _bytes(t).numel()
        assert t.data_ptr() == full.data_ptr() + G and full.numel() == n + 2 * G, 'workspace %r was replaced after guarded()' % (k,)
        for name, g, at in (('below', full[:G], -G), ('above', full[G + n:], n)):
            bad = (g != GUARD_BYTE).nonzero()
            assert bad.numel() == 0, ('workspace %r: %d bytes of the guard %s it were written, the first at byte %d of the workspace'
                                      % (k, bad.numel(), name, at + int(bad[0])))


def poison(model, how):
    assert how in ('zero', 'nan'), how
    for t in workspaces(model):
        _bytes(t).fill_(0 if how == 'zero' else 0xFF)


def poison_outputs(model):
    for name in ('grads', 'class_grads'):
        t = getattr(model, name, None)
        if t is not None:
            t.fill_(float('nan'))


def untouched(t):
    """Every byte of t still holds the 'nan' poison: nothing wrote there."""
    return bool((_bytes(t) == 0xFF).all())


def contract_runs(model, call, stale, hows=HOWS):
    """call() -> dict of output tensors (copies), run on the guarded workspaces of `model` from each state of `hows`; stale()
    is the complete call with other data that precedes the 'stale' run.  The guards are checked after every call.
    -> {how: outputs}."""
    guarded(model)
    out = {}
    for how in hows:
        if how == 'stale':
            poison(model, 'nan')                   # what no call writes holds no luck either, whatever ran before
            stale()
            check_guards(model)
        else:
            poison(model, 'zero' if how.startswith('zero') else how)
        poison_outputs(model)
        out[how] = call()
        check_guards(model)
    return out


# ---------------------------------------------------------------------------------------------------------------- comparisons
def assert_finite(name, t):
    t = t if torch.is_tensor(t) else torch.as_tensor(t)
    if t.is_floating_point():
        bad = int((~torch.isfinite(t)).sum())
        assert bad == 0, '%s: %d of %d values are not finite' % (name, bad, t.numel())


def ratio(got, clean):
    """max|got - clean| / max|clean| (NaN where got holds one; the difference itself where clean is all zero)."""
    if got.numel() == 0:
        return 0.0
    d = float((got.double() - clean.double()).abs().max())
    m = float(clean.double().abs().max())
    return d / m if m > 0 else d


def assert_within(name, got, clean, rel, floor=0.0):
    """max|got - clean| <= rel * max|clean| + floor; -> the ratio max|d| / max|clean|.  A NaN fails."""
    assert got.shape == clean.shape and got.dtype == clean.dtype, (name, got.shape, clean.shape)
    if got.numel() == 0:
        return 0.0
    d = float((got.double() - clean.double()).abs().max())
    m = float(clean.double().abs().max())
    assert d <= rel * m + floor, '%s: max difference %.3e of %.3e (bound %.1e relative + %.1e)' % (name, d, m, rel, floor)
    return d / m if m > 0 else 0.0


def grad_segments(model):
    """[(name, slice)] of the flat parameter / gradient vector, one per parameter tensor: kernel, gamma and beta (or bias) of
    every layer, then what the model keeps behind its layers (FidModel: dense kernel and bias)."""
    segs = []
    for l, d in enumerate(model.layers):
        n = d['cout'] * d['ksize'] * d['ksize'] * d['cin']
        segs.append(('dW(%d)' % l, slice(d['w_off'], d['w_off'] + n)))
        if d['has_bn']:
            segs.append(('dgamma(%d)' % l, slice(d['gamma_off'], d['gamma_off'] + d['cout'])))
            segs.append(('dbeta(%d)' % l, slice(d['beta_off'], d['beta_off'] + d['cout'])))
        else:
            segs.append(('dbias(%d)' % l, slice(d['beta_off'], d['beta_off'] + d['cout'])))
    if hasattr(model, 'kernel_off'):
        segs.append(('d dense kernel', slice(model.kernel_off, model.bias_off)))
        segs.append(('d dense bias', slice(model.bias_off, model.n_params)))
    covered = sum(s.stop - s.start for _, s in segs)
    assert covered == model.n_params, (covered, model.n_params)
    return segs
