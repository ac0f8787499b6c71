"""tests/workspace_poison.py on a fake model (a `_ws` dict of CPU tensors and a Python "call"): the harness passes a call that
writes before it reads, reports one that reads a float it has not written -- under 'nan' and under 'stale' -- and reports a
single byte written into either guard.  No device."""
import pytest
import torch

import workspace_poison as wp

KEY = (1, 16, True)


class FakeModel(object):
    """A workspace of 48 floats: tmp [0, 16), out [16, 32), late [32, 48).  One call: tmp = 2 x; out = 3 tmp + bias;
    late = out * x, written last -- the next call finds it full; the result is out, the gradient its running sum.
    bug 'read':  out[15] is formed from late[0] instead of tmp[15]: a float this call has not written yet.
    bug 'below' / 'above': one byte in front of / behind the workspace is written."""

    def __init__(self, bug=None, scratch=False):
        self.bug = bug
        self._ws = {KEY: torch.empty(48 * 4, dtype=torch.uint8)}
        self.grads = torch.zeros(16)
        if scratch:
            self._det_scratch = torch.empty(8, dtype=torch.float64)
            self._det_key = 'k'

    def run(self, x, bias):
        raw = self._ws[KEY]
        ws = raw.view(torch.float32)
        tmp, out, late = ws[0:16], ws[16:32], ws[32:48]
        tmp.copy_(2.0 * x)
        src = tmp.clone()
        if self.bug == 'read':
            src[15] = late[0]
        out.copy_(3.0 * src + bias)
        late.copy_(out * x)
        if self.bug in ('below', 'above'):
            at = raw.storage_offset() + (-1 if self.bug == 'below' else raw.numel())
            torch.as_strided(raw, (1,), (1,), at).fill_(0)
        self.grads.copy_(torch.cumsum(out, 0))
        return dict(out=out.clone(), grads=self.grads.clone())


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(16, generator=g) + 0.5, torch.rand(16, generator=g)


def _runs(model):
    x, b = _inputs(1)
    x2, b2 = _inputs(2)
    return wp.contract_runs(model, lambda: model.run(x, b), lambda: model.run(x2, b2))


def _verdict(outs):
    """{how: None, or what the comparison with the zero-filled run reports}"""
    res = {}
    for how in ('zero2', 'nan', 'stale'):
        try:
            for name, t in outs[how].items():
                wp.assert_finite('%s %s' % (how, name), t)
                wp.assert_within('%s %s' % (how, name), t, outs['zero'][name], 1e-6)
            res[how] = None
        except AssertionError as e:
            res[how] = str(e)
    return res


def test_a_call_that_writes_before_it_reads_passes_under_every_poison():
    m = FakeModel()
    outs = _runs(m)
    assert sorted(outs) == sorted(wp.HOWS)
    assert _verdict(outs) == dict(zero2=None, nan=None, stale=None)
    x, b = _inputs(1)
    assert torch.equal(outs['nan']['out'], 3.0 * (2.0 * x) + b)
    wp.check_guards(m)


def test_a_float_read_before_it_is_written_is_reported_under_nan_and_under_stale():
    outs = _runs(FakeModel(bug='read'))
    v = _verdict(outs)
    assert v['zero2'] is None                      # zero-filled runs agree with each other: the ordinary suite's view of the bug
    assert v['nan'] is not None and 'not finite' in v['nan'], v
    assert v['stale'] is not None and 'max difference' in v['stale'], v
    # and the on/off style of test -- the same input twice in one workspace -- does not see it
    m = FakeModel(bug='read')
    x, b = _inputs(1)
    m.run(x, b)
    first = m.run(x, b)
    assert torch.equal(m.run(x, b)['out'], first['out'])


@pytest.mark.parametrize('side', ['below', 'above'])
def test_one_byte_written_into_a_guard_is_reported(side):
    with pytest.raises(AssertionError, match='guard %s' % side):
        _runs(FakeModel(bug=side))


def test_the_gradient_vector_is_poisoned_before_every_run():
    m = FakeModel()
    seen = []
    x, b = _inputs(1)

    def call():
        seen.append(bool(torch.isnan(m.grads).all()))
        return m.run(x, b)
    wp.contract_runs(m, call, lambda: m.run(*_inputs(2)))
    assert seen == [True] * 4


def test_guards_fills_and_the_detection_scratch():
    m = FakeModel(scratch=True)
    before = m._ws[KEY]
    assert wp.guarded(m) is m
    ws, scr = m._ws[KEY], m._det_scratch
    assert ws.data_ptr() != before.data_ptr() and ws.shape == before.shape and ws.dtype == torch.uint8
    assert scr.dtype == torch.float64 and scr.shape == (8,)
    full = m._ws_guards[(id(m._ws), KEY)]
    assert full.numel() == ws.numel() + 2 * wp.G and ws.data_ptr() == full.data_ptr() + wp.G and wp.G % 256 == 0
    assert bool((full[:wp.G] == 0xA5).all()) and bool((full[wp.G + ws.numel():] == 0xA5).all())
    wp.guarded(m)                                   # a second call leaves guarded workspaces where they are
    assert m._ws[KEY].data_ptr() == ws.data_ptr()
    wp.poison(m, 'nan')
    assert bool(torch.isnan(ws.view(torch.float32)).all()) and bool(torch.isnan(scr).all())
    assert bool((ws.view(torch.int32) == -1).all()) and bool((scr.view(torch.int64) == -1).all())
    assert wp.untouched(ws) and wp.untouched(scr[2:4])
    ws.view(torch.float32)[7] = 1.0
    assert not wp.untouched(ws)
    wp.poison(m, 'zero')
    assert not ws.any() and not scr.any()
    wp.check_guards(m)
    m._ws[KEY] = torch.empty(48 * 4, dtype=torch.uint8)       # the host reallocated: the guards no longer stand around it
    with pytest.raises(AssertionError, match='replaced'):
        wp.check_guards(m)
    wp.release(m)
    assert m._ws == {} and m._det_scratch is None and m._det_key is None
    with pytest.raises(AssertionError):
        wp.check_guards(m)                          # nothing to check is no pass


def test_comparisons_fail_on_nan_and_on_the_bound():
    clean = torch.tensor([1.0, -4.0, 0.5], dtype=torch.float64)
    assert wp.assert_within('t', clean + torch.tensor([0.0, 0.0, 2e-6], dtype=torch.float64), clean, 1e-6) == pytest.approx(5e-7)
    with pytest.raises(AssertionError):
        wp.assert_within('t', clean + torch.tensor([0.0, 0.0, 8e-6], dtype=torch.float64), clean, 1e-6)
    with pytest.raises(AssertionError):
        wp.assert_within('t', torch.tensor([1.0, float('nan'), 0.5], dtype=torch.float64), clean, 1e-6)
    with pytest.raises(AssertionError):
        wp.assert_finite('t', torch.tensor([1.0, float('inf')]))
    wp.assert_finite('t', torch.tensor([3, -1], dtype=torch.int32))
    assert wp.assert_within('t', torch.zeros(3), torch.zeros(3), 1e-5, 1e-9) == 0.0
    assert wp.ratio(clean * 1.5, clean) == pytest.approx(0.5) and wp.ratio(torch.zeros(0), torch.zeros(0)) == 0.0


def test_gradient_segments_cover_the_detector_layout():
    from face_vijnana_yolov3_amd import engine
    from face_vijnana_yolov3_amd._lib import lib

    class Layout(object):
        layers = engine.layer_table()
        n_params = int(lib().fv_param_count())
    segs = wp.grad_segments(Layout)
    assert len(segs) == 3 * 52 + 2 and segs[0][0] == 'dW(0)' and segs[-1][0] == 'dbias(52)'
    assert segs[0][1] == slice(0, 32 * 27) and segs[-1][1].stop == Layout.n_params
