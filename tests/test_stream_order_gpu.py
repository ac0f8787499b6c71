"""The stream contract on a delayed non-default stream (tests/stream_order.py has the harness and the table).

Every entry point runs once on a fresh stream behind a sleep, with stale-but-valid data in its inputs until a copy on that
stream replaces it: a launch, memset, table upload or zero-fill that is not ordered on the context's stream computes from the
stale problem and the comparison with the reference fails.  Then the step-level joins: what a training step returns is
complete in stream order, Adam may follow it directly, and the bucket reports hand over finished ranges."""
import time

import pytest
import torch

import stream_order as so

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', so.CASES, ids=[c.name for c in so.CASES])
def test_entry_point_on_a_delayed_stream(case):
    so.run_delayed(case)


@pytest.mark.parametrize('case', so.STEP_CASES, ids=[c.name for c in so.STEP_CASES])
def test_step_is_joined_when_it_returns(case):
    """grads, loss and BN state cloned on the stream right after the call equal the serial schedule's, and fv_adam_step enqueued
    directly behind the step reads the gradients a full device synchronise would have shown."""
    so.run_delayed(case)


def _bucket_step(on_side, early_bn):
    """One fv_train_step at (2, 64) with the overlap on, on a delayed stream, with a bucket callback.  -> dict.
    early_bn: option "early_bn_fused".  With it on, the first layer's weight-gradient joins both outstanding weight-gradients
    itself (schedule.h bn_layer_backward); with 0 the step's closing WgradPipe::finish() is the only join of the last two."""
    eng = so.model('engine')
    ctx, dev = eng.ctx, eng.dev
    eng.ensure_optimizer()
    g = so._gen(77)
    real = so._to(dict(x=so._u(g, (2, 64, 64, 3), 0.0, 1.0), yt=so._u(g, (2, 2, 2, 6), 0.0, 1.0)), dev)
    stale = so._to(dict(x=so._u(g, (2, 64, 64, 3), 0.0, 1.0), yt=so._u(g, (2, 2, 2, 6), 0.0, 1.0)), dev)
    side = torch.cuda.ExternalStream(ctx.side_stream(), device=dev)
    scratch = torch.zeros_like(eng.grads)

    def rehearse(off, cnt):                # the callback's own host work, on a buffer of its own: part of the measured host time
        if on_side:
            with torch.cuda.stream(side):
                scratch[off:off + cnt].mul_(2)
        else:
            scratch[off:off + cnt].clone()
    with so._Options(ctx, {'overlap': 0, 'early_bn_fused': early_bn}):
        walls = []
        for _ in range(2):                 # the first run also loads what the callback launches
            so._reset(eng)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.forward_backward(real['x'], real['yt'], on_bucket=rehearse)
            walls.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
        wall = max(walls)
        serial = eng.grads.clone()
    work = {k: v.clone() for k, v in stale.items()}
    ranges, parts = [], []

    def report(off, cnt):
        ranges.append((off, cnt))
        if on_side:                        # stands in for the collective: in place, on the side stream, exact
            with torch.cuda.stream(side):
                eng.grads[off:off + cnt].mul_(2)
        else:                              # on the context's stream, at the moment the range is reported
            parts.append(eng.grads[off:off + cnt].clone())
    torch.cuda.synchronize()
    joined = None
    ctx.set_bucket_on_side(on_side)
    try:
        with so._Options(ctx, {'overlap': 1, 'early_bn_fused': early_bn}):
            with so.delayed_stream(ctx, so.delay_ms(wall)) as d:
                d.sleep()
                for k in work:
                    work[k].copy_(real[k])
                so._reset(eng)
                eng.forward_backward(work['x'], work['yt'], on_bucket=report)
                after = eng.grads.clone()
                sleeping = d.still_sleeping()
                if on_side:
                    d.S.wait_stream(side)          # as parallel.py joins the side stream before Adam
                    joined = eng.grads.clone()
    finally:
        ctx.set_bucket_on_side(False)
    try:
        assert sleeping, 'the step returned after the sleep had ended'
        d.S.synchronize()
    finally:
        torch.cuda.synchronize()
    # the ranges tile [0, n_params) in descending order
    assert ranges[0][0] + ranges[0][1] == eng.n_params and ranges[-1][0] == 0
    assert all(ranges[i][0] == ranges[i + 1][0] + ranges[i + 1][1] for i in range(len(ranges) - 1))
    return dict(eng=eng, serial=serial, ranges=ranges, parts=parts, after=after, joined=joined)


def _close_to_serial(got, serial):
    d = float((got - serial).abs().max())
    assert d <= so.GRAD_REL * float(serial.abs().max()) + so.GRAD_FLOOR, d


@pytest.mark.parametrize('early_bn', [1, 0])
def test_bucket_reports_hand_over_finished_ranges(early_bn):
    """Default mode: a clone of the range enqueued on the context's stream when the callback fires is bit-equal to the same
    range of the gradients after the call (both from one run: no tolerance)."""
    r = _bucket_step(False, early_bn)
    cat = torch.cat(r['parts'][::-1])
    assert cat.numel() == r['eng'].n_params
    assert so.same_bits(cat, r['after'])
    _close_to_serial(r['after'], r['serial'])


@pytest.mark.parametrize('early_bn', [1, 0])
def test_bucket_reports_on_the_side_stream(early_bn):
    """fv_set_bucket_on_side(1): the callback doubles its range in place on the side stream.  WgradPipe::submit records ev_wg
    before the callback, so the step's return joins the weight-gradients, not the callback's work: right after the call every
    element is complete and either not yet doubled or doubled; once the side stream is joined everything is doubled."""
    r = _bucket_step(True, early_bn)
    after, joined = r['after'], r['joined']
    finite = bool(torch.isfinite(joined).all())
    whole = bool(((after == joined) | (after * 2 == joined)).all())      # (plain bools: no tensor reaches the assertion's report)
    assert finite, 'the gradients hold values that are not finite after the side stream was joined'
    assert whole, 'an element behind the step was neither the finished gradient nor its double'
    _close_to_serial(joined / 2, r['serial'])
    done = sum(1 for o, c in r['ranges'] if so.same_bits(after[o:o + c], joined[o:o + c]))
    print('bucket_on_side: %d of %d ranges were already doubled when the clone behind the step ran' % (done, len(r['ranges'])))


def test_zz_report_the_delays():
    print('stream_order: %.0f _sleep cycles per ms, longest delay used %.0f ms' % (so.cycles_per_ms(), so.LONGEST_DELAY_MS[0]))
