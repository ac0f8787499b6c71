"""The stream contract of the C ABI (include/fv_hotpath.h at fv_set_stream), checked on a delayed non-default stream.

Every test of the suite binds its context to the null stream, where a launch on stream 0, a memset on the wrong stream or a
wrapper that zero-fills on another stream than the kernel that accumulates are all invisible.  run_delayed() takes that luck
away for one entry point:

  1. two valid problems of one shape, `real` (seed) and `stale` (seed + 1), are built on the default stream.  Indices, labels,
     offsets, geometry and counts are the same valid values in both; only pixels, activations, coefficients and targets differ;
  2. the call runs on the context's ordinary stream for both and every output of `real` must differ from `stale` by more than
     100 x the comparison tolerance (bitwise for exact cases): a case that cannot tell the problems apart is rejected;
  3. on a fresh stream S (torch.cuda.stream(S) + ctx.set_stream, restored in `finally`) the input buffers hold `stale`; a
     torch.cuda._sleep of max(20 ms, 4 x the call's host time), capped at 500 ms, is enqueued, an event recorded, `real` copied
     into the inputs device to device, the call made and every output cloned on S at once;
  4. entry points that do not synchronise the host must return while the sleep still runs (`not ev_sleep.query()`): everything
     was enqueued while the inputs held `stale`, so whatever is not ordered behind the copy on S has consumed stale data;
  5. after S.synchronize() (not a device synchronise) the clones are compared with the `real` reference.

The table CASES is keyed by ABI symbol; tests/test_stream_order_cpu.py keeps it complete against the header.  Nothing in here
needs a GPU to import.  No graph capture, one process, nothing runs in a loop until it fails.
"""
import contextlib
import ctypes
import time

import numpy as np
import torch

DELAY_MIN_MS, DELAY_MAX_MS, DELAY_FACTOR = 20.0, 500.0, 4.0
STAT_REL = 1e-6                       # fp64-atomic statistics: tests/test_workspace_contract_gpu.py
GRAD_REL, GRAD_FLOOR = 1e-5, 1e-9     # float-atomic dW of a whole step: test_net_gpu.test_side_stream_overlap_equals_serial
LOSS_REL = 1e-6

# Declared symbols that enqueue nothing: host getters / setters and the pure-CPU JPEG front end.
EXEMPT = {
    'fv_abi_version': 'host getter',
    'fv_create': 'makes the context; enqueues one event pair at most',
    'fv_destroy': 'host teardown',
    'fv_last_error': 'host getter',
    'fv_set_stream': 'the harness itself calls it around every case',
    'fv_set_bucket_on_side': 'host setter (its effect is tested by the bucket tests)',
    'fv_side_stream': 'host getter',
    'fv_set_bn_zero_debias_step': 'host setter',
    'fv_set_option': 'host setter',
    'fv_get_option': 'host getter',
    'fv_set_conv_scratch': 'host setter (the tail-split case lends the scratch through it)',
    'fv_profile_enable': 'host setter',
    'fv_det_ap_sweep_workspace_bytes': 'size query',
    'fv_num_layers': 'host getter',
    'fv_layer': 'host getter',
    'fv_param_count': 'host getter',
    'fv_state_count': 'host getter',
    'fv_workspace_bytes': 'size query',
    'fv_train_workspace_tensor': 'layout query',
    'fv_conv2d_stat_rows': 'size query',
    'fv_bn_bwd_scratch_floats': 'size query',
    'fv_bn_stat_slots': 'size query',
    'fv_train_bn_in_1x1_plan': 'plan query, needs no device',
    'fv_yolov3_train_bn_in_1x1_plan': 'plan query, needs no device',
    'fv_colsum_partial_doubles': 'size query',
    'fv_yolo_loss_partial_doubles': 'size query',
    'fv_jpeg_parse': 'pure host code',
    'fv_jpeg_entropy_decode': 'pure host code',
    'fv_jpeg_plane_bytes': 'size query',
    'fv_jpeg_encode_workspace_bytes': 'size query',
    'fv_fid_param_count': 'host getter',
    'fv_fid_workspace_bytes': 'size query',
    'fv_fid_train_step_dp': 'the data-parallel form: covered by the multi-rank tests (test_fid_dp_gpu.py)',
    'fv_fid_dense_partial_floats': 'size query',
    'fv_fid_batch_workspace_bytes': 'size query',
    'fv_fid_margin_workspace_bytes': 'size query',
    'fv_fid_cls_workspace_bytes': 'size query',
    'fv_recon_param_count': 'host getter',
    'fv_recon_workspace_bytes': 'size query',
    'fv_yolov3_num_layers': 'host getter',
    'fv_yolov3_layer': 'host getter',
    'fv_yolov3_param_count': 'host getter',
    'fv_yolov3_state_count': 'host getter',
    'fv_yolov3_workspace_bytes': 'size query',
    'fv_yolov3_train_workspace_bytes': 'size query',
    'fv_yolov3_train_workspace_tensor': 'layout query',
    'fv_yolov3_train_workspace_head': 'layout query',
    'fv_yolo_det_scratch_bytes': 'size query',
}


class Case(object):
    """One row of the table.  make(seed, device) -> dict of input tensors; call(ctx, inputs) -> dict of outputs (device tensors,
    or host objects for entry points that hand back host data).  host_sync: a one-line reason when the entry point waits for
    the stream by design (step 4 is skipped, nothing else).  tol(ctx, name, ref, inputs) -> the allowed |difference| of output
    `name` (a number or a tensor; 0: bit-exact); None: every output is bit-exact.  may_tie: outputs (counts, indices, flags)
    that two valid problems may share, excused from step 2 alone.  options / ref_options: context options of the delayed run
    and of the reference runs.  ctx(): the context the call runs on.  extra / post: see run_delayed."""

    def __init__(self, name, symbols, make, call, host_sync=None, tol=None, may_tie=(), ctx=None, options=None, ref_options=None,
                 extra=None, post=None, ref64=None):
        self.name, self.symbols, self.make, self.call = name, tuple(symbols), make, call
        self.host_sync, self.tol, self.may_tie = host_sync, tol, tuple(may_tie)
        self.ctx = ctx or shared_ctx
        self.options, self.ref_options = dict(options or {}), dict(ref_options or {})
        self.extra, self.post, self.ref64 = extra, post, ref64

    @property
    def exact(self):
        return self.tol is None


CASES = []
STEP_CASES = []


def table_symbols():
    out = {}
    for c in CASES + STEP_CASES:
        for s in c.symbols:
            out.setdefault(s, []).append(c.name)
    return out


# ------------------------------------------------------------------------------------------------------------------ harness
_CTX = {}
_CAL = {}
LONGEST_DELAY_MS = [0.0]


def shared_ctx():
    if 'ctx' not in _CTX:
        from face_vijnana_yolov3_amd._lib import Context
        _CTX['ctx'] = Context(0)
    return _CTX['ctx']


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, measured once with an event pair around one sleep."""
    if 'c' not in _CAL:
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20000000
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        _CAL['c'] = n / max(e0.elapsed_time(e1), 1e-3)
        print('stream_order: torch.cuda._sleep runs %.0f cycles per ms' % _CAL['c'])
    return _CAL['c']


def delay_ms(wall_seconds):
    return min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * 1e3 * wall_seconds))


class _Options(object):
    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.before = {k: self.ctx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            self.ctx.set_option(k, v)


class Delayed(object):
    """What the block of delayed_stream() sees: the stream S and, after sleep(), the event behind the sleep."""

    def __init__(self, S, ms):
        self.S, self.ms, self.ev = S, ms, None

    def sleep(self):
        torch.cuda._sleep(int(self.ms * cycles_per_ms()))
        self.ev = torch.cuda.Event()
        self.ev.record(self.S)

    def still_sleeping(self):
        return not self.ev.query()


@contextlib.contextmanager
def delayed_stream(ctx, ms):
    """Bind torch and the context to a fresh stream S for the block and put the context back on the stream it had (the null
    stream of a default Context) afterwards, as DeviceStager.stage does."""
    cycles_per_ms()
    LONGEST_DELAY_MS[0] = max(LONGEST_DELAY_MS[0], ms)
    dev = torch.device('cuda', ctx.device)
    before = torch.cuda.current_stream(dev).cuda_stream
    S = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(S):
            ctx.set_stream(S.cuda_stream)
            yield Delayed(S, ms)
    finally:
        ctx.set_stream(before)


def _snap(out):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def same_bits(a, b):
    """Equal as stored: tensors bit for bit (a NaN equals itself), host objects by value."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.numel() == 0:
            return True
        return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return a == b


def _tol(case, ctx, name, ref, inputs):
    if case.tol is None or not torch.is_tensor(ref):
        return 0
    t = case.tol(ctx, name, ref, inputs)
    return t


def _is_zero(t):
    return (not torch.is_tensor(t)) and t == 0


def differs(case, ctx, name, a, b, inputs):
    """Step 2: do the two problems' outputs `name` differ by more than 100 x the tolerance somewhere?"""
    t = _tol(case, ctx, name, a, inputs)
    if _is_zero(t):
        return not same_bits(a, b)
    if a.shape != b.shape:
        return True
    return bool(((a.double() - b.double()).abs() > 100.0 * (t.double() if torch.is_tensor(t) else float(t))).any())


def close(case, ctx, name, got, ref, inputs):
    """Step 5 -> (ok, message)."""
    t = _tol(case, ctx, name, ref, inputs)
    if _is_zero(t):
        if same_bits(got, ref):
            return True, ''
        if torch.is_tensor(got) and torch.is_tensor(ref) and got.shape == ref.shape:
            bad = int((got != ref).sum())
            return False, '%s: %d of %d elements differ from the reference (bit-exact case)' % (name, bad, ref.numel())
        return False, '%s differs from the reference (bit-exact case)' % name
    if got.shape != ref.shape:
        return False, '%s: shape %r, reference %r' % (name, tuple(got.shape), tuple(ref.shape))
    d = (got.double() - ref.double()).abs()
    tt = t.double() if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64, device=d.device)
    bad = ~(d <= tt)                      # a NaN fails
    if bool(bad.any()):
        return False, '%s: %d elements beyond the tolerance, max difference %.3e (largest tolerance %.3e)' % (
            name, int(bad.sum()), float(torch.nan_to_num(d, nan=float('inf')).max()), float(tt.max()))
    return True, ''


def run_delayed(case, seed=1234):
    ctx = case.ctx()
    dev = torch.device('cuda', ctx.device)
    real, stale = case.make(seed, dev), case.make(seed + 1, dev)
    assert sorted(real) == sorted(stale)
    for k in real:
        assert real[k].shape == stale[k].shape and real[k].dtype == stale[k].dtype and real[k].is_contiguous(), k

    # ---- 2. the references on the ordinary stream, and the power of the case to tell the two problems apart
    refs, walls = [], []
    with _Options(ctx, dict(case.options, **case.ref_options)):
        for p in (real, stale):
            work = {k: v.clone() for k, v in p.items()}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = case.call(ctx, work)
            walls.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            refs.append(_snap(out))
    ref = refs[0]
    for name in ref:
        if name not in case.may_tie:
            assert differs(case, ctx, name, ref[name], refs[1][name], real), \
                '%s: output %r does not tell the real problem from the stale one' % (case.name, name)
    del refs[1:]
    ms = delay_ms(max(walls))

    # ---- 3. the delayed run.  Every buffer exists before the block and lives until the final synchronise.
    work = {k: v.clone() for k, v in stale.items()}
    torch.cuda.synchronize()
    extra = {}
    with _Options(ctx, case.options):
        with delayed_stream(ctx, ms) as d:
            d.sleep()
            for k in work:
                work[k].copy_(real[k])
            out = case.call(ctx, work)
            clones = _snap(out)
            if case.extra is not None:
                extra = _snap(case.extra(ctx, work))
            sleeping = d.still_sleeping()
    # ---- 4. nothing waited for the stream: all of it was enqueued while the inputs held the stale problem
    print('%s: delay %.0f ms (host time of the call %.2f ms), returned %s the sleep' % (
        case.name, ms, 1e3 * max(walls), 'during' if sleeping else 'AFTER'))
    try:
        if not case.host_sync:
            assert sleeping, ('%s returned after the %.0f ms sleep had ended: either the call waits for the stream (it is not marked '
                              'host_sync) or enqueueing took more than %.0f x the reference run' % (case.name, ms, DELAY_FACTOR))
        # ---- 5. S alone is waited for; then the comparison
        d.S.synchronize()
        assert sorted(clones) == sorted(ref)
        errors = []
        for name in ref:
            ok, msg = close(case, ctx, name, clones[name], ref[name], real)
            if not ok:
                errors.append(msg)
        assert not errors, '%s on a delayed stream: %s' % (case.name, '; '.join(errors))
    finally:
        torch.cuda.synchronize()
    if case.post is not None:
        case.post(ctx, work, extra)
    del work, out, clones, extra, real, stale
    return ms


# ------------------------------------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _u(g, shape, lo=-1.0, hi=1.0, dtype=torch.float32):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def _signed(g, shape, lo=0.5, hi=1.0):
    return torch.where(_u(g, shape) > 0, 1.0, -1.0).float() * _u(g, shape, lo, hi)


def _to(d, dev):
    return {k: v.contiguous().to(dev) for k, v in d.items()}


def _stat_tol(exact_names=()):
    def tol(ctx, name, ref, inputs):
        if name in exact_names or not ref.is_floating_point():
            return 0
        return STAT_REL * float(ref.double().abs().max())
    return tol


def _add(name, symbols, make, call, **kw):
    CASES.append(Case(name, symbols, make, call, **kw))


SYNC_TABLE = 'uploads its table and waits for the stream once, by design (header)'


# ---- convolution forward, four forms
def _conv_fwd(name, B, H, cin, cout, k, s, stats, wmax=1.0, scratch=False):
    def make(seed, dev):
        g = _gen(seed)
        if scratch and torch.device(dev).type == 'cuda' and 'scratch' not in _CTX:
            _CTX['scratch'] = torch.empty(64 << 20, dtype=torch.uint8, device=dev)       # lent before the delayed block, kept
        return _to(dict(x=_u(g, (B, H, H, cin)), w=_u(g, (cout, k, k, cin), -wmax, wmax)), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        if scratch:
            ctx.set_conv_scratch(_CTX['scratch'])
        try:
            if stats:
                out, psum, psq = ops.conv2d_forward(ctx, p['x'], p['w'], stride=s, stats=True)
                return dict(out=out, psum=psum, psq=psq)
            return dict(out=ops.conv2d_forward(ctx, p['x'], p['w'], stride=s))
        finally:
            if scratch:
                ctx.set_conv_scratch(None)
    _add(name, ('fv_conv2d_forward',), make, call)


_conv_fwd('conv2d_forward[tile]', 2, 8, 128, 256, 3, 1, True)
_conv_fwd('conv2d_forward[conv_small]', 1, 26, 512, 256, 1, 1, False)
_conv_fwd('conv2d_forward[persistent 1x1]', 9, 96, 32, 128, 1, 1, False)
_conv_fwd('conv2d_forward[tail split, lent scratch, H=100]', 2, 100, 256, 128, 3, 1, True, wmax=0.1, scratch=True)


def _first_layer():
    def make(seed, dev):
        return _to(dict(w=_u(_gen(seed), (32, 3, 3, 3))), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(packed=ops.pack_first_layer(ctx, p['w']))
    _add('pack_first_layer', ('fv_pack_first_layer',), make, call)


_first_layer()


def _dgrad():
    B, H, cin, cout, k, s, cpad = 3, 12, 64, 128, 3, 2, 128

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(dy=_u(g, (B, H // s, H // s, cpad)), w=_u(g, (cout, k, k, cin)), add=_u(g, (B, H, H, cin))), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(dx=ops.conv2d_dgrad(ctx, p['dy'], p['w'], (H, H), s, addend=p['add']), wt=ops.transpose_weights(ctx, p['w'], cpad))
    _add('conv2d_dgrad[stride 2]', ('fv_conv2d_dgrad', 'fv_transpose_weights'), make, call)


_dgrad()


def _wgrad_bound_tol(bound_of):
    """test_ops_gpu._check: |error| <= 2e-6 * bound + 1e-6 per element, bound = the same sum over absolute values."""
    def tol(ctx, name, ref, inputs):
        if name != 'dw':
            return 0
        return 2e-6 * bound_of(ctx, inputs).double() + 1e-6
    return tol


def _wgrad(name, B, H, cin, cout, k, s):
    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(x=_u(g, (B, H, H, cin)), dy=_u(g, (B, H // s, H // s, cout))), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(dw=ops.conv2d_wgrad(ctx, p['x'], p['dy'], cout, k, s))       # the wrapper zero-fills dw, the kernel accumulates

    def bound(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return ops.conv2d_wgrad(ctx, p['x'].abs(), p['dy'].abs(), cout, k, s)
    _add(name, ('fv_conv2d_wgrad',), make, call, tol=_wgrad_bound_tol(bound))


_wgrad('conv2d_wgrad[generic]', 2, 16, 64, 64, 3, 1)
_wgrad('conv2d_wgrad[fused taps]', 3, 13, 32, 64, 3, 1)


def _slots_forward():
    B, H, cin, cout = 3, 13, 32, 64

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(x=_u(g, (B, H, H, cin)), w=_u(g, (cout, 3, 3, cin)), gamma=_u(g, (cout,), 0.5, 1.5), beta=_signed(g, (cout,)),
                        mm=_u(g, (cout,), -0.2, 0.2), mv=_u(g, (cout,), 0.5, 1.5), skip=_u(g, (B, H, H, cout))), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        sl = ops.stat_slots(cout, p['x'].device)                  # zeroed by the wrapper, added to by the conv, summed by the BN
        z = ops.conv2d_forward_slots(ctx, p['x'], p['w'], 1, sl)
        out, mean, invstd, scale, shift = ops.bn_act_slots(ctx, z, sl, p['gamma'], p['beta'], 1e-3, 0.99, p['mm'], p['mv'], p['skip'])
        return dict(z=z, out=out, mean=mean, invstd=invstd, scale=scale, shift=shift, mm=p['mm'], mv=p['mv'])
    _add('conv2d_forward_slots + bn_act_slots', ('fv_conv2d_forward_slots', 'fv_bn_act_slots'), make, call, tol=_stat_tol(('z',)))


_slots_forward()


def _bn_vectors(g, C):
    return dict(scale=_u(g, (C,), 0.5, 1.5), shift=_signed(g, (C,)), mean=_u(g, (C,), -0.3, 0.3), invstd=_u(g, (C,), 0.5, 2.0))


def _dgrad_bnred():
    B, H, cin, cout, s = 2, 16, 32, 64, 2

    def make(seed, dev):
        g = _gen(seed)
        d = dict(dy=_u(g, (B, H // s, H // s, cout)), w=_u(g, (cout, 3, 3, cin)), bn_z=_u(g, (B, H, H, cin), -2.0, 2.0))
        d.update(_bn_vectors(g, cin))
        return _to(d, dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        v = (p['scale'], p['shift'], p['mean'], p['invstd'])
        sl = ops.stat_slots(cin, p['dy'].device)
        dx = ops.conv2d_dgrad_bnred(ctx, p['dy'], p['w'], (H, H), s, p['bn_z'], *v, sl)
        dz, dgamma, dbeta = ops.bn_bwd_slots(ctx, dx, p['bn_z'], *v, sl, True)
        return dict(dx=dx, dz=dz, dgamma=dgamma, dbeta=dbeta)
    _add('conv2d_dgrad_bnred + bn_bwd_slots', ('fv_conv2d_dgrad_bnred', 'fv_bn_bwd_slots'), make, call, tol=_stat_tol(('dx',)))


_dgrad_bnred()


def _in_slots(z_in, cin):
    """The slots as the producing conv's epilogue leaves them (tests/test_bn_in_1x1_gpu.py)."""
    from face_vijnana_yolov3_amd._lib import lib
    ns = lib().fv_bn_stat_slots(cin)
    sl = torch.zeros((ns, 2, cin), dtype=torch.float64)
    for k, part in enumerate(z_in.double().view(-1, cin).chunk(ns, 0)):
        sl[k, 0] = part.sum(0)
        sl[k, 1] = (part * part).sum(0)
    return sl


def _bn_stats_in():
    B, H, cin, cout = 1, 13, 64, 128

    def make(seed, dev):
        g = _gen(seed)
        z_in = _u(g, (B, H, H, cin), -2.0, 2.0)
        return _to(dict(z_in=z_in, in_slots=_in_slots(z_in, cin), gamma=_u(g, (cin,), 0.5, 1.5), beta=_signed(g, (cin,)),
                        w=_u(g, (cout, 1, 1, cin), -0.2, 0.2), mm=_u(g, (cin,), -0.2, 0.2), mv=_u(g, (cin,), 0.5, 1.5),
                        skip=_u(g, (B, H, H, cin))), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        sl = ops.stat_slots(cout, p['z_in'].device)
        z, a, mean, invstd, scale, shift = ops.conv2d_forward_slots_bn_stats_in(ctx, p['z_in'], p['in_slots'], p['gamma'], p['beta'], p['w'], sl,
                                                                                1e-3, 0.99, p['mm'], p['mv'], p['skip'])
        return dict(z=z, a=a, mean=mean, invstd=invstd, scale=scale, shift=shift, mm=p['mm'], mv=p['mv'], sums=sl.sum(0))
    # the vectors come from the caller's slots in a fixed order: exact; the consumer's slot sums are fp64 atomics
    _add('conv2d_forward_slots_bn_stats_in', ('fv_conv2d_forward_slots_bn_stats_in',), make, call,
         tol=_stat_tol(('z', 'a', 'mean', 'invstd', 'scale', 'shift', 'mm', 'mv')))


_bn_stats_in()


def _bn_in():
    B, H, s = 2, 16, 1

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(z_in=_u(g, (B, H, H, 32), -2.0, 2.0), scale=_u(g, (32,), 0.5, 1.5), shift=_signed(g, (32,)),
                        w=_u(g, (64, 3, 3, 32)), dy=_u(g, (B, H // s, H // s, 64))), dev)

    def fwd(ctx, p):
        from face_vijnana_yolov3_amd import ops
        sl = ops.stat_slots(64, p['z_in'].device)
        z = ops.conv2d_forward_slots_bn_in(ctx, p['z_in'], p['scale'], p['shift'], p['w'], s, sl)
        return dict(z=z, sums=sl.sum(0))
    _add('conv2d_forward_slots_bn_in', ('fv_conv2d_forward_slots_bn_in',), make, fwd, tol=_stat_tol(('z',)))

    def wgrad(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(dw=ops.conv2d_wgrad_bn_in(ctx, p['z_in'], p['scale'], p['shift'], p['dy'], 64, 3, s))

    def bound(ctx, p):
        from face_vijnana_yolov3_amd import ops
        a = torch.nn.functional.leaky_relu(p['z_in'] * p['scale'] + p['shift'], 0.1)
        return ops.conv2d_wgrad(ctx, a.abs(), p['dy'].abs(), 64, 3, s)
    _add('conv2d_wgrad_bn_in', ('fv_conv2d_wgrad_bn_in',), make, wgrad, tol=_wgrad_bound_tol(bound))


_bn_in()


def _wgrad_bn_bwd():
    B, H, W, C = 1, 72, 112, 32                      # the shape tests/test_early_bn_fused_gpu.py pins this kernel at

    def make(seed, dev):
        from face_vijnana_yolov3_amd._lib import lib
        g = _gen(seed)
        rows, ns = B * H * W, lib().fv_bn_stat_slots(C)
        d = dict(x=_u(g, (B, H, W, 3), 0.0, 1.0), g=_u(g, (B, H, W, C)), z=_u(g, (B, H, W, C), -2.0, 2.0),
                 slots=(_u(g, (ns, 2, C), 0.0, 1.0, torch.float64) - 0.3) * 0.6 * rows / ns)
        d.update(_bn_vectors(g, C))
        return _to(d, dev)

    def args(p):
        return (p['g'], p['z'], p['scale'], p['shift'], p['mean'], p['invstd'])

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        dw, dgamma, dbeta = ops.conv2d_wgrad_bn_bwd(ctx, p['x'], *args(p), p['slots'])
        return dict(dw=dw, dgamma=dgamma, dbeta=dbeta)

    def bound(ctx, p):
        from face_vijnana_yolov3_amd import ops
        dz, _, _ = ops.bn_bwd_slots(ctx, *args(p), p['slots'].clone(), True)
        return ops.conv2d_wgrad(ctx, p['x'].abs(), dz.abs(), C, 3, 1)
    _add('conv2d_wgrad_bn_bwd', ('fv_conv2d_wgrad_bn_bwd',), make, call, tol=_wgrad_bound_tol(bound))


_wgrad_bn_bwd()


# ---- elementwise operators
def _bn_ops():
    rows, C = 1000, 32

    def make_fin(seed, dev):
        g = _gen(seed)
        z = _u(g, (4, 250, C), -2.0, 2.0).double()
        return _to(dict(psum=z.sum(1).float(), psq=(z * z).sum(1).float(), gamma=_u(g, (C,), 0.5, 1.5), beta=_signed(g, (C,)),
                        mm=_u(g, (C,), -0.2, 0.2), mv=_u(g, (C,), 0.5, 1.5)), dev)

    def fin(ctx, p):
        from face_vijnana_yolov3_amd import ops
        mean, invstd, scale, shift = ops.bn_finalize(ctx, p['psum'], p['psq'], rows, p['gamma'], p['beta'], 1e-3, 0.99, p['mm'], p['mv'])
        return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, mm=p['mm'], mv=p['mv'])
    _add('bn_finalize', ('fv_bn_finalize',), make_fin, fin)

    def make(seed, dev):
        g = _gen(seed)
        d = dict(g=_u(g, (rows, C)), z=_u(g, (rows, C), -2.0, 2.0), skip=_u(g, (rows, C)))
        d.update(_bn_vectors(g, C))
        return _to(d, dev)

    def act(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(out=ops.bn_act(ctx, p['z'], p['scale'], p['shift'], p['skip']))

    def act64(p):
        return dict(out=torch.nn.functional.leaky_relu(p['z'].double() * p['scale'].double() + p['shift'].double(), 0.1) + p['skip'].double())
    _add('bn_act', ('fv_bn_act',), make, act, ref64=act64)

    def bwd(ctx, p):
        from face_vijnana_yolov3_amd import ops
        dz, dgamma, dbeta = ops.bn_bwd(ctx, p['g'], p['z'], p['scale'], p['shift'], p['mean'], p['invstd'])
        return dict(dz=dz, dgamma=dgamma, dbeta=dbeta)
    _add('bn_bwd', ('fv_bn_bwd',), make, bwd)


_bn_ops()


def _adam_scale():
    n = 100003                                      # odd: the vector tail

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(p=_u(g, (n,)), g=_u(g, (n,)), m=_u(g, (n,), -0.1, 0.1), v=_u(g, (n,), 0.0, 0.1)), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        ops.adam_step(ctx, p['p'], p['g'], p['m'], p['v'], 3, 1e-3, 0.9, 0.999)
        return dict(p=p['p'], m=p['m'], v=p['v'])

    def ref64(p):
        g, m, v = p['g'].double(), p['m'].double(), p['v'].double()
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        lr = 1e-3 * np.sqrt(1 - 0.999 ** 4) / (1 - 0.9 ** 4)
        return dict(p=p['p'].double() - lr * m / (v.sqrt() + 1e-7), m=m, v=v)
    _add('adam_step[odd n]', ('fv_adam_step',), make, call, ref64=ref64)

    def make_s(seed, dev):
        return _to(dict(v=_u(_gen(seed), (35713,))), dev)

    def scale(ctx, p):
        ctx.scale(p['v'], 0.125)
        return dict(v=p['v'])
    _add('scale', ('fv_scale',), make_s, scale, ref64=lambda p: dict(v=p['v'].double() * 0.125))

    def profiled(ctx, p):
        from face_vijnana_yolov3_amd import ops
        ctx.profile(True)                               # the launch is bracketed by an event pair on the context's stream
        try:
            ops.adam_step(ctx, p['p'], p['g'], p['m'], p['v'], 3, 1e-3, 0.9, 0.999)
            recs = ctx.profile_collect()
        finally:
            ctx.profile(False)
        assert sum(r['launches'] for r in recs.values()) >= 1, recs
        return dict(p=p['p'], m=p['m'], v=p['v'])
    _add('profile_collect', ('fv_profile_collect',), make, profiled, host_sync='fv_profile_collect synchronises by design (header)')


_adam_scale()


def _losses():
    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(yp=_u(g, (338, 6), 0.02, 0.98), yt=_u(g, (338, 6), 0.0, 1.0)), dev)

    def mse(ctx, p):
        from face_vijnana_yolov3_amd import ops
        loss, dy, db = ops.mse_loss_grad(ctx, p['yp'], p['yt'])
        return dict(loss=loss, dy=dy, db=db)

    def mse64(p):
        d = p['yp'].double() - p['yt'].double()
        return dict(loss=(d * d).mean().reshape(1), db=(2 * d / d.numel()).sum(0))
    _add('mse_loss_grad', ('fv_mse_loss_grad',), make, mse, ref64=mse64)

    def fd(ctx, p):
        from face_vijnana_yolov3_amd import ops
        loss, dy = ops.fd_loss_grad(ctx, p['yp'], p['yt'])
        return dict(loss=loss, dy=dy)
    _add('fd_loss_grad', ('fv_fd_loss_grad',), make, fd)


_losses()


def _upsample_colsum():
    B, Hs, C1, C2 = 2, 5, 8, 12

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(src=_u(g, (B, Hs, Hs, C1)), skip=_u(g, (B, 2 * Hs, 2 * Hs, C2)), g=_u(g, (B, 2 * Hs, 2 * Hs, C1 + C2))), dev)

    def up(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(out=ops.upsample_concat(ctx, p['src'], p['skip']))

    def up64(p):
        s = p['src'].double().repeat_interleave(2, 1).repeat_interleave(2, 2)
        return dict(out=torch.cat([s, p['skip'].double()], 3))
    _add('upsample_concat', ('fv_upsample_concat',), make, up, ref64=up64)

    def bwd(ctx, p):
        from face_vijnana_yolov3_amd import ops
        g_up, g_skip = ops.upsample_concat_bwd(ctx, p['g'], C1)
        return dict(g_up=g_up, g_skip=g_skip)
    _add('upsample_concat_bwd', ('fv_upsample_concat_bwd',), make, bwd)

    def make_c(seed, dev):
        return _to(dict(dy=_u(_gen(seed), (513, 256))), dev)                   # 513 rows: two chunks

    def colsum(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(out=ops.colsum(ctx, p['dy'], 255))
    _add('colsum[513 rows]', ('fv_colsum',), make_c, colsum, ref64=lambda p: dict(out=p['dy'].double()[:, :255].sum(0)))


_upsample_colsum()


def _yolo_losses():
    ncls, cpad, cells = 1, 32, (3 * 4, 3 * 16, 3 * 64)

    def make(seed, dev):
        g = _gen(seed)
        d = {}
        for s, c in enumerate(cells):
            d['y%d' % s] = _u(g, (c, 3 * (5 + ncls)), -4.0, 4.0)
            d['t%d' % s] = _u(g, (c, 3 * (5 + ncls)), 0.0, 1.0)
        return _to(d, dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd import ops
        loss, dy3 = ops.yolo_loss_grad(ctx, [p['y%d' % s] for s in range(3)], [p['t%d' % s] for s in range(3)], ncls, cpad)
        return dict(loss=loss, dy0=dy3[0], dy1=dy3[1], dy2=dy3[2])
    _add('yolo_loss_grad', ('fv_yolo_loss_grad',), make, call)

    S, counts, ncd = 96, (1, 5, 4), 4

    def make_d(seed, dev):
        import yolo_det_loss_ref as ref
        from face_vijnana_yolov3_amd import data
        ys, ts = ref.planted_case(S, counts, ncd, seed, data.YOLO_ANCHORS)
        d = {}
        for s in range(3):
            d['y%d' % s] = torch.from_numpy(ys[s]).reshape(-1, 3 * (5 + ncd))
            d['t%d' % s] = torch.from_numpy(ts[s]).reshape(-1, 3 * (5 + ncd))
        return _to(d, dev)

    def det(ctx, p):
        from face_vijnana_yolov3_amd import data, ops
        conf = data.det_loss_conf({'yolo': dict(box_loss='giou', max_boxes=4)})
        loss, dy3, stats = ops.yolo_det_loss_grad(ctx, [p['y%d' % s] for s in range(3)], [p['t%d' % s] for s in range(3)], len(counts), S,
                                                  ncd, 32, conf)
        return dict(loss=loss, dy0=dy3[0], dy1=dy3[1], dy2=dy3[2], stats=stats)
    _add('yolo_det_loss_grad', ('fv_yolo_det_loss_grad',), make_d, det)


_yolo_losses()


# ---- the FaceIdentifier head
def _fid_ops():
    per, F, M = 5, 4096, 15

    def make(seed, dev):
        g = _gen(seed)
        return _to(dict(x0=_u(g, (per, F)), x1=_u(g, (per, F)), x2=_u(g, (per, F)), w=_u(g, (F, 64), -0.05, 0.05), bias=_u(g, (64,), -0.1, 0.1),
                        dE=_u(g, (M, 64))), dev)

    def towers(p):
        return [p['x0'], p['x1'], p['x2']]

    def l2(ctx, p):
        from face_vijnana_yolov3_amd import ops
        pre, u = ops.fid_towers_dense_l2(ctx, towers(p), M, p['w'], p['bias'])
        return dict(pre=pre, u=u)
    _add('fid_towers_dense_l2[per=5]', ('fv_fid_towers_dense_l2',), make, l2)

    def dgrad(ctx, p):
        from face_vijnana_yolov3_amd import ops
        ops.fid_towers_dense_dgrad(ctx, p['dE'], p['w'], towers(p), M)           # written into the towers' rows
        return dict(dx0=p['x0'], dx1=p['x1'], dx2=p['x2'])
    _add('fid_towers_dense_dgrad[per=5]', ('fv_fid_towers_dense_dgrad',), make, dgrad)

    def wgrad(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(dw=ops.fid_towers_dense_wgrad(ctx, towers(p), p['dE'], M, F))
    _add('fid_towers_dense_wgrad[per=5]', ('fv_fid_towers_dense_wgrad',), make, wgrad)

    def dense(ctx, p):
        from face_vijnana_yolov3_amd._lib import lib, ptr
        n = max(1, lib().fv_fid_dense_partial_floats(per, F))
        part = torch.empty(n, dtype=torch.float32, device=p['w'].device)
        pre = torch.empty((per, 64), dtype=torch.float32, device=p['w'].device)
        out = torch.empty_like(pre)
        ctx.check(lib().fv_fid_dense_l2(ctx.handle, ptr(p['x0']), per, F, ptr(p['w']), ptr(p['bias']), ptr(part), ptr(pre), ptr(out)),
                  'fv_fid_dense_l2')
        return dict(pre=pre, u=out)
    _add('fid_dense_l2', ('fv_fid_dense_l2',), make, dense)

    def make_pre(rows):
        def make_(seed, dev):
            pre = _u(_gen(seed), (rows, 64), -0.7, 1.0)
            u = torch.nn.functional.normalize(torch.relu(pre.double()) + 1e-3, dim=1).float()
            W = _u(_gen(seed + 50), (301, 64), -0.5, 0.5)
            # labels: valid and the same in both problems; they are inputs so that no call copies from the host
            return _to(dict(pre=pre, u=u, W=W, sub=torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=torch.int32),
                            labels=torch.arange(21, dtype=torch.int32) * 37 % 301), dev)
        return make_

    def triplet(ctx, p):
        from face_vijnana_yolov3_amd import ops
        loss, dE, dbias = ops.fid_triplet_loss_grad(ctx, p['pre'], p['u'])
        return dict(loss=loss, dE=dE, dbias=dbias)
    _add('fid_triplet_loss_grad', ('fv_fid_triplet_loss_grad',), make_pre(15), triplet)

    def batch(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return ops.fid_batch_triplet_loss_grad(ctx, p['pre'], p['u'], p['sub'])
    _add('fid_batch_triplet_loss_grad', ('fv_fid_batch_triplet_loss_grad',), make_pre(8), batch, may_tie=('pos_index', 'neg_index', 'kind'))

    def margin(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return ops.fid_margin_softmax_loss_grad(ctx, p['pre'], p['u'], p['labels'], p['W'], kind=1, margin=0.5)
    _add('fid_margin_softmax_loss_grad', ('fv_fid_margin_softmax_loss_grad',), make_pre(21), margin, may_tie=('pred',))

    def make_q(seed, dev):
        g = _gen(seed)
        return _to(dict(q=_u(g, (5, 64)), r=_u(g, (7, 64))), dev)

    def match(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        idx, dist = fi.fid_match(ctx, p['q'], p['r'])
        return dict(idx=idx, dist=dist)
    _add('fid_match', ('fv_fid_match',), make_q, match, may_tie=('idx',))

    def make_ids(seed, dev):
        return _to(dict(ids=torch.nn.functional.normalize(_u(_gen(seed), (12, 64), -0.2, 1.0), dim=1),
                        sub=torch.tensor([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], dtype=torch.int32)), dev)

    def pairs(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        blocks = [(0, 5, 0, 5, 0, 0), (5, 3, 8, 4, 10, 1)]                       # a triangle of 10 pairs, a rectangle of 12
        dists, counts = fi.fid_pair_dists(ctx, p['ids'], blocks, [0.5, 1.0, 1.5], n_dists=22)
        return dict(dists=dists, counts=counts)
    _add('fid_pair_dists', ('fv_fid_pair_dists',), make_ids, pairs, host_sync=SYNC_TABLE, may_tie=('counts',))

    def mine(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        i32 = lambda v: np.asarray(v, np.int32)
        neg, kind, d_ap, d_an = fi.fid_mine_negatives(ctx, p['ids'], p['sub'], i32([0, 3, 6]), i32([0, 2, 4, 6]), i32([1, 2, 4, 5, 7, 8]))
        return dict(neg=neg, kind=kind, d_ap=d_ap, d_an=d_an)
    _add('fid_mine_negatives', ('fv_fid_mine_negatives',), make_ids, mine, host_sync=SYNC_TABLE, may_tie=('neg', 'kind'))


_fid_ops()


def _recon_ops():
    def make_h(seed, dev):
        g = _gen(seed)
        return _to(dict(ids=_u(g, (3, 64), -0.3, 1.0), w=_u(g, (1024, 64), -0.2, 0.2), bias=_u(g, (1024,))), dev)

    def head(ctx, p):
        from face_vijnana_yolov3_amd import ops
        u, x = ops.recon_dense_head(ctx, p['ids'], p['w'], p['bias'])
        return dict(u=u, x=x)
    _add('recon_dense_head', ('fv_recon_dense_head',), make_h, head)

    def make_l(seed, dev):
        g = _gen(seed)
        return _to(dict(x=_u(g, (77, 64)), skip=_u(g, (77, 64)), scale=_u(g, (64,), 0.5, 1.5), shift=_u(g, (64,))), dev)

    def l2(ctx, p):
        from face_vijnana_yolov3_amd import ops
        y, d = ops.l2norm_affine(ctx, p['x'], p['scale'], p['shift'], skip=p['skip'])
        return dict(y=y, d=d)

    def l264(p):
        d = p['x'].double() - p['skip'].double()
        l = torch.nn.functional.leaky_relu(d, 0.1)
        return dict(d=d, y=l / (l * l).sum(1, keepdim=True).clamp_min(1e-12).sqrt() * p['scale'].double() + p['shift'].double())
    _add('l2norm_affine', ('fv_l2norm_affine',), make_l, l2, ref64=l264)

    def make_t(seed, dev):
        g = _gen(seed)
        return _to(dict(x=_u(g, (2, 6, 6, 128)), w=_u(g, (128, 3, 3, 64))), dev)

    def tr(ctx, p):
        from face_vijnana_yolov3_amd import ops
        return dict(out=ops.conv2d_transpose(ctx, p['x'], p['w'], 2))
    _add('conv2d_transpose[stride 2]', ('fv_conv2d_transpose',), make_t, tr)


_recon_ops()


# ---- pre- and post-processing
SIZES = ((17, 23), (40, 56))
OFFS = [0, 17 * 23 * 3]
HW = [17, 23, 40, 56]
CROPS = [(0, 2, 3, 10, 12), (1, 0, 0, 40, 56), (1, 5, 6, 20, 30)]


def _make_packed(seed, dev):
    rng = np.random.default_rng(seed)
    buf = np.concatenate([rng.integers(0, 256, (h, w, 3), dtype=np.uint8).reshape(-1) for h, w in SIZES])
    return _to(dict(buf=torch.from_numpy(buf)), dev)


def _preproc():
    S = 64

    def images(p):
        return (p['buf'], OFFS, HW)

    def batch(ctx, p):
        from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
        out, geom = letterbox_batch_device(ctx, None, S, p['buf'].device, packed=images(p))
        return dict(x=out, geom=[tuple(g) for g in geom])
    _add('letterbox_batch', ('fv_letterbox_batch',), _make_packed, batch, may_tie=('geom',))

    def make_one(seed, dev):
        return _to(dict(img=torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (40, 56, 3), dtype=np.uint8))), dev)

    def one(ctx, p):
        from face_vijnana_yolov3_amd.postproc import letterbox_device
        return dict(x=letterbox_device(ctx, p['img'], S)[0])
    _add('letterbox', ('fv_letterbox',), make_one, one)

    def crops(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        return dict(x=fi.letterbox_crops(ctx, images(p), CROPS, S))
    _add('letterbox_crops', ('fv_letterbox_crops',), _make_packed, crops)

    def augment(ctx, p):
        from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
        place = [(0, 0, 17, 23, 32, 5, 7, 1), (2, 3, 30, 40, 64, 0, 0, 0)]
        colour = [(0.1, 1.2, 0.9), (0.0, 1.0, 1.0)]
        return dict(x=letterbox_batch_device(ctx, None, S, p['buf'].device, packed=images(p), aug=(place, colour))[0])
    _add('letterbox_augment_batch', ('fv_letterbox_augment_batch',), _make_packed, augment)

    def mosaic(ctx, p):
        from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
        tiles = [(0, 0, 0, 0, 17, 23, 64, 0, 0, 0, 0, 0, 32, 64), (0, 1, 0, 0, 40, 56, 64, 0, 0, 1, 32, 0, 64, 64)]
        colour = [(0.0, 1.0, 1.0), (-0.1, 0.8, 1.1)]
        return dict(x=letterbox_batch_device(ctx, None, S, p['buf'].device, packed=images(p), mosaic=(tiles, colour, 1))[0])
    _add('letterbox_mosaic_batch', ('fv_letterbox_mosaic_batch',), _make_packed, mosaic)

    def nearest(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        return dict(x=fi.crop_nearest_u8(ctx, images(p), CROPS, 32))
    _add('crop_nearest_u8', ('fv_crop_nearest_u8',), _make_packed, nearest)

    def make_store(seed, dev):
        return _to(dict(store=torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (6, 64), dtype=np.uint8))), dev)

    def gather(ctx, p):
        from face_vijnana_yolov3_amd import face_identification as fi
        return dict(x=fi.gather_crops_f32(ctx, p['store'], (np.arange(130) * 5) % 6))      # 130 indices: two launches
    _add('gather_u8_f32', ('fv_gather_u8_f32',), make_store, gather)

    def make_draw(seed, dev):
        d = _make_packed(seed, dev)
        d['masks'] = torch.from_numpy(np.random.default_rng(seed + 7).integers(0, 256, 16, dtype=np.uint8)).to(dev)
        return d

    def draw(ctx, p):
        from face_vijnana_yolov3_amd import annotate, face_identification as fi
        prims = [annotate.Outline(k % 2, k - 3, k // 2, 10 + k, 8 + k, 1 + k % 3, (k * 7 % 256, 255 - k, 40)) for k in range(33)]
        prims.append(annotate.MaskBlend(1, 3, 4, 4, 4, 0, (200, 10, 90), None))          # 34 primitives: two launches
        fi.draw_prims_u8(ctx, images(p), prims, p['masks'])
        return dict(buf=p['buf'])
    _add('draw_prims_u8', ('fv_draw_prims_u8',), make_draw, draw)

    def encode(ctx, p):
        from face_vijnana_yolov3_amd import jpeg
        return dict(files=jpeg.encode_batch(ctx, p['buf'], OFFS, HW, p['buf'].device))
    _add('jpeg_encode_batch', ('fv_jpeg_encode_measure', 'fv_jpeg_encode_emit'), _make_packed, encode,
         host_sync='the measure -> emit size read-back waits for the stream once, by design')

    def coefs(ctx, p):
        from face_vijnana_yolov3_amd import jpeg
        return dict(coefs=[list(c) for c in jpeg.encode_coefs(ctx, p['buf'], OFFS, HW, p['buf'].device)])
    _add('jpeg_encode_coefs', ('fv_jpeg_encode_coefs',), _make_packed, coefs,
         host_sync='the test aid copies the coefficients to the host, which waits for the stream')


_preproc()


def _jpeg_stage():
    shapes = [(45, 67, 0), (33, 17, 2)]                       # 4:4:4 and 4:2:0

    def make(seed, dev):
        from test_jpeg_cpu import _jpeg
        from face_vijnana_yolov3_amd import jpeg
        rng = np.random.default_rng(seed)
        datas = [_jpeg(rng, h, w, sub, 90) for h, w, sub in shapes]
        infos = [jpeg.parse(d) for d in datas]
        plan = jpeg.BatchPlan(infos)
        coefs = np.zeros(plan.total_coefs, np.int16)
        for i, d in enumerate(datas):
            jpeg.entropy_decode(d, infos[i], coefs[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
        if 'plan' in _CTX:                                    # both problems share one layout and one set of tables
            assert bytes(_CTX['plan'].descs) == bytes(plan.descs)
        _CTX.setdefault('plan', plan)
        return _to(dict(coefs=torch.from_numpy(coefs)), dev)

    def call(ctx, p):
        from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
        keep = []
        x, _ = letterbox_batch_device(ctx, None, 64, p['coefs'].device, packed=('jpeg', p['coefs'], _CTX['plan']), keep=keep)
        return dict(x=x, rgb=keep[0][0])
    _add('jpeg_reconstruct_batch + letterbox_batch', ('fv_jpeg_reconstruct_batch',), make, call)


_jpeg_stage()


def _postproc():
    def make_head(seed, dev):
        g = _gen(seed)
        gt = torch.tensor([[10.0, 10.0, 380.0, 280.0], [100.0, 50.0, 200.0, 200.0]], dtype=torch.float64).repeat(3, 1)
        # geom, gt_off: valid records, the same in both problems
        return _to(dict(head=_u(g, (3, 13, 13, 6), -2.0, 4.0), gt=gt + _u(g, (6, 4), 0.0, 8.0, torch.float64),
                        geom=torch.tensor([[300, 400, 52, 52, 0, 0]] * 3, dtype=torch.int32), gt_off=torch.tensor([0, 2, 4, 6], dtype=torch.int64)), dev)

    def decode(ctx, p):
        from face_vijnana_yolov3_amd import postproc
        return postproc.decode_nms(ctx, p['head'], 416, 0.5, 0.5, 60)
    _add('decode_nms', ('fv_decode_nms',), make_head, decode, may_tie=('count',))

    def metric(ctx, p):
        from face_vijnana_yolov3_amd import det_metric, postproc
        res = postproc.decode_nms(ctx, p['head'], 416, 0.5, 0.5, 60)
        rows, nrows = det_metric.rows_from_nms(ctx, res, p['geom'], 416)
        iou, flag = det_metric.match_rows(ctx, rows, nrows, p['gt'], p['gt_off'], 2)
        out = det_metric.ap_sweep(ctx, rows, nrows, iou, flag, [0.3, 0.5], 6)                 # memsets on the stream
        return dict(rows=rows, nrows=nrows, iou=iou, flag=flag, result=out['result'], n_det=out['n_det'])
    _add('det_rows_from_nms + det_match_rows + det_ap_sweep', ('fv_det_rows_from_nms', 'fv_det_match_rows', 'fv_det_ap_sweep'), make_head,
         metric, may_tie=('nrows', 'flag', 'n_det'))

    def make_iou(seed, dev):
        g = _gen(seed)
        a, b = _u(g, (1000, 4), 0.0, 100.0, torch.float64), _u(g, (1000, 4), 0.0, 100.0, torch.float64)
        a[:, 2:] += a[:, :2]
        b[:, 2:] += b[:, :2]
        return _to(dict(a=a, b=b), dev)

    def iou(ctx, p):
        from face_vijnana_yolov3_amd._lib import lib, ptr
        out = torch.empty(1000, dtype=torch.float64, device=p['a'].device)
        ctx.check(lib().fv_bbox_iou_pairs(ctx.handle, ptr(p['a']), ptr(p['b']), 1000, ptr(out)), 'fv_bbox_iou_pairs')
        return dict(iou=out)
    _add('bbox_iou_pairs', ('fv_bbox_iou_pairs',), make_iou, iou)

    ncls = 2

    def make_y(seed, dev):
        g = _gen(seed)
        return _to({'y%d' % s: _u(g, (2, 2 << s, 2 << s, 3 * (5 + ncls)), -3.0, 3.0) for s in range(3)}, dev)

    def masked(out, count):
        """Rows past count[b] are not specified: cleared on the device, in stream order, before anything is compared."""
        cap = out['objness'].shape[-1]
        live = torch.arange(cap, device=count.device)[None, :] < count.reshape(-1, 1)
        z = lambda t, m: torch.where(m, t, torch.zeros_like(t))
        return dict(boxes=z(out['boxes'], live[..., None]), objness=z(out['objness'], live), classes=z(out['classes'], live[..., None]),
                    count=count)

    def ybatch(ctx, p):
        from face_vijnana_yolov3_amd import yolov3
        out = yolov3.decode_nms_batch(ctx, p['y0'], p['y1'], p['y2'], (48, 64), net_hw=(64, 64))
        return masked(out, out['count'])
    _add('yolo_decode_nms_batch', ('fv_yolo_decode_nms_batch',), make_y, ybatch, may_tie=('count',))

    def yone(ctx, p):
        from face_vijnana_yolov3_amd import yolov3
        return yolov3.decode_nms(ctx, p['y0'][0], p['y1'][0], p['y2'][0], (48, 64), net_hw=(64, 64))
    _add('yolo_decode_nms', ('fv_yolo_decode_nms',), make_y, yone, host_sync='the one-image wrapper reads the count back (count.item())')


_postproc()


# ---- network level
_MODELS = {}


def model(kind):
    if kind not in _MODELS:
        from face_vijnana_yolov3_amd import face_identification as fi
        if kind == 'engine':
            from face_vijnana_yolov3_amd.engine import Engine
            m = Engine(0)
            m.init_synthetic(29)
        elif kind == 'yolov3':
            from face_vijnana_yolov3_amd.yolov3 import Yolov3
            m = Yolov3(0, out_channels=27)
            m.init_synthetic(33)
        elif kind == 'fid':
            m = fi.FidModel(64, 0)
            m.init_synthetic(41)
            m.init_dense(41)
            m.dense_bias().copy_(0.1 * torch.rand(64, generator=_gen(42)))
            m.init_classes(7, 3)
        else:
            fid = fi.FidModel(32, 0)
            fid.init_synthetic(51)
            fid.init_dense(51)
            m = fi.ReconModel.from_identifier(fid, seed=51)
            g = _gen(52)
            for l in range(len(m.layers)):
                for which in range(4):
                    sl = m.bn_slice(l, which)
                    m.params[sl] = (0.5 + torch.rand(sl.stop - sl.start, generator=g)).to(m.dev)
        m.state0 = m.state.clone()
        torch.cuda.synchronize()
        _MODELS[kind] = m
    return _MODELS[kind]


def _images(B, S, n=1, labels=None):
    def make(seed, dev):
        g = _gen(seed)
        d = {'x%d' % i: _u(g, (B, S, S, 3), 0.0, 1.0) for i in range(n)}
        if labels is not None:
            d['labels'] = torch.tensor(labels, dtype=torch.int32)        # valid, the same in both problems, already on the device
        return _to(d, dev)
    return make


def _network():
    def infer(ctx, p):
        return dict(y=model('engine').predict_device(p['x0']))
    _add('forward_infer[1, 96]', ('fv_forward_infer',), _images(1, 96), infer, ctx=lambda: model('engine').ctx)

    def base(ctx, p):
        feat, y = model('engine').predict_base_device(p['x0'], with_head=True)
        return dict(feat=feat, y=y)
    _add('forward_base[1, 96]', ('fv_forward_base',), _images(1, 96), base, ctx=lambda: model('engine').ctx)

    def yolo(ctx, p):
        ys = model('yolov3').predict_device(p['x0'])
        return dict(y13=ys[0], y26=ys[1], y52=ys[2])
    _add('yolov3_forward[1, 96]', ('fv_yolov3_forward',), _images(1, 96), yolo, ctx=lambda: model('yolov3').ctx)

    def extract(ctx, p):
        return dict(ids=model('fid').extract_device(p['x0']))
    _add('fid_extract[3, 64]', ('fv_fid_extract',), _images(3, 64), extract, ctx=lambda: model('fid').ctx)

    def make_ids(seed, dev):
        return _to(dict(ids=torch.nn.functional.normalize(_u(_gen(seed), (3, 64), 0.0, 1.0), dim=1)), dev)

    def recon(ctx, p):
        return dict(image=model('recon').predict_device(p['ids']))
    _add('recon_forward[3, 32]', ('fv_recon_forward',), make_ids, recon, ctx=lambda: model('recon').ctx)


_network()


# ---- the training steps: the return join (section 3).  Reference: the serial schedule ("overlap" = 0) on the ordinary stream.
def _step_tol(ctx, name, ref, inputs):
    if not ref.is_floating_point():
        return 0
    top = float(ref.double().abs().max())
    if name in ('grads', 'class_grads'):
        return GRAD_REL * top + GRAD_FLOOR
    if name == 'loss':
        return LOSS_REL * top
    return STAT_REL * top


def _adam_extra(kind):
    """fv_adam_step enqueued on S directly behind the step ..."""
    def extra(ctx, p):
        from face_vijnana_yolov3_amd import ops
        m = model(kind)
        b = _MODELS[kind + ':adam']
        b['p'].copy_(m.params)
        b['m'].zero_()
        b['v'].zero_()
        ops.adam_step(ctx, b['p'], m.grads, b['m'], b['v'], 0, 1e-3, 0.9, 0.999)
        return dict(p=b['p'], grads=m.grads)
    return extra


def _adam_post(kind):
    """... gives the parameters the same gradients give after a full device synchronise (same run: bit for bit)."""
    def post(ctx, p, extra):
        from face_vijnana_yolov3_amd import ops
        m = model(kind)
        b = _MODELS[kind + ':adam']
        assert same_bits(extra['grads'], m.grads), 'the gradients changed after the step had returned and its stream had drained'
        b['p'].copy_(m.params)
        b['m'].zero_()
        b['v'].zero_()
        ops.adam_step(ctx, b['p'], m.grads, b['m'], b['v'], 0, 1e-3, 0.9, 0.999)
        torch.cuda.synchronize()
        assert same_bits(extra['p'], b['p']), 'fv_adam_step enqueued right behind the step read unfinished gradients'
    return post


def _adam_buffers(kind):
    m = model(kind)
    m.ensure_optimizer()
    if kind + ':adam' not in _MODELS:
        _MODELS[kind + ':adam'] = dict(p=torch.empty_like(m.params), m=torch.empty_like(m.params), v=torch.empty_like(m.params))


def _reset(m):
    m.state.copy_(m.state0)
    m.bn_updates = 0
    m.grads.fill_(float('nan'))                      # documented as overwritten


def _step(name, symbol, kind, make, run, early, may_tie=()):
    def make_(seed, dev):
        _adam_buffers(kind)
        return make(seed, dev)

    def call(ctx, p):
        m = model(kind)
        _reset(m)
        out = run(m, p)
        out.update(grads=m.grads, state=m.state)
        return out
    opts = {'overlap': 1} if early else {'overlap': 1, 'early_bn_fused': 0}
    STEP_CASES.append(Case('%s[%s]' % (name, 'overlap' if early else 'overlap, early_bn_fused=0'), (symbol,), make_, call, tol=_step_tol,
                           may_tie=may_tie, ctx=lambda: model(kind).ctx, options=opts, ref_options={'overlap': 0},
                           extra=_adam_extra(kind), post=_adam_post(kind)))


def _steps():
    def engine_make(B, S):
        def make(seed, dev):
            g = _gen(seed)
            return _to(dict(x=_u(g, (B, S, S, 3), 0.0, 1.0), yt=_u(g, (B, S // 32, S // 32, 6), 0.0, 1.0)), dev)
        return make

    def engine_run(m, p):
        return dict(loss=m.forward_backward(p['x'], p['yt']))

    def yolo_make(seed, dev):
        g = _gen(seed)
        d = dict(x=_u(g, (2, 64, 64, 3), 0.0, 1.0))
        for dv in (32, 16, 8):
            d['t%d' % dv] = _u(g, (2, 64 // dv, 64 // dv, 27), 0.0, 1.0)
        return _to(d, dev)

    def yolo_run(m, p):
        m.det_loss = None
        return dict(loss=m.forward_backward(p['x'], [p['t32'], p['t16'], p['t8']]))

    def det_make(seed, dev):
        import yolo_det_loss_ref as ref
        from face_vijnana_yolov3_amd import data
        _, ts = ref.planted_case(64, (4, 1), 4, seed, data.YOLO_ANCHORS)
        d = dict(x=_u(_gen(seed), (2, 64, 64, 3), 0.0, 1.0))
        for dv, t in zip((32, 16, 8), ts):
            d['t%d' % dv] = torch.from_numpy(t).reshape(2, 64 // dv, 64 // dv, 27)
        return _to(d, dev)

    def det_run(m, p):
        from face_vijnana_yolov3_amd import data
        m.det_loss = data.det_loss_conf({'yolo': dict(box_loss='giou', max_boxes=4)})
        try:
            loss = m.forward_backward(p['x'], [p['t32'], p['t16'], p['t8']])
        finally:
            m.det_loss = None
        return dict(loss=loss, det_stats=m.det_stats)

    def fid_run(m, p):
        from face_vijnana_yolov3_amd._lib import lib, ptr
        ws = m._workspace(2, 64, True)
        m.ctx.set_bn_zero_debias_step(1)
        rc = lib().fv_fid_train_step(m.ctx.handle, ptr(m.params), ptr(m.state), ptr(p['x0']), ptr(p['x1']), ptr(p['x2']), 2, 64, ptr(ws),
                                     ws.numel(), ptr(m.grads), ptr(m._loss))
        m.ctx.check(rc, 'fv_fid_train_step')
        return dict(loss=m._loss)

    def batch_run(m, p):
        loss = m.forward_backward_batch(p['x0'], p['labels'], 'batch_hard')
        return dict(loss=loss, **m.batch_selection)

    def cls_run(m, p):
        m.class_grads.fill_(float('nan'))
        loss = m.forward_backward_classes(p['x0'], p['labels'], 'arcface')
        return dict(loss=loss, class_grads=m.class_grads, **m.class_selection)

    for early in (True, False):
        _step('train_step[2, 64]', 'fv_train_step', 'engine', engine_make(2, 64), engine_run, early)
        _step('train_step[4, 96]', 'fv_train_step', 'engine', engine_make(4, 96), engine_run, early)
        _step('yolov3_train_step[27, 2, 64]', 'fv_yolov3_train_step', 'yolov3', yolo_make, yolo_run, early)
        _step('yolov3_train_step_det[27, 2, 64]', 'fv_yolov3_train_step_det', 'yolov3', det_make, det_run, early)
        _step('fid_train_step[2, 64]', 'fv_fid_train_step', 'fid', _images(2, 64, 3), fid_run, early)
        _step('fid_batch_train_step[5, 64]', 'fv_fid_batch_train_step', 'fid', _images(5, 64, labels=[4, 7, 7, 4, 7]), batch_run, early,
              may_tie=('pos_index', 'neg_index', 'kind'))
        _step('fid_cls_train_step[5, 64]', 'fv_fid_cls_train_step', 'fid', _images(5, 64, labels=[6, 0, 3, 3, 1]), cls_run, early, may_tie=('pred',))


_steps()
