"""In-batch triplet mining on the GPU: fv_fid_batch_triplet_loss_grad against its numpy restatement
(tests/batch_triplet_ref.py) -- the selection compared for equality, loss and gradients within the bounds of
test_ops_gpu.py::test_fid_triplet_loss_and_gradient with 3B replaced by M --, fv_fid_batch_train_step against the float64 oracle
with test_fid_gpu.py's rules and constants, and FaceIdentifier.train() with hps['batch_mining'] in the three input tiers."""
import functools
import os

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import crop_store as cs
from face_vijnana_yolov3_amd import face_identification as fi
import batch_triplet_ref as ref
import test_fid_gpu as fg
import test_fid_mining_gpu as mg

pytestmark = pytest.mark.gpu

U23, U24 = 2.0 ** -23, 2.0 ** -24
FV_ERR_INVALID = -1
NAMES = ('pos_index', 'neg_index', 'kind', 'd_ap', 'd_an')


def _ctx():
    return fg._model(64).ctx


def _filled():
    """Outputs holding values the operator never writes: whatever is still there afterwards was not touched."""
    def out(M):
        return dict(loss=torch.full((1,), float('nan')).cuda(), dE=torch.full((M, 64), float('nan')).cuda(),
                    dbias=torch.full((64,), float('nan')).cuda(), pos_index=torch.full((M,), -7, dtype=torch.int32).cuda(),
                    neg_index=torch.full((M,), -7, dtype=torch.int32).cuda(), kind=torch.full((M,), -7, dtype=torch.int32).cuda(),
                    d_ap=torch.full((M,), -7.5, dtype=torch.float64).cuda(), d_an=torch.full((M,), -7.5, dtype=torch.float64).cuda())
    return out


def _run(pre, u, subjects, margin=0.2, mode=0, weight=1.0):
    from face_vijnana_yolov3_amd import ops
    M = len(pre)
    o = ops.fid_batch_triplet_loss_grad(_ctx(), torch.from_numpy(pre).cuda(), torch.from_numpy(u).cuda(),
                                        torch.from_numpy(np.asarray(subjects, np.int32)).cuda(), margin, mode, weight, out=_filled()(M))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _compare(got, want, M, what):
    """Selection: equality, d_ap / d_an by their bits.  Loss 2^-23 relative; dE 2^-23 |ref| + 1e-12 max|ref|; dbias M 2^-24 sum|dE
    column| + 2^-23 |ref|.  Every figure is printed before it is asserted."""
    for k in NAMES[:3]:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    for k in NAMES[3:]:
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (what, k)
    loss, rl = float(got['loss'][0]), float(want['loss'])
    e_dE = np.abs(got['dE'].astype(np.float64) - want['dE'])
    lim_dE = U23 * np.abs(want['dE']) + 1e-12 * np.abs(want['dE']).max()
    e_db = np.abs(got['dbias'].astype(np.float64) - want['dbias'])
    lim_db = M * U24 * np.abs(want['dE']).sum(0) + U23 * np.abs(want['dbias'])
    print('%s: loss %.9g ref %.9g; dE worst err/limit %.3g; dbias worst err/limit %.3g; V %d, active %d'
          % (what, loss, rl, (e_dE / np.maximum(lim_dE, 1e-300)).max(), (e_db / np.maximum(lim_db, 1e-300)).max(), want['V'],
             int(want['active'].sum())))
    assert abs(loss - rl) <= U23 * abs(rl), what
    assert np.isfinite(got['dE']).all() and (e_dE <= lim_dE).all(), what
    assert (e_db <= lim_db).all(), what


# ----------------------------------------------------------------------------- 1. the operator on random batches
SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1024]      # a wave and a 256-thread stride with one to either side; the limit


@functools.lru_cache(maxsize=None)
def _random(M, mode):
    pre, u, subjects = ref.random_case(M, 700 + M)
    return pre, u, subjects, ref.batch_triplet(pre, u, subjects, 0.2, mode)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('M', SIZES)
def test_batch_triplet_loss_and_gradient(M, mode):
    pre, u, subjects, want = _random(M, mode)
    if M >= 63:
        assert np.bincount(subjects).min() >= 2 and want['V'] == M and 0 < want['active'].sum()
    got = _run(pre, u, subjects, 0.2, mode)
    _compare(got, want, M, 'M=%d mode=%d' % (M, mode))
    # the gradient weight is a factor: 0.25 scales every stored bit pattern exactly and leaves the loss alone
    got4 = _run(pre, u, subjects, 0.2, mode, 0.25)
    assert np.array_equal(got4['loss'], got['loss']) and np.array_equal(got4['dE'], got['dE'] * np.float32(0.25))
    assert np.array_equal(got4['dbias'], got['dbias'] * np.float32(0.25))
    # the same inputs give the same bits
    again = _run(pre, u, subjects, 0.2, mode)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k


# ----------------------------------------------------------------------------- 2. hand cases and built rows
@pytest.mark.parametrize('name', sorted(ref.hand_cases()))
def test_batch_triplet_hand_case(name):
    c = ref.hand_cases()[name]
    u = ref.l2n_relu(c['pre'])
    for margin in (c['margin'], 2.0):              # 2.0: every valid anchor's hinge passes, so the gradient terms are all exercised
        want = ref.batch_triplet(c['pre'], u, c['subjects'], margin, c['mode'])
        if margin == c['margin']:
            assert [(int(p), int(n), int(k)) for p, n, k in zip(want['pos_index'], want['neg_index'], want['kind'])] == c['want']
        else:
            assert want['active'].sum() == want['V']
        got = _run(c['pre'], u, c['subjects'], margin, c['mode'])
        _compare(got, want, len(u), '%s margin %g' % (name, margin))
        if want['V'] == 0:
            assert got['loss'][0] == 0.0 and not got['dE'].any() and not got['dbias'].any()


@functools.lru_cache(maxsize=None)
def _built(mode):
    """M = 257 with: a tenth of the rows of subject -1; twenty rows copied over another row of their subject; one subject cut down
    to two identical rows (dap exactly 0); a dead row (every pre <= 0); a row with 0 < sum relu(pre)^2 <= 1e-12."""
    M = 257
    pre, _, subjects = ref.random_case(M, 911, unknown=0.1)
    rng = np.random.RandomState(912)
    known = np.flatnonzero(subjects >= 0)
    copied, touched = [], set()
    for r in (int(v) for v in rng.permutation(known)):
        same = [int(q) for q in np.flatnonzero(subjects == subjects[r]) if q != r and int(q) not in touched]
        if same and r not in touched and len(copied) < 20:
            pre[r] = pre[same[0]]
            copied.append((r, same[0]))
            touched |= {r, same[0]}
    lone = next(s for s in range(subjects.max() + 1) if (subjects == s).sum() >= 3 and not touched & set(np.flatnonzero(subjects == s).tolist()))
    rows = np.flatnonzero(subjects == lone)
    subjects[rows[2:]] = -1
    pre[rows[1]] = pre[rows[0]]
    free = [int(r) for r in known if r not in touched and subjects[r] >= 0 and subjects[r] != lone]
    dead, tiny = free[0], free[1]
    pre[dead] = -np.abs(pre[dead]); pre[dead, 7] = 0.0
    pre[tiny] = np.abs(pre[tiny]) * np.float32(1e-8)
    u = ref.l2n_relu(pre)
    return pre, u, subjects, copied, (int(rows[0]), int(rows[1])), dead, tiny, ref.batch_triplet(pre, u, subjects, 0.2, mode)


@pytest.mark.parametrize('mode', [0, 1])
def test_batch_triplet_built_rows(mode):
    pre, u, subjects, copied, pair, dead, tiny, want = _built(mode)
    M = len(pre)
    unknown = np.flatnonzero(subjects < 0)
    # asserted on the restatement before the device is looked at
    assert 20 <= len(unknown) <= 40 and len(copied) == 20
    assert (want['kind'][unknown] == 3).all() and not np.isin(want['pos_index'], unknown).any() and not np.isin(want['neg_index'], unknown).any()
    assert not want['dE'][unknown].any()
    for r, q in copied:
        assert np.array_equal(u[r], u[q])
    assert want['d_ap'][pair[0]] == 0.0 and want['d_ap'][pair[1]] == 0.0 and want['pos_index'][pair[0]] == pair[1]
    assert (pre[dead] <= 0).all() and want['ss'][dead] == 0.0 and not want['dE'][dead].any() and not u[dead].any()
    assert 0.0 < want['ss'][tiny] <= 1e-12 and (pre[tiny] > 0).any()
    valid = want['kind'] != 3
    inactive = valid & ~want['active']
    assert inactive.sum() >= 1 and want['active'].sum() >= 1 and (np.abs(want['h'][valid]) > 1e-9).all()
    assert np.isin(tiny, np.concatenate([want['pos_index'][want['active']], want['neg_index'][want['active']], np.flatnonzero(want['active'])]))
    got = _run(pre, u, subjects, 0.2, mode)
    _compare(got, want, M, 'built rows, mode %d' % mode)
    assert not got['dE'][unknown].any() and not got['dE'][dead].any()
    # an inactive anchor that nobody chose gets nothing at all: its own term is absent
    chosen = set(want['pos_index'][want['active']].tolist()) | set(want['neg_index'][want['active']].tolist())
    alone = [i for i in np.flatnonzero(inactive) if i not in chosen]
    assert alone
    assert not got['dE'][alone].any()


# ----------------------------------------------------------------------------- 3. refused arguments
def test_refused_arguments_leave_the_outputs_untouched():
    from face_vijnana_yolov3_amd._lib import lib, ptr
    M = 6
    pre, u, subjects = ref.random_case(M, 5)
    pre, u, sub = torch.from_numpy(pre).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(subjects).cuda()
    big = torch.zeros((1025, 64)).cuda()
    o = _filled()(1025)
    keep = {k: v.clone() for k, v in o.items()}
    order = ('loss', 'dE', 'dbias') + NAMES

    def call(pre=pre, u=u, sub=sub, M=M, margin=0.2, mode=0, weight=1.0, null=None):
        outs = [None if k == null else ptr(o[k]) for k in order]
        return lib().fv_fid_batch_triplet_loss_grad(_ctx().handle, ptr(pre), ptr(u), ptr(sub), M, margin, mode, weight, *outs)
    bad = [dict(M=0), dict(M=-1), dict(M=1025, pre=big, u=big, sub=torch.zeros(1025, dtype=torch.int32).cuda()), dict(mode=2), dict(mode=-1),
           dict(margin=0.0), dict(margin=-0.2), dict(margin=float('nan')), dict(margin=float('inf')), dict(weight=0.0),
           dict(weight=-1.0), dict(weight=float('nan')), dict(weight=float('inf'))] + [dict(null=k) for k in order]
    for change in bad:
        assert call(**change) == FV_ERR_INVALID, change
    for what in ('pre', 'u', 'sub'):
        outs = [ptr(o[k]) for k in order]
        args = dict(pre=ptr(pre), u=ptr(u), sub=ptr(sub)); args[what] = None
        assert lib().fv_fid_batch_triplet_loss_grad(_ctx().handle, args['pre'], args['u'], args['sub'], M, 0.2, 0, 1.0, *outs) == FV_ERR_INVALID
    torch.cuda.synchronize()
    for k in order:
        assert np.array_equal(o[k].cpu().numpy().view(np.uint8), keep[k].cpu().numpy().view(np.uint8)), k
    assert call() == 0                             # and the valid call, last: M rows are written, the rest is not
    torch.cuda.synchronize()
    assert bool((o['kind'][:M] != -7).all()) and int(o['kind'][M]) == -7 and float(o['d_an'][M]) == -7.5
    assert bool(torch.isfinite(o['dE'][:M]).all()) and bool(torch.isnan(o['dE'][M:]).all())
    # the step checks its batch before anything is enqueued
    m = fg._model(64)
    m.ensure_optimizer()
    with pytest.raises(ValueError, match='1024'):
        m.forward_backward_batch(torch.zeros((1025, 64, 64, 3)), np.zeros(1025, np.int32))
    with pytest.raises(ValueError, match='mode'):
        m.forward_backward_batch(torch.zeros((2, 64, 64, 3)), np.zeros(2, np.int32), 'semi_hard')
    with pytest.raises(ValueError, match='one subject per image'):
        m.forward_backward_batch(torch.zeros((2, 64, 64, 3)), np.zeros(3, np.int32))
    assert m.bn_updates == 0


# ----------------------------------------------------------------------------- 4. the step against the float64 oracle
GAP = 1e-3


def _oracle_select(u, subjects, mode):
    """The operator's rules on the oracle's own float64 IDs -> (pos, neg, h) of the valid anchors, after asserting that every
    choice beats its runner-up by more than GAP in distance (in mode 1 also that no candidate lies within GAP of a class boundary),
    that no chosen distance is 0 and that every |h| > GAP: fp32 towers cannot flip a choice or a hinge."""
    M = len(subjects)
    D = torch.sqrt(((u[:, None, :] - u[None, :, :]) ** 2).sum(-1)).numpy()
    anchors, pos, neg = [], [], []
    for i in range(M):
        own = [r for r in range(M) if r != i and subjects[r] == subjects[i] >= 0]
        other = np.asarray([r for r in range(M) if subjects[r] >= 0 and subjects[r] != subjects[i]], np.int64)
        if subjects[i] < 0 or not own or not len(other):
            continue
        byd = sorted(own, key=lambda r: -D[i, r])
        p = byd[0]
        assert len(byd) == 1 or D[i, p] - D[i, byd[1]] > GAP, (i, 'positive runner-up')
        dap = D[i, p]
        n, k, _, dan = ref.mine_one(dap, other, D[i, other], fi.TRIPLET_MARGIN, 1 - mode)
        rest = D[i, other[other != n]]
        assert (np.abs(rest - dan) > GAP).all(), (i, 'negative runner-up')
        if mode == 1:
            assert (np.abs(D[i, other] - dap) > GAP).all() and (np.abs(D[i, other] - (dap + fi.TRIPLET_MARGIN)) > GAP).all(), (i, 'class boundary')
        assert dap > 0 and dan > 0
        anchors.append(i); pos.append(p); neg.append(int(n))
    return anchors, pos, neg


def _oracle_batch_step(p, s, x, subjects, S, mode, sel=None):
    sp = fg._SlicedParams(p)
    (u,), _, ns = fg.towers(sp, s, [x], S, training=True, ema_step=1)
    if sel is None:
        sel = _oracle_select(u.detach().double(), subjects, mode)
    a, pp, nn = (torch.as_tensor(v, dtype=torch.int64) for v in sel)
    h = torch.sqrt(((u[a] - u[pp]) ** 2).sum(-1)) - torch.sqrt(((u[a] - u[nn]) ** 2).sum(-1)) + fi.TRIPLET_MARGIN
    loss = torch.clamp(h, min=0.0).mean()
    return loss.detach(), sp.grad(loss), ns.detach(), h.detach(), sel


# (subjects, mode, seed): the seeds were searched on the CPU for the assertions of _oracle_select and the two below to hold
STEP_CASES = [([0, 0, 1, 1], 0, 60), ([0, 0, 0, 1, 1, 2, 2, -1], 1, 60)]


@pytest.mark.parametrize('subjects,mode,seed', STEP_CASES)
def test_fid_batch_train_step_matches_oracle(subjects, mode, seed):
    from oracle import net_oracle as no
    S, M = 64, len(subjects)
    m = fg._model(S)
    p64, s64 = fg.fid_params(S, seed)
    x = fg._images(M, S, seed + 1)
    l64, g64, ns64, h, sel = _oracle_batch_step(p64, s64, x, subjects, S, mode)
    valid = [i for i, s_ in enumerate(subjects) if s_ >= 0]
    assert sel[0] == valid                                      # every row of a known subject is a valid anchor here
    assert (h.abs() > GAP).all() and (h > 0).sum() >= len(valid) - 1, h
    l32, g32, ns32, _, _ = _oracle_batch_step(p64.float(), s64.float(), x.float(), subjects, S, mode, sel)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    loss = m.forward_backward_batch(x.float(), np.asarray(subjects, np.int32), mode).item()
    assert m.bn_updates == 1
    got = {k: v.cpu().numpy() for k, v in m.batch_selection.items()}
    want_pos, want_neg = np.full(M, -1), np.full(M, -1)
    want_pos[sel[0]], want_neg[sel[0]] = sel[1], sel[2]
    assert np.array_equal(got['pos_index'], want_pos) and np.array_equal(got['neg_index'], want_neg)
    assert ((got['kind'] == 3) == (want_pos < 0)).all()
    print('loss %.9g, float64 %.9g, float32 %.9g' % (loss, l64.item(), l32.item()))
    assert abs(loss - l64.item()) <= 4 * abs(l32.item() - l64.item()) + 1e-5 * abs(l64.item())
    fg._within(m.state.cpu(), ns64, ns32, 'bn moving state after one update')
    g = m.grads.cpu()
    for e in no.param_layout()[0][:fi.NUM_BASE_LAYERS]:
        sl = slice(e['w_off'], e['w_off'] + e['cout'] * e['k'] * e['k'] * e['cin'])
        fg._grad_close(g[sl], g64[sl], g32[sl], 'dW ' + e['name'])
        for nm in ('gamma_off', 'beta_off'):
            sl = slice(e[nm], e[nm] + e['cout'])
            fg._grad_close(g[sl], g64[sl], g32[sl], nm + ' ' + e['name'])
    k, b = fi.dense_offsets(S)
    fg._grad_close(g[k:b], g64[k:b], g32[k:b], 'dense kernel')
    fg._grad_close(g[b:b + 64], g64[b:b + 64], g32[b:b + 64], 'dense bias')
    assert len(g) == b + 64 and torch.isfinite(g).all()


# ----------------------------------------------------------------------------- 5. properties
def test_a_batch_of_inactive_anchors_gives_zero_loss_and_gradients():
    """The construction of test_fid_gpu.py::test_inactive_hinge_gives_zero_loss_and_gradients on one tower: rows [A, A, N, N] of
    subjects [0, 0, 1, 1], the dense layer built so that A's ReLU units and N's are disjoint (distance sqrt 2) -- every anchor is
    valid, its positive at distance ~0, its negative far beyond the margin."""
    S = 64
    m = fg._model(S)
    p64, s64 = fg.fid_params(S, 41)
    xa, xn = fg._images(1, S, 42), fg._images(1, S, 43)
    x = torch.cat([xa, xa, xn, xn])
    subjects = np.asarray([0, 0, 1, 1], np.int32)
    _, (feat,), _ = fg.towers(p64, s64, [x], S, training=True)
    feat = feat.reshape(4, -1)
    fa, fn = feat[0], feat[2]
    d, mid = fa - fn, (fa + fn) / 2
    c = 1.0 / (d @ d)
    k, b = fi.dense_offsets(S)
    p64[k:b] = (torch.cat([d[:, None].expand(-1, 32), -d[:, None].expand(-1, 32)], dim=1) * c).reshape(-1)
    p64[b:b + 32] = -c * (mid @ d)
    p64[b + 32:b + 64] = c * (mid @ d)
    (u,), _, _ = fg.towers(p64, s64, [x], S, training=True)
    D = torch.sqrt(((u[:, None] - u[None]) ** 2).sum(-1))
    assert D[0, 1] < 1e-6 and D[2, 3] < 1e-6 and (D[:2, 2:] > 1.2).all()          # every h < 0.2 - 1.2
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    st0 = m.state.clone()
    for mode in ('batch_hard', 'batch_semi_hard'):
        loss = m.forward_backward_batch(x.float(), subjects, mode).item()
        sel = {k_: v.cpu().numpy() for k_, v in m.batch_selection.items()}
        assert loss == 0.0 and (sel['kind'] == 2).all() and sel['pos_index'].tolist() == [1, 0, 3, 2]
        assert torch.count_nonzero(m.grads).item() == 0
    assert not torch.equal(m.state, st0) and m.bn_updates == 2


def test_training_on_a_labelled_batch_makes_progress():
    S = 64
    m = fg._model(S)
    p64, s64 = fg.fid_params(S, 51)
    a, p, n = fg._active_triplet(2, S, 52)           # n: the anchors plus a little noise -- another subject's rows, very near
    x = torch.cat([a, n]).float()
    subjects = np.asarray([0, 0, 1, 1], np.int32)
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    losses = [m.train_on_labelled_batch(x, subjects, 'batch_hard', 1e-5, 0.99, 0.99).item() for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[0] > 0 and m.bn_updates == 6 and m.iterations == 6
    assert losses[-1] < losses[0], losses


def test_the_batch_workspace_does_not_evict_the_others():
    S = 64
    m = fg._model(S)
    m.ensure_optimizer()
    ws_train, ws_infer = m._workspace(2, S, True), m._workspace(3, S, False)
    big = m._batch_workspace(6)
    assert m._batch_workspace(4) is big and m._workspace(2, S, True) is ws_train and m._workspace(3, S, False) is ws_infer
    m._workspace(1, S, True)
    assert m._batch_workspace(6) is big


# ----------------------------------------------------------------------------- 6. end to end
def test_train_with_batch_mining_end_to_end_in_the_three_tiers(tmp_path, monkeypatch, capsys):
    mg._make_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    fed = []
    real = fi.FidModel.train_on_labelled_batch

    def record(self, x, subjects, mode, *a, **k):
        loss = real(self, x, subjects, mode, *a, **k)
        fed.append(dict(x=self._as_input(x).clone(), subjects=np.asarray(subjects).copy(), mode=mode, loss=float(loss.item())))
        return loss
    monkeypatch.setattr(fi.FidModel, 'train_on_labelled_batch', record)
    tiers = {cs.RESIDENT: {}, cs.PER_BATCH: dict(crop_store_mb=0), cs.HOST: dict(crop_store=False)}
    made = []
    real_init = cs.TripletInputs.__init__
    monkeypatch.setattr(cs.TripletInputs, '__init__', lambda self, *a, **k: (real_init(self, *a, **k), made.append(self.tier))[0])
    first = {}
    for tier, more in tiers.items():
        del fed[:]
        if os.path.exists('face_identifier.h5'):
            os.remove('face_identifier.h5')
        ident = fi.FaceIdentifier(mg._conf(tmp_path, batch_mining='batch_semi_hard', pk_subjects=2, pk_crops=3, pk_seed=5, **more))
        ident.train()
        assert made[-1] == tier and os.path.exists('face_identifier.h5')
        out = capsys.readouterr().out
        lines = [line for line in out.splitlines() if line.startswith('Epoch')]
        assert len(lines) == 2 and all('anchors (batch_semi_hard)' in line and 'active:' in line and 'nan' not in line for line in lines)
        # the batches fed are pk_batches' with the same seed, two epochs drawn from one generator
        tr_gen = fi.TrainingSequence(str(tmp_path), dict(ident.hps), ident.nn_arch, load_flag=True)
        assert len(tr_gen.img_triplet_pairs) == mg.N_SUBJECTS * 3 + 1                    # the pickle is the reference's list
        codes = fi.subject_codes(list(tr_gen.db['subject_id']))
        rng = np.random.default_rng(5)
        want = [b for _ in range(2) for b in fi.pk_batches(codes, 2, 3, rng)]
        assert len(want) == 4 and all(len(b) == 6 for b in want)
        assert [b for e in ident.last_batch_mining['batches'] for b in e] == want
        assert len(fed) == 4 and ident.model.iterations == 4 and ident.model.bn_updates == 4
        for f, b in zip(fed, want):
            assert np.array_equal(f['subjects'], codes[b]) and f['mode'] == 'batch_semi_hard' and tuple(f['x'].shape) == (6, mg.S5, mg.S5, 3)
        assert sum(ident.last_batch_mining['counts']) == 12 and ident.last_batch_mining['counts'][3] == 0
        # the first batch's crops: bit for bit the store's gather of those rows
        labels = list(tr_gen.db.index)
        store = cs.CropStore(ident.model.ctx, len(labels), mg.S5, ident.model.dev)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=2) as pool:
            store.load([tr_gen.path(label) for label in labels], list(range(len(labels))), pool)
        assert torch.equal(fed[0]['x'], store.gather(want[0]))
        first[tier] = fed[0]['loss']
        print('%s: step losses %r' % (tier, [f['loss'] for f in fed]))
    # the first step has no earlier atomics in its history: the three tiers feed the same bits and get the same loss
    assert np.isfinite(list(first.values())).all() and len(set(first.values())) == 1, first
