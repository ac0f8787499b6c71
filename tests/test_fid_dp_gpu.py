"""Data-parallel FaceIdentifier training on the GPU (fi_conf.multi_gpu / num_gpus; the reference wraps the triplet model in
keras.utils.multi_gpu_model, face_identification.py:303-312, 348-361): fv_fid_train_step_dp's loss weight and bucket callback,
parallel.DataParallelTrainer over a FidModel (a world-size-1 `nccl` group; two ranks on the one GPU over gloo) and
FaceIdentifier.train() with two ranks.

The float64 restatement of the step and every tolerance are those of test_fid_gpu.py (_grad_close: 6 x the fp32-CPU error with a
2e-2 floor in relative L2 per tensor; _within: 4 x with floor 1e-6; loss: 4 x the fp32 error + 1e-5 relative).  Where two runs are
compared bit for bit, only values are compared that no float atomic touches: the forward pass (BN statistics are summed in fp64
slots and rounded once), the loss kernel (one workgroup, fixed order) and the dense weight-gradient (every element stored once)."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import face_identification as fi
from test_fid_gpu import _active_triplet, _grad_close, _model, _oracle_step, _within, fid_params  # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
_CASE = {}


def _case():
    """Active-hinge batch of B = 2 at S = 64 with its float64 and fp32 oracle steps (made once)."""
    if not _CASE:
        p64, s64 = fid_params(S, 23)
        xs = _active_triplet(2, S, 32)
        l64, g64, ns64, h = _oracle_step(p64, s64, xs, S, ema_step=1)
        assert (h > 0.02).all(), h
        l32, g32, ns32, _ = _oracle_step(p64.float(), s64.float(), [x.float() for x in xs], S, ema_step=1)
        _CASE.update(p=p64.float(), s=s64.float(), xs=[x.float() for x in xs], l64=l64.item(), l32=l32.item(), g64=g64, g32=g32.double(),
                     ns64=ns64, ns32=ns32)
    return _CASE


def _start(m, c):
    m.params.copy_(c['p']); m.state.copy_(c['s'])
    m.bn_updates = 0


def _tensors():
    """(name, slice) of every tensor of the fv_fid_param_count layout at S."""
    from oracle import net_oracle as no
    out = []
    for e in no.param_layout()[0][:fi.NUM_BASE_LAYERS]:
        out.append(('dW ' + e['name'], slice(e['w_off'], e['w_off'] + e['cout'] * e['k'] * e['k'] * e['cin'])))
        for nm in ('gamma_off', 'beta_off'):
            out.append((nm + ' ' + e['name'], slice(e[nm], e[nm] + e['cout'])))
    k, b = fi.dense_offsets(S)
    return out + [('dense kernel', slice(k, b)), ('dense bias', slice(b, b + 64))]


def _grads_close(g, g64, g32, what, only_base=False):
    for name, sl in _tensors()[:-2 if only_base else None]:
        _grad_close(g[sl], g64[sl], g32[sl], '%s: %s' % (what, name))


def _old_entry(m, xs):
    """fv_fid_train_step itself (FidModel.forward_backward goes through the new entry)."""
    from face_vijnana_yolov3_amd._lib import ptr
    m.ensure_optimizer()
    xa, xp, xn = (m._as_input(x) for x in xs)
    ws = m._workspace(xa.shape[0], S, True)
    return m._train_call('fv_fid_train_step', ptr(xa), ptr(xp), ptr(xn), xa.shape[0], S, ptr(ws), ws.numel(), ptr(m.grads), ptr(m._loss))


# ----------------------------------------------------------------------------- 1. weight 1 is the old step
def test_weight_one_without_callback_is_the_old_step():
    m, c = _model(S), _case()
    _start(m, c)
    loss_old = _old_entry(m, c['xs']).clone()
    torch.cuda.synchronize()
    state_old = m.state.clone()
    _start(m, c)
    loss_new = m.forward_backward(*c['xs'], on_bucket=None, loss_weight=1.0).clone()
    torch.cuda.synchronize()
    assert m.bn_updates == 3
    print('loss old %.9g new %.9g, state max diff %.3e' % (loss_old.item(), loss_new.item(), (m.state - state_old).abs().max().item()))
    assert torch.equal(loss_old, loss_new)
    assert torch.equal(m.state, state_old)
    assert abs(loss_new.item() - c['l64']) <= 4 * abs(c['l32'] - c['l64']) + 1e-5 * abs(c['l64'])
    _within(m.state.cpu(), c['ns64'], c['ns32'], 'bn moving state after a -> p -> n')
    g = m.grads.cpu()
    _grads_close(g, c['g64'], c['g32'], 'weight 1')
    assert torch.isfinite(g).all()


# ----------------------------------------------------------------------------- 2. the weight scales the gradients, not the loss
def test_loss_weight_scales_every_gradient_and_leaves_the_loss():
    m, c = _model(S), _case()
    k, b = fi.dense_offsets(S)
    _start(m, c)
    loss1 = m.forward_backward(*c['xs']).clone()
    g1 = m.grads.clone()
    _start(m, c)
    loss_q = m.forward_backward(*c['xs'], loss_weight=0.25).clone()
    gq = m.grads.clone()
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss_q)
    assert g1[b:b + 64].abs().max().item() > 0 and g1[k:b].abs().max().item() > 0
    print('dense bias max |gq - 0.25 g1| %.3e, dense kernel %.3e' % ((gq[b:b + 64] - 0.25 * g1[b:b + 64]).abs().max().item(),
                                                                    (gq[k:b] - 0.25 * g1[k:b]).abs().max().item()))
    assert torch.equal(gq[b:b + 64], 0.25 * g1[b:b + 64])        # one workgroup, fixed order; scaled once where it is rounded
    assert torch.equal(gq[k:b], 0.25 * g1[k:b])                  # every element stored once from exactly scaled dE rows
    _grads_close(gq.cpu(), 0.25 * c['g64'], 0.25 * c['g32'], 'weight 0.25', only_base=True)
    _start(m, c)
    loss_o = m.forward_backward(*c['xs'], loss_weight=0.375).clone()
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss_o)
    _grads_close(m.grads.cpu(), 0.375 * c['g64'], 0.375 * c['g32'], 'weight 0.375')


# ----------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize('weight', [0.0, -0.5, float('nan'), float('inf')])
def test_a_loss_weight_that_is_not_finite_and_positive_is_refused(weight):
    from face_vijnana_yolov3_amd._lib import FvError
    m, c = _model(S), _case()
    _start(m, c)
    m.ensure_optimizer()
    m.grads.fill_(7.0)
    with pytest.raises(FvError, match=r'\(-1\).*loss_weight'):     # FV_ERR_INVALID
        m.forward_backward(*c['xs'], loss_weight=weight)
    torch.cuda.synchronize()
    assert m.bn_updates == 0
    assert torch.equal(m.grads, torch.full_like(m.grads, 7.0))
    assert torch.equal(m.state, c['s'].to(m.dev))


# ----------------------------------------------------------------------------- 4. bucket contract
@pytest.mark.parametrize('overlap,on_side', [(True, 0), (True, 1), (False, 0), (False, 1)])
def test_bucketed_ranges_are_complete_when_reported(overlap, on_side):
    """Every reported range is copied, on the stream the contract names, at the moment it is reported; after the step every copy
    equals the final gradient range bit for bit -- a range reported before the third tower had added to it would not."""
    m, c = _model(S), _case()
    _start(m, c)
    m.ensure_optimizer()
    side = torch.cuda.ExternalStream(m.ctx.side_stream(), device=m.dev)
    snap = torch.full_like(m.grads, float('nan'))
    ranges = []
    early = bool(overlap and on_side)

    def on_bucket(off, cnt):
        ranges.append((off, cnt))
        with torch.cuda.stream(side if early else torch.cuda.current_stream(m.dev)):
            snap[off:off + cnt].copy_(m.grads[off:off + cnt])
    torch.cuda.synchronize()
    try:
        m.ctx.set_overlap(overlap)
        m.ctx.set_bucket_on_side(on_side)
        m.forward_backward(*c['xs'], on_bucket=on_bucket)
    finally:
        m.ctx.set_bucket_on_side(False)
        m.ctx.set_overlap(True)
    torch.cuda.synchronize()
    k, b = fi.dense_offsets(S)
    assert ranges[0] == (b, 64) and ranges[1] == (k, b - k)        # dense bias, dense kernel: before any base range
    assert ranges[0][0] >= k
    assert ranges[0][0] + ranges[0][1] == m.n_params and ranges[-1][0] == 0
    for (o0, _c0), (o1, c1) in zip(ranges, ranges[1:]):
        assert o1 + c1 == o0, 'descending, contiguous: (%d, %d) after offset %d' % (o1, c1, o0)
    assert len(ranges) == 2 + fi.NUM_BASE_LAYERS
    assert torch.isfinite(m.grads).all() and m.grads[:k].abs().max().item() > 0
    bad = [(o, n) for o, n in ranges if not torch.equal(snap[o:o + n], m.grads[o:o + n])]
    assert not bad, 'ranges reported before they were complete: %r' % bad[:5]
    _grads_close(m.grads.cpu(), c['g64'], c['g32'], 'overlap %r on_side %r' % (overlap, on_side))


# ----------------------------------------------------------------------------- 5. world-size-1 nccl group
WORLD1 = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import torch, torch.distributed as dist
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd.parallel import DataParallelTrainer
from test_fid_gpu import _active_triplet, fid_params
S = 64
m = fi.FidModel(S, 0)                                      # the context before the communicator
p64, s64 = fid_params(S, 51)
xs = [x.float().cuda() for x in _active_triplet(2, S, 52)]
def start():
    m.params.copy_(p64.float()); m.state.copy_(s64.float())
    m.iterations = 0; m.bn_updates = 0; m.m = m.v = m.grads = None
def run(step):
    for _ in range(3):
        loss = step()
    torch.cuda.synchronize()
    return m.params.clone(), float(loss.item())
plain = lambda: m.train_on_batch(*xs, 1e-5, 0.99, 0.99)
start()
pa, la = run(plain)
start()
pb, lb = run(plain)
spread = (pa - pb).double().norm().item()
dist.init_process_group('nccl', store=dist.HashStore(), rank=0, world_size=1, device_id=m.dev)
start()                                                    # before the trainer: it binds its buckets to m.grads
tr = DataParallelTrainer(m, world_size=1, rank=0, bucket_bytes=1 << 20, force_bucket_path=True)
assert tr.collective
pc, lc = run(lambda: tr.train_on_inputs(xs, 1e-5, 0.99, 0.99))
cover = sorted(tr.reducer.launched)
assert cover[0][0] == 0 and cover[-1][1] == m.n_params and all(cover[i][1] == cover[i + 1][0] for i in range(len(cover) - 1)), cover[:4]
assert len(cover) >= 5, len(cover)
assert tr.collectives_launched >= 3 * (len(cover) + 1), (tr.collectives_launched, len(cover))
assert m.iterations == 3 and m.bn_updates == 9
moved = (pa - p64.float().cuda()).double().norm().item()
diff = (pc - pa).double().norm().item()
print('plain spread %%.6e, bucket path vs plain %%.6e, three steps moved the parameters by %%.6e; losses %%r' %% (spread, diff, moved, (la, lb, lc)))
assert torch.isfinite(pc).all() and moved > 0
assert diff <= 4 * spread, (diff, spread)
tr.shutdown()
dist.destroy_process_group()
print('FID_WORLD1_OK buckets=%%d collectives=%%d' %% (len(cover), tr.collectives_launched))
'''


def test_world_size_one_nccl_group_trains_a_fid_model_like_the_plain_step():
    """Three steps through DataParallelTrainer (1 MiB buckets over RCCL) against three plain steps from the same start.  Gradients
    differ run to run in the float-atomic order and Adam turns that into parameter differences; the bound is therefore measured
    in the test: the L2 distance between the parameters of two PLAIN runs, x 4."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    r = subprocess.run([sys.executable, '-c', WORLD1 % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert 'FID_WORLD1_OK' in r.stdout


# ----------------------------------------------------------------------------- 6. two ranks over gloo
N_GLOBAL, P_SEED, X_SEED = 3, 61, 33     # dense kernel: a plain mean of the slice gradients is 0.33 (relative L2) from the weighted sum

TWO_RANKS = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np, torch
from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd.parallel import DataParallelTrainer, slice_batch
from test_fid_gpu import _active_triplet, fid_params
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
out, S, N = %(out)r, %(s)d, %(n)d
m = fi.FidModel(S, 0)
p64, s64 = fid_params(S, %(p_seed)d)
m.params.copy_(p64.float()); m.state.copy_(s64.float())
if rank:
    m.init_dense(seed=rank)                       # deliberately different: the trainer must broadcast rank 0's
tr = DataParallelTrainer(m, world_size=world, rank=rank, bucket_bytes=16 << 20)
lo, hi, weight = slice_batch(N, world, rank)      # 1 + 2 triplets
xs = [x[lo:hi].float().cuda() for x in _active_triplet(N, S, %(x_seed)d)]
if rank == 0:
    np.save(os.path.join(out, 'p0.npy'), m.params.cpu().numpy()); np.save(os.path.join(out, 's0.npy'), m.state.cpu().numpy())
losses = [float(tr.train_on_inputs(xs, 1e-4, 0.99, 0.99, weight=weight).item())]
torch.cuda.synchronize()
if rank == 0:
    np.save(os.path.join(out, 'g1.npy'), m.grads.cpu().numpy()); np.save(os.path.join(out, 'p1.npy'), m.params.cpu().numpy())
    np.save(os.path.join(out, 's1.npy'), m.state.cpu().numpy())
for _ in range(2):
    losses.append(float(tr.train_on_inputs(xs, 1e-4, 0.99, 0.99, weight=weight).item()))
torch.cuda.synchronize()
cover = sorted(tr.reducer.launched)
ok_cover = cover[0][0] == 0 and cover[-1][1] == m.n_params and all(cover[i][1] == cover[i + 1][0] for i in range(len(cover) - 1))
np.savez(os.path.join(out, 'rank%%d.npz' %% rank), params=m.params.cpu().numpy(), state=m.state.cpu().numpy(), losses=np.array(losses),
         ok_cover=ok_cover, nbuckets=len(cover), iterations=m.iterations, bn_updates=m.bn_updates, lo=lo, hi=hi, weight=weight)
tr.shutdown()
'''


def _torchrun(script, port, timeout=900, **env_more):
    env = dict(os.environ, FV_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1', **env_more)
    env.pop('FV_COMM_STREAM', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_two_ranks_match_the_merged_triplet_batch_oracle(tmp_path):
    from oracle import net_oracle as no
    # ---- the merged-batch oracle first (CPU): the uneven split must tell weighting from averaging before anything runs
    p64, s64 = fid_params(S, P_SEED)
    p0, s0 = p64.float(), s64.float()
    xs = _active_triplet(N_GLOBAL, S, X_SEED)
    slices = ((0, 1), (1, 3))
    g64 = torch.zeros_like(p64); g32 = torch.zeros_like(p64); plain_mean = torch.zeros_like(p64)
    st64 = torch.zeros_like(s64); st32 = torch.zeros_like(s64)
    for lo, hi in slices:
        w = (hi - lo) / float(N_GLOBAL)
        mine = [x[lo:hi] for x in xs]
        _, gr, ns, h = _oracle_step(p0.double(), s0.double(), mine, S, ema_step=1)
        assert (h > 0.02).all(), h
        _, gr32, ns32, _ = _oracle_step(p0, s0, [x.float() for x in mine], S, ema_step=1)
        g64 += w * gr; g32 += w * gr32.double(); plain_mean += gr / 2
        st64 += ns / 2; st32 += ns32.double() / 2
    k, b = fi.dense_offsets(S)
    n64 = g64[k:b].norm().item()
    rel_mean = (plain_mean[k:b] - g64[k:b]).norm().item() / n64
    rel32 = (g32[k:b] - g64[k:b]).norm().item() / n64
    print('dense kernel: plain mean of the slice gradients is %.3e from the weighted sum (fp32 oracle %.3e)' % (rel_mean, rel32))
    assert rel_mean > max(6 * rel32, 2e-2)                       # outside _grad_close's bound: averaging would be caught

    script = tmp_path / 'worker.py'
    script.write_text(TWO_RANKS % dict(root=ROOT, out=str(tmp_path), s=S, n=N_GLOBAL, p_seed=P_SEED, x_seed=X_SEED))
    _torchrun(script, 30100 + os.getpid() % 300)
    a = np.load(tmp_path / 'rank0.npz'); c = np.load(tmp_path / 'rank1.npz')
    assert (int(a['lo']), int(a['hi']), int(c['lo']), int(c['hi'])) == (0, 1, 1, 3)
    assert a['ok_cover'] and c['ok_cover'] and a['nbuckets'] >= 5 and c['nbuckets'] == a['nbuckets']
    assert a['iterations'] == 3 and c['iterations'] == 3 and a['bn_updates'] == 9 and c['bn_updates'] == 9
    assert np.array_equal(a['params'], c['params'])              # identical start (broadcast), reduced gradients and BN state
    assert np.array_equal(a['state'], c['state'])
    assert np.isfinite(a['losses']).all() and np.isfinite(c['losses']).all()
    assert not np.array_equal(a['losses'], c['losses'])          # each rank reports its own slice's loss
    assert np.array_equal(np.load(tmp_path / 'p0.npy'), p0.numpy()) and np.array_equal(np.load(tmp_path / 's0.npy'), s0.numpy())

    got = torch.from_numpy(np.load(tmp_path / 'g1.npy')).double()
    for name, sl in _tensors():
        _grad_close(got[sl], g64[sl], g32[sl], 'reduced gradient: ' + name)
    s1 = torch.from_numpy(np.load(tmp_path / 's1.npy'))
    _within(s1, st64, st32, 'bn moving state: mean over ranks of the per-slice a -> p -> n updates')
    p1 = torch.from_numpy(np.load(tmp_path / 'p1.npy')).double()
    rp, _, _ = no.keras_adam(p0.double(), got, torch.zeros_like(got), torch.zeros_like(got), 0, 1e-4, 0.99, 0.99)
    torch.testing.assert_close(p1, rp, rtol=1e-6, atol=2e-7)


# ----------------------------------------------------------------------------- 7. FaceIdentifier.train() with two ranks
TRAIN_WORKER = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r)
os.chdir(%(out)r)
from face_vijnana_yolov3_amd import face_identification as fi
rank = int(os.environ['RANK'])
rec = dict(rank=rank, saves=0, sequences=[])
seq_init, save = fi._TripletSequence.__init__, fi.FidModel.save
def init(self, raw_data_path, hps, nn_arch, load_flag=True):
    seq_init(self, raw_data_path, hps, nn_arch, load_flag=load_flag)
    rows = [[int(v) for v in t] for t in self.img_triplet_pairs]
    rec['sequences'].append(dict(load_flag=bool(load_flag), n=len(rows), sha=hashlib.sha256(json.dumps(rows).encode()).hexdigest()))
def counted_save(self, path):
    rec['saves'] += 1
    return save(self, path)
fi._TripletSequence.__init__ = init
fi.FidModel.save = counted_save
with open('conf.json') as f:
    conf = json.load(f)
ident = fi.FaceIdentifier(conf)
assert (ident.world, ident.rank) == (2, rank)
ident.train()
rec.update(iterations=ident.model.iterations, bn_updates=ident.model.bn_updates, step=conf['fi_conf']['hps']['step'])
with open('train_rank%%d.json' %% rank, 'w') as f:
    json.dump(rec, f)
'''


def test_face_identifier_train_with_two_ranks(tmp_path):
    import pandas as pd
    from PIL import Image
    rng = np.random.RandomState(1)
    os.makedirs(tmp_path / 'subject_faces')
    rows, crops = [], []
    for sid in range(3):
        base = rng.randint(0, 256, (S, S, 3))
        for j in range(2):
            img = np.clip(base + rng.randint(-20, 21, (S, S, 3)), 0, 255).astype(np.uint8)
            name = 'f%d_%d.png' % (sid, j)
            Image.fromarray(img).save(tmp_path / 'subject_faces' / name)
            rows.append(dict(subject_id=sid, face_file=name)); crops.append(img)
    pd.DataFrame(rows).to_csv(tmp_path / 'subject_image_db.csv')
    conf = {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(tmp_path), multi_gpu=True, num_gpus=2,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=dict(image_size=S, dense1_dim=64),
                            hps=dict(lr=1e-4, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=2)),
            'fd_conf': {}}
    (tmp_path / 'conf.json').write_text(json.dumps(conf))
    script = tmp_path / 'train_worker.py'
    script.write_text(TRAIN_WORKER % dict(root=ROOT, out=str(tmp_path)))
    r = _torchrun(script, 30500 + os.getpid() % 300, FV_DEVICE='0')           # both ranks on the one GPU
    recs = [json.loads((tmp_path / ('train_rank%d.json' % k)).read_text()) for k in range(2)]
    # rank 0 built, shuffled and pickled the list; rank 1 read it: one list
    assert [len(x['sequences']) for x in recs] == [1, 1]
    assert recs[0]['sequences'][0]['load_flag'] is False and recs[1]['sequences'][0]['load_flag'] is True
    assert recs[0]['sequences'][0]['sha'] == recs[1]['sequences'][0]['sha'] and recs[0]['sequences'][0]['n'] == 3
    assert os.path.exists(tmp_path / 'img_triplet_pairs.pickle')
    # 3 triplets, batch_size 2: a batch of 2 (one triplet per rank) and one of 1 < 2 ranks, skipped on both
    assert [x['step'] for x in recs] == [2, 2]
    assert [x['iterations'] for x in recs] == [1, 1] and [x['bn_updates'] for x in recs] == [3, 3]
    assert 'skipped (fewer triplets than ranks)' in r.stdout and r.stdout.count('skipped (fewer triplets than ranks)') == 1
    assert [x['saves'] for x in recs] == [1, 0]
    assert sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / 'face_identifier*'))) == ['face_identifier.h5']
    # the saved model, reloaded in this process
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        conf['fi_conf'].update(model_loading=True, multi_gpu=False, num_gpus=1)
        again = fi.FaceIdentifier(conf)
        ids = again.fid_extractor.predict(np.asarray(crops))
    finally:
        os.chdir(cwd)
    assert again.model.iterations == 1
    assert ids.shape == (6, 64) and np.isfinite(ids).all()
    assert (np.abs(np.linalg.norm(ids.astype(np.float64), axis=1) - 1.0) < 1e-5).all()
    assert math.isfinite(float(ids.sum()))
