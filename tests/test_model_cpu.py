"""The host side the three device models share, without a GPU: Engine and Yolov3 checkpoints (the Keras-layout .h5 with this
build's Adam state under /fv, and the .npz of rounds 1-2), their refusals, and the synthetic initialisation.  The models are built
with their vectors on the host (`__new__`, no device), as tests/test_fid_cpu.py builds a FidModel."""
import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import weights
from face_vijnana_yolov3_amd._lib import FvError, lib
from face_vijnana_yolov3_amd.engine import Engine, layer_table
from face_vijnana_yolov3_amd.yolov3 import Yolov3, yolov3_layer_table


def _host_model(cls, seed=3, adam=False, out_channels=18):
    """An Engine or a Yolov3 whose vectors live on the host (save / load / init_synthetic touch no device call)."""
    m = cls.__new__(cls)
    if cls is Yolov3:
        m.out_channels = out_channels
        m.layers = yolov3_layer_table(out_channels)
        m.n_params = int(lib().fv_yolov3_param_count(out_channels))
        m.n_state = int(lib().fv_yolov3_state_count(out_channels))
    else:
        m.layers = layer_table()
        m.n_params = int(lib().fv_param_count())
        m.n_state = int(lib().fv_state_count())
    g = torch.Generator().manual_seed(seed)
    m.params = torch.randn(m.n_params, generator=g)
    m.state = torch.rand(m.n_state, generator=g)
    m.grads = m.m = m.v = None
    if adam:
        m.grads = torch.zeros(m.n_params)
        m.m = torch.randn(m.n_params, generator=g)
        m.v = torch.rand(m.n_params, generator=g)
    m.iterations, m.bn_updates, m.bn_zero_debias = 7, 0, False
    return m


def _blank(cls, **kw):
    m = _host_model(cls, seed=11, **kw)
    m.params.zero_(); m.state.zero_(); m.iterations = 0
    return m


def _same(a, b):
    assert torch.equal(a.params, b.params) and torch.equal(a.state, b.state) and a.iterations == b.iterations
    assert (a.m is None) == (b.m is None)
    if a.m is not None:
        assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def _h5_expected(path, m, nested, **extras):
    """The file weights.write_keras_h5 writes for these vectors: save() must write exactly these bytes."""
    ex = dict(iterations=np.int64(m.iterations))
    ex.update(extras)
    if m.m is not None:
        ex['adam_m'] = m.m.numpy(); ex['adam_v'] = m.v.numpy()
    weights.write_keras_h5(path, m.layers, m.params.numpy(), m.state.numpy(), nested=nested, extras=ex)
    with open(path, 'rb') as f:
        return f.read()


def test_engine_h5_round_trip(tmp_path):
    a = _host_model(Engine, adam=True)
    for nested in ('model_1', None):
        path = str(tmp_path / 'face_detector.h5')
        if nested:
            a.save(path)
        else:
            a.save(path, nested=None)
        with open(path, 'rb') as f:
            assert f.read() == _h5_expected(str(tmp_path / 'expected.h5'), a, nested)
        b = _blank(Engine)
        b.load(path)
        _same(a, b)


@pytest.mark.parametrize('adam', [False, True])
def test_engine_npz_round_trip(tmp_path, adam):
    a = _host_model(Engine, adam=adam)
    path = str(tmp_path / 'engine.npz')
    a.save(path)
    with np.load(path) as d:
        assert sorted(d.files) == sorted(['params', 'state', 'iterations'] + (['m', 'v'] if adam else []))
        assert int(d['iterations']) == 7 and np.array_equal(d['params'], a.params.numpy())
    b = _blank(Engine)
    b.load(path)
    _same(a, b)


def test_engine_loads_a_base_file_only_when_asked(tmp_path):
    """yolov3_base.h5 holds no head: refused by default; with require_all=False the base is read and the head keeps its values."""
    a = _host_model(Engine)
    path = str(tmp_path / 'yolov3_base.h5')
    weights.write_keras_h5(path, a.layers[:-1], a.params.numpy(), a.state.numpy(), nested=None)
    b = _blank(Engine)
    with pytest.raises(FvError, match='lacks'):
        b.load(path)
    b.params.fill_(0.5)
    b.load(path, require_all=False)
    head = a.layers[-1]['w_off']
    assert torch.equal(b.params[:head], a.params[:head]) and bool((b.params[head:] == 0.5).all())
    assert torch.equal(b.state, a.state) and b.iterations == 0 and b.m is None


def test_yolov3_h5_round_trip(tmp_path):
    a = _host_model(Yolov3, adam=True)
    path = str(tmp_path / 'yolov3.h5')
    a.save(path)
    with open(path, 'rb') as f:
        assert f.read() == _h5_expected(str(tmp_path / 'expected.h5'), a, None, out_channels=np.int64(18))
    b = _blank(Yolov3)
    b.load(path)
    _same(a, b)


@pytest.mark.parametrize('adam', [False, True])
def test_yolov3_npz_round_trip(tmp_path, adam):
    a = _host_model(Yolov3, adam=adam)
    path = str(tmp_path / 'yolov3.npz')
    a.save(path)
    with np.load(path) as d:
        assert sorted(d.files) == sorted(['params', 'state', 'iterations', 'out_channels'] + (['m', 'v'] if adam else []))
        assert int(d['out_channels']) == 18
    b = _blank(Yolov3)
    b.load(path)
    _same(a, b)


@pytest.mark.parametrize('ext', ['h5', 'npz'])
def test_yolov3_refuses_another_out_channels(tmp_path, ext):
    a = _host_model(Yolov3)
    path = str(tmp_path / ('yolov3.' + ext))
    a.save(path)
    b = _blank(Yolov3, out_channels=255)
    with pytest.raises(ValueError, match='18 output channels, this one has 255'):
        b.load(path)
    assert not b.params.any() and b.iterations == 0


def test_yolov3_refuses_missing_tensors(tmp_path):
    a = _host_model(Yolov3)
    path = str(tmp_path / 'yolov3_base.h5')
    weights.write_keras_h5(path, a.layers[:52], a.params.numpy(), a.state.numpy(), nested=None)
    with pytest.raises(ValueError, match='lacks'):
        _blank(Yolov3).load(path)


def test_synthetic_init_shares_the_base():
    """init_synthetic draws the base layers first: the detector and the three-scale model get the same base from one seed, and
    every kernel / BN vector follows the documented distributions."""
    e, y = _blank(Engine), _blank(Yolov3)
    e.init_synthetic(7); y.init_synthetic(7)
    d = e.layers[51]
    n_p, n_s = d['beta_off'] + d['cout'], d['var_off'] + d['cout']
    assert torch.equal(e.params[:n_p], y.params[:n_p]) and torch.equal(e.state[:n_s], y.state[:n_s])
    for m in (e, y):
        for d in m.layers:
            k, cin, cout = d['ksize'], d['cin'], d['cout']
            w = m.params[d['w_off']:d['w_off'] + cout * k * k * cin]
            assert not (m.params[d['beta_off']:d['beta_off'] + cout]).any()
            if d['has_bn']:
                assert bool((m.params[d['gamma_off']:d['gamma_off'] + cout] == 1).all())
                assert bool((m.state[d['var_off']:d['var_off'] + cout] == 1).all())
                assert not m.state[d['mean_off']:d['mean_off'] + cout].any()
            else:
                assert float(w.abs().max()) <= float(np.sqrt(6.0 / (k * k * cin + k * k * cout)))
    again = _blank(Engine)
    again.init_synthetic(7)
    assert torch.equal(again.params, e.params) and torch.equal(again.state, e.state)

