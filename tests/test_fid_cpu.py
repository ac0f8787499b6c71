"""FaceIdentifier host side without a GPU: the flat parameter layout, configuration checks, the face_identifier.h5 round trip and
the reference's triplet list (face_identification.py:1490-1601)."""
import os
import pickle
from collections import Counter

import numpy as np
import pytest
import torch

from face_vijnana_yolov3_amd import face_identification as fi


def _conf(tmp_path, **arch):
    nn_arch = dict(image_size=64, dense1_dim=64)
    nn_arch.update(arch)
    return {'fi_conf': dict(mode='train', resource_type='uccs', raw_data_path=str(tmp_path), multi_gpu=False, num_gpus=1,
                            yolov3_base_model_load=False, model_loading=False, nn_arch=nn_arch,
                            hps=dict(lr=1e-3, beta_1=0.99, beta_2=0.99, decay=0.0, epochs=1, step=1, batch_size=1)),
            'fd_conf': {}}


def test_fid_param_count_and_layout():
    from face_vijnana_yolov3_amd._lib import lib
    L = lib()
    assert L.fv_abi_version() == 4
    assert L.fv_fid_param_count(416) == 51660576
    assert fi.feature_size(416) == 173056
    k, b = fi.dense_offsets(416)
    assert k == 40584928 and b == 40584928 + 173056 * 64 and b + 64 == 51660576
    # the base layers sit exactly at their detector offsets; the detector's head starts where the dense kernel does
    layers = fi.base_layers()
    assert len(layers) == 52 and layers[-1]['beta_off'] + layers[-1]['cout'] == k
    d = fi.dense_offsets(64)
    assert L.fv_fid_param_count(64) == d[1] + 64 == 40584928 + 4096 * 64 + 64
    assert L.fv_fid_param_count(100) == 0 and L.fv_fid_param_count(0) == 0
    assert L.fv_fid_workspace_bytes(0, 64, 1) == 0 and L.fv_fid_workspace_bytes(1, 65, 0) == 0
    # training keeps three towers that share one set of weight images: between one and three detector training workspaces
    assert L.fv_workspace_bytes(2, 64, 1) < L.fv_fid_workspace_bytes(2, 64, 1) < 3 * L.fv_workspace_bytes(2, 64, 1)
    assert 0 < L.fv_fid_workspace_bytes(2, 64, 0) < L.fv_fid_workspace_bytes(2, 64, 1)
    assert L.fv_fid_dense_partial_floats(3, 173056) == 676 * 3 * 64 and L.fv_fid_dense_partial_floats(3, 100) == 0


def test_dense1_dim_other_than_64_raises(tmp_path):
    with pytest.raises(ValueError, match='dense1_dim'):
        fi.FaceIdentifier(_conf(tmp_path, dense1_dim=128))
    with pytest.raises(ValueError, match='multiple of 32'):
        fi.FaceIdentifier(_conf(tmp_path, image_size=100))


def test_main_rejects_unimplemented_modes(tmp_path, monkeypatch):
    import json
    monkeypatch.chdir(tmp_path)
    conf = _conf(tmp_path)
    conf['fi_conf']['mode'] = 'evaluate'
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match='evaluate'):
        fi.main()


def _host_model(S):
    """A FidModel whose vectors live on the host (save / load touch no device call)."""
    m = fi.FidModel.__new__(fi.FidModel)
    m.image_size = S
    m.layers = fi.base_layers()
    m.F = fi.feature_size(S)
    m.kernel_off, m.bias_off = fi.dense_offsets(S)
    m.n_params = m.bias_off + 64
    from face_vijnana_yolov3_amd._lib import lib
    m.n_state = int(lib().fv_state_count())
    g = torch.Generator().manual_seed(3)
    m.params = torch.randn(m.n_params, generator=g)
    m.state = torch.rand(m.n_state, generator=g)
    m.grads = m.m = m.v = None
    m.iterations, m.bn_updates = 7, 21
    return m


def test_face_identifier_h5_round_trip(tmp_path):
    from face_vijnana_yolov3_amd.hdf5_lite import read_hdf5
    a = _host_model(32)
    path = str(tmp_path / 'face_identifier.h5')
    a.save(path)
    datasets, attrs = read_hdf5(path)
    # Keras layout: the base as the nested model 'base', the dense layer in its own group
    assert datasets['/model_weights/dense1/dense1/kernel:0'].shape == (1024, 64)
    assert datasets['/model_weights/dense1/dense1/bias:0'].shape == (64,)
    assert datasets['/model_weights/base/conv_0/kernel:0'].shape == (3, 3, 3, 32)
    assert '/model_weights/base/bnorm_73/moving_variance:0' in datasets
    np.testing.assert_array_equal(datasets['/model_weights/dense1/dense1/kernel:0'],
                                  a.params[a.kernel_off:a.bias_off].numpy().reshape(1024, 64))
    b = _host_model(32)
    b.params.zero_(); b.state.zero_(); b.iterations = b.bn_updates = 0
    b.load(path)
    assert torch.equal(a.params, b.params) and torch.equal(a.state, b.state)
    assert (b.iterations, b.bn_updates) == (7, 21)
    # a file of another image size does not fit
    c = _host_model(64)
    with pytest.raises(Exception, match='dense1'):
        c.load(path)


def _write_db(tmp_path, sizes):
    import pandas as pd
    from PIL import Image
    rows = []
    os.makedirs(tmp_path / 'subject_faces', exist_ok=True)
    rng = np.random.RandomState(0)
    for sid, n in enumerate(sizes):
        for j in range(n):
            name = 's%d_%d.png' % (sid, j)
            Image.fromarray(rng.randint(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / 'subject_faces' / name)
            rows.append(dict(subject_id=100 + sid, face_file=name))
    pd.DataFrame(rows).to_csv(tmp_path / 'subject_image_db.csv')     # the reference's layout: a running index column first
    return rows


def test_triplet_list_and_steps(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sizes = [3, 4, 1, 2]
    rows = _write_db(tmp_path, sizes)
    np.random.seed(5)
    hps = dict(batch_size=4, step=1)
    seq = fi.TrainingSequence(str(tmp_path), hps, dict(image_size=32), load_flag=False)
    trip = seq.img_triplet_pairs
    subj = [r['subject_id'] for r in rows]
    # every pair k < l within a subject once, the negative from another subject
    assert len(trip) == sum(n * (n - 1) // 2 for n in sizes) == 10
    assert all(subj[a] == subj[p] and a < p and subj[n] != subj[a] for a, p, n in trip)
    assert Counter(subj[a] for a, _, _ in trip) == Counter({100: 3, 101: 6, 103: 1})
    assert len({(a, p) for a, p, _ in trip}) == 10
    # steps: whole batches plus the short last one; the pickle holds the shuffled list
    assert hps['step'] == len(seq) == 3 == fi.num_batches(10, 4)
    with open(tmp_path / 'img_triplet_pairs.pickle', 'rb') as f:
        assert pickle.load(f) == trip
    x, y = seq[2]
    assert x['input_a'].shape == (2, 32, 32, 3) and x['input_n'].shape == (2, 32, 32, 3) and y['output'].shape == (2, 192)
    assert x['input_p'].dtype == np.float32 and 0.0 <= x['input_p'].min() and x['input_p'].max() <= 1.0
    assert seq[0][0]['input_a'].shape == (4, 32, 32, 3)
    # load_flag=True reads the same list back
    again = fi.TrainingSequence(str(tmp_path), dict(batch_size=4), dict(image_size=32), load_flag=True)
    assert again.img_triplet_pairs == trip and len(again) == 3
