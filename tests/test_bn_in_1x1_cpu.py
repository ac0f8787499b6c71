"""Option "bn_in_1x1" without a device: which normalise passes the schedules fold into the next layer's 1x1 conv
(fv_train_bn_in_1x1_plan / fv_yolov3_train_bn_in_1x1_plan list the decision train_bn_forward makes).

Only the first 1x1 conv of a residual block (role 1: 1x1, stride 1, fed by the layer in front of it) may take the pass of its
producer: a 3x3 or strided consumer, one fed by a route or a concatenation, and a detection head keep the pass in front.  With
the option 0 nothing is folded: the schedule makes the launches it made before."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def L():
    from face_vijnana_yolov3_amd.build import build_library
    build_library()
    from face_vijnana_yolov3_amd._lib import lib
    return lib()


def _plan(L, graph, option, B, S):
    from face_vijnana_yolov3_amd.engine import layer_table
    from face_vijnana_yolov3_amd.yolov3 import yolov3_layer_table
    if graph == 'detector':
        layers = layer_table()
        out = (ctypes.c_int32 * len(layers))()
        assert L.fv_train_bn_in_1x1_plan(option, B, S, out, len(layers)) == 0
    else:
        layers = yolov3_layer_table(255)
        out = (ctypes.c_int32 * len(layers))()
        assert L.fv_yolov3_train_bn_in_1x1_plan(option, B, S, 255, out, len(layers)) == 0
    return layers, list(out)


@pytest.mark.parametrize('graph', ['detector', 'three_scale'])
@pytest.mark.parametrize('B,S', [(40, 416), (16, 608), (2, 64)])
def test_option_off_folds_nothing(L, graph, B, S):
    _, folded = _plan(L, graph, 0, B, S)
    assert not any(folded)


@pytest.mark.parametrize('graph', ['detector', 'three_scale'])
@pytest.mark.parametrize('option', [1, 2])
@pytest.mark.parametrize('B,S', [(40, 416), (16, 608), (2, 64)])
def test_only_the_first_conv_of_a_residual_block_takes_the_pass(L, graph, option, B, S):
    layers, folded = _plan(L, graph, option, B, S)
    assert not folded[-1]
    for l, f in enumerate(folded):
        if not f:
            continue
        d, dn = layers[l], layers[l + 1]
        assert d['has_bn'] and dn['has_bn']                                       # not a detection head, and not in front of one
        assert dn['role'] == 1 and dn['ksize'] == 1 and dn['stride'] == 1        # never 3x3, strided, route- or concatenation-fed
        assert dn['cin'] == d['cout'] and dn['in_div'] == d['out_div']            # fed by the layer whose pass it takes
        assert dn['cin'] % 32 == 0 and dn['cin'] <= 512 and dn['cout'] > 32       # what the kernel takes


@pytest.mark.parametrize('graph', ['detector', 'three_scale'])
def test_option_2_folds_every_block_the_kernel_takes(L, graph):
    layers, folded = _plan(L, graph, 2, 40, 416)
    want = [1 if l + 1 < len(layers) and layers[l + 1]['role'] == 1 and 32 < layers[l + 1]['cout'] and layers[l + 1]['cin'] <= 512 else 0
            for l in range(len(layers))]
    assert folded == want
    assert sum(folded) == 18          # 2 at 104^2, 8 at 52^2, 8 at 26^2 (208^2 has 32 output channels, 13^2 has 1024 input channels)
    _, on = _plan(L, graph, 1, 40, 416)
    assert all(a <= b for a, b in zip(on, folded))   # the default is a selection among them


def test_bad_arguments(L):
    out = (ctypes.c_int32 * 4)()
    assert L.fv_train_bn_in_1x1_plan(1, 40, 416, out, 4) != 0          # wrong layer count
    assert L.fv_train_bn_in_1x1_plan(1, 40, 400, out, 4) != 0
