"""The table of tests/stream_order.py stays complete: every fv_* symbol include/fv_hotpath.h declares is either a row of the
delayed-stream table or exempt with a reason, and the rows' two problems can be told apart.  Needs no GPU."""
import pytest
import torch

import stream_order as so
from test_abi_symbols import declared_symbols

# the only rows that may skip the "returned while the sleep still ran" assertion (each row carries its reason)
HOST_SYNC_SYMBOLS = {'fv_fid_pair_dists', 'fv_fid_mine_negatives', 'fv_profile_collect', 'fv_jpeg_encode_measure', 'fv_jpeg_encode_emit',
                     'fv_jpeg_encode_coefs', 'fv_yolo_decode_nms'}


def test_every_declared_symbol_is_a_row_or_exempt():
    declared = set(declared_symbols())
    table = set(so.table_symbols())
    exempt = set(so.EXEMPT)
    assert not table & exempt, sorted(table & exempt)
    assert not declared - table - exempt, 'neither a row nor exempt: %s' % sorted(declared - table - exempt)
    assert not (table | exempt) - declared, 'not declared in the header: %s' % sorted((table | exempt) - declared)


def test_exemptions_carry_a_one_line_reason():
    for sym, why in so.EXEMPT.items():
        assert isinstance(why, str) and why.strip() and '\n' not in why, sym


def test_rows_are_well_formed():
    names = [c.name for c in so.CASES + so.STEP_CASES]
    assert len(names) == len(set(names))
    for c in so.CASES + so.STEP_CASES:
        assert c.symbols and callable(c.make) and callable(c.call), c.name
        if c.host_sync:
            assert isinstance(c.host_sync, str) and c.host_sync.strip(), c.name
            assert set(c.symbols) <= HOST_SYNC_SYMBOLS, (c.name, 'a new host_sync row needs its entry point named here')
    assert not any(c.host_sync for c in so.STEP_CASES)


def test_the_return_join_rows_cover_both_schedules_of_every_step():
    steps = {'fv_train_step', 'fv_yolov3_train_step', 'fv_yolov3_train_step_det', 'fv_fid_train_step', 'fv_fid_batch_train_step',
             'fv_fid_cls_train_step'}
    for early in (1, 0):
        got = {s for c in so.STEP_CASES for s in c.symbols if c.options.get('early_bn_fused', 1) == early}
        assert got == steps, (early, sorted(steps - got))
    for c in so.STEP_CASES:
        assert c.options['overlap'] == 1 and c.ref_options == {'overlap': 0}, c.name


def test_delay_rule():
    assert so.delay_ms(0.0) == 20.0 and so.delay_ms(0.010) == 40.0 and so.delay_ms(1.0) == 500.0


def test_same_bits():
    nan = torch.tensor([float('nan'), 1.0])
    assert so.same_bits(nan, nan.clone()) and not so.same_bits(nan, torch.tensor([float('nan'), 2.0]))
    assert not so.same_bits(torch.zeros(2), torch.zeros(3)) and not so.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert so.same_bits([b'ab', (1, 2)], [b'ab', (1, 2)]) and not so.same_bits([b'ab'], [b'ac'])


REF64 = [c for c in so.CASES if c.ref64 is not None]


@pytest.mark.parametrize('case', REF64, ids=[c.name for c in REF64])
def test_the_two_problems_differ_through_the_float64_reference(case):
    """Step 2 of the harness without a GPU, where the operation has a plain float64 reference: every input differs between
    seed and seed + 1 unless it is an index, and every reference output differs by more than 100 x the case's tolerance (the
    rows with a reference are bit-exact ones: the outputs must simply not be equal, element for element almost everywhere)."""
    real, stale = case.make(1234, 'cpu'), case.make(1235, 'cpu')
    assert sorted(real) == sorted(stale)
    for k in real:
        assert real[k].shape == stale[k].shape and real[k].dtype == stale[k].dtype
        if real[k].is_floating_point():
            assert not torch.equal(real[k], stale[k]), k
            assert bool(torch.isfinite(real[k]).all()) and bool(torch.isfinite(stale[k]).all()), k
    a, b = case.ref64(real), case.ref64(stale)
    assert case.exact
    for name in a:
        assert a[name].shape == b[name].shape
        assert float((a[name] != b[name]).double().mean()) > 0.9, name


HOSTABLE = [c for c in so.CASES if c.ctx is so.shared_ctx]


@pytest.mark.parametrize('case', HOSTABLE, ids=[c.name for c in HOSTABLE])
def test_builders_make_two_valid_problems_of_one_shape(case):
    """Every operator row's builder, on the host: same keys, shapes and types; integer inputs (labels, offsets, geometry) are
    the same valid values in both problems; float inputs are finite (no NaN ever stands in for data)."""
    real, stale = case.make(1234, 'cpu'), case.make(1235, 'cpu')
    assert sorted(real) == sorted(stale)
    differ = False
    for k in real:
        assert real[k].shape == stale[k].shape and real[k].dtype == stale[k].dtype and real[k].is_contiguous(), k
        if real[k].dtype in (torch.int32, torch.int64):
            assert torch.equal(real[k], stale[k]), k
        elif real[k].is_floating_point():
            assert bool(torch.isfinite(real[k]).all()), k
        differ = differ or not torch.equal(real[k], stale[k])
    assert differ
