"""JPEG decode split host / device, GPU half (csrc/jpeg.hip: jpeg_idct_kernel, jpeg_color_kernel through the C ABI): the RGB
pixels the device reconstructs from the host's Huffman-decoded coefficients are bit-identical to Pillow's -- the reference's
reader (`imread`, face_detection.py:112, 656, 798) -- for every sampling mode, odd sizes, restart intervals and mixed batches;
the letterboxed network input is therefore the same tensor as through the Pillow path, and FaceDetector.test() writes the
same rows either way.  The differential contract of DESIGN.md section 12 on the device: every size 1..24 x 1..24, every file of
the stream corpus (tests/jpeg_stream_ref.py) that the host half accepts, the kernels' grid-stride loops, and a truncated file
through every loader."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from test_jpeg_cpu import CASES, _jpeg  # noqa: E402  (tests/ is on sys.path under pytest's rootdir conftest)


@pytest.fixture(scope='module')
def ctx():
    from face_vijnana_yolov3_amd._lib import Context
    return Context(0)


def _device_decode(ctx, datas):
    from face_vijnana_yolov3_amd import jpeg
    infos = [jpeg.parse(d) for d in datas]
    assert all(i is not None for i in infos)
    plan = jpeg.BatchPlan(infos)
    coefs = np.empty(plan.total_coefs, np.int16)
    for i, d in enumerate(datas):
        jpeg.entropy_decode(d, infos[i], coefs[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
    rgb = jpeg.reconstruct_batch(ctx, plan, torch.from_numpy(coefs).cuda(), torch.device('cuda', 0)).cpu().numpy()
    return [rgb[plan.rgb_off[i]:plan.rgb_off[i] + I.height * I.width * 3].reshape(I.height, I.width, 3) for i, I in enumerate(infos)], plan


def test_device_pixels_equal_pillow_in_one_mixed_batch(ctx):
    rng = np.random.default_rng(7)
    cases = CASES + [(480, 640, 2, 90, False, 0), (601, 333, 1, 75, False, 7), (768, 1024, 2, 85, False, 0), (1080, 1920, 2, 92, False, 0),
                     (333, 601, 0, 60, True, 0)]
    datas = [_jpeg(rng, *c) for c in cases]
    got, _plan = _device_decode(ctx, datas)
    for c, d, g in zip(cases, datas, got):
        want = np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        assert g.shape == want.shape and np.array_equal(g, want), (c, int(np.abs(g.astype(int) - want.astype(int)).max()))


def _against_pillow(names, datas, got):
    bad = []
    for name, d, g in zip(names, datas, got):
        want = np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        if g.shape != want.shape or not np.array_equal(g, want):
            bad.append((name, 'shape' if g.shape != want.shape else int(np.abs(g.astype(int) - want.astype(int)).max())))
    return bad


def test_size_sweep_on_the_device_equals_pillow(ctx):
    """Every size 1..24 x 1..24 in every sampling mode (the CPU sweep's 2304 files) in ONE mixed batch: jpeg_color_kernel's
    chroma_at replicates where the image has at most two chroma columns, as libjpeg's jinit_upsampler selects."""
    from test_jpeg_cpu import sweep_files
    names, datas = zip(*sweep_files())
    got, _plan = _device_decode(ctx, list(datas))
    bad = _against_pillow(names, datas, got)
    assert not bad, (len(bad), bad[:20])


def test_stream_corpus_on_the_device_equals_pillow(ctx):
    """Every file of the stream corpus that the host half accepts, in one mixed batch: device pixels == Pillow's, per file --
    among them the blocks AT the bound of the accepted coefficient range (int32 dequantisation, 64-bit IDCT temporaries)."""
    import jpeg_stream_ref as sr
    from test_jpeg_cpu import _product
    files = [(name, data) for name, data, _planes, _expect in sr.corpus() if _product(data) is not None]
    assert len(files) >= 100 and {'aligned_at_bound', 'random_at_bound', 'gray_long_ri1', 'ac_size_10'} <= {n for n, _ in files}
    names, datas = zip(*files)
    got, _plan = _device_decode(ctx, list(datas))
    bad = _against_pillow(names, datas, got)
    assert not bad, bad


def test_grid_size_does_not_change_the_pixels(ctx):
    """fv_jpeg_reconstruct_batch with the plan's max_blocks / max_pixels (the grid size) and with both 1: one workgroup per
    image walks every block and every pixel in the kernels' grid-stride loops -- the same RGB buffer, and Pillow's."""
    from face_vijnana_yolov3_amd import jpeg
    from face_vijnana_yolov3_amd._lib import ptr
    rng = np.random.default_rng(10)
    cases = [(33, 17, 2, 80, False, 0), (100, 130, 1, 30, False, 2), (40, 56, 0, 85, True, 0), (45, 67, 0, 90, False, 0), (150, 90, 2, 75, False, 5)]
    datas = [_jpeg(rng, *c) for c in cases]
    infos = [jpeg.parse(d) for d in datas]
    plan = jpeg.BatchPlan(infos)
    assert plan.max_blocks > 128 and plan.max_pixels > 256          # more than one workgroup's worth: the loops do iterate
    coefs = np.empty(plan.total_coefs, np.int16)
    for i, d in enumerate(datas):
        jpeg.entropy_decode(d, infos[i], coefs[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
    dev = torch.device('cuda', 0)
    coefs_dev = torch.from_numpy(coefs).to(dev)
    descs = torch.frombuffer(bytearray(bytes(plan.descs)), dtype=torch.uint8).to(dev)
    out = []
    for max_blocks, max_pixels in ((plan.max_blocks, plan.max_pixels), (1, 1)):
        planes = torch.zeros(plan.plane_bytes, dtype=torch.uint8, device=dev)
        rgb = torch.full((plan.rgb_bytes,), 77, dtype=torch.uint8, device=dev)
        rc = jpeg._fn().fv_jpeg_reconstruct_batch(ctx.handle, ptr(coefs_dev), ptr(descs), plan.n, ptr(planes), ptr(rgb), max_blocks, max_pixels)
        ctx.check(rc, 'fv_jpeg_reconstruct_batch')
        out.append(rgb.cpu().numpy())
    assert np.array_equal(out[0], out[1])
    got = [out[1][plan.rgb_off[i]:plan.rgb_off[i] + I.height * I.width * 3].reshape(I.height, I.width, 3) for i, I in enumerate(infos)]
    assert not _against_pillow(cases, datas, got)


def test_letterbox_of_narrow_images_from_coefficients_equals_pillow(ctx):
    """3 x 40 and 40 x 3 as 4:2:0 (one and two chroma columns / rows) through letterbox_batch_device, from coefficients and from
    Pillow's pixels: the same tensor."""
    from face_vijnana_yolov3_amd import jpeg
    from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
    rng = np.random.default_rng(12)
    datas = [_jpeg(rng, h, w, 2, 88) for (h, w) in [(3, 40), (40, 3), (4, 40), (40, 4)]]
    infos = [jpeg.parse(d) for d in datas]
    plan = jpeg.BatchPlan(infos)
    coefs = torch.empty(plan.total_coefs, dtype=torch.int16).pin_memory()
    for i, d in enumerate(datas):
        jpeg.entropy_decode(d, infos[i], coefs.numpy()[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
    dev = torch.device('cuda', 0)
    x1, g1 = letterbox_batch_device(ctx, None, 96, dev, packed=('jpeg', coefs, plan))
    raws = [np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas]
    x2, g2 = letterbox_batch_device(ctx, raws, 96, dev)
    assert g1 == g2 and torch.equal(x1, x2)


def test_loaders_treat_a_truncated_file_as_pillow_does(ctx, tmp_path, monkeypatch):
    """A file cut in the middle of its scan (Pillow: OSError) through the three other callers of entropy_decode: FaceDetector.test()
    with hps.device_jpeg on and off, create_db's load_batch with device_jpeg on and off, CropStore.load against Pillow's reader --
    the same exception type either way; each caller hands the file the strict scan refuses to Pillow, which raises."""
    from concurrent.futures import ThreadPoolExecutor
    from face_vijnana_yolov3_amd import crop_store, face_detection
    from face_vijnana_yolov3_amd import face_identification as fi
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    from face_vijnana_yolov3_amd.postproc import PinnedRing
    from test_jpeg_cpu import _outcome, truncated_file
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(face_detection, 'DEBUG', False)
    root = str(tmp_path / 'imgs'); os.makedirs(root)
    rng = np.random.default_rng(13)
    good, bad = truncated_file(rng, 64, 64)
    paths = [os.path.join(root, n) for n in ('img_0.jpg', 'img_1.jpg')]
    open(paths[0], 'wb').write(good)
    open(paths[1], 'wb').write(bad)
    # create_db: load_batch
    with ThreadPoolExecutor(max_workers=2) as pool:
        ring = PinnedRing(3)
        a, b = (_outcome(lambda: fi.load_batch(paths, pool, ring, dj)) for dj in (True, False))
        assert a[0] == b[0] == 'raised' and a[1] is b[1] is OSError, (a, b)
        assert fi.load_batch(paths[:1], pool, ring, True)[0] == 'jpeg'                        # the ring is usable afterwards
        # the crop store: the damaged file alone goes to Pillow
        store = crop_store.CropStore(ctx, 2, 64, torch.device('cuda', 0))
        a, b = _outcome(lambda: store.load(paths, [0, 1], pool)), _outcome(lambda: fi._imread(paths[1]))
        assert a[0] == b[0] == 'raised' and a[1] is b[1] is OSError, (a, b)
        store.load(paths[:1], [1], pool)
        assert np.array_equal(store.data[1].cpu().numpy(), fi._imread(paths[0]))
    # FaceDetector.test()
    conf = {'mode': 'test', 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'a.csv'), 'multi_gpu': False,
            'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2, 'face_conf_th': 0.5,
                    'nms_iou_th': 0.5, 'num_cands': 60, 'eval_batch_size': 2},
            'nn_arch': {'image_size': 96, 'bb_info_c_size': 6}}
    fd = FaceDetector(conf)
    a = _outcome(fd.test)
    conf['hps']['device_jpeg'] = False
    fd.conf = dict(conf, output_file_path=os.path.join(root, 'b.csv'))
    b = _outcome(fd.test)
    assert a[0] == b[0] == 'raised' and a[1] is b[1] is OSError, (a, b)


def test_letterbox_from_coefficients_equals_letterbox_from_pillow(ctx):
    from face_vijnana_yolov3_amd import jpeg
    from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
    rng = np.random.default_rng(8)
    datas = [_jpeg(rng, h, w, sub, 88) for (h, w, sub) in [(480, 640, 2), (640, 480, 1), (300, 300, 0), (721, 1283, 2)]]
    infos = [jpeg.parse(d) for d in datas]
    plan = jpeg.BatchPlan(infos)
    coefs = torch.empty(plan.total_coefs, dtype=torch.int16).pin_memory()
    for i, d in enumerate(datas):
        jpeg.entropy_decode(d, infos[i], coefs.numpy()[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)])
    dev = torch.device('cuda', 0)
    x1, g1 = letterbox_batch_device(ctx, None, 416, dev, packed=('jpeg', coefs, plan))
    raws = [np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas]
    x2, g2 = letterbox_batch_device(ctx, raws, 416, dev)
    assert g1 == g2 and torch.equal(x1, x2)


def test_facedetector_test_rows_do_not_depend_on_the_decoder(tmp_path, monkeypatch):
    from face_vijnana_yolov3_amd import face_detection
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(face_detection, 'DEBUG', False)
    root = str(tmp_path / 'imgs'); os.makedirs(root)
    rng = np.random.default_rng(9)
    for k, (h, w, sub) in enumerate([(480, 640, 2), (640, 480, 1), (416, 416, 0), (300, 520, 2), (520, 300, 2)]):
        open(os.path.join(root, 'img_%d.jpg' % k), 'wb').write(_jpeg(rng, h, w, sub, 90))
    Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(os.path.join(root, 'img_9.jpg'), progressive=True)   # -> Pillow
    conf = {'mode': 'test', 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'a.csv'), 'multi_gpu': False,
            'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2, 'face_conf_th': 0.5,
                    'nms_iou_th': 0.5, 'num_cands': 60, 'eval_batch_size': 3},
            'nn_arch': {'image_size': 416, 'bb_info_c_size': 6}}
    fd = FaceDetector(conf)
    d = fd.model.layers[-1]
    fd.model.params[d['w_off']:d['beta_off']] *= 0.02                 # a head that depends on the pixels and fires on some cells
    fd.model.params[d['beta_off']] = 0.4; fd.model.params[d['beta_off'] + 5] = 0.4
    fd.test()
    rows_dev = open(conf['output_file_path']).read()
    conf['hps']['device_jpeg'] = False
    fd.conf = dict(conf, output_file_path=os.path.join(root, 'b.csv'))
    fd.test()
    assert rows_dev == open(os.path.join(root, 'b.csv')).read() and len(rows_dev.splitlines()) > 0


def test_training_feeder_through_coefficients_equals_pillow(tmp_path):
    """BatchFeeder with hps.device_jpeg (default) and without: the same letterboxed batch and the same targets."""
    from face_vijnana_yolov3_amd import data
    from face_vijnana_yolov3_amd.engine import Engine
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder
    from face_vijnana_yolov3_amd.postproc import letterbox_batch_device
    root = str(tmp_path)
    data.make_synthetic_uccs(root, n_images=4, seed=5)
    eng = Engine(0)
    xs = []
    for dj in (True, False):
        seq = data.TrainingSequence(root, {'batch_size': 4, 'step': 1, 'device_jpeg': dj}, {'image_size': 416, 'bb_info_c_size': 6})
        f = BatchFeeder(seq, 1, 0, 4)
        packed, y, weight, (_f, slot) = f.load(0)
        assert (isinstance(packed[0], str) and packed[0] == 'jpeg') == dj
        x, _ = letterbox_batch_device(eng.ctx, None, 416, eng.dev, packed=packed)
        xs.append((x.clone(), y.clone()))
        f.close()
    assert torch.equal(xs[0][0], xs[1][0]) and torch.equal(xs[0][1], xs[1][1])


def test_pipelined_input_path_equals_the_serial_one(tmp_path):
    """run_pipelined (batch k+1 staged on its own stream while step k computes, losses reported one step late) against
    train_on_item (everything on the compute stream): same batches in the same order -> the same losses and, up to the float-atomic
    order inside dW, the same parameters after three Adam steps."""
    from face_vijnana_yolov3_amd import data
    from face_vijnana_yolov3_amd.engine import Engine
    from face_vijnana_yolov3_amd.face_detection import BatchFeeder, run_pipelined, train_on_item
    from face_vijnana_yolov3_amd.parallel import DataParallelTrainer
    root = str(tmp_path)
    data.make_synthetic_uccs(root, n_images=6, seed=6)
    hp = {'batch_size': 2, 'step': 1, 'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0}
    res = []
    for pipelined in (False, True):
        eng = Engine(0); eng.init_synthetic(7)
        tr = DataParallelTrainer(eng, world_size=1, rank=0)
        seq = data.TrainingSequence(root, dict(hp), {'image_size': 96, 'bb_info_c_size': 6})
        f = BatchFeeder(seq, 1, 0, 2)
        losses = []
        if pipelined:
            run_pipelined(eng, tr, f, [0, 1, 2], 96, hp, lambda k, loss, item: losses.append((k, float(loss.item()))))
        else:
            for k in range(3):
                losses.append((k, float(train_on_item(eng, tr, f.load(k), 96, hp).item())))
        torch.cuda.synchronize()
        f.close()
        res.append((losses, eng.params.clone()))
    assert [k for k, _ in res[1][0]] == [0, 1, 2]
    for i, ((_, a), (_, b)) in enumerate(zip(res[0][0], res[1][0])):
        assert abs(a - b) <= (1e-6 if i == 0 else 5e-3) * abs(a), (i, a, b)    # later steps: Adam amplifies the atomic-order noise
    torch.testing.assert_close(res[0][1], res[1][1], rtol=0, atol=7e-4)      # three Adam steps of lr 1e-4
