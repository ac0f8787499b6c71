"""hps['loss'] = 'yolo' end to end, by the recipe of tests/test_three_scale_e2e_gpu.py: four synthetic UCCS images at 96x96 in
one batch, one-batch epochs, FaceDetector.train() with the YOLOv3 detection loss (fv_yolov3_train_step_det) and each box loss;
the loss falls, recall at 0.5 in the epoch line rises, the saved model loads bit for bit and detect() finds the faces.

Epochs: 'l2' keeps that test's 160 (measured: loss 500.3 -> 12.0, mean IoU of the assigned slots 0.995, recall at 0.5 1.0).  'giou'
runs 400: at 160 one run in four found only two of the four faces (loss 492.7 -> 10.4, recall 0.75, mean IoU 0.58 .. 0.66 -- the
gradient of 1 - GIoU does not shrink near the optimum, so with Adam at this step size the boxes keep jittering around their
targets, while optimising the logits directly under the same loss reaches IoU 0.99); at 400 the loss reaches 5.6 and every
measured run found at least three."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPOCHS = {'giou': 400, 'l2': 160}


def _conf(root, mode, loss, epochs, batch=4):
    return {'mode': mode, 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-3, 'beta_1': 0.9, 'beta_2': 0.999, 'decay': 0.03, 'epochs': epochs, 'step': 1, 'batch_size': batch,
                    'face_conf_th': 0.5, 'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'log_every': 5, 'loss': loss},
            'nn_arch': {'image_size': 96, 'bb_info_c_size': 6, 'head': 'three_scale', 'num_classes': 1}}


@pytest.mark.parametrize('box_loss', ['giou', 'l2'])
def test_three_scale_trains_with_the_yolo_loss_then_detects(tmp_path, monkeypatch, capsys, box_loss):
    import torch
    from face_vijnana_yolov3_amd import data
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    from face_vijnana_yolov3_amd.postproc import letterbox_device
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / 'train'); os.makedirs(root)
    rng = np.random.default_rng(5)
    from PIL import Image
    import pandas as pd
    rows = []
    for k in range(4):
        h, w = [(240, 320), (320, 240), (300, 300), (200, 360)][k]
        img = rng.integers(0, 64, (h, w, 3), dtype=np.uint8)
        fw, fh = int(w * 0.3), int(h * 0.45)
        fx, fy = int(rng.integers(10, w - fw - 10)), int(rng.integers(10, h - fh - 10))
        img[fy:fy + fh, fx:fx + fw] = rng.integers(160, 256, (fh, fw, 3), dtype=np.uint8)       # a bright "face"
        name = 'img_%d.jpg' % k
        Image.fromarray(img).save(os.path.join(root, name), quality=95)
        rows.append([k, name, 1, float(fx), float(fy), float(fw), float(fh)])
    pd.DataFrame(rows, columns=data.CSV_COLUMNS).to_csv(os.path.join(root, 'training.csv'), index=False)
    loss_conf = 'yolo' if box_loss == 'giou' else {'yolo': {'box_loss': box_loss}}          # 'giou' is the default
    epochs = EPOCHS[box_loss]
    fd = FaceDetector(_conf(root, 'train', loss_conf, epochs))
    assert fd.three_scale and fd.model.det_loss['box_loss'] == box_loss and fd.model.det_loss['max_boxes'] == 256
    losses = []
    orig = fd.model.forward_backward

    def spy(x, t, on_bucket=None):
        out = orig(x, t, on_bucket=on_bucket)
        losses.append(float(out.item()) if len(losses) % 10 == 0 or len(losses) >= epochs - 5 else None)
        return out
    monkeypatch.setattr(fd.model, 'forward_backward', spy)
    fd.train()
    assert fd.model.iterations == epochs and np.isfinite(losses[-1])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('yolo loss')]
    assert len(lines) == epochs
    field = lambda l, name: float(re.search(re.escape(name) + r': ([-0-9.einf]+)', l).group(1))
    recall = [field(l, 'recall@0.5') for l in lines]
    total = [sum(field(l, k) for k in ('box', 'obj', 'noobj', 'cls')) for l in lines]
    print('%s: loss %.4f -> %.4f, recall@0.5 %.2f -> %.2f, mean IoU %.3f -> %.3f, ignored %.4f -> %.4f'
          % (box_loss, losses[0], losses[-1], recall[0], recall[-1], field(lines[0], 'mean IoU'), field(lines[-1], 'mean IoU'),
             field(lines[0], 'ignored'), field(lines[-1], 'ignored')))
    assert abs(total[0] - losses[0]) <= 1e-3 * abs(losses[0]) + 1e-3               # the four parts of the line are the loss
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert recall[-1] > recall[0], (recall[0], recall[-1])
    assert os.path.exists(FaceDetector.MODEL_PATH)
    conf2 = _conf(root, 'test', loss_conf, epochs); conf2['model_loading'] = True
    fd2 = FaceDetector(conf2)
    assert torch.equal(fd2.model.params, fd.model.params) and torch.equal(fd2.model.state, fd.model.state)
    hits = 0
    for k, r in enumerate(rows):
        raw = data._pil_loader(os.path.join(root, r[1]))
        x, geom = letterbox_device(fd2.model.ctx, raw, 96)
        boxes = fd2.detect(x[None])
        h, w = raw.shape[:2]
        m = max(h, w)
        _, _, pad_t, _, pad_l, _ = data.letterbox_geometry(h, w, 96)
        ox, oy = (0, pad_t) if w >= h else (pad_l, 0)
        gx1, gy1 = r[3] / m * 96 + ox, r[4] / m * 96 + oy
        gx2, gy2 = (r[3] + r[5]) / m * 96 + ox, (r[4] + r[6]) / m * 96 + oy
        for b in boxes:
            ix = max(0.0, min(b.xmax, gx2) - max(b.xmin, gx1)) * max(0.0, min(b.ymax, gy2) - max(b.ymin, gy1))
            un = (b.xmax - b.xmin) * (b.ymax - b.ymin) + (gx2 - gx1) * (gy2 - gy1) - ix
            if un > 0 and ix / un >= 0.5 and b.get_score() >= 0.5:
                hits += 1
                break
    print('%s: detect() found %d of 4 faces after %d epochs' % (box_loss, hits, epochs))
    assert hits >= 3, hits
