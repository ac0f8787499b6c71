"""hps['validate'] without a GPU: data.validate_conf, the refusal on more than one rank, and the numpy restatement of the three
device calls (tests/det_metric_ref.py) against the host metric of evaluate.py -- detection_ious / pr_curve exactly, integrate_pr
within the error estimate quad itself returns for the same interpolant plus 1e-9."""
import json
import os

import numpy as np
import pytest

import det_metric_ref as ref


def _conf(root, validate):
    return {'mode': 'train', 'raw_data_path': root, 'test_path': root, 'output_file_path': os.path.join(root, 'solution_fd.csv'),
            'multi_gpu': False, 'num_gpus': 1, 'yolov3_base_model_load': False, 'model_loading': False,
            'hps': {'lr': 1e-4, 'beta_1': 0.99, 'beta_2': 0.99, 'decay': 0.0, 'epochs': 1, 'step': 1, 'batch_size': 2,
                    'face_conf_th': 0.5, 'nms_iou_th': 0.5, 'num_cands': 60, 'face_region_ratio_th': 0.8, 'validate': validate},
            'nn_arch': {'image_size': 96, 'bb_info_c_size': 6}}


def test_validate_conf_defaults():
    from face_vijnana_yolov3_amd.data import validate_conf
    assert validate_conf(None) is None and validate_conf(False) is None
    c = validate_conf(True, 'some/dir')
    assert c['path'] == 'some/dir' and c['every'] == 1 and c['save_best'] is False
    assert c['iou_ths'] == [float(t) for t in np.arange(0.5, 1.0, 0.05)] and len(c['iou_ths']) == 10
    c = validate_conf({'path': 'held_out', 'every': 3, 'iou_ths': [0.5, 1], 'save_best': True}, 'some/dir')
    assert c == {'path': 'held_out', 'every': 3, 'iou_ths': [0.5, 1.0], 'save_best': True}
    assert validate_conf({'iou_ths': [0.05 * k for k in range(1, 17)]}, 'd')['iou_ths'][-1] == 0.05 * 16


@pytest.mark.parametrize('bad', [
    3, 'yes', [], {'evry': 1}, {'path': 7}, {'path': ''}, {'every': 0}, {'every': 1.5}, {'every': True}, {'save_best': 1},
    {'iou_ths': []}, {'iou_ths': 0.5}, {'iou_ths': [0.0, 0.5]}, {'iou_ths': [0.5, 1.01]}, {'iou_ths': [0.6, 0.5]},
    {'iou_ths': [0.5, 0.5]}, {'iou_ths': [0.5, 'x']}, {'iou_ths': [float('nan')]}, {'iou_ths': [k / 20 for k in range(1, 18)]}])
def test_validate_conf_refuses(bad):
    from face_vijnana_yolov3_amd.data import validate_conf
    with pytest.raises(ValueError, match='validate'):
        validate_conf(bad, 'some/dir')


def test_validate_conf_needs_a_path():
    from face_vijnana_yolov3_amd.data import validate_conf
    with pytest.raises(ValueError, match='validate.path'):
        validate_conf(True, None)


def test_face_detector_refuses_a_bad_validate_before_a_device(tmp_path):
    """The ValueError comes from the constructor, ahead of the Engine (which raises FvError on a machine without a GPU)."""
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    with pytest.raises(ValueError, match='validate'):
        FaceDetector(_conf(str(tmp_path), {'every': 0}))
    with pytest.raises(ValueError, match='validate'):
        FaceDetector(_conf(str(tmp_path), {'unknown': 1}))


def test_validate_refused_on_ranks_before_a_rank_is_started(tmp_path, monkeypatch):
    from face_vijnana_yolov3_amd import data, face_detection, parallel
    conf = _conf(str(tmp_path), True)
    conf['multi_gpu'] = True; conf['num_gpus'] = 2
    monkeypatch.chdir(tmp_path)
    json.dump({'fd_conf': conf, 'fi_conf': {}}, open('face_vijnana_yolov3.json', 'w'))
    started = []
    monkeypatch.setattr(parallel, 'launch_ranks', lambda *a, **k: started.append(a) or 0)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(NotImplementedError, match='validate'):
        face_detection.main()
    assert not started
    data.refuse_validate_on_ranks({'validate': True}, 1)                  # one rank: served
    data.refuse_validate_on_ranks({}, 2); data.refuse_validate_on_ranks({'validate': False}, 2)
    with pytest.raises(NotImplementedError):
        data.refuse_validate_on_ranks({'validate': {'every': 2}}, 2)


def test_validate_line_leaves_out_absent_thresholds():
    from face_vijnana_yolov3_amd.data import validate_line
    res = dict(iou_ths=[0.5, 0.75], ap=[0.5, 0.25], mean_ap=0.375, n_det=7, n_images=3, n_gt=5)
    assert validate_line(res) == 'val - AP50 0.5000 AP75 0.2500 mAP 0.3750 (7 detections on 3 images, 5 faces)'
    res = dict(iou_ths=[0.6], ap=[0.5], mean_ap=0.5, n_det=1, n_images=1, n_gt=1)
    assert validate_line(res) == 'val - mAP 0.5000 (1 detections on 1 images, 1 faces)'


# ----------------------------------------------------------------------------- the numpy restatement against evaluate.py
def _check_pair(gt, sol, ths, want=None):
    """The restatement over two csv files: conf / IoU lists equal to detection_ious', curves equal to pr_curve's (and the golden's),
    trapezoid AP within quad's own error estimate + 1e-9 of integrate_pr.  -> the largest |trapezoid - quad| seen."""
    import pandas as pd
    from face_vijnana_yolov3_amd import evaluate as ev
    rows, nrows, g, off, gt_count = ref.frames_from_csv(gt, sol)
    iou, flag = ref.match_rows(rows, nrows, g, off)
    conf, ious = ref.compact(rows, nrows, iou, flag)
    hconf, hious = ev.detection_ious(pd.read_csv(gt), pd.read_csv(sol, header=None))
    assert np.array_equal(conf, hconf) and np.array_equal(ious, hious)
    order, counts, ap, prec, rec = ref.ap_sweep(conf, ious, ths, gt_count)
    worst = 0.0
    for t, th in enumerate(ths):
        ps, rs = ev.pr_curve(hconf, hious, gt_count, th)
        assert np.array_equal(counts[t] / np.arange(1, len(conf) + 1), ps) and np.array_equal(counts[t] / float(gt_count), rs)
        if want is not None:
            assert np.array_equal(ps, want[th][0]) and np.array_equal(rs, want[th][1])
        q, err = ref.quad_with_error(ps, rs)
        assert q == ev.integrate_pr(ps, rs)
        assert abs(ap[t] - q) <= err + 1e-9, (th, ap[t], q, err)
        if want is not None:
            assert abs(ap[t] - want[th][2]) <= err + 1e-9
        assert prec[t] == ps[-1] and rec[t] == rs[-1]
        worst = max(worst, abs(ap[t] - q))
    return worst


def test_reference_helper_on_the_golden_cases(tmp_path):
    cases = list(ref.golden_cases(tmp_path))
    assert len(cases) == 4
    worst = max(_check_pair(gt, sol, ths, want) for _ci, gt, sol, ths, want in cases)
    print('largest |trapezoid - quad| on the golden cases: %.3e' % worst)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_helper_on_the_loop_oracle_generator(tmp_path, seed):
    gt, sol = ref.write_csv_pair(str(tmp_path), *ref.loop_oracle_rows(seed))
    worst = _check_pair(gt, sol, [float(t) for t in np.arange(0.5, 1.0, 0.05)])
    print('largest |trapezoid - quad|, seed %d: %.3e' % (seed, worst))


def test_reference_rows_are_what_write_rows_writes():
    """rows_from_nms restates _project_back + _write_rows: float(str(v)) of every csv field is the value itself."""
    import io
    from face_vijnana_yolov3_amd.face_detection import FaceDetector
    from face_vijnana_yolov3_amd.postproc import BoundBox
    rng = np.random.default_rng(3)
    S = 96
    geoms = [(480, 640, 12, 12, 0, 0), (640, 480, 0, 0, 12, 12), (416, 416, 0, 0, 0, 0)]
    for h, w, pt, pb, pl, pr in geoms:
        b = np.sort(rng.integers(0, S, (5, 2, 2)), axis=1).reshape(5, 4)[:, (0, 2, 1, 3)]
        score = rng.uniform(0.1, 1.0, 5).astype(np.float32)
        rows, nrows = ref.rows_from_nms(b[None], score[None], np.array([5]), np.array([[h, w, pt, pb, pl, pr]]), S)
        fd = FaceDetector.__new__(FaceDetector)
        fd.image_size = S
        boxes = [BoundBox(np.int64(r[0]), np.int64(r[1]), np.int64(r[2]), np.int64(r[3]), objness=1.0, classes=[s]) for r, s in zip(b, score)]
        fd._project_back(boxes, (h, w, pt, pb, pl, pr))
        f = io.StringIO()
        FaceDetector._write_rows(f, 'a.jpg', boxes)
        got = np.array([[float(v) for v in line.split(',')[1:]] for line in f.getvalue().splitlines()])
        assert nrows[0] == 5 and np.array_equal(got, rows[0, :5])


def test_reference_match_edge_cases():
    # touching boxes: negative "overlap" product of two negative extents is positive in the reference's arithmetic only when both
    # axes touch; one touching axis gives 0 -> no pair
    out, flag = ref.match_image([[0, 0, 10, 10]], [[10, 0, 10, 10]])
    assert flag == 0 and out[0] == -1.0
    # zero-area pair: 0 / 0 = nan is never > 0
    out, flag = ref.match_image([[5, 5, 0, 0]], [[5, 5, 0, 0]])
    assert flag == 0 and out[0] == -1.0
    # ties: duplicated boxes go to the smaller ground-truth index, then the smaller detection
    out, flag = ref.match_image([[0, 0, 10, 10], [0, 0, 10, 10]], [[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]])
    assert flag == 1 and list(out) == [1.0, 1.0, -1.0]
