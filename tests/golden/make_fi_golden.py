#!/opt/conda/bin/python3.9
"""Mint golden vectors for face identification by RUNNING the reference's own functions (build container only):

    /opt/conda/bin/python3.9 tests/golden/make_fi_golden.py      # the interpreter that has h5py / scipy, which the modules import

Third-party packages that are not installed here (keras, cv2, skimage, matplotlib, ipyparallel) are stand-in modules, as in
make_golden.py.  Nothing of the reference is altered or copied; only the inputs and outputs below are written.

tests/golden/fi_test.npz -- FaceIdentifier.test() (fi.py:994-1153) on an instance made with object.__new__:
  * imread returns synthetic float64 frames whose pixels hold (row, column, frame index), so every crop the reference cuts
    tells where it came from; cv.resize / cv.copyMakeBorder are shape-only numpy stand-ins;
  * fd.detect returns preset boxes in network coordinates (int corners, as decode_netout's int() leaves them);
  * fid_extractor.predict returns a registered ID plus delta along one axis, delta a function of the crop: distances are
    exactly 0.125, 0.25 (= sim_th: kept), 0.375, 0.5 or 1.0, exact in fp32 and fp64, every other distance far away.
  Recorded: the frames processed (in the reference's order), their boxes, each crop the reference passed to predict (frame,
  y0, x0, rows, cols) with the ID it got, the registry and the csv text.  Cases: boxes on the top and left edges (empty crops),
  a frame with more than 60 passing boxes, frames of several aspect ratios.

tests/golden/cal_acc_fi.npz -- evaluate.cal_acc_fi (evaluate.py:225-329) on synthetic gt / solution csvs with unknown subjects
(-1), wrong ids, images without detections, a detection on an image outside the ground truth and IoU ties (a gt overlapped
equally by two detections; two gts overlapping one detection equally), at every threshold of np.arange(0.5, 1.0, 0.05).
"""
import io
import os
import pickle
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src/space'
S = 416
SIM_TH = 0.25


class _Any:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Any()

    def __getattr__(self, n):
        return _Any()


def _install_stubs():
    names = ['keras', 'keras.layers', 'keras.layers.merge', 'keras.models', 'keras.utils', 'keras.utils.data_utils',
             'keras.optimizers', 'keras.backend', 'keras.engine', 'keras.engine.input_layer', 'skimage', 'skimage.io',
             'skimage.transform', 'skimage.draw', 'cv2', 'matplotlib', 'matplotlib.pyplot', 'ipyparallel']
    for n in names:
        sys.modules[n] = types.ModuleType(n)
    for n in ['Conv2D', 'Input', 'BatchNormalization', 'LeakyReLU', 'ZeroPadding2D', 'UpSampling2D', 'Lambda', 'Concatenate',
              'Dense', 'Flatten', 'Reshape', 'ReLU', 'Conv2DTranspose']:
        setattr(sys.modules['keras.layers'], n, _Any)
    for n in ('add', 'concatenate', 'subtract'):
        setattr(sys.modules['keras.layers.merge'], n, _Any)
    sys.modules['keras.models'].Model = _Any
    sys.modules['keras.models'].load_model = _Any
    sys.modules['keras.utils'].multi_gpu_model = _Any
    sys.modules['keras'].optimizers = _Any()
    sys.modules['keras'].backend = _Any()
    sys.modules['keras.engine.input_layer'].InputLayer = _Any
    sys.modules['keras.utils.data_utils'].Sequence = type('Sequence', (), {})
    for n in ('imread', 'imsave'):
        setattr(sys.modules['skimage.io'], n, None)
    sys.modules['skimage.transform'].resize = None
    sys.modules['skimage.draw'].polygon_perimeter = None
    sys.modules['skimage.draw'].set_color = None
    cv = sys.modules['cv2']
    cv.INTER_CUBIC, cv.BORDER_CONSTANT = 2, 0


# --------------------------------------------------------------------------- FaceIdentifier.test()
FRAMES = [('f0_wide.jpg', 90, 160), ('f1_tall.jpg', 120, 80), ('f2_square.jpg', 100, 100), ('f3_many.jpg', 75, 200),
          ('f4_none.jpg', 64, 96)]
SUBJECTS = [3, 7, 11, 12, 20, 31]
DELTAS = [0.125, 0.25, 0.375, 0.5, 1.0, 0.125, 0.125]


def registry():
    reg = np.zeros((len(SUBJECTS), 64), np.float32)
    for k in range(len(SUBJECTS)):
        reg[k, (5 * k) % 64] = 2.0 + k
        reg[k, (5 * k + 1) % 64] = -1.5
    return reg


def stub_id(frame, y0, x0, h, w):
    """The facial ID the predict stand-in returns for a crop: a registered ID plus DELTAS[...] along one axis."""
    reg = registry()
    k = (3 * y0 + 5 * x0 + h + 2 * w + frame) % len(SUBJECTS)
    delta = DELTAS[(y0 + 2 * x0 + 3 * h + w + frame) % len(DELTAS)]
    v = reg[k].copy()
    v[(y0 + x0 + 7) % 64] += np.float32(delta)
    return v


def frame_boxes(fi, h, w, rng):
    """Boxes in network coordinates (xmin, ymin, xmax, ymax), score; some on the top / left edge of the letterboxed image."""
    if w >= h:
        h_p = int(h / w * S); pad_t = (S - h_p) // 2; pad_l = 0; w_p = S
    else:
        w_p = int(w / h * S); pad_l = (S - w_p) // 2; pad_t = 0; h_p = S
    n = {0: 9, 1: 8, 2: 7, 3: 130, 4: 0}[fi]
    out = []
    for b in range(n):
        bw, bh = int(rng.integers(12, 120)), int(rng.integers(12, 120))
        x0 = int(rng.integers(pad_l, pad_l + w_p - 8)); y0 = int(rng.integers(pad_t, pad_t + h_p - 8))
        if b == 0:
            y0 = pad_t            # projects to ymin = 0: t - 1 = -1, an empty crop
        if b == 1:
            x0 = pad_l            # left edge
        if b == 2:
            y0 = max(pad_t - 5, 0)    # inside the padding: clamped to 0 as well
        out.append((x0, y0, min(x0 + bw, S), min(y0 + bh, S), float(rng.uniform(0.5, 1.0))))
    return out


def mint_test(ref_fi, ref_yd):
    rng = np.random.default_rng(5)
    cv = sys.modules['cv2']
    state = {'last_resize': None, 'file': None}
    crops, ids, order = [], [], []
    boxes_of = {}
    for fi_, (name, h, w) in enumerate(FRAMES):
        boxes_of[name] = frame_boxes(fi_, h, w, rng)

    def imread(path):
        name = os.path.basename(path)
        fi_ = [f[0] for f in FRAMES].index(name)
        _, h, w = FRAMES[fi_]
        img = np.zeros((h, w, 3), np.float64)
        img[..., 0] = np.arange(h)[:, None]; img[..., 1] = np.arange(w)[None, :]; img[..., 2] = fi_
        state['file'] = name
        order.append(name)
        return img

    def resize(img, size, interpolation=None):
        state['last_resize'] = img
        return np.zeros((size[1], size[0]) + img.shape[2:], np.float64)

    def copyMakeBorder(img, t, b, l, r, border, value=None):
        return np.pad(img, ((t, b), (l, r), (0, 0)))

    cv.resize, cv.copyMakeBorder = resize, copyMakeBorder
    ref_fi.imread = imread
    ref_fi.cv = cv

    class FD:
        def detect(self, image):
            assert image.shape == (1, S, S, 3)
            return [ref_yd.BoundBox(b[0], b[1], b[2], b[3], objness=b[4], classes=[np.float32(b[4])])
                    for b in boxes_of[state['file']]]

    class Extractor:
        def predict(self, x):
            assert x.shape[0] == 1
            c = state['last_resize']
            frame, y0, x0 = int(round(c[0, 0, 2] * 255)), int(round(c[0, 0, 0] * 255)), int(round(c[0, 0, 1] * 255))
            rec = (frame, y0, x0, c.shape[0], c.shape[1])
            crops.append(rec)
            v = stub_id(*rec)
            ids.append(v)
            return v[np.newaxis]

    obj = object.__new__(ref_fi.FaceIdentifier)
    reg = registry()
    with tempfile.TemporaryDirectory() as tmp:
        for name, h, w in FRAMES:
            open(os.path.join(tmp, name), 'wb').close()
        obj.conf = {'test_path': tmp, 'output_file_path': os.path.join(tmp, 'solution_fi.csv')}
        obj.nn_arch = {'image_size': S}
        obj.hps = {'sim_th': SIM_TH}
        obj.fd = FD()
        obj.fid_extractor = Extractor()
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            with open('ref_facial_id_db.pickle', 'wb') as f:
                pickle.dump({s: reg[k] for k, s in enumerate(SUBJECTS)}, f)
            ref_fi.DEBUG = False
            obj.test()
            csv = open(obj.conf['output_file_path']).read()
        finally:
            os.chdir(cwd)
    out = {'image_size': np.int64(S), 'sim_th': np.float64(SIM_TH), 'subjects': np.asarray(SUBJECTS, np.int64), 'registry': reg,
           'order': np.asarray(order), 'frame_names': np.asarray([f[0] for f in FRAMES]),
           'frame_hw': np.asarray([(f[1], f[2]) for f in FRAMES], np.int64),
           'crops': np.asarray(crops, np.int64).reshape(-1, 5), 'crop_ids': np.asarray(ids, np.float32).reshape(-1, 64),
           'csv': np.frombuffer(csv.encode(), np.uint8)}
    for name, _, _ in FRAMES:
        b = np.asarray(boxes_of[name], np.float64).reshape(-1, 5)
        out['boxes_' + name] = b[:, :4].astype(np.int64)
        out['scores_' + name] = b[:, 4]
    rows = csv.count('\n')
    per = {n: csv.count(n + ',') for n, _, _ in FRAMES}
    print('test(): %d crops predicted, %d rows %r' % (len(crops), rows, per))
    assert per['f3_many.jpg'] == 60, 'the many-box frame must hit the 60-row limit'
    assert any(',' in l and l for l in csv.splitlines())
    return out


# --------------------------------------------------------------------------- cal_acc_fi
def acc_case(seed, n_img):
    rng = np.random.default_rng(seed)
    gt = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    sol = []
    fid = 0
    for k in range(n_img):
        name = 'img_%03d.jpg' % k
        kind = ['match', 'match', 'none', 'far', 'tie_det', 'tie_gt'][k % 6] if seed == 0 else \
            rng.choice(['match', 'match', 'match', 'none', 'far'])
        if kind == 'tie_det':       # one gt, two identical detections (equal IoU), different ids
            sid = int(rng.integers(1, 9))
            gt.append('%d,%s,%d,100,100,50,50' % (fid, name, sid)); fid += 1
            sol.append('%s,%d,105,100,50,50,0.9' % (name, sid))
            sol.append('%s,%d,105,100,50,50,0.8' % (name, sid + 1))
            continue
        if kind == 'tie_gt':        # two gts overlapped equally by one detection
            gt.append('%d,%s,%d,100,100,40,40' % (fid, name, 4)); fid += 1
            gt.append('%d,%s,%d,160,100,40,40' % (fid, name, 5)); fid += 1
            sol.append('%s,%d,130,100,40,40,0.7' % (name, 5))
            continue
        for f in range(int(rng.integers(1, 5))):
            x, y = rng.uniform(1, 700, 2); w, h = rng.uniform(24, 140, 2)
            sid = int(rng.choice([-1, -1, 1, 2, 3, 4, 5, 6]))
            gt.append('%d,%s,%d,%.1f,%.1f,%.1f,%.1f' % (fid, name, sid, x, y, w, h)); fid += 1
            if kind == 'match' and rng.random() < 0.85:
                j = rng.normal(0, 0.15, 4) * np.array([w, h, w, h])
                did = sid if rng.random() < 0.6 else int(rng.choice([-1, 1, 2, 3, 7]))
                sol.append('%s,%d,%r,%r,%r,%r,%r' % (name, did, float(x + j[0]), float(y + j[1]), float(max(w + j[2], 4)),
                                                    float(max(h + j[3], 4)), float(rng.uniform(0.3, 1.0))))
        if kind == 'match':
            for _ in range(int(rng.integers(0, 3))):
                sol.append('%s,%d,%r,%r,%r,%r,%r' % (name, int(rng.choice([-1, 2, 9])), float(rng.uniform(1, 800)),
                                                    float(rng.uniform(1, 800)), float(rng.uniform(10, 90)),
                                                    float(rng.uniform(10, 90)), float(rng.uniform(0.05, 0.9))))
        elif kind == 'far':
            sol.append('%s,%d,%r,5000.0,12.0,12.0,%r' % (name, int(rng.choice([-1, 3])), 5000.0 + float(rng.uniform(0, 9)),
                                                      float(rng.uniform(0.5, 0.99))))
    sol.append('zz_not_in_gt.jpg,3,1.0,1.0,10.0,10.0,0.987654')
    return '\n'.join(gt) + '\n', '\n'.join(sol) + '\n'


def mint_acc(ref_ev):
    out = {}
    ths = np.arange(0.5, 1.0, 0.05)
    cases = [(0, 12), (1, 30), (2, 60)]
    with tempfile.TemporaryDirectory() as tmp:
        for ci, (seed, n_img) in enumerate(cases):
            gt, sol = acc_case(seed, n_img)
            gp, sp = os.path.join(tmp, 'gt.csv'), os.path.join(tmp, 'sol.csv')
            open(gp, 'w').write(gt); open(sp, 'w').write(sol)
            out['case%d_gt' % ci] = np.frombuffer(gt.encode(), np.uint8)
            out['case%d_sol' % ci] = np.frombuffer(sol.encode(), np.uint8)
            res = []
            for th in ths:
                so = sys.stdout
                sys.stdout = io.StringIO()           # the function prints its progress
                try:
                    res.append(ref_ev.cal_acc_fi(gp, sp, th))
                finally:
                    sys.stdout = so
            out['case%d_counts' % ci] = np.asarray([r[:4] for r in res], np.int64)
            out['case%d_acc' % ci] = np.asarray([r[4] for r in res], np.float64)
            print('cal_acc_fi case %d: %r' % (ci, [tuple(int(v) for v in r[:4]) for r in res[:2]]))
    out['thresholds'] = ths
    out['ncases'] = np.int64(len(cases))
    return out


def main():
    _install_stubs()
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    warnings.simplefilter('ignore')
    import evaluate as ref_ev
    import face_identification as ref_fi
    import yolov3_detect as ref_yd
    np.savez_compressed(os.path.join(HERE, 'fi_test.npz'), **mint_test(ref_fi, ref_yd))
    np.savez_compressed(os.path.join(HERE, 'cal_acc_fi.npz'), **mint_acc(ref_ev))
    print('wrote fi_test.npz, cal_acc_fi.npz')


if __name__ == '__main__':
    main()
