#!/opt/conda/bin/python3.9
"""Mint the golden of the FaceIdentifier data mode by RUNNING the reference's own create_db_fi / save_extracted_face
(fi.py:78-280) for both resource types (build container only):

    /opt/conda/bin/python3.9 tests/golden/make_data_golden.py

Third-party packages that are not installed (keras, cv2, skimage, matplotlib, ipyparallel) are the stand-in modules of
make_fi_golden.py.  Nothing of the reference is copied; only the inputs and outputs below are written.

tests/golden/create_db_fi.npz
  * imread returns int64 frames whose pixels hold (row, column, frame index), so every cut tells where it came from;
  * cv.resize / cv.copyMakeBorder are recording stand-ins: the crop's origin and shape, the requested (w_p, h_p), the four pads;
  * imsave records the directory, the name and the shape; ipp.Client()[:] is a serial stand-in (push sets the module's globals,
    sync_imports does nothing, map_sync is list(map(...)));
  * recorded per resource type: the input csv text, the frames (name, rows, columns), the db csv text as to_csv() wrote it, the
    saved names in order and per crop (frame, y0, x0, h, w, w_p, h_p, pad_t, pad_b, pad_l, pad_r).

One thing about the UCCS branch.  create_db_fi binds np, pd, cv, imread and imsave as FUNCTION-LOCAL names (the import statements
under `with pView.sync_imports():` in its VGGFace2 branch), so in the UCCS branch `pd.read_csv` is an unbound local: as written
that branch raises UnboundLocalError under every Python 3.  The minter asserts exactly that, then runs the function's own text
(inspect.getsource, at run time, nothing stored) with the four import statements that bind them turned into `pass`, in the reference module's own
namespace -- the statements that do the work are the reference's, unaltered.  The VGGFace2 branch runs as it is.

Cases (each asserted below to occur): subject -1; a row with a zero field; fractional FACE_X / FACE_Y (int() matters); boxes
running past the right and the bottom edge (the slice clips, so the db's w, h differ from the csv's); wide, tall and square
crops; odd padding; subjects out of order in the csv (groupby walks them sorted); a frame cut several times; VGGFace2 rows with
negative x, with w == 0, and more than one skipped row (res.remove(None) removes one at most; pd.concat drops the rest); VGGFace2
boxes clipped by the image.  Rows on which the reference itself raises (an empty cut: 0 / 0) are not among the inputs."""
import inspect
import os
import re
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = '/root/reference/src/space'
S = 416

UCCS_FRAMES = [('frame_a.jpg', 300, 400), ('frame_b.jpg', 500, 350), ('frame_c.jpg', 240, 240)]
#               FACE_ID, FILE, SUBJECT_ID, FACE_X, FACE_Y, FACE_WIDTH, FACE_HEIGHT
UCCS_ROWS = [
    (0, 'frame_a.jpg', 12, 10.7, 20.3, 91.0, 62.0),      # fractional corner; wide, odd padding
    (1, 'frame_a.jpg', -1, 50.0, 60.0, 40.0, 40.0),      # unknown subject: skipped
    (2, 'frame_b.jpg', 3, 100.0, 120.0, 51.0, 121.0),    # tall
    (3, 'frame_a.jpg', 3, 380.0, 100.0, 60.0, 30.0),     # past the right edge: clipped to 21 columns
    (4, 'frame_b.jpg', 7, 30.0, 470.0, 45.0, 70.0),      # past the bottom edge
    (5, 'frame_c.jpg', 7, 41.0, 41.0, 81.0, 81.0),       # square
    (6, 'frame_c.jpg', 12, 5.0, 5.0, 0.0, 50.0),         # zero width: skipped
    (7, 'frame_c.jpg', 12, 1.0, 1.0, 239.0, 239.0),      # l - 1 == 0: starts at the first pixel
    (8, 'frame_b.jpg', 12, 200.6, 300.9, 33.5, 77.25),   # all four fractional; tall, odd padding
    (9, 'frame_a.jpg', 5, 120.0, 40.0, 64.0, 0.0),       # zero height: skipped, and subject 5 ends with no row at all
    (10, 'frame_a.jpg', 3, 2.0, 2.0, 397.0, 297.0),      # nearly the whole frame
    (11, 'frame_b.jpg', 7, 300.0, 450.0, 120.0, 120.0),  # past both edges
    (12, 'frame_c.jpg', -1, 0.0, 10.0, 20.0, 20.0),      # unknown subject AND a zero field
]

VGG_FRAMES = [('n000002/0001_01', 200, 180), ('n000002/0002_01', 150, 260), ('n000009/0001_02', 120, 120),
              ('n000009/0005_01', 333, 222), ('n000040/0003_03', 90, 400), ('n000040/0010_01', 256, 256)]
#             NAME_ID, X, Y, W, H
VGG_ROWS = [
    ('n000002/0001_01', 20, 30, 100, 141),    # tall, odd padding
    ('n000002/0002_01', -3, 10, 80, 80),      # negative x: skipped
    ('n000002/0002_01', 40, 20, 161, 99),     # wide, odd padding
    ('n000009/0001_02', 10, 10, 0, 50),       # w == 0: skipped
    ('n000009/0001_02', 0, 0, 120, 120),      # the whole image; square
    ('n000009/0005_01', 150, 300, 100, 100),  # clipped right and bottom
    ('n000040/0003_03', 5, -1, 60, 60),       # negative y: skipped
    ('n000040/0003_03', 100, 10, 280, 70),    # wide
    ('n000040/0010_01', 200, 30, 90, 200),    # clipped right
    ('n000040/0010_01', 16, 16, 64, -4),      # h < 0: skipped
]


def uccs_csv():
    out = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    out += ['%d,%s,%d,%r,%r,%r,%r' % r for r in UCCS_ROWS]
    return '\n'.join(out) + '\n'


def vgg_csv():
    return '\n'.join(['NAME_ID,X,Y,W,H'] + ['%s,%d,%d,%d,%d' % r for r in VGG_ROWS]) + '\n'


class Recorder(object):
    """The stand-ins of imread, cv.resize, cv.copyMakeBorder and imsave, and what they saw."""

    def __init__(self, frames, key_of_path):
        self.frames = frames
        self.key_of_path = key_of_path
        self.crops, self.saved, self.read = [], [], []
        self._cut = None

    def imread(self, path):
        key = self.key_of_path(path)
        fi = [f[0] for f in self.frames].index(key)
        _, h, w = self.frames[fi]
        img = np.zeros((h, w, 3), np.int64)
        img[..., 0] = np.arange(h)[:, None]; img[..., 1] = np.arange(w)[None, :]; img[..., 2] = fi
        self.read.append(key)
        return img

    def resize(self, img, size, interpolation=None):
        assert interpolation == 'INTER_NEAREST', interpolation
        assert img.ndim == 3 and img.shape[0] >= 1 and img.shape[1] >= 1, 'an empty cut: not a golden input'
        assert size[0] >= 1 and size[1] >= 1, 'cv.resize would raise: not a golden input'
        self._cut = (int(img[0, 0, 2]), int(img[0, 0, 0]), int(img[0, 0, 1]), img.shape[0], img.shape[1], int(size[0]), int(size[1]))
        return np.zeros((size[1], size[0], 3), np.int64)

    def copyMakeBorder(self, img, t, b, l, r, border, value=None):
        assert border == 'BORDER_CONSTANT' and list(value) == [0, 0, 0]
        self.crops.append(self._cut + (int(t), int(b), int(l), int(r)))
        self._cut = None
        return np.pad(img, ((t, b), (l, r), (0, 0)))

    def imsave(self, path, arr):
        assert arr.shape == (S, S, 3) and arr.dtype == np.uint8, (arr.shape, arr.dtype)
        self.saved.append((os.path.basename(os.path.dirname(path)), os.path.basename(path)))

    def install(self, ref_fi, cv):
        cv.resize, cv.copyMakeBorder = self.resize, self.copyMakeBorder
        cv.INTER_NEAREST, cv.BORDER_CONSTANT = 'INTER_NEAREST', 'BORDER_CONSTANT'
        ref_fi.cv = ref_fi.cv2 = cv
        ref_fi.imread, ref_fi.imsave = self.imread, self.imsave
        sys.modules['skimage.io'].imread, sys.modules['skimage.io'].imsave = self.imread, self.imsave


class _SyncImports(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class SerialView(object):
    """ipp.Client() and its [:] view, run serially in this process."""

    def __init__(self, module):
        self.module = module

    def push(self, names):
        for k, v in names.items():
            setattr(self.module, k, v)

    def sync_imports(self):
        return _SyncImports()

    def map_sync(self, fn, items):
        return list(map(fn, items))

    def __getitem__(self, _all):
        return self


def uccs_function(ref_fi):
    """create_db_fi with its function-local imports turned into `pass` (see the module docstring)."""
    src = inspect.getsource(ref_fi.create_db_fi)
    lines, dropped = [], 0
    for line in src.splitlines():
        m = re.match(r'^(\s+)(import \w+ as \w+|from skimage\.io import imread, imsave)\s*$', line)
        if m:
            line = m.group(1) + 'pass'; dropped += 1
        lines.append(line)
    assert dropped == 4, dropped            # numpy, pandas, cv2, skimage.io
    ns = ref_fi.__dict__
    exec(compile('\n'.join(lines).replace('def create_db_fi(', 'def _create_db_fi_uccs(', 1), ref_fi.__file__, 'exec'), ns)
    return ns['_create_db_fi_uccs']


def run(fn, conf, tmp, db_name):
    cwd = os.getcwd()
    os.chdir(tmp)
    so = sys.stdout
    sys.stdout = open(os.devnull, 'w')       # 'Save <name>' per crop
    try:
        fn(conf)
    finally:
        sys.stdout.close()
        sys.stdout = so
        os.chdir(cwd)
    return open(os.path.join(tmp, db_name)).read()


def pack(prefix, csv_in, frames, rec, db_csv):
    return {prefix + '_csv_in': np.frombuffer(csv_in.encode(), np.uint8), prefix + '_frames': np.asarray([f[0] for f in frames]),
            prefix + '_frame_hw': np.asarray([(f[1], f[2]) for f in frames], np.int64),
            prefix + '_crops': np.asarray(rec.crops, np.int64).reshape(-1, 11),
            prefix + '_saved': np.asarray([s[1] for s in rec.saved]), prefix + '_dir': np.asarray(sorted(set(s[0] for s in rec.saved))),
            prefix + '_db_csv': np.frombuffer(db_csv.encode(), np.uint8)}


def mint_uccs(ref_fi, cv):
    rec = Recorder(UCCS_FRAMES, os.path.basename)
    rec.install(ref_fi, cv)
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, 'raw')
        os.makedirs(os.path.join(raw, 'training'))
        os.makedirs(os.path.join(raw, 'subject_faces', 'stale'))          # must be emptied
        open(os.path.join(raw, 'training', 'training.csv'), 'w').write(uccs_csv())
        conf = {'fi_conf': {'resource_type': 'uccs', 'raw_data_path': raw, 'nn_arch': {'image_size': S}}}
        try:
            run(ref_fi.create_db_fi, conf, tmp, 'subject_image_db.csv')
            raise AssertionError('the reference\'s UCCS branch ran as written: drop uccs_function()')
        except UnboundLocalError:
            pass
        assert not rec.crops and not rec.saved
        db_csv = run(uccs_function(ref_fi), conf, tmp, 'subject_image_db.csv')
        assert os.listdir(os.path.join(raw, 'subject_faces')) == [], 're-created empty (imsave is a stand-in)'
    c = np.asarray(rec.crops, np.int64)
    rows = {r[0]: r for r in UCCS_ROWS}
    kept = [r for r in UCCS_ROWS if r[2] != -1 and min(r[3:]) > 0]
    assert len(c) == len(kept) == len(rec.saved) == db_csv.count('\n') - 1
    assert any(r[2] == -1 for r in UCCS_ROWS) and any(min(r[3:]) == 0 and r[2] != -1 for r in UCCS_ROWS)
    assert any(r[3] != int(r[3]) for r in kept), 'fractional FACE_X'
    fhw = {i: f[1:] for i, f in enumerate(UCCS_FRAMES)}
    assert any(cc[2] + cc[4] == fhw[cc[0]][1] for cc in c) and any(cc[1] + cc[3] == fhw[cc[0]][0] for cc in c), 'clipped at an edge'
    csv_wh = sorted((int(r[5]), int(r[6])) for r in kept)
    assert sorted((int(cc[4]), int(cc[3])) for cc in c) != csv_wh, 'db w, h differ from the csv\'s'
    assert any(cc[4] > cc[3] for cc in c) and any(cc[4] < cc[3] for cc in c) and any(cc[4] == cc[3] for cc in c), 'wide, tall, square'
    assert any(cc[7] != cc[8] for cc in c) and any(cc[9] != cc[10] for cc in c), 'odd padding, both axes'
    order = [int(l.split(',')[1]) for l in db_csv.splitlines()[1:]]
    assert order == sorted(order) and [r[2] for r in kept] != order, 'walked by sorted subject, unlike the csv'
    assert len(set(cc[0] for cc in c)) < len(c), 'a frame cut more than once'
    print('uccs: %d rows -> %d crops, subjects %r' % (len(UCCS_ROWS), len(c), sorted(set(order))))
    return pack('uccs', uccs_csv(), UCCS_FRAMES, rec, db_csv)


def mint_vgg(ref_fi, cv):
    rec = Recorder(VGG_FRAMES, lambda p: '/'.join(p[:-4].replace('\\', '/').split('/')[-2:]))
    rec.install(ref_fi, cv)
    import pandas
    ref_fi.pandas, ref_fi.numpy = pandas, np
    sys.modules['ipyparallel'].Client = lambda: SerialView(ref_fi)
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, 'raw')
        os.makedirs(os.path.join(raw, 'subject_faces_vggface2', 'stale'))
        open(os.path.join(raw, 'loose_bb_train.csv'), 'w').write(vgg_csv())
        conf = {'fi_conf': {'resource_type': 'vggface2', 'raw_data_path': raw, 'nn_arch': {'image_size': S}}}
        db_csv = run(ref_fi.create_db_fi, conf, tmp, 'subject_image_vggface2_db.csv')
        assert os.listdir(os.path.join(raw, 'subject_faces_vggface2')) == []
    c = np.asarray(rec.crops, np.int64)
    skipped = [r for r in VGG_ROWS if r[1] < 0 or r[2] < 0 or r[3] <= 0 or r[4] <= 0]
    assert len(skipped) > 1 and any(r[1] < 0 for r in skipped) and any(r[3] == 0 for r in skipped)
    assert len(c) == len(VGG_ROWS) - len(skipped) == len(rec.saved) == db_csv.count('\n') - 1
    kept = [r for r in VGG_ROWS if r not in skipped]
    assert [(cc[1], cc[2]) for cc in c] == [(r[2], r[1]) for r in kept], 'row order'
    assert any(cc[4] != r[3] for cc, r in zip(c, kept)) and any(cc[3] != r[4] for cc, r in zip(c, kept)), 'clipped by the image'
    assert any(cc[4] > cc[3] for cc in c) and any(cc[4] < cc[3] for cc in c) and any(cc[4] == cc[3] for cc in c)
    assert any(cc[7] != cc[8] for cc in c) and any(cc[9] != cc[10] for cc in c)
    print('vggface2: %d rows -> %d crops (%d skipped)' % (len(VGG_ROWS), len(c), len(skipped)))
    return pack('vgg', vgg_csv(), VGG_FRAMES, rec, db_csv)


def main():
    from make_fi_golden import _install_stubs
    _install_stubs()
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    warnings.simplefilter('ignore')
    import face_identification as ref_fi
    cv = sys.modules['cv2']
    out = {'image_size': np.int64(S)}
    out.update(mint_uccs(ref_fi, cv))
    out.update(mint_vgg(ref_fi, cv))
    np.savez_compressed(os.path.join(HERE, 'create_db_fi.npz'), **out)
    print('wrote create_db_fi.npz')


if __name__ == '__main__':
    main()
