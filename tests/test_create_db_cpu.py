"""The FaceIdentifier data mode on the host: the record enumerators, the letterbox geometry and the db text against the
reference's own create_db_fi / save_extracted_face (tests/golden/create_db_fi.npz, minted by tests/golden/make_data_golden.py),
the skip rules, the batching by source file and main()'s dispatch."""
import json
import os

import numpy as np
import pytest

from face_vijnana_yolov3_amd import face_identification as fi
from face_vijnana_yolov3_amd.data import letterbox_geometry


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'create_db_fi.npz'))


def _tree(golden, prefix, tmp_path):
    """The golden's input csv at its place under tmp_path -> (raw_data_path, hw_of over the golden's frame table, frame names)."""
    raw = tmp_path / 'raw'
    names = [str(n) for n in golden[prefix + '_frames']]
    hw = {n: tuple(int(v) for v in golden[prefix + '_frame_hw'][i]) for i, n in enumerate(names)}
    text = bytes(golden[prefix + '_csv_in']).decode()
    if prefix == 'uccs':
        os.makedirs(raw / 'training')
        (raw / 'training' / 'training.csv').write_text(text)
        key = os.path.basename
    else:
        os.makedirs(raw)
        (raw / 'loose_bb_train.csv').write_text(text)
        key = lambda p: '/'.join(p[:-4].split(os.sep)[-2:])
    return str(raw), (lambda p: hw[key(p)]), names, key


def _records(golden, prefix, tmp_path):
    raw, hw_of, names, key = _tree(golden, prefix, tmp_path)
    S = int(golden['image_size'])
    fn = fi.uccs_records if prefix == 'uccs' else fi.vggface2_records
    records, skipped = fn(raw, S, hw_of)
    return records, skipped, names, key, raw


@pytest.mark.parametrize('prefix', ['uccs', 'vgg'])
def test_records_reproduce_the_references_crops_names_and_order(golden, prefix, tmp_path):
    records, skipped, names, key, raw = _records(golden, prefix, tmp_path)
    want = golden[prefix + '_crops']
    assert skipped == {'empty': 0, 'side_rounds_to_0': 0}
    assert len(records) == len(want)
    assert [(names.index(key(r.source)),) + tuple(r.rect) for r in records] == [tuple(int(v) for v in c[:5]) for c in want]
    assert [r.name for r in records] == [str(n) for n in golden[prefix + '_saved']]
    sub = 'training' if prefix == 'uccs' else 'train'
    assert all(r.source.startswith(os.path.join(raw, sub) + os.sep) for r in records)
    assert str(golden[prefix + '_dir'][0]) == fi.db_files('uccs' if prefix == 'uccs' else 'vggface2')[1]


@pytest.mark.parametrize('prefix', ['uccs', 'vgg'])
def test_db_text_is_the_references_byte_for_byte(golden, prefix, tmp_path):
    records, *_ = _records(golden, prefix, tmp_path)
    assert fi.db_csv_text(records).encode() == bytes(golden[prefix + '_db_csv'])


@pytest.mark.parametrize('prefix', ['uccs', 'vgg'])
def test_geometry_is_the_references(golden, prefix, tmp_path):
    S = int(golden['image_size'])
    for c in golden[prefix + '_crops']:
        assert letterbox_geometry(int(c[3]), int(c[4]), S) == tuple(int(v) for v in c[5:11])
        assert fi.lb_side_ok(int(c[3]), int(c[4]), S)


def test_db_text_is_what_the_readers_of_the_package_read(golden, tmp_path):
    import pandas as pd
    records, *_ = _records(golden, 'uccs', tmp_path)
    (tmp_path / 'db.csv').write_text(fi.db_csv_text(records))
    db = pd.read_csv(tmp_path / 'db.csv').iloc[:, 1:]
    assert list(db.columns) == ['subject_id', 'face_file', 'w', 'h']
    assert list(db.face_file) == [r.name for r in records] and list(db.subject_id) == [r.row[0] for r in records]
    assert fi.db_csv_text([]) == ',subject_id,face_file,w,h\n'


def _uccs(tmp_path, rows):
    os.makedirs(tmp_path / 'training', exist_ok=True)
    text = 'FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT\n'
    (tmp_path / 'training' / 'training.csv').write_text(text + ''.join('%d,%s,%d,%r,%r,%r,%r\n' % ((i,) + r) for i, r in enumerate(rows)))


def test_uccs_skip_rules(tmp_path):
    """Port only: the rows the reference raises on (an empty cut divides 0 by 0, a side of 0 pixels makes cv.resize raise) are
    skipped and counted; its own skips (-1, a field <= 0, NaN) are not counted."""
    _uccs(tmp_path, [('a.jpg', 4, 10.0, 10.0, 30.0, 30.0),        # kept
                     ('a.jpg', 4, 0.5, 10.0, 30.0, 30.0),         # l - 1 == -1: counts from the end, empty
                     ('a.jpg', 4, 10.0, 0.9, 30.0, 30.0),         # t - 1 == -1
                     ('a.jpg', 4, 150.0, 10.0, 30.0, 30.0),       # beyond the right edge: empty
                     ('a.jpg', 4, 10.0, 10.0, 1.5, 30.0),         # r - 1 == l - 1: empty
                     ('a.jpg', 4, 10.0, 10.0, 2.0, 90.0),         # 1 x 89: int(1 / 89 * 64) == 0
                     ('a.jpg', 4, 10.0, 10.0, 0.0, 30.0),         # the reference's own skip
                     ('a.jpg', 4, 10.0, 10.0, 30.0, -2.0),
                     ('a.jpg', 4, 10.0, float('nan'), 30.0, 30.0),
                     ('a.jpg', -1, 10.0, 10.0, 30.0, 30.0),
                     ('b.jpg', 2, 1.0, 1.0, 500.0, 500.0)])       # clipped to the frame: 99 x 119
    records, skipped = fi.uccs_records(str(tmp_path), 64, lambda p: (100, 120))
    assert skipped == {'empty': 4, 'side_rounds_to_0': 1}
    assert [(r.name, r.rect, r.row) for r in records] == [
        ('b_2_1_1.jpg', (0, 0, 100, 120), (2, 'b_2_1_1.jpg', 120, 100)),
        ('a_4_10_10.jpg', (9, 9, 29, 29), (4, 'a_4_10_10.jpg', 29, 29))]


def test_vggface2_skip_rules(tmp_path):
    (tmp_path / 'loose_bb_train.csv').write_text('NAME_ID,X,Y,W,H\nn1/f1,0,0,10,10\nn1/f2,50,200,10,10\nn1/f3,-1,0,5,5\n'
                                                 'n2/f1,0,0,0,5\nn2/f2,3,0,1,90\nn2/f3,110,90,50,50\n')
    records, skipped = fi.vggface2_records(str(tmp_path), 64, lambda p: (100, 120))
    assert skipped == {'empty': 1, 'side_rounds_to_0': 1}        # n1/f2 starts below the image; n2/f2 is 1 x 90
    assert [(r.name, r.rect, r.row) for r in records] == [
        ('n1_f1.jpg', (0, 0, 10, 10), ('n1', 'n1_f1.jpg', 10, 10)),
        ('n2_f3.jpg', (90, 110, 10, 10), ('n2', 'n2_f3.jpg', 10, 10))]
    assert records[0].source == os.path.join(str(tmp_path), 'train', 'n1', 'f1.jpg')


def test_source_batches_group_by_file_under_both_budgets():
    R = fi.CropRecord
    recs = [R('a', None, '0', None), R('b', None, '1', None), R('a', None, '2', None), R('c', None, '3', None),
            R('d', None, '4', None), R('b', None, '5', None), R('d', None, '6', None), R('d', None, '7', None)]
    hw = {'a': (10, 10), 'b': (10, 20), 'c': (100, 100), 'd': (10, 10)}
    flat = lambda bs: [[(s, ii) for s, ii in b] for b in bs]
    # a file's crops stay together, files in order of first appearance
    assert flat(fi.source_batches(recs, hw.get, 1 << 30, 1 << 30)) == [[('a', [0, 2]), ('b', [1, 5]), ('c', [3]), ('d', [4, 6, 7])]]
    # bytes: a + b = 900 fits 1 000, c (30 000) is over on its own and still gets a batch
    assert flat(fi.source_batches(recs, hw.get, 1000, 1 << 30)) == [[('a', [0, 2]), ('b', [1, 5])], [('c', [3])], [('d', [4, 6, 7])]]
    # crops: at most 4 per batch; d's three stay together
    assert flat(fi.source_batches(recs, hw.get, 1 << 30, 4)) == [[('a', [0, 2]), ('b', [1, 5])], [('c', [3]), ('d', [4, 6, 7])]]
    assert fi.source_batches([], hw.get) == []


def test_slice_rect_is_crop_rects_rule():
    from face_vijnana_yolov3_amd.postproc import BoundBox
    for box in [(5, 7, 40, 30), (0, 7, 40, 30), (5, 0, 40, 30), (90, 70, 300, 300), (1, 1, 2, 2), (1, 1, 3, 3)]:
        assert fi.crop_rect(BoundBox(*box), 80, 100) == fi.slice_rect(box[1] - 1, box[3] - 1, box[0] - 1, box[2] - 1, 80, 100)
    assert fi.slice_rect(-1, 10, 0, 10, 80, 100) is None and fi.slice_rect(0, 10, 0, 10, 80, 100) == (0, 0, 10, 10)


def _conf(tmp_path, mode, resource_type='uccs'):
    return {'fi_conf': dict(mode=mode, resource_type=resource_type, raw_data_path=str(tmp_path), nn_arch=dict(image_size=64, dense1_dim=64),
                            hps={}, model_loading=False)}


def test_main_dispatches_data_before_any_model_is_built(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(_conf(tmp_path, 'data')))
    seen = []
    monkeypatch.setattr(fi, 'create_db_fi', lambda conf: seen.append(conf['fi_conf']['mode']))
    monkeypatch.setattr(fi, 'FaceIdentifier', lambda conf: pytest.fail('the data mode builds no model'))
    fi.main()
    assert seen == ['data']
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(_conf(tmp_path, 'evaluate')))
    with pytest.raises(NotImplementedError, match='available: data, train, fid_db, test'):
        fi.main()
    # the data mode exists for two resource types; main() says so for any other, or none, before anything is touched
    for conf in (_conf(tmp_path, 'data', resource_type='lfw'), {'fi_conf': {'mode': 'data'}}):
        (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(conf))
        with pytest.raises(NotImplementedError, match='available: uccs, vggface2'):
            fi.main()
    assert seen == ['data']


def test_data_mode_without_the_library_fails_with_the_packages_error(tmp_path, monkeypatch):
    """No CPU path: with libfv_hotpath.so absent the mode raises FvError (not NotImplementedError), and before it has touched
    the faces directory."""
    from face_vijnana_yolov3_amd import _lib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'absent.so'))
    os.makedirs(tmp_path / 'subject_faces')
    (tmp_path / 'subject_faces' / 'old.jpg').write_bytes(b'x')
    (tmp_path / 'face_vijnana_yolov3.json').write_text(json.dumps(_conf(tmp_path, 'data')))
    with pytest.raises(_lib.FvError):
        fi.main()
    assert os.listdir(tmp_path / 'subject_faces') == ['old.jpg']


def test_create_db_fi_rejects_an_unknown_resource_type(tmp_path):
    with pytest.raises(ValueError, match='resource type is not valid'):
        fi.create_db_fi(_conf(tmp_path, 'data', resource_type='lfw'))
