#!/opt/conda/bin/python3.9
"""Mint golden vectors for face verification by RUNNING the reference's own cal_VAL_FAR (evaluate.py:196-223, which calls
cal_face_pairs_dists, evaluate.py:129-194) on synthetic subject databases (build container only):

    /opt/conda/bin/python3.9 tests/golden/make_pairs_golden.py      # the interpreter that has h5py 3 / scipy / NumPy < 2

Stand-ins as in make_fi_golden.py (keras, cv2, skimage, ...).  Two shims more: h5py 3 dropped Dataset.value, which the reference
reads per pair, so it is restored as `d[()]`; and the reference writes the builtin `vars` as val_far.h5's 'vals'
(evaluate.py:221), which h5py cannot store, so the module gets an array named `vars` and that write succeeds.  Nothing of the
reference is altered or copied; only the inputs and outputs below are written.

tests/golden/face_pairs.npz, per case c:
  case<c>_csv        subject_image_db.csv as written (running index, subject_id, face_file, w, h; rows shuffled, so csv order is
                     not subject order), uint8 text;
  case<c>_names      face files of subject_facial_ids.h5 and case<c>_ids their float32 (64,) IDs (unit norm: a subject centre plus
                     noise of a per-subject scale, so same-identity distances spread over ~0.1-1.0 and different ones reach below 1);
  case<c>_seed       np.random.seed before the call (the different-identity subject draw);
  case<c>_same_dists, case<c>_diff_dists   face_pairs_dists.h5 as the reference wrote it (float64 arrays of float32 values:
                     that SciPy's norm returns snrm2's result as a Python float);
  case<c>_sim_ths, case<c>_vals, case<c>_fars   cal_VAL_FAR's return values at np.arange(0.1, 1.1, 0.1);
  case<c>_draw       the (S // 2, 2) subject-index draw (np.random.choice replayed with the seed).
Cases: an odd subject count with subject -1 drawn into a pair, an even count, a small database with singletons.  Draws are
rejected when any distance lies within 1e-5 of a float32 threshold, so 1-ulp differences cannot move a count.
"""
import io
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fi_golden import REF, _install_stubs  # noqa: E402

THS = np.arange(0.1, 1.1, 0.1)
# (number of subjects incl. -1, files per subject range, -1 must be drawn, seed)
CASES = [(41, (1, 12), True, 11), (40, (1, 10), False, 22), (17, (1, 6), False, 33)]


def synth(S, sizes, rng):
    sids = [-1] + sorted(int(v) for v in rng.choice(np.arange(1, 500), S - 1, replace=False))
    g = rng.normal(size=64)
    g /= np.linalg.norm(g)
    rows, ids = [], {}
    for sid in sids:
        n = int(rng.integers(sizes[0], sizes[1] + 1)) if sid != -1 else 5
        c = g + 0.11 * rng.normal(size=64)
        c /= np.linalg.norm(c)
        sigma = rng.uniform(0.01, 0.09)
        for f in range(n):
            v = c + sigma * rng.normal(size=64)
            name = 'sub%03d_%02d.jpg' % (sid if sid >= 0 else 999, f)
            ids[name] = (v / np.linalg.norm(v)).astype(np.float32)
            rows.append((sid, name, int(rng.integers(20, 90)), int(rng.integers(20, 90))))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order], ids


def near_threshold(dists):
    d = np.asarray(dists, np.float64)
    return any(np.any(np.abs(d - float(np.float32(t))) < 1e-5) for t in THS)


def run_case(ref_ev, h5py, S, sizes, need_minus1, seed):
    import pandas as pd
    rng = np.random.default_rng(seed)
    while True:
        rows, ids = synth(S, sizes, rng)
        np.random.seed(seed)
        draw = np.random.choice(range(S), size=(S // 2, 2), replace=False)
        if need_minus1 and not np.any(draw == 0):             # subject -1 is key 0 of the sorted list
            seed += 1000
            continue
        with tempfile.TemporaryDirectory() as tmp:
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                pd.DataFrame(rows, columns=['subject_id', 'face_file', 'w', 'h']).to_csv('subject_image_db.csv')
                with h5py.File('subject_facial_ids.h5', 'w') as f:
                    for name, v in ids.items():
                        f[name] = v
                np.random.seed(seed)
                so = sys.stdout
                sys.stdout = io.StringIO()                    # the reference prints its progress
                try:
                    sim_ths, vals, fars = ref_ev.cal_VAL_FAR(THS)
                finally:
                    sys.stdout = so
                with h5py.File('face_pairs_dists.h5', 'r') as f:
                    same, diff = f['same_dists'][()], f['diff_dists'][()]
                csv = open('subject_image_db.csv').read()
            finally:
                os.chdir(cwd)
        if near_threshold(same) or near_threshold(diff):
            seed += 1000
            continue
        names = sorted(ids)
        return {'csv': np.frombuffer(csv.encode(), np.uint8), 'names': np.asarray(names),
                'ids': np.asarray([ids[n] for n in names], np.float32), 'seed': np.int64(seed), 'same_dists': same,
                'diff_dists': diff, 'sim_ths': np.asarray(sim_ths), 'vals': np.asarray(vals), 'fars': np.asarray(fars),
                'draw': draw.astype(np.int64)}


def main():
    _install_stubs()
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    warnings.simplefilter('ignore')
    import h5py
    h5py.Dataset.value = property(lambda d: d[()])
    import evaluate as ref_ev
    ref_ev.vars = np.zeros(1)
    out = {}
    for c, (S, sizes, need, seed) in enumerate(CASES):
        r = run_case(ref_ev, h5py, S, sizes, need, seed)
        for k, v in r.items():
            out['case%d_%s' % (c, k)] = v
        print('case %d: seed %d, %d ids, %d same (%s), %d diff (%s), vals %s, fars %s' % (
            c, r['seed'], len(r['ids']), len(r['same_dists']), r['same_dists'].dtype, len(r['diff_dists']),
            r['diff_dists'].dtype, np.round(r['vals'], 3), np.round(r['fars'], 3)))
    out['ncases'] = np.int64(len(CASES))
    np.savez_compressed(os.path.join(HERE, 'face_pairs.npz'), **out)
    print('wrote face_pairs.npz')


if __name__ == '__main__':
    main()
