"""fv_fid_mine_negatives' contract restated in numpy, float64 throughout, the sum of squares taken as a loop over the 64
dimensions in order -- the chain the device runs, so every output is compared for equality.  Test infrastructure: the product
does not import it.  Also the generator of the random cases and the hand cases the CPU and GPU tests share."""
import numpy as np

DIM = 64
KIND_SEMI_HARD, KIND_VIOLATING, KIND_EASY, KIND_NONE = 0, 1, 2, 3


def dists_to(ids, a):
    """D(a, r) for every row r: sqrt of the float64 sum, in dimension order, of the squared float64 differences."""
    ids = np.asarray(ids, np.float32)
    s = np.zeros(len(ids), np.float64)
    x = ids[a].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(ids.shape[1]):
            d = x[k] - ids[:, k].astype(np.float64)
            s = s + d * d
        return np.sqrt(s)


def eligible(D, subjects, a):
    """The rows anchor a may take a negative from, ascending: a known subject other than its own, and a distance that is a number."""
    return np.flatnonzero((subjects >= 0) & (subjects != subjects[a]) & ~np.isnan(D))


def mine_one(dap, E, De, margin, mode):
    """One triplet: dap = D(a, p), E = eligible rows (ascending), De = their distances -> (neg_index, kind, d_ap, d_an).
    np.argmin / np.argmax return the first extremum, which in ascending E is the lowest row among equals."""
    if np.isnan(dap):
        return -1, KIND_NONE, np.nan, np.inf
    hi = dap + np.float64(margin)
    band = (De > dap) & (De < hi)
    near = De <= dap
    far = De >= hi
    if mode == 1:
        if not len(E):
            return -1, KIND_NONE, dap, np.inf
        k = np.argmin(De)
        return int(E[k]), (KIND_SEMI_HARD if band[k] else KIND_VIOLATING if near[k] else KIND_EASY), dap, De[k]
    if band.any():
        k = np.flatnonzero(band)[np.argmin(De[band])]
        return int(E[k]), KIND_SEMI_HARD, dap, De[k]
    if near.any():
        k = np.flatnonzero(near)[np.argmax(De[near])]
        return int(E[k]), KIND_VIOLATING, dap, De[k]
    if far.any():
        k = np.flatnonzero(far)[np.argmin(De[far])]
        return int(E[k]), KIND_EASY, dap, De[k]
    return -1, KIND_NONE, dap, np.inf


def mine_negatives(ids, subjects, pairs, margin, mode):
    """pairs: (a, p) per triplet -> (neg_index int32, kind int32, d_ap float64, d_an float64), one entry per pair."""
    subjects = np.asarray(subjects, np.int32)
    t = len(pairs)
    neg, kind = np.empty(t, np.int32), np.empty(t, np.int32)
    d_ap, d_an = np.empty(t, np.float64), np.empty(t, np.float64)
    cache = {}
    for j, (a, p) in enumerate(pairs):
        a, p = int(a), int(p)
        if a not in cache:
            D = dists_to(ids, a)
            E = eligible(D, subjects, a)
            cache[a] = (D, E, D[E])
        D, E, De = cache[a]
        neg[j], kind[j], d_ap[j], d_an[j] = mine_one(D[p], E, De, margin, mode)
    return neg, kind, d_ap, d_an


# ----------------------------------------------------------------------------- cases
def random_case(n, n_subjects=12, seed=0, unknown=0.0):
    """ids = l2_normalize(relu(centre[subject] + 0.6 * noise)) float32, a subject drawn per row; `unknown`: the share of rows whose
    subject is then set to -1.  -> (ids, subjects int32, pairs: every k < l of every subject, anchor-major)."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(n_subjects, DIM)
    subjects = rng.randint(0, n_subjects, n).astype(np.int32)
    x = np.maximum(centres[subjects] + 0.6 * rng.randn(n, DIM), 0.0)
    ids = (x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), 1e-12))).astype(np.float32)
    if unknown:
        subjects[rng.rand(n) < unknown] = -1
    return ids, subjects, same_subject_pairs(subjects)


def same_subject_pairs(subjects):
    pairs = []
    for s in sorted(set(int(v) for v in subjects if v >= 0)):
        own = np.flatnonzero(subjects == s)
        pairs += [(int(own[k]), int(own[l])) for k in range(len(own) - 1) for l in range(k + 1, len(own))]
    return pairs


def _unit(*coords):
    v = np.zeros(DIM, np.float32)
    v[:len(coords)] = coords
    return v


def hand_cases():
    """name -> dict(ids, subjects, pairs, margin, mode, want): want = [(neg_index, kind)] per pair, worked out by hand.
    Distances along one axis are differences of the first coordinate."""
    f32 = np.float32
    cases = {}
    # anchor at 0, positive at 0.5 (dap 0.5, band (0.5, 0.7)): rows 2 and 3 lie in the band, row 2 nearer
    cases['kind0_band'] = dict(ids=[_unit(0), _unit(.5), _unit(.625), _unit(.6875), _unit(2), _unit(.25)], subjects=[0, 0, 1, 1, 2, 2],
                               pairs=[(0, 1)], want=[(2, 0)])
    # none in the band; rows 2, 3 violate (D 0.25, 0.375 <= 0.5): the mildest is the larger D, row 3; row 4 is easy
    cases['kind1_mildest'] = dict(ids=[_unit(0), _unit(.5), _unit(.25), _unit(.375), _unit(2)], subjects=[0, 0, 1, 1, 2],
                                  pairs=[(0, 1)], want=[(3, 1)])
    # hardest mode on the same rows: the nearest, row 2, and it is a violating one
    cases['hardest_kind1'] = dict(cases['kind1_mildest'], mode=1, want=[(2, 1)])
    # every other subject beyond the band: the nearest of them, row 3 (D 1) before row 2 (D 2)
    cases['kind2_easy'] = dict(ids=[_unit(0), _unit(.5), _unit(2), _unit(1)], subjects=[0, 0, 1, 2], pairs=[(0, 1)], want=[(3, 2)])
    # one subject only: nothing is eligible
    cases['kind3_one_subject'] = dict(ids=[_unit(0), _unit(.5), _unit(.25)], subjects=[3, 3, 3], pairs=[(0, 1), (2, 0)],
                                      want=[(-1, 3), (-1, 3)])
    # rows 2 and 4 are the same vector (and 3 a farther one): the lower index
    cases['duplicate_lower_index'] = dict(ids=[_unit(0), _unit(.5), _unit(.625), _unit(.6875), _unit(.625)], subjects=[0, 0, 1, 1, 2],
                                          pairs=[(0, 1)], want=[(2, 0)])
    # duplicated violating rows 3 and 2 at the largest D <= dap: the lower index again
    cases['duplicate_violating'] = dict(ids=[_unit(0), _unit(.5), _unit(.375), _unit(.375), _unit(.25)], subjects=[0, 0, 1, 2, 2],
                                        pairs=[(0, 1)], want=[(2, 1)])
    # the positive duplicates the anchor (dap 0, band (0, 0.2)): row 2 at 0.125 is in it; row 3, another duplicate of the anchor,
    # has D 0 <= dap and would be the violating choice only were the band empty -- as for pair (0, 1) of the second case
    cases['dap_zero'] = dict(ids=[_unit(0), _unit(0), _unit(.125), _unit(0)], subjects=[0, 0, 1, 1], pairs=[(0, 1)], want=[(2, 0)])
    cases['dap_zero_violating'] = dict(ids=[_unit(0), _unit(0), _unit(.5), _unit(0)], subjects=[0, 0, 1, 1], pairs=[(0, 1)],
                                       want=[(3, 1)])
    # row 2 would be the band's nearest but holds a NaN: ignored, row 3 it is
    nan_row = _unit(.625); nan_row[40] = np.nan
    cases['nan_row_ignored'] = dict(ids=[_unit(0), _unit(.5), nan_row, _unit(.6875)], subjects=[0, 0, 1, 1], pairs=[(0, 1)], want=[(3, 0)])
    # a NaN in the anchor: every distance is NaN, kind 3; a NaN in the positive alone: dap is NaN, kind 3 as well
    nan_anchor = _unit(0); nan_anchor[7] = np.nan
    cases['nan_anchor'] = dict(ids=[nan_anchor, _unit(.5), _unit(.625), nan_row], subjects=[0, 0, 1, 0], pairs=[(0, 1), (1, 3)],
                               want=[(-1, 3), (-1, 3)])
    # row 2 (subject -1) is the nearest in the band and never chosen; an anchor of subject -1 may still be asked for: every known
    # subject's rows are eligible for it (dap 0.3125: rows 1 and 3 violate at D 0.0625 and 0.125, row 0 at 0.5625 is easy)
    cases['unknown_never_chosen'] = dict(ids=[_unit(0), _unit(.5), _unit(.5625), _unit(.6875), _unit(.25)], subjects=[0, 0, -1, 1, -1],
                                         pairs=[(0, 1), (2, 4)], want=[(3, 0), (3, 1)])
    cases['n1'] = dict(ids=[_unit(1)], subjects=[0], pairs=[(0, 0)], want=[(-1, 3)])
    cases['n2_two_subjects'] = dict(ids=[_unit(0), _unit(3)], subjects=[0, 1], pairs=[(0, 0), (1, 1)], want=[(1, 2), (0, 2)])
    cases['n2_one_subject'] = dict(ids=[_unit(0), _unit(3)], subjects=[0, 0], pairs=[(0, 1)], want=[(-1, 3)])
    for c in cases.values():
        c['ids'] = np.asarray(c['ids'], f32)
        c['subjects'] = np.asarray(c['subjects'], np.int32)
        c.setdefault('margin', 0.2)
        c.setdefault('mode', 0)
    return cases
