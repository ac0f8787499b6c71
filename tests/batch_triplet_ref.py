"""fv_fid_batch_triplet_loss_grad's contract (include/fv_hotpath.h) restated in numpy, float64 throughout.
The selection reuses the distance and the class table of tests/mine_negatives_ref.py (the same chain of float64 operations as the
device runs, so indices, kinds and the bits of d_ap / d_an are compared for equality); the gradient is written out, as _ref_triplet
of tests/test_ops_gpu.py is, because autograd through a distance of exactly 0 gives NaN.  Test infrastructure: the product does not
import it.  Also the hand cases the CPU and GPU tests share."""
import numpy as np

from mine_negatives_ref import DIM, KIND_NONE, dists_to, eligible, mine_one

MODE_BATCH_HARD, MODE_BATCH_SEMI_HARD = 0, 1


def l2n_relu(pre):
    """u = float32(l2_normalize(relu(pre))) computed in float64: what the dense call hands the loss."""
    r = np.maximum(np.asarray(pre, np.float64), 0.0)
    return (r / np.sqrt(np.maximum((r * r).sum(-1, keepdims=True), 1e-12))).astype(np.float32)


def select(u, subjects, margin, mode):
    """-> pos_index, neg_index, kind (int32), d_ap, d_an (float64), one entry per row."""
    u = np.asarray(u, np.float32)
    subjects = np.asarray(subjects, np.int32)
    M = len(u)
    pos, neg, kind = np.full(M, -1, np.int32), np.full(M, -1, np.int32), np.full(M, KIND_NONE, np.int32)
    d_ap, d_an = np.full(M, np.nan, np.float64), np.full(M, np.inf, np.float64)
    for i in range(M):
        if subjects[i] < 0:
            continue
        D = dists_to(u, i)
        own = np.flatnonzero((subjects == subjects[i]) & (np.arange(M) != i) & ~np.isnan(D))
        if not len(own):
            continue
        p = own[np.argmax(D[own])]                       # the first maximum: the lowest row among equals
        E = eligible(D, subjects, i)
        # mine_one's mode 0 is the semi-hard table, 1 the nearest: the other way round from this operator's
        n, k, dap, dan = mine_one(D[p], E, D[E], margin, 1 - mode)
        if n < 0:
            continue
        pos[i], neg[i], kind[i], d_ap[i], d_an[i] = p, n, k, dap, dan
    return pos, neg, kind, d_ap, d_an


def l2_relu_bwd(pre, du, weight):
    pre = np.asarray(pre, np.float64)
    r = np.maximum(pre, 0.0)
    ss = (r * r).sum(-1, keepdims=True)
    s = 1.0 / np.sqrt(np.maximum(ss, 1e-300))
    uu = r * s
    dr = np.where(ss > 1e-12, s * (du - uu * (uu * du).sum(-1, keepdims=True)), du * 1e6)
    return np.where(pre > 0, dr * weight, 0.0)


def batch_triplet(pre, u, subjects, margin=0.2, mode=0, weight=1.0):
    """-> dict(loss, dE (M, 64), dbias (64,), pos_index, neg_index, kind, d_ap, d_an, h (nan where invalid), du, ss): float64."""
    pre = np.asarray(pre, np.float32)
    u = np.asarray(u, np.float32)
    M = len(u)
    pos, neg, kind, d_ap, d_an = select(u, subjects, margin, mode)
    valid = kind != KIND_NONE
    V = int(valid.sum())
    h = np.where(valid, d_ap - np.where(valid, d_an, 0.0) + np.float64(margin), np.nan)
    loss = 0.0
    for i in np.flatnonzero(valid):                      # anchor order
        loss = loss + max(h[i], 0.0)
    loss = loss / V if V else 0.0
    u64 = u.astype(np.float64)

    def inv(d):
        return 1.0 / (V * d) if d > 0.0 else 0.0
    active = valid & (np.where(valid, h, -1.0) >= 0.0)
    du = np.zeros((M, DIM), np.float64)
    for r in range(M):
        total = np.zeros(DIM, np.float64)
        if active[r]:                                    # the row's own anchor term first
            total = inv(d_ap[r]) * (u64[r] - u64[pos[r]]) - inv(d_an[r]) * (u64[r] - u64[neg[r]])
        # then what the active anchors send to r, in anchor order: the positive term, then the negative term (one of them at most)
        for i in np.flatnonzero(active & ((pos == r) | (neg == r))):
            if pos[i] == r:
                total = total - inv(d_ap[i]) * (u64[i] - u64[r])
            if neg[i] == r:
                total = total + inv(d_an[i]) * (u64[i] - u64[r])
        du[r] = total
    dE = l2_relu_bwd(pre, du, weight)
    r = np.maximum(pre.astype(np.float64), 0.0)
    return dict(loss=loss, dE=dE, dbias=dE.sum(0), pos_index=pos, neg_index=neg, kind=kind, d_ap=d_ap, d_an=d_an, h=h, du=du,
                ss=(r * r).sum(-1), active=active, V=V)


# ----------------------------------------------------------------------------- cases
def _row(*coords):
    v = np.zeros(DIM, np.float32)
    v[:len(coords)] = coords
    return v


def hand_cases():
    """name -> dict(pre, subjects, mode, margin, want): want = [(pos_index, neg_index, kind)] per row, worked out by hand.  pre rows
    are unit vectors cos(t) e0 + sin(t) e1 (their u is themselves up to rounding), so D between two rows is the chord 2 sin(dt / 2)."""
    def at(t):
        return _row(np.cos(t), np.sin(t))
    cases = {}
    cases['m1'] = dict(pre=[at(0)], subjects=[0], want=[(-1, -1, 3)])
    # two rows of one subject: positives, but no negative anywhere -> V = 0
    cases['one_subject'] = dict(pre=[at(0), at(.3)], subjects=[0, 0], want=[(-1, -1, 3)] * 2)
    # two rows of different subjects: negatives, but no positive
    cases['no_positive'] = dict(pre=[at(0), at(.3)], subjects=[0, 1], want=[(-1, -1, 3)] * 2)
    # rows 0, 1 of subject 0 and the lone row 2 of subject 1 beyond the band of both: V = 2, row 2 only ever a negative (easy)
    cases['two_and_one'] = dict(pre=[at(0), at(.1), at(1.2)], subjects=[0, 0, 1], want=[(1, 2, 2), (0, 2, 2), (-1, -1, 3)])
    # row 1 duplicates row 0: D(0, 1) = 0 < D(0, 2), so the positive of both is row 2; row 2's positives tie and the lower wins;
    # the negatives 4 (dup of 3) and 3 tie for anchors 0 .. 2: the lower index; anchors 3 and 4 are each other's positive at
    # distance 0 and take row 2, the nearest of the other subject (chord(.9) = 0.87 >= 0 + 0.2: easy)
    cases['duplicates'] = dict(pre=[at(0), at(0), at(.1), at(1.0), at(1.0)], subjects=[0, 0, 0, 1, 1],
                               want=[(2, 3, 2), (2, 3, 2), (0, 3, 2), (4, 2, 2), (3, 2, 2)], mode=0)
    # a pair of duplicates alone in its subject: dap is exactly 0 (the gradient of that distance is 0)
    cases['dap_zero'] = dict(pre=[at(0), at(0), at(.1)], subjects=[0, 0, 1], want=[(1, 2, 0), (0, 2, 0), (-1, -1, 3)], mode=1)
    # rows of subject -1 are no anchor, no positive (row 3 equals row 0's subject in nothing) and no negative (row 2 would be nearest)
    cases['unknown_rows'] = dict(pre=[at(0), at(.1), at(.15), at(.05), at(1.2)], subjects=[0, 0, -1, -1, 1],
                                 want=[(1, 4, 2), (0, 4, 2), (-1, -1, 3), (-1, -1, 3), (-1, -1, 3)])
    # mode 1, anchor 0 with its positive at chord(0.4) = 0.397: a semi-hard negative (row 2 at chord(.5) = 0.495 inside (0.397, 0.597));
    # anchor 1 has rows 2, 3 at chord(.1), chord(.2) <= dap and row 4 beyond the band: the mildest violating one, row 3
    cases['semi_kind0'] = dict(pre=[at(0), at(.4), at(.5), at(.2), at(1.5)], subjects=[0, 0, 1, 2, 3], mode=1,
                               want=[(1, 2, 0), (0, 3, 1), (-1, -1, 3), (-1, -1, 3), (-1, -1, 3)])
    # mode 0 on the same rows: the nearest negative of anchor 0 is row 3 (chord(.2) <= dap: violating), of anchor 1 row 2
    cases['hard_kind1'] = dict(cases['semi_kind0'], mode=0, want=[(1, 3, 1), (0, 2, 1), (-1, -1, 3), (-1, -1, 3), (-1, -1, 3)])
    # mode 1 with nothing in the band: the mildest violating one -- for anchor 0 row 3 (chord(.3)) before row 2 (chord(.2)), for
    # anchor 1 (at .4) row 2 (chord(.2)) before row 3 (chord(.1))
    cases['semi_kind1'] = dict(pre=[at(0), at(.4), at(.2), at(.3), at(1.5)], subjects=[0, 0, 1, 2, 3], mode=1,
                               want=[(1, 3, 1), (0, 2, 1), (-1, -1, 3), (-1, -1, 3), (-1, -1, 3)])
    # mode 1 with every other subject beyond the band: the nearest easy one, row 3
    cases['semi_kind2'] = dict(pre=[at(0), at(.1), at(1.5), at(1.2)], subjects=[0, 0, 1, 2], mode=1,
                               want=[(1, 3, 2), (0, 3, 2), (-1, -1, 3), (-1, -1, 3)])
    for c in cases.values():
        c['pre'] = np.asarray(c['pre'], np.float32)
        c['subjects'] = np.asarray(c['subjects'], np.int32)
        c.setdefault('margin', 0.2)
        c.setdefault('mode', 0)
    return cases


def random_case(M, seed, unknown=0.0, scale=0.6):
    """pre = centre[subject] + scale * noise (about half of the entries negative: ReLU cuts them), about M / 6 subjects, every
    subject holding several rows -> (pre float32, u float32, subjects int32)."""
    rng = np.random.RandomState(seed)
    n_subjects = max(1, M // 6)
    subjects = (np.arange(M) % n_subjects).astype(np.int32)
    rng.shuffle(subjects)
    centres = rng.randn(n_subjects, DIM)
    pre = (centres[subjects] + scale * rng.randn(M, DIM)).astype(np.float32)
    if unknown:
        subjects[rng.rand(M) < unknown] = -1
    return pre, l2n_relu(pre), subjects
