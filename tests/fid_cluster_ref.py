"""fv_fid_cluster's contract (csrc/fid_cluster.h) restated in NumPy float64, and the cases the CPU and GPU tests share.

The distance is accumulated dimension by dimension in a Python loop over the 64 columns: that is the operator's summation order
(np.sum pairs differently).  Nothing in here needs a GPU or the library."""
import numpy as np

DIM = 64
MAX_N = 65536


def distances(ids):
    """(n, n) float64: sqrt of the sum, in dimension order, of the squared float64 differences.  NaN where a row holds NaN / inf."""
    x = np.asarray(ids, np.float32).astype(np.float64)
    n = len(x)
    s = np.zeros((n, n))

    def block(r0):                                       # row blocks keep the temporaries small; each sum's order is 0..63
        rows = x[r0:r0 + 128]
        with np.errstate(invalid='ignore', over='ignore'):
            for k in range(DIM):
                d = rows[:, k][:, None] - x[:, k][None, :]
                d *= d
                s[r0:r0 + 128] += d
            np.sqrt(s[r0:r0 + 128], out=s[r0:r0 + 128])

    starts = range(0, n, 128)
    if n <= 1024:
        for r0 in starts:
            block(r0)
    else:                                                # NumPy's loops release the interpreter lock: blocks run side by side
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(block, starts))
    return s


def cluster(ids, eps, min_pts, D=None):
    """-> dict(labels int32, via int32, n_nbr int32, core uint8, n_clusters int32 (1,)) as the header defines them."""
    D = distances(ids) if D is None else D
    n = len(D)
    with np.errstate(invalid='ignore'):
        nbr = D <= eps                                   # a NaN is not a neighbour
    n_nbr = nbr.sum(1).astype(np.int32)
    core = n_nbr >= min_pts
    labels = np.full(n, -1, np.int32)
    via = np.full(n, -1, np.int32)
    core_nbr = nbr & core[None, :]
    c = 0
    for i in np.flatnonzero(core):                       # ascending: a new cluster is numbered by its smallest core index
        if labels[i] >= 0:
            continue
        seen = np.zeros(n, bool)
        seen[i] = True
        front = np.array([i])
        while len(front):
            reach = core_nbr[front].any(0) & ~seen
            seen |= reach
            front = np.flatnonzero(reach)
        labels[seen] = c
        c += 1
    via[core] = np.flatnonzero(core)
    for i in np.flatnonzero(~core):
        cand = np.flatnonzero(core_nbr[i])
        if len(cand):
            r = cand[np.argmin(D[i, cand])]              # the first minimum: the lowest index among equal distances
            via[i] = r
            labels[i] = labels[r]
    return dict(labels=labels, via=via, n_nbr=n_nbr, core=core.astype(np.uint8), n_clusters=np.array([c], np.int32))


def tied_borders(out, D):
    """Border rows whose smallest core distance is shared by more than one core neighbour."""
    core = out['core'].astype(bool)
    rows = []
    for i in np.flatnonzero(~core & (out['via'] >= 0)):
        d = D[i, core & (D[i] <= D[i, out['via'][i]])]
        if len(d) > 1:
            rows.append(i)
    return np.asarray(rows, np.int64)


def classes(out):
    """(clusters, core rows, border rows, noise rows)"""
    core = out['core'].astype(bool)
    return int(out['n_clusters'][0]), int(core.sum()), int((~core & (out['labels'] >= 0)).sum()), int((out['labels'] < 0).sum())


# ------------------------------------------------------------------------------------------------------------------ generators
def mixed(n, seed, centres=30):
    """n rows around `centres` random centres in 64 dimensions, a spread per row drawn from U[0.2, 1.6], rows normalised."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, DIM))
    which = rng.integers(0, centres, n)
    spread = rng.uniform(0.2, 1.6, n)
    x = c[which] + spread[:, None] * rng.standard_normal((n, DIM))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def points(coords):
    """Rows whose first coordinates are `coords` (multiples of 1/8), the other dimensions 0."""
    x = np.zeros((len(coords), DIM), np.float32)
    for i, p in enumerate(coords):
        x[i, :len(p)] = p
    assert (x * 8 == np.round(x * 8)).all() or not np.isfinite(x).all()
    return x


def lattice(n, seed, side=16, dims=3):
    """n rows on the 1/8 lattice: integer coordinates in [0, side) in `dims` dimensions, times 1/8; every D ** 2 is exact."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, DIM), np.float32)
    x[:, :dims] = rng.integers(0, side, (n, dims)) / 8.0
    return x


def chain(n, eps, seed):
    """n rows spaced exactly eps (a multiple of 1/8) apart along dimension 0, in shuffled order -> (ids, position of every row)."""
    pos = np.random.default_rng(seed).permutation(n)
    x = np.zeros((n, DIM), np.float32)
    x[:, 0] = pos * eps
    assert (x[:, 0].astype(np.float64) == pos * float(eps)).all()
    return x, pos


def chain_expected(pos, min_pts):
    """The outputs for chain() at the chain's eps: inner rows have 3 neighbours, the two ends 2."""
    n = len(pos)
    row_at = np.argsort(pos)
    n_nbr = np.where((pos == 0) | (pos == n - 1), 2, 3).astype(np.int32)
    core = n_nbr >= min_pts
    labels = np.full(n, -1, np.int32)
    via = np.full(n, -1, np.int32)
    if core.any():
        labels[:] = 0                                    # the core rows are one run of the chain; the ends border it
        via[core] = np.flatnonzero(core)
        for end, inner in ((0, 1), (n - 1, n - 2)):
            if not core[row_at[end]]:
                via[row_at[end]] = row_at[inner]
    return dict(labels=labels, via=via, n_nbr=n_nbr, core=core.astype(np.uint8), n_clusters=np.array([int(core.any())], np.int32))


def copies(groups, per, seed):
    """groups * per rows: c * e_0 for c = 0 .. groups - 1, `per` copies each, shuffled -> (ids, the group of every row)."""
    g = np.random.default_rng(seed).permutation(np.repeat(np.arange(groups), per))
    x = np.zeros((len(g), DIM), np.float32)
    x[:, 0] = g
    return x, g


def copies_expected(g, per, min_pts):
    """The outputs for copies() at eps 0.5: a row's neighbours are its `per` copies, in closed form (no n x n matrix)."""
    n = len(g)
    n_nbr = np.full(n, per, np.int32)
    if per < min_pts:
        return dict(labels=np.full(n, -1, np.int32), via=np.full(n, -1, np.int32), n_nbr=n_nbr, core=np.zeros(n, np.uint8),
                    n_clusters=np.zeros(1, np.int32))
    _, first = np.unique(g, return_index=True)           # the smallest row of every group
    number = np.empty(len(first), np.int32)
    number[np.argsort(first)] = np.arange(len(first), dtype=np.int32)
    return dict(labels=number[g], via=np.arange(n, dtype=np.int32), n_nbr=n_nbr, core=np.ones(n, np.uint8),
                n_clusters=np.array([len(first)], np.int32))


# ------------------------------------------------------------------------------------------------------------------ hand cases
def _line(x0, y, step=0.25, count=5):
    return [(x0 + step * k, y) for k in range(count)]


def _expect(labels, via, n_nbr, core):
    return dict(labels=np.asarray(labels, np.int32), via=np.asarray(via, np.int32), n_nbr=np.asarray(n_nbr, np.int32),
                core=np.asarray(core, np.uint8), n_clusters=np.array([max(labels) + 1], np.int32))


def hand_cases():
    """[(name, ids, eps, min_pts, expected outputs written out by hand)] on the 1/8 lattice."""
    cases = []
    pair = points([(0.0,), (1.0,)])
    cases.append(('a pair at exactly eps is a neighbour', pair, 1.0, 2, _expect([0, 0], [0, 1], [2, 2], [1, 1])))
    cases.append(('a pair at the next double below eps is not', pair, float(np.nextafter(1.0, 0.0)), 2,
                  _expect([-1, -1], [-1, -1], [1, 1], [0, 0])))
    # five rows 1/4 apart are each other's neighbours at eps 1 (5 each: core at min_pts 5); the origin sees one end of each line
    A, B = _line(-2.0, 0.0), _line(1.0, 0.0)             # A: -2 .. -1 (row 4 is at -1), B: 1 .. 2 (row 0 is at 1)
    ids = points(A + B + [(0.0, 0.0)])                   # the cores at distance 1 from the origin are rows 4 (A) and 5 (B)
    cases.append(('a border row equidistant from two clusters goes to the lower index', ids, 1.0, 5,
                  _expect([0] * 5 + [1] * 5 + [0], list(range(10)) + [4], [5, 5, 5, 5, 6, 6, 5, 5, 5, 5, 3], [1] * 10 + [0])))
    ids = points(B[1:] + A + [(0.0, 0.0), B[0]])         # the same with B's near end last: rows 8 (A's -1) and 10 tie, cluster 1 wins
    cases.append(('the lower index, not the lower cluster', ids, 1.0, 5,
                  _expect([0] * 4 + [1] * 5 + [1, 0], list(range(9)) + [8, 10], [5, 5, 5, 5, 5, 5, 5, 5, 6, 3, 6], [1] * 9 + [0, 1])))
    A, B = _line(-2.0, 0.0), _line(0.75, 0.0)            # B's near end at 0.75 (row 5), its next at 1.0 (row 6)
    ids = points(A + B + [(0.0, 0.0)])
    cases.append(('a nearer core with the higher index wins over a farther one', ids, 1.0, 5,
                  _expect([0] * 5 + [1] * 5 + [1], list(range(10)) + [5], [5, 5, 5, 5, 6, 6, 6, 5, 5, 5, 4], [1] * 10 + [0])))
    nan_row = np.zeros(DIM, np.float32)
    nan_row[5] = np.nan
    inf_row = np.zeros(DIM, np.float32)
    inf_row[0] = np.inf
    ids = points([(0.0, 0.0), (5.0, 0.0), (5.0, 0.125), (0.0, 0.0), (10.0, 0.0)])
    ids[3] = nan_row
    cases.append(('min_pts 1: every row without NaN is core, isolated rows are clusters of one', ids, 0.25, 1,
                  _expect([0, 1, 1, -1, 2], [0, 1, 2, -1, 4], [1, 2, 2, 0, 1], [1, 1, 1, 0, 1])))
    ids = points([(1.0, 1.0), (3.0, 3.0), (1.0, 1.0), (1.0, 1.0)])
    cases.append(('duplicated rows at eps 0', ids, 0.0, 3, _expect([0, -1, 0, 0], [0, -1, 2, 3], [3, 1, 3, 3], [1, 0, 1, 1])))
    ids = points([(0.0,), (0.125,), (0.25,), (0.0,), (0.0,)])
    ids[3], ids[4] = nan_row, inf_row
    cases.append(('a NaN row and an inf row are noise without neighbours', ids, 10.0, 2,
                  _expect([0, 0, 0, -1, -1], [0, 1, 2, -1, -1], [3, 3, 3, 0, 0], [1, 1, 1, 0, 0])))
    Y, X = _line(0.0, 0.0), _line(0.0, 10.0)             # X's border (2, 10) comes first: the numbering looks at core rows only
    ids = points([(2.0, 10.0)] + Y + X)
    cases.append(('clusters are numbered by their smallest core index', ids, 1.0, 5,
                  _expect([1] + [0] * 5 + [1] * 5, [10] + list(range(1, 11)), [2] + [5] * 9 + [6], [0] + [1] * 10)))
    return cases
