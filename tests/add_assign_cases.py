"""Cases and a numpy list model for the tests of amd_ivf_add without precomputed_idx: the one way of changing a resident index in which
the engine decides by itself where a vector goes (a k = 1 coarse ranking on the device, in blocks of 2^18).  numpy and the CPU oracle
only: the CPU test of the cases' preconditions (test_add_assign_cases_cpu.py) and the GPU test (test_gpu_add_assign.py) both read it;
the engine is never imported here.

The expected list of a vector is always oracle.knn(metric, x, cen, 1)[1][:, 0]; -1 means "not stored".  The expected lists are the
numpy restatement of IndexIVFFlat::add_core below (Model): append in input order, id = xids[i] or ntotal_before + i, a skipped vector
still counts into ntotal.

A case is a Case: centroids and a sequence of adds (x, xids or None).  An add that does not pass the gate of the matrix-core ranking
(takes_pick) must leave amd_ivf_last_coarse_pick at 0; one that passes it must leave it above 0 where `picks` is set (it is not
where every ranking may come back flagged: no usable fp16 scale, ties everywhere).  `empty_ok`: lists may stay empty (more lists than vectors, a
metric or data under which nothing promises every list a vector).  `tied`: how many rankings of the first add tie for the first
place, where the case promises a number."""
import collections
import functools

import numpy as np

PICK_MIN_N, PICK_MIN_NLIST, PICK_MAX_NLIST = 256, 68, 4096  # coarse_dev's gate at nprobe = 1: n >= 256, 4 * 1 + 64 <= nlist <= 4096
ADD_BLOCK = 1 << 18                                          # amd_ivf_add ranks in blocks of this many vectors

Case = collections.namedtuple("Case", "name metric cen adds picks empty_ok tied")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _case(name, metric, cen, adds, picks=True, empty_ok=False, tied=None):
    cen = np.ascontiguousarray(cen, dtype=np.float32)
    adds = tuple((np.ascontiguousarray(x, dtype=np.float32), None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)) for x, ids in adds)
    _freeze(cen, *[a for pair in adds for a in pair])
    return Case(name, metric, cen, adds, picks, empty_ok, tied)


def takes_pick(n, nlist):
    return n >= PICK_MIN_N and PICK_MIN_NLIST <= nlist <= PICK_MAX_NLIST


# ------------------------------------------------------------------------------------------ the model
def expected_keys(metric, x, cen, nthreads=1):
    from oracle import pyoracle
    return pyoracle.knn(metric, x, cen, 1, nthreads=nthreads)[1][:, 0].copy()


class Model:
    """the lists as IndexIVFFlat::add_core keeps them"""

    def __init__(self, nlist, d):
        self.nlist, self.d, self.ntotal = nlist, d, 0
        self.rows = [[] for _ in range(nlist)]  # (chunks of rows, joined when read)
        self.idl = [[] for _ in range(nlist)]

    def add(self, x, xids, keys):
        keys = np.asarray(keys, dtype=np.int64)
        ids = np.asarray(xids, dtype=np.int64) if xids is not None else self.ntotal + np.arange(len(x), dtype=np.int64)
        for l in np.unique(keys[keys >= 0]):
            m = keys == l  # (a boolean mask keeps input order)
            self.rows[l].append(x[m])
            self.idl[l].append(ids[m])
        self.ntotal += len(x)

    def codes(self, l):
        return np.concatenate(self.rows[l]) if self.rows[l] else np.empty((0, self.d), np.float32)

    def ids(self, l):
        return np.concatenate(self.idl[l]) if self.idl[l] else np.empty(0, np.int64)

    def sizes(self):
        return np.array([sum(len(c) for c in self.idl[l]) for l in range(self.nlist)], dtype=np.int64)

    def flat(self):
        """-> (rows, list numbers, ids) list by list: what oracle.Lists and Handle.set_lists_from_assign take"""
        sz = self.sizes()
        return (np.concatenate([self.codes(l) for l in range(self.nlist)]).astype(np.float32).reshape(-1, self.d),
                np.repeat(np.arange(self.nlist, dtype=np.int64), sz), np.concatenate([self.ids(l) for l in range(self.nlist)]))


def model_of(case, seed=None, nthreads=1):
    """the expected lists after every add of the case (seed: rows added before them, see seed_rows)"""
    m = Model(*case.cen.shape)
    if seed is not None:
        m.add(seed, None, expected_keys(case.metric, seed, case.cen))
    for x, ids in case.adds:
        m.add(x, ids, expected_keys(case.metric, x, case.cen, nthreads))
    return m


def seed_rows(case):
    """rows that make an index more than four times as long as everything the case adds -- a journal that writes at most a quarter of
    the entries is applied in place (apply_journal) --: copies of the first sixteen centroids, which are finite whatever the case adds"""
    n = 4 * sum(len(x) for x, _ in case.adds) + 1
    return np.ascontiguousarray(case.cen[(7 * np.arange(n)) % min(16, len(case.cen))])


def finite_queries(case, nq=32):
    """up to nq finite rows of what the case adds, from its front and its end: the queries of the search check"""
    x = np.concatenate([x for x, _ in case.adds])
    x = x[np.isfinite(x).all(axis=1)]
    out = np.concatenate([x[:nq // 2], x[-(nq - nq // 2):]]) if len(x) > nq else x
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------ gate edges
GATE_N = (255, 256, 257)
GATE_NLIST = (67, 68, 4096, 4097)
GATE_D = (4, 8, 30, 64)


@functools.lru_cache(maxsize=None)
def gate_case(kind, metric, n, nlist):
    """one add of n vectors against nlist centroids, on both sides of every term of the gate.  The first min(n / 2, nlist) vectors lie next
    to one centroid each, the others half way between two: the best and the second-best centroid of those differ by little."""
    d = GATE_D[(GATE_N.index(n) + GATE_NLIST.index(nlist) + (kind == "bytes")) % 4]
    rs = np.random.RandomState(1000 * n + nlist + 7 * metric + (kind == "bytes"))
    near = np.arange(min(n // 2, nlist))
    a, b = rs.randint(0, nlist, n - len(near)), rs.randint(0, nlist, n - len(near))
    if kind == "bytes":
        cen = rs.randint(0, 256, size=(nlist, d)).astype(np.float32)
        x = np.concatenate([cen[near] + rs.randint(-3, 4, size=(len(near), d)),
                            np.floor((cen[a] + cen[b]) / 2) + rs.randint(-1, 2, size=(len(a), d))])
        x = np.clip(x, 0, 255)
    else:
        pool = rs.randn(nlist, d)
        if metric == 0:
            pool /= np.linalg.norm(pool, axis=1, keepdims=True)
        cen = (pool + 1e-3 * rs.randn(nlist, d)).astype(np.float32)  # centroids = jittered samples
        x = np.concatenate([pool[near] + 0.02 * rs.randn(len(near), d), (pool[a] + pool[b]) / 2 + 2e-3 * rs.randn(len(a), d)])
    return _case(f"gate-{kind}-m{metric}-n{n}-nl{nlist}", metric, cen, [(x, None)],
                 empty_ok=nlist > n or metric == 0)  # (4096 / 4097 lists: at least nlist - n stay empty; IP: the longest centroids take all)


GATE_CASES = [(kind, metric, n, nlist) for kind in ("float", "bytes") for metric in (1, 0) for n in GATE_N for nlist in GATE_NLIST]


# ------------------------------------------------------------------------------------------ ties
TIE_N, TIE_NLIST, TIE_D = 300, 96, 8
TIE_COUNTS = (1, 7, 8, 9)  # on both sides of the flagged list's padding to a multiple of eight


def _tie_table(rs):
    """small integers; centroid 1 is a copy of centroid 0, centroids 2 and 3 differ by two in the first coordinate (-1 and +1) and in
    nothing else.  Both pairs are long vectors, so that under IP their multiples rank them first."""
    while True:
        cen = rs.randint(-8, 9, size=(TIE_NLIST, TIE_D)).astype(np.float32)
        cen[0] = 8 * rs.choice([-1, 1], TIE_D)
        cen[1] = cen[0]
        cen[2] = 8 * rs.choice([-1, 1], TIE_D)
        cen[3] = cen[2]
        cen[2, 0], cen[3, 0] = -1, 1
        if len(np.unique(cen, axis=0)) == TIE_NLIST - 1 and abs(float(cen[0] @ cen[2])) < 200:
            return cen


def _top2(metric, x, cen):
    from oracle import pyoracle
    return pyoracle.knn(metric, x, cen, 2)[0]


@functools.lru_cache(maxsize=None)
def tie_case(metric, count, where):
    """300 vectors of which exactly `count` tie for the first place, by the reference's own distances (the builder draws candidates and
    keeps what the oracle's k = 2 distances say): next to the duplicated centroid, at equal distance from the two distinct ones
    (small integers: the distances are exact) and, under IP, the all-zero vector.  where: "first" puts the first tied vector at index
    0, "last" puts the last one at the last index; the others are spread in between.  The other vectors are reals around centroids."""
    rs = np.random.RandomState(500 + 10 * count + metric + 3 * (where == "last"))
    cen = _tie_table(rs)
    m = 40 * count + 40
    if metric == 1:
        dup = cen[0] + rs.randint(-1, 2, size=(m, TIE_D))
        mid = cen[2] + rs.randint(-1, 2, size=(m, TIE_D))
        mid[:, 0] = 0              # (half way between centroids 2 and 3 in the one coordinate in which they differ)
    else:
        dup = cen[0] * rs.randint(2, 6, size=(m, 1)) + rs.randint(-1, 2, size=(m, TIE_D))
        mid = cen[2] * rs.randint(2, 6, size=(m, 1)) + rs.randint(-1, 2, size=(m, TIE_D))
        mid[:, 0] = 0              # (orthogonal to the difference of centroids 2 and 3)
    cand = np.empty((2 * m, TIE_D), np.float32)
    cand[0::2], cand[1::2] = dup, mid
    if metric == 0:
        cand = np.concatenate([np.zeros((1, TIE_D), np.float32), cand])  # (every inner product of the zero vector is 0)
    cand = cand[np.sort(np.unique(cand, axis=0, return_index=True)[1])]
    D = _top2(metric, cand, cen)
    tied = cand[D[:, 0] == D[:, 1]][:count]
    assert len(tied) == count, (metric, count, len(tied))
    free = (cen[rs.randint(4, TIE_NLIST, size=3 * TIE_N)] * (1.0 if metric == 1 else 3.0) + 0.3 * rs.randn(3 * TIE_N, TIE_D)).astype(np.float32)
    D = _top2(metric, free, cen)
    free = free[D[:, 0] != D[:, 1]][:TIE_N - count]
    assert len(free) == TIE_N - count
    pos = np.unique(np.linspace(0, TIE_N - 1, count).astype(np.int64)) if count > 1 else np.array([0 if where == "first" else TIE_N - 1])
    if where == "first" and count > 1:
        pos[-1] = TIE_N - 2
    if where == "last" and count > 1:
        pos[0] = 1
    assert len(pos) == count
    x = np.empty((TIE_N, TIE_D), np.float32)
    mask = np.zeros(TIE_N, bool)
    mask[pos] = True
    x[mask], x[~mask] = tied, free
    return _case(f"tie-m{metric}-{count}-{where}", metric, cen, [(x, None)], empty_ok=True, tied=count)  # (list 1 at least: of the duplicated centroids the heap names 0)


@functools.lru_cache(maxsize=None)
def zero_table_case():
    """IP against an all-zero centroid table: every distance of every vector is 0, every ranking ties (and is flagged)"""
    rs = np.random.RandomState(77)
    x = rs.randint(-8, 9, size=(TIE_N, TIE_D)).astype(np.float32)
    return _case("tie-zero-table", 0, np.zeros((TIE_NLIST, TIE_D), np.float32), [(x, None)], picks=False, empty_ok=True,
                 tied=TIE_N)  # (all distances equal: the heap names one list for every vector, 95 stay empty)


TIE_CASES = [(metric, count, where) for metric in (1, 0) for count in TIE_COUNTS for where in ("first", "last")]


# ------------------------------------------------------------------------------------------ non-finite
@functools.lru_cache(maxsize=None)
def nonfinite_case(metric, n):
    """reals around 96 centroids, among them vectors with one NaN, +inf or -inf component (the first, one in the middle, the last
    vector among them) and an all-zero vector.  Under L2 every distance of such a vector is NaN or +inf and the reference's heap admits
    none: the vector is not stored.  Under IP a +-inf component gives +-inf products, of which the heap admits +inf.
    picks is off: the matrix x holds a non-finite value, so it has no fp16 scale and, at the default "coarse_pick" 2, every ranking
    comes back flagged.  The flag that coarse_pick_kernel sets for a single non-finite ranking is reached with "coarse_pick" 1 (fp32
    operands, no scale): test_gpu_add_assign.py adds the 300-vector cases that way too."""
    d, nlist = 8, TIE_NLIST
    rs = np.random.RandomState(900 + n + metric)
    cen = rs.randn(nlist, d).astype(np.float32)
    x = (cen[np.arange(n) % nlist] * (1.0 if metric == 1 else 3.0) + 0.3 * rs.randn(n, d)).astype(np.float32)
    x[0, 3] = np.nan
    x[n // 2, 0] = np.inf
    x[n // 2 + 1, d - 1] = -np.inf
    x[n // 2 + 2] = 0.0
    x[n // 3, 5] = np.inf
    x[n // 3, 6] = np.nan
    x[n - 1, 1] = np.inf if metric == 0 else np.nan
    return _case(f"nonfinite-m{metric}-n{n}", metric, cen, [(x, None)], picks=False, empty_ok=True)  # (n = 17: fewer vectors than lists; skipped vectors)


NONFINITE_CASES = [(metric, n) for metric in (1, 0) for n in (300, 17)]


@functools.lru_cache(maxsize=None)
def nonfinite_bytes_case(n):
    """byte-valued vectors (integers 0 .. 255, L2) around byte-valued centroids, three of them with a NaN or infinite component: those
    are not stored, and the lists that result hold bytes only -- they must get their byte codes as the same lists given whole do"""
    d, nlist = 8, TIE_NLIST
    rs = np.random.RandomState(950 + n)
    cen = rs.randint(20, 236, size=(nlist, d)).astype(np.float32)
    x = np.clip(cen[np.arange(n) % nlist] + rs.randint(-9, 10, size=(n, d)), 0, 255).astype(np.float32)
    x[0, 2] = np.nan
    x[n // 2, 7] = np.inf
    x[n - 1, 0] = -np.inf
    return _case(f"nonfinite-bytes-n{n}", 1, cen, [(x, None)], picks=False, empty_ok=True)  # (n = 17: fewer vectors than lists)


# ------------------------------------------------------------------------------------------ ids
@functools.lru_cache(maxsize=None)
def ids_case(metric):
    """three adds without ids (300, 5 and 256 vectors: the ids go on from ntotal), then one with ids of its own, not in order and
    partly above 2^32"""
    d, nlist = 30, TIE_NLIST
    rs = np.random.RandomState(1300 + metric)
    cen = rs.randn(nlist, d).astype(np.float32)
    draw = lambda n: (cen[rs.randint(0, nlist, n)] * (1.0 if metric == 1 else 3.0) + 0.3 * rs.randn(n, d)).astype(np.float32)
    own = (rs.permutation(40).astype(np.int64) + 1) * 1000003 + 7
    own[::3] += (1 << 32) + (1 << 40)
    own[5] = (1 << 62) + 1
    x0 = draw(300)
    x0[:nlist] = cen + np.float32(0.01)  # (no list stays empty)
    return _case(f"ids-m{metric}", metric, cen, [(x0, None), (draw(5), None), (draw(256), None), (draw(40), own)],
                 empty_ok=metric == 0)  # (IP: nothing promises a short centroid a vector)


# ------------------------------------------------------------------------------------------ the block edge
BLOCK_D = 4
BLOCK_CASES = [(1, 68), (0, 16)]  # (metric, nlist): the picked path / the exact path (fewer than 68 lists)


@functools.lru_cache(maxsize=None)
def block_case(metric, nlist):
    """2^18 + 3 byte-valued vectors of four dimensions in one call: one full block of amd_ivf_add and a second one of three vectors"""
    rs = np.random.RandomState(1700 + nlist)
    cen = rs.randint(0, 256, size=(nlist, BLOCK_D)).astype(np.float32)
    x = rs.randint(0, 256, size=(ADD_BLOCK + 3, BLOCK_D)).astype(np.float32)
    return _case(f"block-m{metric}-nl{nlist}", metric, cen, [(x, None)], empty_ok=metric == 0)  # (IP over bytes: the few longest centroids take every vector)


@functools.lru_cache(maxsize=None)
def block_keys(metric, nlist):
    """the oracle's list numbers of the block case, computed once"""
    c = block_case(metric, nlist)
    k = expected_keys(metric, c.adds[0][0], c.cen, nthreads=8)
    _freeze(k)
    return k


# ------------------------------------------------------------------------------------------ the history
@functools.lru_cache(maxsize=None)
def history_case(metric):
    """three adds of 300, 17 and 300 vectors for one handle that also ranks (coarse) and searches in between"""
    d, nlist = 30, TIE_NLIST
    rs = np.random.RandomState(2100 + metric)
    cen = rs.randn(nlist, d).astype(np.float32)
    draw = lambda n: (cen[rs.randint(0, nlist, n)] * (1.0 if metric == 1 else 3.0) + 0.3 * rs.randn(n, d)).astype(np.float32)
    return _case(f"history-m{metric}", metric, cen, [(draw(300), None), (draw(17), None), (draw(300), None)], empty_ok=True)  # (random draws of 96 lists)


def small_cases():
    """every case but the block edge, by name"""
    out = [gate_case(*a) for a in GATE_CASES] + [tie_case(*a) for a in TIE_CASES] + [zero_table_case()]
    out += [nonfinite_case(*a) for a in NONFINITE_CASES] + [nonfinite_bytes_case(n) for n in (300, 17)] + [ids_case(m) for m in (1, 0)]
    return collections.OrderedDict((c.name, c) for c in out)
