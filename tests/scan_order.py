"""Index contents whose rows reach a scan in a chosen key order (NumPy and the tests' own
references only), for tests/test_gpu_scan_order.py, tests/test_gpu_exact_scan_order.py and
their preconditions in tests/test_scan_order_cpu.py.

Every scan of the library prunes on a running bound, so which of its branches run depends on
the order in which the keys arrive.  For one *designated query* the builders here return
lists whose keys (the L2 distance, or the negated similarity for the inner product) are
pairwise distinct in fp32, and ids that ascend with the wanted position: the device image of
a list is sorted by label, so the scan meets the rows in exactly that order.

`improving`  keys strictly decrease with the label: every row beats every row before it.
`worsening`  keys strictly increase with the label: the first k rows are the result.
`one_wave`   the rows i with (i >> 6) & 3 == 0 -- the chunks of wave 0 of a 256-row pass, in
             the IVF-PQ and in the exact scans alike -- hold the best keys, improving among
             themselves; all other rows are worse than all of them, in worsening order.

IVF-PQ: centroids are integers in [-3, 3], the codebook integers in [-2, 2]; sub-quantizer 0's
entry j is (j, 0, ...), sub-quantizer 1's is (j, 0, ...) for L2 and (256 j, 0, ...) for the
inner product, where the designated query has 1 in the two matching coordinates.  All other
code bytes are random.  Exact scans: two wide coordinates in 0..255, small integers elsewhere,
coordinate 2 + l largest in the rows of list l (centroid l is 8 e_(2+l), so that both metrics
assign the row to it).  Every term and partial sum is an integer below 2^24, exact in fp32 in
any order; the 8-bit scalar quantizers decode to non-integers, so there the rows are ordered
by the key the reference (tests/indexsq_ref.py, tests/ivfsq_ref.py) computes.

Four times the rows needed are drawn, one row per distinct fp32 key is kept, and the kept
rows are sorted into the order.  A batch is five copies of the designated query (a G = 4 item
whose four pairs overflow their queues in the same chunk, and a second item of one pair) and
random integer queries, which see the same lists in an unrelated order.
"""
import zlib
from types import SimpleNamespace

import numpy as np

L2, IP = "l2", "ip"
ORDERS = ("improving", "worsening", "one_wave")
SIZES = (4700, 1537, 300, 0)   # a little over 3 (JB = 6) and 4.5 (JB = 4) super-batches and two row
                               # ranges; one JB = 6 super-batch + 1; fewer rows than k = 400; empty
N_SAME, N_RANDOM = 5, 8
DRAW = 4                       # candidates drawn per row kept
F = np.float32

PQ_SHAPES = {"d32_m8": (32, 8), "d64_m16": (64, 16), "d64_m32": (64, 32), "d96_m48": (96, 48),
             "d128_m64": (128, 64)}
EXACT_D = 36                   # one staged step of 32 and the 4-wide remainder


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def wave0(n):
    """The positions of a list that wave 0 of a 256-row pass scans."""
    return (np.arange(n) >> 6) & 3 == 0


def ranks(n, order):
    """r[i]: the rank (0 = best key) of the row at position i of a list of n rows."""
    i = np.arange(n)
    if order == "improving":
        return n - 1 - i
    if order == "worsening":
        return i
    assert order == "one_wave", order
    w = wave0(n)
    n0 = int(w.sum())
    r = np.empty(n, np.int64)
    r[w] = n0 - 1 - np.arange(n0)
    r[~w] = n0 + np.arange(n - n0)
    return r


def arrange(keys, n, order, rng):
    """Of the candidates with fp32 keys `keys`, n with pairwise distinct keys, as candidate
    numbers in position order.  Fewer than n distinct keys is an error."""
    keys = np.asarray(keys)
    assert keys.dtype == F
    _, first = np.unique(keys, return_index=True)  # ascending key
    if len(first) < n:
        raise ValueError(f"{len(first)} distinct keys among {len(keys)} candidates, {n} wanted")
    kept = first[np.sort(rng.permutation(len(first))[:n])]  # still ascending key
    return kept[ranks(n, order)]


def expected_ids(ids, order, k):
    """The designated query's result over one list with labels `ids` in position order."""
    ids = np.asarray(ids)
    if order == "improving":
        return ids[::-1][:k]
    if order == "worsening":
        return ids[:k]
    return ids[np.argsort(ranks(len(ids), order))][:k]


def list_ids(j, n):
    """Labels of the j-th list's rows in position order: ascending, with gaps."""
    return 1_000_000 * (j + 1) + 3 * np.arange(n, dtype=np.int64)


def queries(rng, q, n_random=N_RANDOM, lo=-3, hi=4):
    xq = rng.integers(lo, hi, size=(N_SAME + n_random, len(q))).astype(F)
    xq[:N_SAME] = q
    return xq


# ---------------------------------------------------------------- IVF-PQ
def pq_keys(cent_l, cb, q, codes, metric):
    """float64 keys of the rows `codes` of a list with centroid cent_l for query q."""
    M = cb.shape[0]
    y = cb[np.arange(M)[None, :], codes].reshape(len(codes), cent_l.shape[0]).astype(np.float64) + cent_l.astype(np.float64)
    q = q.astype(np.float64)
    return -(y @ q) if metric == IP else ((q - y) ** 2).sum(1)


def pq_contents(shape, metric, order, nlist=4, place=(0, 1, 2, 3), sizes=SIZES):
    """An IVF-PQ index of `nlist` lists of which place[j] holds sizes[j] rows in `order`."""
    d, M = PQ_SHAPES[shape]
    dsub = d // M
    rng = np.random.default_rng(seed_of("pq", shape, metric, order, nlist))
    cent = rng.integers(-3, 4, size=(nlist, d)).astype(F)
    cb = rng.integers(-2, 3, size=(M, 256, dsub)).astype(F)
    cb[:2] = 0
    cb[0, :, 0] = np.arange(256)
    cb[1, :, 0] = np.arange(256) * (256 if metric == IP else 1)
    q = rng.integers(-3, 4, size=d).astype(F)
    if metric == IP:
        q[0] = q[dsub] = 1
    c = SimpleNamespace(d=d, M=M, metric=metric, order=order, nlist=nlist, place=tuple(place), sizes=tuple(sizes),
                        cent=cent, cb=cb, q=q, xq=queries(rng, q), keys=[], list_ids=[])
    list_no, codes, ids = [], [], []
    for j, n in enumerate(sizes):
        cand = rng.integers(0, 256, size=(DRAW * n, M), dtype=np.uint8)
        k64 = pq_keys(cent[place[j]], cb, q, cand, metric)
        pos = arrange(k64.astype(F), n, order, rng)
        c.keys.append(k64[pos])
        c.list_ids.append(list_ids(j, n))
        list_no.append(np.full(n, place[j], np.int64))
        codes.append(cand[pos])
        ids.append(c.list_ids[j])
    c.list_no, c.ids = np.concatenate(list_no), np.concatenate(ids)
    c.codes = np.ascontiguousarray(np.concatenate(codes))
    return c


def dis0(c, xq, rows):
    """What a preassigned L2 search is given per probe: |x - centroid|^2, an exact integer
    (None for the inner product, where the scan forms <x, centroid> itself)."""
    if c.metric == IP:
        return None
    cc = c.cent[np.maximum(rows, 0)].astype(np.float64)
    d2 = ((xq[:, None, :].astype(np.float64) - cc) ** 2).sum(-1)
    assert d2.max() < 2 ** 24
    return np.where(rows >= 0, d2, 0).astype(F)


def probe_rows(c, nq, which):
    """[nq][len(which)] probes: the lists place[j], j in which, for every query."""
    return np.tile(np.asarray([c.place[j] for j in which], np.int64), (nq, 1))


# ---------------------------------------------------------------- the exact scans
def exact_centroids(d=EXACT_D):
    cent = np.zeros((len(SIZES), d), F)
    for l in range(len(SIZES)):
        cent[l, 2 + l] = 8
    return cent


def exact_candidates(rng, n, l, d=EXACT_D):
    x = rng.integers(-3, 4, size=(n, d)).astype(F)
    x[:, :2] = rng.integers(0, 256, size=(n, 2))
    x[:, 2 + l] = 8
    return x


def exact_query(rng, metric, d=EXACT_D):
    q = rng.integers(-3, 4, size=d).astype(F)
    if metric == IP:
        q[0], q[1] = 1, 256
    return q


def exact_keys64(q, x, metric):
    q, x = q.astype(np.float64), x.astype(np.float64)
    return -(x @ q) if metric == IP else ((q - x) ** 2).sum(1)


def exact_lists(tag, metric, order, keyfn=None, sizes=SIZES, n_random=N_RANDOM):
    """Rows for the lists of sizes `sizes` (list l around exact_centroids()[l]), each in
    `order` for the designated query by keyfn(q, l, candidates) -> fp32 keys (default: the
    exact integer key).  xb, ids and list_of hold the rows list after list, in position order."""
    rng = np.random.default_rng(seed_of("exact", tag, metric, order, sizes))
    q = exact_query(rng, metric)
    c = SimpleNamespace(metric=metric, order=order, sizes=tuple(sizes), cent=exact_centroids(), q=q,
                        xq=queries(rng, q, n_random), keys=[], list_ids=[])
    xb, ids, list_of = [], [], []
    for l, n in enumerate(sizes):
        cand = exact_candidates(rng, DRAW * n, l)
        keys = exact_keys64(q, cand, metric).astype(F) if keyfn is None else np.asarray(keyfn(q, l, cand), F)
        pos = arrange(keys, n, order, rng)
        c.keys.append(keys[pos].astype(np.float64))
        c.list_ids.append(list_ids(l, n))
        xb.append(cand[pos])
        ids.append(c.list_ids[l])
        list_of.append(np.full(n, l, np.int64))
    c.xb, c.ids, c.list_of = np.concatenate(xb), np.concatenate(ids), np.concatenate(list_of)
    return c


def sq_trained_8bit(d=EXACT_D):
    """sq.trained of QT_8bit, [vmin (d), vdiff (d)], fixed by hand so that a row's code does not
    depend on which rows are kept: [0, 255] for the wide coordinates, [-3, 8] elsewhere (a
    residual below -3 is clamped).  The decoded values are no integers."""
    vmin, vdiff = np.full(d, -3, F), np.full(d, 11, F)
    vmin[:2], vdiff[:2] = 0, 255
    return np.concatenate([vmin, vdiff])


# ---------------------------------------------------------------- one case per exact index
def metric_id(metric):
    """faiss's METRIC_INNER_PRODUCT / METRIC_L2, as the references take it."""
    return 0 if metric == IP else 1


def ivfflat_case(metric, order):
    return exact_lists("ivfflat", metric, order)


def ivfsq_case(qtype, by_residual, metric, order):
    """c.trained is the quantizer's table; the keys are tests/ivfsq_ref.py's for the designated
    query (for the inner product with by_residual: its <q, centroid> added, in fp32)."""
    import ivfsq_ref as R

    cent = exact_centroids()
    trained = sq_trained_8bit() if qtype == R.QT_8BIT else np.zeros(0, F)

    def keyfn(q, l, cand):
        ref = R.Ref(cand, cent, qtype, metric_id(metric), by_residual, trained=trained)
        assert (ref.list_of == l).all()
        dis = ref.pair(q, l, F(np.dot(q.astype(np.float64), cent[l].astype(np.float64))))
        return -dis if metric == IP else dis

    c = exact_lists(("ivfsq", qtype, by_residual), metric, order, keyfn)
    c.qtype, c.by_residual, c.trained = qtype, by_residual, trained
    return c


def sq_case(qtype, nb, metric, order):
    """An IndexScalarQuantizer of nb rows in `order` as a whole; keys from tests/indexsq_ref.py."""
    import indexsq_ref as S

    trained = sq_trained_8bit() if qtype == S.QT_8BIT else np.zeros(0, F)

    def keyfn(q, l, cand):
        dis = S.Ref(cand, qtype, metric_id(metric), trained).dist(q[None])[0]
        return -dis if metric == IP else dis

    c = exact_lists(("sq", qtype), metric, order, keyfn, sizes=(nb,))
    c.qtype, c.trained = qtype, trained
    return c


def flat_case(nb, nq, metric, order):
    """An IndexFlat of nb rows in `order` as a whole, and nq queries."""
    return exact_lists("flat", metric, order, sizes=(nb,), n_random=nq - N_SAME)
