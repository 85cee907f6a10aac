"""Every host-side batch split of search, add and train ("Host-side splits"), reached
with batches that the library cuts into chunks, against the references the indexes' own test
files use: labels, distances, lists, codes and trained tables are compared bit for bit.

The cut comes from the library (``faiss_amd.index.ivf_search_split``, ``sq_search_plan``,
``flat_search_plan``, ``ivf_pass_rows``, ``kmeans_assign_rows``, ``host_pass_rows``,
``flat_search_query_chunk``): every case asserts from it that its batch goes in two full chunks
and a short last one (``cut``), so that a changed constant makes the case fail, not pass in one
chunk.  Three loops take one full chunk and a short one, because their batch cannot grow: the
scalar quantizer's training of IndexIVFScalarQuantizer uses at most 100 000 rows (one pass of 65 536
and one of 34 464), and the d = 2048 rows of the staging buffers are one shared 268 MB fixture.

Two conditions are asserted on every expected search result before the GPU's is looked at:

* shifted pointers (``assert_shifted``): at every in-chunk position the expected D row and the
  expected I row differ from those at the same position of the chunk before, so that an input
  pointer that is not advanced, or an output written at the first chunk's offset, shows;
* stale bounds (``assert_bound_grows``, the scans that share a bound per query: IVF-Flat, IVF-SQ,
  IndexScalarQuantizer, IndexFlat): the k-th key (distance, or negated similarity) at every in-chunk
  position exceeds the one at the same position of the chunk before, so that a bound left over
  from that chunk prunes true results.  L2 queries lie farther from the base chunk by chunk; inner
  product data are non-negative and the queries are scaled down chunk by chunk.  A position whose
  predecessor has fewer than k results is left out: such a query never sets its bound.

Labels are a permutation with gaps.  In the k = 10 cases most probed lists are empty and one
query per chunk has fewer candidates than k.

IVF-PQ's own two splits have a case each as well, for no existing test holds them to a
reference.  Its query chunk (1048 queries at k = 1000 and nprobe 32, 4096 at M = 64) is above every
batch the suite searches (128 queries at C3, 1024 at k = 10).  Its add passes (65 536 rows at nlist
1024) are taken sixteen times by the ``sift1m`` fixture of tests/test_gpu_configs.py, which adds
1e6 rows in one call, but ``test_c2_encode_parity_and_result_shape`` compares the first 20 000 rows
with the oracle's encoding, all of the first pass, and the searches there run against an oracle
that is given the GPU's lists.
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import indexflat_ref as FL
import indexsq_ref as SQ
import ivfflat_ref as RF
import ivfsq_ref as RS
from faiss_amd import _lib
from faiss_amd import index as fidx
from oracle import oracle as O

pytestmark = pytest.mark.gpu

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
F = np.float32
FMAX = np.finfo(np.float32).max
QT_FP16, QT_8BIT = SQ.QT_FP16, SQ.QT_8BIT
# the index kinds of the IVF cases: (name, qtype or None for IVF-Flat, by_residual)
FLAT, SQ8, SQ8R, SQ16 = ("flat", None, False), ("sq8", QT_8BIT, False), ("sq8r", QT_8BIT, True), ("sq16", QT_FP16, False)
SEARCH_KINDS = [pytest.param(k, id=k[0]) for k in (FLAT, SQ8, SQ8R)]
ADD_KINDS = [pytest.param(k, id=k[0]) for k in (FLAT, SQ8R, SQ16)]


# ----------------------------------------------------------------- the cut and the conditions
def cut(n, chunk, full=2):
    """The chunks [q0, q1) of a batch of n taken `chunk` at a time: `full` full ones and a short one."""
    assert chunk >= 1 and full * chunk < n < (full + 1) * chunk, (n, chunk)
    return [(q0, min(n, q0 + chunk)) for q0 in range(0, n, chunk)]


def pairs(chunks):
    """(rows of the chunk before, rows of the chunk) at the same in-chunk positions."""
    return [(slice(a0, a0 + b1 - b0), slice(b0, b1)) for (a0, _), (b0, b1) in zip(chunks, chunks[1:])]


def assert_shifted(want, chunks):
    D, I = want
    for prev, cur in pairs(chunks):
        assert (I[cur] != I[prev]).any(1).all() and (D[cur] != D[prev]).any(1).all()


def assert_bound_grows(want, chunks, metric):
    last = want[0][:, -1].astype(np.float64)
    key = -last if metric == IP else last  # a missing k-th result: +FMAX
    for prev, cur in pairs(chunks):
        has_bound = key[prev] < FMAX
        assert has_bound.sum() * 2 > has_bound.size and (key[cur][has_bound] > key[prev][has_bound]).all()


def conditions(want, chunks, metric):
    assert_shifted(want, chunks)
    assert_bound_grows(want, chunks, metric)


def check(got, want):
    D, I = got
    np.testing.assert_array_equal(np.asarray(I), want[1])
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.tobytes() == want[0].tobytes(), np.abs(D - want[0]).max()


def gapped_ids(seed, n):
    return (np.random.default_rng(seed).permutation(3 * n)[:n]).astype(np.int64) + 11


def device_search(ix, xq, k, Iq=None, Dq=None):
    """search_device / search_preassigned_device into outputs the caller owns (prefilled)."""
    import torch

    tx = torch.from_numpy(xq).cuda()
    D = torch.full((len(xq), k), float("nan"), dtype=torch.float32, device="cuda")
    I = torch.full((len(xq), k), -7, dtype=torch.int64, device="cuda")
    if Iq is None:
        rD, rI = ix.search_device(tx, k, D=D, I=I)
    else:
        rD, rI = ix.search_preassigned_device(tx, k, torch.from_numpy(Iq).cuda(), torch.from_numpy(Dq).cuda(), D=D, I=I)
    torch.cuda.synchronize()
    assert rD.data_ptr() == D.data_ptr() and rI.data_ptr() == I.data_ptr()
    return D.cpu().numpy(), I.cpu().numpy()


def slots(sizes, nprobe):
    """The row ranges of the nprobe longest lists: the bound the search plans with."""
    r = np.sort(-(-np.asarray(sizes) // RF.RANGE_ROWS))[::-1]
    return int(r[:nprobe].sum())


def make_ref(kind, xb, cent, metric, ids):
    _, qtype, by_residual = kind
    if qtype is None:
        return RF.Ref(xb, cent, metric, ids)
    return RS.Ref(xb, cent, qtype, metric, by_residual, ids)


def make_index(kind, ref, d, nlist, metric):
    _, qtype, by_residual = kind
    if qtype is None:
        ix = faiss.IndexIVFFlat(None, d, nlist, metric)
        ix.set_trained(ref.cent)
    else:
        ix = faiss.IndexIVFScalarQuantizer(None, d, nlist, qtype, metric, by_residual)
        ix.set_trained(ref.cent, ref.trained)
    return ix


def entry_bytes(kind):
    return 12 if kind[2] else 8


# ------------------------------------------ 1a / 1b: IvfLists::search_dev (IVF-Flat, IVF-SQ)
SCALE = {L2: (1.1, 1.3, 1.5), IP: (1.0, 0.6, 0.36)}  # of the queries of chunk 0, 1, 2


@functools.lru_cache(maxsize=None)
def sparse_base(metric):
    """1a: 65536 unit centroids in the non-negative orthant, 2 928 rows within 0.002 of 96 of
    them (80 lists of 36 rows, 16 of 3), so that nearly every probed list is empty."""
    rng = np.random.default_rng(101)
    nlist, d = 65536, 4
    cent = np.abs(rng.standard_normal((nlist, d))) + 0.05
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(F)
    hot = rng.choice(nlist, 96, replace=False)
    of = rng.permutation(np.repeat(hot, [36] * 80 + [3] * 16))
    xb = np.abs(cent[of] + 0.002 * rng.standard_normal((len(of), d))).astype(F)
    return cent, xb, gapped_ids(102, len(xb)), hot


def sparse_queries(metric, chunk):
    """2 chunk + 5 queries along the directions of lists that hold rows, scaled per chunk (L2: away
    from the unit sphere the rows lie on; inner product: down); in chunk c the query at position
    c + 1 points at a list of three rows."""
    cent, _, _, hot = sparse_base(metric)
    rng = np.random.default_rng(103)
    nq = 2 * chunk + 5
    # (another list at the same position of the next chunk: 17 further on among the 80)
    of = hot[(np.tile(rng.integers(0, 80, chunk), 3)[:nq] + 17 * (np.arange(nq) // chunk)) % 80]
    for c in range(3):
        of[c * chunk + c + 1] = hot[80 + c]
    scale = np.repeat(np.array(SCALE[metric], F), chunk)[:nq, None]
    return np.abs(cent[of] * scale + 0.0005 * rng.standard_normal((nq, 4))).astype(F)


@functools.lru_cache(maxsize=None)
def dense_base(metric):
    """1b (the data of test_many_partial_lists_merge_in_rounds at d = 4): 64 lists, all probed."""
    rng = np.random.default_rng(111)
    draw = (lambda n: rng.random((n, 4))) if metric == IP else (lambda n: rng.standard_normal((n, 4)))
    xb, cent = draw(6000).astype(F), draw(64).astype(F)
    if metric == IP:  # unit centroids: the largest inner product is the nearest direction, and no list is empty
        cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(F)
    return cent, xb, gapped_ids(112, len(xb))


def spread_queries(seed, metric, nq, chunk, d=4):
    """Queries of three chunks: L2 around 0, 1.5 and 3 in every coordinate (the base is standard
    normal); inner product in [0.5, 1) scaled by 1, 0.4, 0.16 (the base is uniform in [0, 1))."""
    rng = np.random.default_rng(seed)
    step = np.repeat(np.arange(3, dtype=F), chunk)[:nq, None]
    if metric == IP:
        return ((0.5 + 0.5 * rng.random((nq, d))) * F(0.4) ** step).astype(F)
    return (0.3 * rng.standard_normal((nq, d)) + 1.5 * step).astype(F)


@functools.lru_cache(maxsize=None)
def ivf_search_case(row, kind, metric):
    """(reference, queries, chunks, k, nprobe, Iq, Dq, expected of search, expected of
    search_preassigned), the conditions asserted on both expectations."""
    if row == "1a":
        nlist, k, nprobe = 65536, 10, 4
        cent, xb, ids, _ = sparse_base(metric)
    else:
        nlist, k, nprobe = 64, 1024, 64
        cent, xb, ids = dense_base(metric)
    ref = make_ref(kind, xb, cent, metric, ids)
    sizes = np.bincount(ref.list_of, minlength=nlist)
    if row == "1b":
        assert sizes.min() > 0 and sizes.max() < RF.RANGE_ROWS
    split = fidx.ivf_search_split(10 ** 6, nlist, k, nprobe, 4, slots(sizes, nprobe), entry_bytes(kind),
                                  kind[2] and metric == L2)
    chunk = split["query_chunk"]
    # which bound binds: the [chunk][nlist] entries (1a) or the partial lists (1b)
    assert chunk == ((1 << 28) // (nlist * entry_bytes(kind)) if row == "1a" else (1 << 31) // (split["S"] * k * 24))
    assert (split["S"], split["fan"]) == ((16, 16) if row == "1a" else (256, 2))
    nq = 2 * chunk + 5
    chunks = cut(nq, chunk)
    xq = sparse_queries(metric, chunk) if row == "1a" else spread_queries(113, metric, nq, chunk)
    Dc, Ic = O.coarse_search(xq, cent, nprobe, metric=metric)
    want = ref.search(xq, k, nprobe=nprobe)
    conditions(want, chunks, metric)
    # preassigned: a skipped probe and a repeated list in rows of every chunk, coarse values that
    # are not the quantizer's (three quarters of them; the repeat's own value must not be read)
    Iq, Dq = Ic.copy(), (F(0.75) * Dc).astype(F)
    for q0, _ in chunks:
        Iq[q0, 1] = -1
        Iq[q0 + 4, 3] = Iq[q0 + 4, 0]
        Dq[q0 + 4, 3] = 123.0
        if row == "1b":
            Iq[q0, [7, 20, 33]] = -1
    want_pre = ref.search(xq, k, Iq=Iq, Dq=Dq) if kind[1] is not None else ref.search(xq, k, Iq=Iq)
    conditions(want_pre, chunks, metric)
    if row == "1a":
        probed = sizes[Ic]
        for q0, q1 in chunks:
            assert (probed[q0:q1] == 0).any() and (want[1][q0:q1, -1] == -1).any() and (want[1][q0:q1, -1] >= 0).any()
    return ref, xq, chunks, k, nprobe, Iq, Dq, want, want_pre


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", SEARCH_KINDS)
@pytest.mark.parametrize("row", ["1a", "1b"])
def test_ivf_search_in_query_chunks(row, kind, metric):
    """1a: the [chunk][nlist] keys and buckets bound the chunk (nlist 65536: 512 queries, 341 with
    the probe column of by_residual).  1b: the partial lists do (k 1024, S 256: 341 queries).
    search, search_preassigned (Iq + q0 np, Dq + q0 np) and search_device into caller's outputs."""
    ref, xq, chunks, k, nprobe, Iq, Dq, want, want_pre = ivf_search_case(row, kind, metric)
    ix = make_index(kind, ref, 4, len(ref.cent), metric)
    ix.add_with_ids(ref.xb, ref.ids)
    ix.nprobe = nprobe
    check(ix.search(xq, k), want)
    check(ix.search_preassigned(xq, k, Iq, Dq), want_pre)
    check(device_search(ix, xq, k), want)
    check(device_search(ix, xq, k, Iq, Dq), want_pre)


# ---------------------------------------------- 2: ivfpq_sq_index::search_dev (IndexScalarQuantizer)
def topk_of(dis, k, metric):
    """indexsq_ref's top-k (the k smallest (key, label), labels = positions) of its distances
    dis [nq][nb], nb > k, by selection: a full sort of 1369 x 65537 keys takes 9 s."""
    key = -dis if metric == IP else dis
    kth = np.partition(key, k - 1, axis=1)[:, k - 1]
    D, I = np.empty((len(dis), k), F), np.empty((len(dis), k), np.int64)
    for q in range(len(dis)):
        cand = np.nonzero(key[q] <= kth[q])[0]  # ascending labels; at least k of them
        I[q] = cand[np.argsort(key[q][cand], kind="stable")[:k]]
        D[q] = dis[q][I[q]]
    return D, I


@functools.lru_cache(maxsize=None)
def sq_search_case(qtype, metric):
    nb, k = 65537, 1024
    chunk = fidx.sq_search_plan(10 ** 6, nb, k)["query_chunk"]
    assert chunk == (1 << 31) // (128 * k * 24) and fidx.sq_search_plan(10 ** 6, nb, k)["S"] == 128
    nq = 2 * chunk + 5
    chunks = cut(nq, chunk)
    assert fidx.sq_search_plan(nq, nb, k)["query_chunk"] == chunk
    rng = np.random.default_rng(121)
    xb = (rng.random((nb, 4)) if metric == IP else rng.standard_normal((nb, 4))).astype(F)
    xq = spread_queries(122, metric, nq, chunk)
    ref = SQ.Ref(xb, qtype, metric)
    want = topk_of(ref.dist(xq), k, metric)
    sample = np.concatenate([np.arange(q0, q0 + 3) for q0, _ in chunks])  # the reference's own sort, on nine rows
    check((want[0][sample], want[1][sample]), ref.search(xq[sample], k))
    conditions(want, chunks, metric)
    return xb, xq, ref.trained, k, want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", [pytest.param(QT_FP16, id="fp16"), pytest.param(QT_8BIT, id="8bit")])
def test_indexsq_search_in_query_chunks(qtype, metric):
    """k 1024 over 65537 codes: 17 row ranges, S 128, 682 queries per chunk of partial lists."""
    xb, xq, trained, k, want = sq_search_case(qtype, metric)
    ix = faiss.IndexScalarQuantizer(4, qtype, metric)
    ix.set_trained(trained)
    ix.add(xb)
    check(ix.search(xq, k), want)
    check(device_search(ix, xq, k), want)


# ---------------------------------------------------------- 3: flat_query_chunk (IndexFlat)
@functools.lru_cache(maxsize=None)
def flat_case(metric):
    nb, k, rows, nq = 3200, 1024, 128, 2731
    plan = fidx.flat_search_plan(nq, nb, k, rows)
    assert (plan["S"], plan["query_chunk"]) == (32, 1365)  # the limit (2^31 / (32 k 24) = 2730) halves 2731
    chunks = cut(nq, plan["query_chunk"])
    assert chunks[-1] == (2730, 2731)  # the last chunk keeps the plan of 1365 queries for one
    rng = np.random.default_rng(131)
    xb = (rng.random((nb, 4)) if metric == IP else rng.standard_normal((nb, 4))).astype(F)
    xq = spread_queries(132, metric, nq, plan["query_chunk"])
    want = FL.search(xq, xb, k, metric)
    conditions(want, chunks, metric)
    return xb, xq, k, rows, want


@pytest.mark.parametrize("metric", METRICS)
def test_indexflat_search_in_query_chunks(metric):
    xb, xq, k, rows, want = flat_case(metric)
    ix = faiss.IndexFlat(4, metric)
    ix.set_range_rows(rows)
    ix.add(xb)
    check(ix.search(xq, k), want)
    check(device_search(ix, xq, k), want)


# ------------------------------------------------------------------ 4: ivfpq_flat_search
@pytest.mark.parametrize("metric", METRICS)
def test_stateless_flat_search_in_query_chunks(metric):
    """The [chunk][nb] distance matrix within 256 MiB: 64 queries at nb = 2^20."""
    nb, k = 1 << 20, 10
    chunk = fidx.flat_search_query_chunk(10 ** 6, nb)
    assert chunk == 64
    nq = 2 * chunk + 5
    chunks = cut(nq, chunk)
    rng = np.random.default_rng(141)
    xb = (rng.random((nb, 4)) if metric == IP else rng.standard_normal((nb, 4))).astype(F)
    xq = spread_queries(142, metric, nq, chunk)
    want = FL.search(xq, xb, k, metric)
    assert_shifted(want, chunks)
    D, I = np.full((nq, k), np.nan, F), np.full((nq, k), -7, np.int64)
    _lib.check(_lib.load().ivfpq_flat_search(0, 4, nb, xb.ctypes.data_as(_lib.c_f32p), nq, xq.ctypes.data_as(_lib.c_f32p),
                                             k, metric, D.ctypes.data_as(_lib.c_f32p), I.ctypes.data_as(_lib.c_i64p)))
    check((D, I), want)


# ------------------------------------- 5: ivfpq_index::query_chunk, and IVF-PQ's add passes
PQ_D, PQ_M = 16, 8


def pq_pair(metric, nlist, seed):
    """(index, oracle) over seeded quantizers: the oracle is the reference of every IVF-PQ test."""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.random(s)) if metric == IP else (lambda *s: rng.standard_normal(s))
    cent, cb = draw(nlist, PQ_D).astype(F), (0.5 * draw(PQ_M, 256, PQ_D // PQ_M)).astype(F)
    ix = faiss.IndexIVFPQ(None, PQ_D, nlist, PQ_M, 8, metric)
    ix.set_trained(cent, cb)
    ox = O.OracleIVFPQ(PQ_D, nlist, PQ_M, metric=metric)
    ox.set_trained(cent, cb)
    return ix, ox, draw


@pytest.mark.parametrize("metric", METRICS)
def test_ivfpq_search_in_query_chunks(metric):
    """k 1024 with 64 probes: 64 KiB of partial lists per probe and query, 512 queries per chunk."""
    nlist, nprobe, k = 64, 64, 1024
    chunk = fidx.ivfpq_query_chunk(10 ** 6, nlist, PQ_M, nprobe, k)
    assert chunk == (1 << 31) // (nprobe * k * 64)
    nq = 2 * chunk + 5
    chunks = cut(nq, chunk)
    ix, ox, draw = pq_pair(metric, nlist, 151)
    xb, ids = draw(6000, PQ_D).astype(F), gapped_ids(152, 6000)
    xq = spread_queries(153, metric, nq, chunk, PQ_D)
    ox.add_with_ids(xb, ids)
    ox.nprobe = nprobe
    want = ox.search(xq, k)
    assert_shifted(want, chunks)
    ix.add_with_ids(xb, ids)
    ix.nprobe = nprobe
    check(ix.search(xq, k), want)
    check(device_search(ix, xq, k), want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ivfpq_add_in_passes_encodes_as_the_oracle(device):
    """65536 rows per pass at nlist 1024 (lists + r0, x + r0 d, the codes at (q.n + r0) M)."""
    nlist = 1024
    rows = fidx.ivf_pass_rows(10 ** 6, nlist, PQ_D, False)
    assert rows == (1 << 28) // (4 * nlist)
    n = 2 * rows + 5
    cut(n, rows)
    ix, ox, draw = pq_pair(L2, nlist, 154)
    xb, ids = draw(n + 37, PQ_D).astype(F), gapped_ids(155, n + 37)
    ox.add_with_ids(xb, ids)
    if device:
        import torch

        tx, tid = torch.from_numpy(xb).cuda(), torch.from_numpy(ids).cuda()
        ix.add_device(tx[:n], tid[:n])
        ix.add_device(tx[n:], tid[n:])
    else:
        ix.add_with_ids(xb[:n], ids[:n])
        ix.add_with_ids(xb[n:], ids[n:])
    assert ix.ntotal == n + 37
    np.testing.assert_array_equal(ix.invlists.list_sizes(), [len(i) for i in ox.list_ids])
    for l in range(nlist):
        order = np.argsort(ox.list_ids[l], kind="stable")
        np.testing.assert_array_equal(ix.invlists.get_ids(l), ox.list_ids[l][order])
        assert ix.invlists.get_codes(l).tobytes() == ox.list_codes[l][order].tobytes(), l


# ------------------------------------------------- 6a / 6b: the add passes (IvfLists::chunk_rows)
@functools.lru_cache(maxsize=None)
def add_case(kind):
    """nlist 1024: 65536 rows per pass; 2 * 65536 + 5 rows, then 37 more."""
    nlist, d, extra = 1024, 4, 37
    rows = fidx.ivf_pass_rows(10 ** 6, nlist, d, kind[1] is not None)
    assert rows == (1 << 28) // (4 * nlist)
    n = 2 * rows + 5
    cut(n, rows)
    assert fidx.ivf_pass_rows(extra, nlist, d, kind[1] is not None) == extra
    rng = np.random.default_rng(161)
    xb, cent = rng.standard_normal((n + extra, d)).astype(F), rng.standard_normal((nlist, d)).astype(F)
    ref = make_ref(kind, xb, cent, L2, gapped_ids(162, n + extra))
    xq = rng.standard_normal((5, d)).astype(F)
    return ref, n, ref.lists(), xq, ref.search(xq, 10, nprobe=4)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ADD_KINDS)
def test_add_in_passes_builds_the_reference_lists(kind, device):
    """Every pass assigns (and IVF-SQ encodes) its own rows behind the pass before: lists + r0,
    x + r0 d, codes + r0 code_size.  Host rows with labels, and device rows with device labels."""
    ref, n, lists, xq, want = add_case(kind)
    ix = make_index(kind, ref, 4, len(ref.cent), L2)
    if device:
        import torch

        tx, tid = torch.from_numpy(ref.xb).cuda(), torch.from_numpy(ref.ids).cuda()
        ix.add_device(tx[:n], tid[:n])
        ix.add_device(tx[n:], tid[n:])
    else:
        ix.add_with_ids(ref.xb[:n], ref.ids[:n])
        ix.add_with_ids(ref.xb[n:], ref.ids[n:])
    assert ix.ntotal == len(ref.xb)
    np.testing.assert_array_equal(ix.invlists.list_sizes(), [len(i) for i, _ in lists])
    for l, (ids, rows) in enumerate(lists):
        np.testing.assert_array_equal(ix.invlists.get_ids(l), ids)
        assert ix.invlists.get_codes(l).tobytes() == rows.tobytes(), l
    ix.nprobe = 4
    check(ix.search(xq, 10), want)


def test_add_device_in_passes_of_the_segmented_quantizer():
    """6b: from nlist 8192 on a pass is 2^18 rows.  Rows lie 0.01 around centroids 10 apart on a
    grid, in a seeded random order of lists, so the expected lists follow from the construction."""
    import torch

    nlist, d = 8192, 4
    rows = fidx.ivf_pass_rows(10 ** 7, nlist, d, False)
    assert rows == 1 << 18
    n = 2 * rows + 3
    cut(n, rows)
    cent = (10.0 * np.stack(np.unravel_index(np.arange(nlist), (16, 16, 8, 4)), 1)).astype(F)
    g = torch.Generator(device="cuda").manual_seed(6)
    lists = torch.randint(0, nlist, (n,), generator=g, device="cuda")
    tx = torch.from_numpy(cent).cuda()[lists] + 0.01 * torch.randn((n, d), generator=g, device="cuda")
    tid = 3 * torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda") + 7  # decreasing: label order != add order
    ix = faiss.IndexIVFFlat(None, d, nlist, L2)
    ix.set_trained(cent)
    ix.add_device(tx, tid)
    assert ix.ntotal == n
    np.testing.assert_array_equal(ix.invlists.list_sizes(), torch.bincount(lists, minlength=nlist).cpu().numpy())
    order = torch.argsort(lists.flip(0), stable=True)  # rows by list, then by increasing label
    by_list = (n - 1 - order).cpu().numpy()
    off = np.concatenate([[0], np.cumsum(ix.invlists.list_sizes())])
    hid, hx = tid.cpu().numpy(), tx.cpu().numpy()
    last = lists[2 * rows:].cpu().tolist()  # the lists of the short pass's three rows
    for l in sorted(set(range(0, nlist, 61)) | set(last)):  # and 135 more, their rows in both full passes
        sel = by_list[off[l]:off[l + 1]]
        assert sel.min() < rows <= sel.max() and (l not in last or sel.max() >= 2 * rows)
        np.testing.assert_array_equal(ix.invlists.get_ids(l), hid[sel])
        assert ix.invlists.get_codes(l).tobytes() == hx[sel].tobytes()


# --------------------------------------------------------- 7a: KMeans::assign_top1's passes
@pytest.mark.parametrize("metric", METRICS)
def test_ivfflat_training_assigns_in_passes(metric):
    nlist, d, niter, seed = 1024, 4, 2, 77
    rows = fidx.kmeans_assign_rows(10 ** 6, nlist)
    assert rows == (1 << 28) // (4 * nlist)
    n = 2 * rows + 5
    cut(n, rows)
    rng = np.random.default_rng(171)
    x = (rng.random((n, d)) if metric == IP else rng.standard_normal((n, d))).astype(F)
    ix = faiss.IndexIVFFlat(None, d, nlist, metric)
    ix.niter_coarse, ix.seed = niter, seed
    ix.train(x)
    np.testing.assert_array_equal(ix.centroids(), O.kmeans(x, nlist, niter, seed, metric=metric))


def test_indexpq_training_assigns_in_passes():
    """256 centroids per sub-quantizer: 262144 rows per pass (M = 8 is the fewest IndexPQ takes)."""
    M, dsub, niter = 8, 1, 1
    rows = fidx.kmeans_assign_rows(10 ** 7, 256)
    assert rows == (1 << 28) // (4 * 256)
    n = 2 * rows + 5
    cut(n, rows)
    x = np.random.default_rng(172).standard_normal((n, M * dsub)).astype(F)
    ix = faiss.IndexPQ(M * dsub, M, 8)
    ix.niter_pq, ix.seed = niter, 99
    ix.train(x)
    cb = ix.pq.centroids.reshape(M, 256, dsub)
    for m in range(M):
        np.testing.assert_array_equal(
            cb[m], O.kmeans(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]), 256, niter, 99 + 1 + m))


# --------------------------------------------- 7b: ivfpq_ivfsq_index::train_sq's passes
@pytest.mark.parametrize("n", [70000, 140000], ids=["all-rows", "subsample"])
@pytest.mark.parametrize("by_residual", [False, True], ids=["plain", "residual"])
def test_ivfsq_quantizer_trains_in_passes(by_residual, n):
    """The table's minimum and maximum over passes of 65536 staged rows: all 70 000 rows, or the
    100 000 of 140 000 that rand_perm picks, gathered through pick[r0 + i] in every pass."""
    nlist, d = 1024, 4
    m = len(RS.train_rows(n))
    assert m == min(n, RS.SQ_TRAIN_ROWS)
    cut(m, fidx.ivf_pass_rows(m, nlist, d, True), full=1)
    x = np.random.default_rng(173).standard_normal((n, d)).astype(F)
    x[:, 1] += np.linspace(0, 5, n, dtype=F)  # the extremes depend on which rows are seen
    ix = faiss.IndexIVFScalarQuantizer(None, d, nlist, QT_8BIT, L2, by_residual)
    ix.niter_coarse, ix.seed = 1, 78
    ix.train(x)
    cent = ix.centroids()
    np.testing.assert_array_equal(cent, O.kmeans(x, nlist, 1, 78))
    want = RS.train_sq(x, cent, QT_8BIT, L2, by_residual)
    assert ix.sq.trained.dtype == np.float32 and ix.sq.trained.tobytes() == want.tobytes()


# ----------------------------- 8: the staging passes of host rows (CodeStore::host_rows, d = 2048)
WIDE_D = 2048


@functools.lru_cache(maxsize=None)
def wide_rows():
    """32773 x 2048: one pass of 32768 rows (256 MiB of fp32) and one of five."""
    rows = fidx.host_pass_rows(10 ** 6, 4 * WIDE_D)
    assert rows == (1 << 28) // (4 * WIDE_D)
    n = rows + 5
    cut(n, rows, full=1)
    x = np.random.default_rng(181).random((n, WIDE_D), dtype=F)
    x[rows:] += F(0.25) * np.arange(5, dtype=F)[:, None]  # the second pass holds the extremes
    x.setflags(write=False)
    # five queries next to the five rows of the second pass
    xq = (x[rows:] + F(0.001) * np.random.default_rng(182).standard_normal((5, WIDE_D)).astype(F)).astype(F)
    return x, xq, rows


@pytest.mark.parametrize("qtype", [pytest.param(QT_FP16, id="fp16"), pytest.param(QT_8BIT, id="8bit")])
def test_indexsq_host_rows_in_staging_passes(qtype):
    """train, add, sa_encode and sa_decode stage 32768 rows at a time (sa_decode too: its pass is
    sized by the fp32 rows it writes); the nearest rows of the search lie in the second pass."""
    x, xq, rows = wide_rows()
    n = len(x)
    ref = SQ.Ref(x, qtype, L2)
    ix = faiss.IndexScalarQuantizer(WIDE_D, qtype, L2)
    ix.train(x)
    assert ix.sq.trained.tobytes() == ref.trained.tobytes()
    ix.add(x)
    assert ix.ntotal == n and ix.codes.tobytes() == ref.codes.tobytes()
    assert ix.sa_encode(x).tobytes() == ref.codes.tobytes()
    assert ix.sa_decode(ref.codes).tobytes() == ref.dec.tobytes()
    want = ref.search(xq, 10)
    assert (want[1][:, 0] == rows + np.arange(5)).all()
    check(ix.search(xq, 10), want)


def test_indexflat_wide_rows_read_back_and_searched():
    """IndexFlat uploads its host rows in one copy (no pass); the fixture's rows read back from the
    device image, and the same five queries."""
    x, xq, rows = wide_rows()
    ix = faiss.IndexFlat(WIDE_D, L2)
    ix.add(x)
    want = FL.search(xq, x, 10, L2)
    assert (want[1][:, 0] == rows + np.arange(5)).all()
    check(ix.search(xq, 10), want)
    back = np.empty_like(x)
    _lib.check(_lib.load().ivfpq_flat_index_get_rows(ix._h, 0, len(x), back.ctypes.data_as(_lib.c_f32p)))
    assert back.tobytes() == x.tobytes()
