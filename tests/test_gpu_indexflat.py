"""IndexFlat / IndexFlatL2 / IndexFlatIP on the GPU against tests/indexflat_ref.py
(oracle.coarse_search padded to k): labels and distances must be identical, with no
tolerance, on the resident-image path (search, search_device) and on the stateless
ivfpq_flat_search it replaces.  On integer-valued data the float64 result must be identical
too.

G is the range granule and T the row tile of the scan (csrc/flat_scan.h); k <= 64, k <= 256
and k <= 1024 are three list sizes of the kernel, and batches of at most 16 queries and
k > WIDE_MAX_K take its 16-query tile instead of the 64-query one.  set_range_rows cuts small
bases into several ranges; flat_search_plan tells the split a test claims to reach."""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import indexflat_ref as R
from faiss_amd import _lib
from faiss_amd.index import flat_search_plan
from oracle import oracle as O

pytestmark = pytest.mark.gpu

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
G, T, KC = R.RANGE_GRANULE, R.TILE_ROWS, R.K_CHUNK


def normal(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def build(xb, metric, range_rows=0):
    ix = faiss.IndexFlat(xb.shape[1], metric)
    ix.set_range_rows(range_rows)
    if len(xb):
        ix.add(xb)
    return ix


def same(got, want):
    D, I = got
    Dr, Ir = want
    np.testing.assert_array_equal(np.asarray(I), Ir)
    np.testing.assert_array_equal(np.asarray(D), Dr)


def search_device(ix, xq, k, **kw):
    import torch

    D, I = ix.search_device(torch.from_numpy(xq).cuda(), k, **kw)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def stateless(xb, xq, k, metric):
    """The parent path: ivfpq_flat_search uploads the base and writes the distance matrix."""
    xb, xq = np.ascontiguousarray(xb, np.float32), np.ascontiguousarray(xq, np.float32)
    D = np.empty((len(xq), k), np.float32)
    I = np.empty((len(xq), k), np.int64)
    f32p, i64p = _lib.c_f32p, _lib.c_i64p
    _lib.check(_lib.load().ivfpq_flat_search(0, xb.shape[1], len(xb), xb.ctypes.data_as(f32p), len(xq),
                                             xq.ctypes.data_as(f32p), k, metric, D.ctypes.data_as(f32p),
                                             I.ctypes.data_as(i64p)))
    return D, I


# ------------------------------------------------------------------ base sweep
@functools.lru_cache(maxsize=None)
def base(metric):
    xb, xq = normal(1, 5000, 32), normal(3, 37, 32)
    return build(xb, metric), xb, xq


@pytest.mark.parametrize("k", [1, 10, 64, 65, 100, 256, 257, 1000, 1024])
@pytest.mark.parametrize("metric", METRICS)
def test_base_sweep(metric, k):
    ix, xb, xq = base(metric)
    assert ix.ntotal == 5000 and ix.is_trained and ix.metric_type == metric
    assert flat_search_plan(37, 5000, k)["tile_q"] == (R.TILE_Q if k <= R.WIDE_MAX_K else R.TILE_Q_NARROW)
    want = R.search(xq, xb, k, metric)
    same(ix.search(xq, k), want)
    same(search_device(ix, xq, k), want)
    same(stateless(xb, xq, k, metric), want)


# ------------------------------------------------------------------ d sweep
@pytest.mark.parametrize("d", [1, 3, 7, 24, KC - 1, KC, KC + 1, 100, 128, 130])
@pytest.mark.parametrize("metric", METRICS)
def test_d_sweep(metric, d):
    xb, xq = normal(5 + d, 700, d), normal(7 + d, 19, d)
    want = R.search(xq, xb, 10, metric)
    ix = build(xb, metric)
    same(ix.search(xq, 10), want)
    same(search_device(ix, xq, 10), want)


@pytest.mark.parametrize("metric", METRICS)
def test_d768(metric):
    xb, xq = normal(11, 2000, 768), normal(13, 19, 768)
    same(build(xb, metric).search(xq, 10), R.search(xq, xb, 10, metric))


def test_unaligned_device_queries_take_the_scalar_loads():
    """d % 4 == 0 but the query tensor starts 4 bytes off a 16-byte boundary."""
    import torch

    xb, xq = normal(17, 900, 8), normal(19, 21, 8)
    ix = build(xb, L2)
    flat = torch.empty(21 * 8 + 1, dtype=torch.float32, device="cuda")
    xt = flat[1:].view(21, 8)
    xt.copy_(torch.from_numpy(xq))
    assert xt.data_ptr() % 16 == 4
    D, I = ix.search_device(xt, 10)
    same((D.cpu().numpy(), I.cpu().numpy()), R.search(xq, xb, 10, L2))


# ------------------------------------------------------------------ nb at boundaries
@pytest.mark.parametrize("nb", [0, 1, 9, 10, T - 1, T, T + 1])
@pytest.mark.parametrize("metric", METRICS)
def test_nb_boundaries(metric, nb):
    k = 10  # nb = 9 is k - 1, nb = 10 is k
    xb, xq = normal(23, nb, 16), normal(29, 5, 16)
    want = R.search(xq, xb, k, metric)
    if nb < k:
        assert (want[1][:, nb:] == -1).all() and (want[0][:, nb:] == R.pad(metric)).all()
    ix = build(xb, metric)
    same(ix.search(xq, k), want)
    same(search_device(ix, xq, k), want)
    same(ix.search(xq, 300), R.search(xq, xb, 300, metric))  # sixteen-row lists pad alike


@pytest.mark.parametrize("nb", [G - 1, G, G + 1])
@pytest.mark.parametrize("metric", METRICS)
def test_nb_around_the_granule_with_small_ranges(metric, nb):
    xb, xq = normal(31, nb, 16), normal(37, 9, 16)
    p = flat_search_plan(9, nb, 10, range_rows=2 * T)
    assert p["range_rows"] == 2 * T and p["ranges"] == -(-nb // (2 * T)) >= 4
    for rows in (0, 2 * T):  # one range of G (or two), then four or five of 2 T
        same(build(xb, metric, rows).search(xq, 10), R.search(xq, xb, 10, metric))


@pytest.mark.parametrize("nq,k", [(9, 10), (9, 100), (70, 10), (70, 100), (70, 300)])
@pytest.mark.parametrize("metric", METRICS)
def test_two_merge_rounds(metric, nq, k):
    """25 ranges of one row tile: 32 partial lists per query, merged in two rounds or more, on
    the 16-query tile (nq = 9, and k = 300) and on the 64-query tile."""
    nb = 3 * G + 5
    xb, xq = normal(41, nb, 16), normal(43, nq, 16)
    p = flat_search_plan(nq, nb, k, range_rows=T)
    assert p["tile_q"] == (64 if nq > 16 and k <= R.WIDE_MAX_K else 16), p
    assert p["ranges"] == 25 and p["S"] == 32 and p["rounds"] >= 2, p
    same(build(xb, metric, T).search(xq, k), R.search(xq, xb, k, metric))


# ------------------------------------------------------------------ nq boundaries
@functools.lru_cache(maxsize=None)
def nq_case(metric):
    xb, xq = normal(47, 3000, 24), normal(53, 300, 24)
    return build(xb, metric, 4 * T), xb, xq, R.search(xq, xb, 20, metric)


@pytest.mark.parametrize("nq", [1, 15, 16, 17, 63, 64, 65, 300])
@pytest.mark.parametrize("metric", METRICS)
def test_nq_boundaries(metric, nq):
    ix, xb, xq, (Dr, Ir) = nq_case(metric)
    same(ix.search(xq[:nq], 20), (Dr[:nq], Ir[:nq]))
    same(search_device(ix, xq[:nq], 20), (Dr[:nq], Ir[:nq]))


# ------------------------------------------------------------------ ties
def exact(xq, xb, k, metric, ix=None, rows=0):
    """Integer-valued data: the GPU result equals the reference and the float64 result."""
    ix = ix or build(xb, metric, rows)
    want = R.search(xq, xb, k, metric)
    same(want, R.search64(xq, xb, k, metric))
    same(ix.search(xq, k), want)
    same(search_device(ix, xq, k), want)


@pytest.mark.parametrize("k", [10, 100, 300])
@pytest.mark.parametrize("metric", METRICS)
def test_ties_small_integers(metric, k):
    rng = np.random.default_rng(59)
    xb = rng.integers(0, 4, (3000, 8)).astype(np.float32)
    xq = rng.integers(0, 4, (33, 8)).astype(np.float32)
    exact(xq, xb, k, metric, rows=4 * T)


@pytest.mark.parametrize("metric", METRICS)
def test_ties_all_rows_identical(metric):
    xb = np.tile(np.arange(12, dtype=np.float32), (700, 1))
    xq = np.random.default_rng(61).integers(0, 5, (7, 12)).astype(np.float32)
    for k in (1, 64, 200):
        exact(xq, xb, k, metric, rows=T)
        assert (R.search(xq, xb, k, metric)[1] == np.arange(k)).all()


@pytest.mark.parametrize("k", [30, 50, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_ties_across_a_range_boundary(metric, k):
    """60 equal rows, the best of every query, at positions 2 T - 30 .. 2 T + 29 with ranges of
    2 T rows: k = 30 ends at the boundary, 50 inside the run, 100 after it."""
    rng = np.random.default_rng(67)
    xb = rng.integers(5, 9, (6 * T, 8)).astype(np.float32)
    run = np.arange(2 * T - 30, 2 * T + 30)
    xb[run] = 0 if metric == L2 else 9
    xq = (np.zeros((5, 8)) if metric == L2 else np.ones((5, 8))).astype(np.float32)
    xq[:, 0] += np.arange(5) % 2
    assert flat_search_plan(5, len(xb), k, 2 * T)["ranges"] == 3
    exact(xq, xb, k, metric, rows=2 * T)
    assert (R.search(xq, xb, k, metric)[1][:, :min(k, 60)] == run[:min(k, 60)]).all()


def test_query_equal_to_a_row_is_at_distance_zero():
    """Queries that are rows of the base: where the expansion (|x|^2 + |y|^2) - 2 <x, y> of the
    row against itself rounds below 0 (the norms are tree sums, the product an fmaf chain), the
    distance is clamped to exactly 0 and the row is its own nearest neighbour."""
    xb = (normal(71, 2000, 48) * 37.123).astype(np.float32)
    xq = xb[:200].copy()
    # the fmaf chain of <x, x> restated: a product of two floats is exact in float64
    acc = np.zeros(200, np.float32)
    for j in range(48):
        acc = (xq[:, j].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
    n = O.norms(xq)
    below = ((n + n) - np.float32(2) * acc) < 0
    assert below.sum() >= 10  # the data reach the clamp
    D, I = build(xb, L2, 4 * T).search(xq, 5)
    same((D, I), R.search(xq, xb, 5, L2))
    assert (D >= 0).all()
    assert (I[below, 0] == np.flatnonzero(below)).all() and (D[below, 0] == 0).all()


def test_ip_negative_products():
    rng = np.random.default_rng(73)
    xb = -rng.integers(1, 6, (1500, 10)).astype(np.float32)
    xq = rng.integers(1, 6, (11, 10)).astype(np.float32)
    exact(xq, xb, 40, IP, rows=2 * T)
    assert (R.search(xq, xb, 40, IP)[0] < 0).all()


# ------------------------------------------------------------------ float data
@pytest.mark.parametrize("dist", ["normal", "uniform"])
@pytest.mark.parametrize("metric", METRICS)
def test_float_data_three_ranges(metric, dist):
    rng = np.random.default_rng(79)
    gen = rng.standard_normal if dist == "normal" else rng.random
    xb, xq = gen((20000, 128)).astype(np.float32), gen((100, 128)).astype(np.float32)
    assert flat_search_plan(100, 20000, 100, 4 * G)["ranges"] == 5
    ix = build(xb, metric, 4 * G)
    want = R.search(xq, xb, 100, metric)
    same(ix.search(xq, 100), want)
    same(search_device(ix, xq, 100), want)


# ------------------------------------------------------------------ lifecycle
def capacity(ix):
    cap, re = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_flat_index_get_stats(ix._h, None, ctypes.byref(cap), ctypes.byref(re)))
    return cap.value, re.value


def test_lifecycle_adds_reallocations_and_lazy_upload():
    xb, xq = normal(83, 5000, 20), normal(89, 13, 20)
    ix = faiss.IndexFlatL2(20)
    assert ix.uploaded_rows() == 0 and ix._h is None  # no device image before the first device use
    ix.add(xb[:700])
    same(ix.search(xq, 10), R.search(xq, xb[:700], 10, L2))
    assert ix.uploaded_rows() == 700 and capacity(ix) == (1024, 1)
    ix.add(xb[700:1900])  # crosses 1024
    ix.add(xb[1900:1901])
    same(ix.search(xq, 10), R.search(xq, xb[:1901], 10, L2))
    assert ix.uploaded_rows() == 1901  # extended, not rebuilt
    ix.add(xb[1901:])  # crosses 2048 and 4096
    same(ix.search(xq, 70), R.search(xq, xb, 70, L2))
    assert ix.uploaded_rows() == 5000 and ix.ntotal == 5000
    cap, re = capacity(ix)
    assert cap >= 5000 and re == 3
    np.testing.assert_array_equal(ix.xb.reshape(-1, 20), xb)
    ix.reset()
    assert ix.ntotal == 0
    same(ix.search(xq, 3), R.search(xq, xb[:0], 3, L2))
    ix.add(xb[100:400])
    same(ix.search(xq, 3), R.search(xq, xb[100:400], 3, L2))


def test_add_device_then_host_accessors():
    import torch

    xb, xq = normal(97, 3000, 12), normal(101, 9, 12)
    ix = faiss.IndexFlatIP(12)
    ix.add(xb[:500])
    ix.add_device(torch.from_numpy(xb[500:2500]).cuda())
    assert ix.ntotal == 2500 and ix.uploaded_rows() == 500
    np.testing.assert_array_equal(ix.reconstruct_n(400, 300), xb[400:700])
    np.testing.assert_array_equal(ix.reconstruct(2499), xb[2499])
    np.testing.assert_array_equal(ix.xb, xb[:2500].reshape(-1))
    ix.add(xb[2500:])  # the host has every row again; only the new ones are uploaded
    same(ix.search(xq, 25), R.search(xq, xb, 25, IP))
    assert ix.uploaded_rows() == 1000
    only_dev = faiss.IndexFlat(12, L2)
    only_dev.add_device(torch.from_numpy(xb).cuda())
    same(only_dev.search(xq, 25), R.search(xq, xb, 25, L2))
    np.testing.assert_array_equal(only_dev.reconstruct_n(0, 3000), xb)


def test_search_device_on_a_side_stream_with_caller_outputs():
    import torch

    xb, xq = normal(103, 4000, 64), normal(107, 70, 64)
    ix = build(xb, L2, 8 * T)
    side = torch.cuda.Stream()
    xt = torch.from_numpy(xq).cuda()
    D = torch.empty((70, 80), dtype=torch.float32, device="cuda")
    I = torch.empty((70, 80), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        D2, I2 = ix.search_device(xt, 80, D=D, I=I, stream=side.cuda_stream)
    D3, I3 = ix.search_device(xt, 80)  # the current stream, ordered after the side stream's call
    torch.cuda.synchronize()
    assert D2 is D and I2 is I
    want = R.search(xq, xb, 80, L2)
    same((D.cpu().numpy(), I.cpu().numpy()), want)
    same((D3.cpu().numpy(), I3.cpu().numpy()), want)
    with pytest.raises(RuntimeError):
        ix.search_device(xt, 80, D=D[:, :79])
    with pytest.raises(RuntimeError):
        ix.search_device(xt[:, :63], 80)


def test_two_indexes_on_one_device():
    xa, xc, xq = normal(109, 1500, 16), normal(113, 2500, 16), normal(127, 10, 16)
    a, c = build(xa, L2), build(xc, IP)
    same(a.search(xq, 10), R.search(xq, xa, 10, L2))
    same(c.search(xq, 10), R.search(xq, xc, 10, IP))
    same(a.search(xq, 10), R.search(xq, xa, 10, L2))


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("metric", METRICS)
def test_write_read_roundtrip(tmp_path, metric):
    xb, xq = normal(131, 1234, 40), normal(137, 6, 40)
    ix = faiss.index_factory(40, "Flat", metric)
    assert type(ix) is faiss.IndexFlat
    ix.add(xb)
    p = str(tmp_path / "flat.index")
    faiss.write_index(ix, p)
    iy = faiss.read_index(p)
    assert type(iy) is (faiss.IndexFlatIP if metric == IP else faiss.IndexFlatL2)
    assert iy.d == 40 and iy.ntotal == 1234 and iy.metric_type == metric
    want = R.search(xq, xb, 15, metric)
    same(iy.search(xq, 15), want)
    same(ix.search(xq, 15), want)


def test_ivfpq_with_a_user_quantizer_still_trains_syncs_and_searches():
    rng = np.random.default_rng(139)
    d, nlist = 32, 16
    xb = rng.standard_normal((4000, d)).astype(np.float32)
    quantizer = faiss.IndexFlatL2(d)
    index = faiss.IndexIVFPQ(quantizer, d, nlist, 8, 8)
    index.train(xb)
    assert quantizer.ntotal == nlist
    np.testing.assert_array_equal(quantizer.xb.reshape(nlist, d), index.centroids())
    index.add(xb)
    index.nprobe = 4
    D, I = index.search(xb[:20], 5)
    assert (I[:, 0] >= 0).all()
    # the quantizer, searched on its own, is the coarse assignment
    same(quantizer.search(xb[:20], 4), R.search(xb[:20], index.centroids(), 4, L2))


# ------------------------------------------------------------------ caller replays
class FlatIndexReplay:
    """beir faiss_index.py FaissIndex.build / .search / .save / .load, restated: an inner-product
    flat index filled in buffers of 50 000 rows, results mapped through passage_ids."""

    def __init__(self, index, passage_ids):
        self.index = index
        self.ids = np.asarray(passage_ids)

    @classmethod
    def build(cls, passage_ids, emb, index, buffer_size=50000):
        for lo in range(0, len(emb), buffer_size):
            index.add(emb[lo:lo + buffer_size])
        return cls(index, passage_ids)

    def search(self, q, k):
        S, I = self.index.search(q, k)
        return S, self.ids[I]

    def save(self, path):
        faiss.write_index(self.index, path)

    @classmethod
    def load(cls, path, passage_ids):
        return cls(faiss.read_index(path), passage_ids)


def test_beir_flat_ip_flow(tmp_path):
    rng = np.random.default_rng(149)
    emb = rng.standard_normal((120000, 64)).astype(np.float32)
    q = rng.standard_normal((8, 64)).astype(np.float32)
    ids = np.arange(120000) * 3 + 11
    fi = FlatIndexReplay.build(ids, emb, faiss.IndexFlatIP(64))
    assert fi.index.ntotal == 120000 and fi.index.capacity < 2 * 120000 + 64
    Dr, Ir = R.search(q, emb, 10, IP)
    S, P = fi.search(q, 10)
    np.testing.assert_array_equal(S, Dr)
    np.testing.assert_array_equal(P, ids[Ir])
    p = str(tmp_path / "beir.index")
    fi.save(p)
    fj = FlatIndexReplay.load(p, ids)
    assert isinstance(fj.index, faiss.IndexFlatIP)
    S2, P2 = fj.search(q, 10)
    np.testing.assert_array_equal(S2, Dr)
    np.testing.assert_array_equal(P2, ids[Ir])


def test_index_scanner_flow():
    """ralm index_scanner.py: an IndexFlatL2 over the coarse centroids, one query per request."""
    cent, xq = normal(151, 4096, 96), normal(157, 50, 96)
    scanner = faiss.IndexFlatL2(96)
    scanner.add(cent)
    Dr, Ir = R.search(xq, cent, 32, L2)
    assert flat_search_plan(1, 4096, 32)["ranges"] == 4
    for i in range(50):
        D, I = scanner.search(xq[i:i + 1], 32)
        np.testing.assert_array_equal(I[0], Ir[i])
        np.testing.assert_array_equal(D[0], Dr[i])
