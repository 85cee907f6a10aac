"""How the host cuts a batch into chunks, without a GPU: the getters of include/ivfpq.h that
report what each loop computes ("Host-side splits") against values worked out by
hand from kChunkBytes = 2^28 and kPartialBytes = 2^31 of csrc/host_common.h.  The GPU cases of
tests/test_gpu_host_splits.py size their batches from the same getters."""
import ctypes

import pytest

from faiss_amd import _lib
from faiss_amd import index as fidx

SYMBOLS = ["ivfpq_ivf_get_plan", "ivfpq_ivf_get_query_chunk", "ivfpq_ivf_get_pass_rows", "ivfpq_sq_get_plan",
           "ivfpq_get_query_chunk", "ivfpq_host_get_pass_rows", "ivfpq_flat_search_get_query_chunk", "ivfpq_kmeans_get_assign_rows"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


# (k, slots) -> (S, fan): fan = the largest power of two <= min(16, 2048 / k), at least 2;
# S = 4 slots, rounded up to a power of two once it exceeds fan
IVF_PLANS = [((10, 4), (16, 16)), ((10, 1), (4, 16)), ((10, 5), (32, 16)), ((64, 4), (16, 16)), ((100, 4), (16, 16)),
             ((129, 4), (16, 8)), ((1024, 1), (4, 2)), ((1024, 64), (256, 2)), ((1024, 17), (128, 2)), ((10, 0), (4, 16))]


@pytest.mark.parametrize("args,want", IVF_PLANS, ids=["-".join(map(str, a)) for a, _ in IVF_PLANS])
def test_ivf_plan_values(args, want):
    S, fan = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().ivfpq_ivf_get_plan(*args, ctypes.byref(S), ctypes.byref(fan)))
    assert (S.value, fan.value) == want


# (nq, nlist, k, nprobe, d, slots, entry_bytes, resid_queries) -> queries per chunk
IVF_CHUNKS = [
    ((10 ** 6, 65536, 10, 4, 4, 4, 8, False), 512),       # 1a: 2^28 / (65536 * 8)
    ((10 ** 6, 65536, 10, 4, 4, 4, 12, True), 341),       # 1a, by_residual: 2^28 / (65536 * 12)
    ((10 ** 6, 64, 1024, 64, 4, 64, 8, False), 341),      # 1b: S 256 -> 2^31 / (256 * 1024 * 24)
    ((10 ** 6, 64, 1024, 64, 4, 64, 12, True), 341),      # 1b, by_residual: the residual queries allow 262144
    ((10 ** 6, 8, 10, 1024, 2048, 8, 12, True), 32),      # residual queries: 2^28 / (4 * 1024 * 2048)
    ((10 ** 6, 8, 10, 1024, 2048, 8, 12, False), 279620),  # inner product keeps none: 2^31 / (32 * 10 * 24)
    ((1029, 65536, 10, 4, 4, 4, 8, False), 512),
    ((37, 16, 10, 4, 32, 4, 8, False), 37),               # the suite's base fixtures: one chunk
    ((0, 16, 10, 4, 32, 4, 8, False), 1),
]


@pytest.mark.parametrize("args,want", IVF_CHUNKS, ids=[str(i) for i in range(len(IVF_CHUNKS))])
def test_ivf_query_chunk_values(args, want):
    assert fidx.ivf_search_split(*args)["query_chunk"] == want


def test_third_term_of_the_query_chunk_never_binds():
    """(INT32_MAX / 2) / (S k) is twelve times the partial-list term 2^31 / (24 S k)."""
    for S, k in ((4, 1), (16, 10), (256, 1024), (4096, 1024)):
        assert ((1 << 31) - 1) // 2 // (S * k) >= max(1, (1 << 31) // (24 * S * k))


# (nq, nb, k) -> (S, fan, queries per chunk): slots = ceil(nb / 4096)
SQ_PLANS = [((10 ** 6, 65537, 1024), (128, 2, 682)), ((1369, 65537, 1024), (128, 2, 682)),
            ((10 ** 6, 65536, 1024), (64, 2, 1365)), ((10 ** 6, 4097, 1024), (8, 2, 10922)),
            ((37, 5000, 10), (8, 16, 37)), ((10 ** 6, 10 ** 6, 10), (1024, 16, 8738))]


@pytest.mark.parametrize("args,want", SQ_PLANS, ids=["-".join(map(str, a)) for a, _ in SQ_PLANS])
def test_sq_search_plan_values(args, want):
    p = fidx.sq_search_plan(*args)
    assert (p["S"], p["fan"], p["query_chunk"]) == want


def test_flat_index_query_chunk_of_the_table():
    """set_range_rows(128) over 3200 rows: 25 ranges, S 32, limit 2^31 / (32 * 1024 * 24) = 2730;
    2731 queries exceed it and are halved."""
    p = fidx.flat_search_plan(2731, 3200, 1024, 128)
    assert (p["ranges"], p["S"], p["query_chunk"]) == (25, 32, 1365)
    assert fidx.flat_search_plan(2730, 3200, 1024, 128)["query_chunk"] == 2730


def test_pass_rows_values():
    # (n, nlist, d, staged): 2^28 / (4 nlist); 2^18 from nlist 8192 on; staged: also 2^28 / (4 d)
    assert fidx.ivf_pass_rows(10 ** 6, 1024, 4) == 65536
    assert fidx.ivf_pass_rows(10 ** 6, 1024, 4, True) == 65536
    assert fidx.ivf_pass_rows(10 ** 6, 8191, 4) == (1 << 28) // (4 * 8191) == 8193
    assert fidx.ivf_pass_rows(10 ** 6, 8192, 4) == 1 << 18
    assert fidx.ivf_pass_rows(10 ** 6, 262144, 4) == 1 << 18
    assert fidx.ivf_pass_rows(10 ** 6, 4, 2048) == 10 ** 6
    assert fidx.ivf_pass_rows(10 ** 6, 4, 2048, True) == 32768
    assert fidx.ivf_pass_rows(10 ** 6, 8192, 2048, True) == 32768
    assert fidx.ivf_pass_rows(5000, 16, 32, True) == 5000  # the suite's base fixtures: one pass
    assert fidx.ivf_pass_rows(100000, 1024, 4, True) == 65536  # the scalar quantizer's subsample: two passes
    assert fidx.ivf_pass_rows(0, 16, 32) == 1
    # k-means assignment: 2^28 / (4 k)
    assert fidx.kmeans_assign_rows(70000, 1024) == 65536
    assert fidx.kmeans_assign_rows(262145, 256) == 262144
    assert fidx.kmeans_assign_rows(2000, 16) == 2000
    # host rows through a staging buffer: 2^28 / in_bytes
    assert fidx.host_pass_rows(32773, 4 * 2048) == 32768
    assert fidx.host_pass_rows(32773, 2048) == 32773
    assert fidx.host_pass_rows(10 ** 9, 1) == 1 << 28
    # IVF-PQ's search: min(2^28 / max(4 nlist, 1024 M, 16 nloc), 2^31 / (64 nprobe k))
    assert fidx.ivfpq_query_chunk(10 ** 6, 64, 8, 64, 1024) == 512
    assert fidx.ivfpq_query_chunk(10 ** 6, 4096, 64, 32, 1000) == 1048       # C3 with beir's top_k
    assert fidx.ivfpq_query_chunk(10 ** 6, 1024, 16, 16, 10) == 16384        # C2: 16 KiB of table per query
    assert fidx.ivfpq_query_chunk(10 ** 6, 262144, 8, 32, 10) == 64          # 16 bytes of bucket per list
    assert fidx.ivfpq_query_chunk(10 ** 6, 262144, 8, 32, 10, nloc=1024) == 256  # a shard: the 1 MiB of keys
    assert fidx.ivfpq_query_chunk(1024, 1024, 16, 16, 10) == 1024            # bench.py's batch: one chunk
    # the stateless exact search: 2^28 / (4 nb)
    assert fidx.flat_search_query_chunk(133, 1 << 20) == 64
    assert fidx.flat_search_query_chunk(133, 5000) == 133
    assert fidx.flat_search_query_chunk(133, 0) == 133


@pytest.mark.parametrize("call,word", [
    (lambda L: L.ivfpq_ivf_get_plan(0, 4, None, None), "k must be in"),
    (lambda L: L.ivfpq_ivf_get_plan(1025, 4, None, None), "k must be in"),
    (lambda L: L.ivfpq_ivf_get_plan(10, -1, None, None), "slots"),
    (lambda L: L.ivfpq_ivf_get_query_chunk(5, 0, 8, 16, 10, 4, 4, 0, None), "shape"),
    (lambda L: L.ivfpq_ivf_get_query_chunk(5, 16, 8, 16, 0, 4, 4, 0, None), "k must be in"),
    (lambda L: L.ivfpq_ivf_get_pass_rows(-1, 16, 4, 0, None), "shape"),
    (lambda L: L.ivfpq_sq_get_plan(5, -1, 10, None, None, None), "out of range"),
    (lambda L: L.ivfpq_sq_get_plan(5, 100, 2000, None, None, None), "k must be in"),
    (lambda L: L.ivfpq_get_query_chunk(5, 16, 0, 8, 16, 4, 10, None), "shape"),
    (lambda L: L.ivfpq_get_query_chunk(5, 16, 8, 8, 16, 4, 1025, None), "k must be in"),
    (lambda L: L.ivfpq_host_get_pass_rows(5, 0, None), "shape"),
    (lambda L: L.ivfpq_flat_search_get_query_chunk(-1, 5, None), "shape"),
    (lambda L: L.ivfpq_kmeans_get_assign_rows(5, 0, None), "shape"),
])
def test_getters_reject_bad_arguments(call, word):
    lib = _lib.load()
    assert call(lib) != 0
    assert word in lib.ivfpq_last_error().decode()


def test_null_outputs_are_skipped():
    lib = _lib.load()
    assert lib.ivfpq_ivf_get_plan(10, 4, None, None) == 0
    assert lib.ivfpq_ivf_get_query_chunk(5, 16, 8, 16, 10, 4, 4, 0, None) == 0
    assert lib.ivfpq_ivf_get_pass_rows(5, 16, 4, 0, None) == 0
    assert lib.ivfpq_sq_get_plan(5, 100, 10, None, None, None) == 0
    assert lib.ivfpq_get_query_chunk(5, 16, 8, 8, 16, 4, 10, None) == 0
    assert lib.ivfpq_host_get_pass_rows(5, 16, None) == 0
    assert lib.ivfpq_flat_search_get_query_chunk(5, 100, None) == 0
    assert lib.ivfpq_kmeans_get_assign_rows(5, 16, None) == 0
