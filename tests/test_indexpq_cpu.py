"""IndexPQ without a GPU: the C-ABI symbols, argument checks made before any device
call, the "IxPq" file layout, the factory keys and the host-side decode."""
import ctypes
import struct

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib, faiss_io
from faiss_amd import index as fidx

PQ_SYMBOLS = ["ivfpq_pq_create", "ivfpq_pq_free", "ivfpq_pq_train", "ivfpq_pq_set_trained", "ivfpq_pq_add",
              "ivfpq_pq_add_device", "ivfpq_pq_add_codes", "ivfpq_pq_reset", "ivfpq_pq_search",
              "ivfpq_pq_search_device", "ivfpq_pq_ntotal", "ivfpq_pq_is_trained", "ivfpq_pq_get_dims",
              "ivfpq_pq_get_codebook", "ivfpq_pq_get_codes", "ivfpq_pq_debug_plan"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in PQ_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert faiss.IndexPQ is fidx.IndexPQ


@pytest.mark.parametrize("args,word", [((100, 16, 8), "multiple"), ((128, 16, 4), "nbits"),
                                       ((4096, 16, 8), "2048"), ((120, 24, 8), "8, 16, 32, 48, 64")])
def test_create_rejects_bad_shapes_before_any_device_call(args, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    d, M, nbits = args
    assert lib.ivfpq_pq_create(d, M, nbits, faiss.METRIC_L2, 0, ctypes.byref(h)) != 0
    assert word in lib.ivfpq_last_error().decode()
    assert not h.value
    with pytest.raises(RuntimeError, match=word):
        faiss.IndexPQ(d, M, nbits)


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.load()
    assert lib.ivfpq_pq_ntotal(None) == -1
    assert lib.ivfpq_pq_is_trained(None) == 0
    assert lib.ivfpq_pq_reset(None) != 0
    assert lib.ivfpq_pq_free(None) == 0


# (M, k, nq, nb) -> (ranges, rows, S, query chunk), worked out by hand from pq_scan_plan:
#   groups = ceil(min(nq, chunk) / 4), tiles = ceil(nb / 2048),
#   r = min(ceil(1024 / groups), max(1, 12288 // (4 k)), tiles), rows = ceil(tiles / r) * 2048,
#   ranges = ceil(nb / rows), S = 4 ranges; chunk = min(nq, 256 MiB / (M KiB), 4096)
PLANS = [
    ((8, 10, 5, 4873), (3, 2048, 12, 5)),            # 2 groups: min(512, 307, 3 tiles)
    ((8, 10, 4, 4873), (3, 2048, 12, 4)),            # the tail chunk of 4100 queries
    ((8, 1, 4100, 4873), (1, 6144, 4, 4096)),        # 1024 groups: one range of all 3 tiles
    ((8, 64, 2049, 4873), (2, 4096, 8, 2049)),       # 513 groups: ceil(1024 / 513) = 2
    ((128, 10, 4100, 4873), (2, 4096, 8, 2048)),     # 128 KiB of table per query: chunk 2048, 512 groups
    ((8, 10, 5, 67589), (34, 2048, 136, 5)),         # 34 tiles < 307
    ((8, 64, 5, 67589), (34, 2048, 136, 5)),         # 34 tiles < 48
    ((8, 96, 5, 67589), (17, 4096, 68, 5)),          # 12288 // 384 = 32 -> 2 tiles each -> 17 ranges
    ((8, 256, 1, 49152), (12, 4096, 48, 1)),         # 12288 // 1024 = 12, 24 tiles
    ((8, 257, 1, 49152), (8, 6144, 32, 1)),          # 12288 // 1028 = 11 -> 3 tiles each -> 8 ranges
    ((8, 1000, 1, 18432), (3, 6144, 12, 1)),         # 12288 // 4000 = 3, 9 tiles
    ((16, 1024, 37, 1), (1, 2048, 4, 37)),           # one row
]


@pytest.mark.parametrize("args,want", PLANS, ids=["-".join(map(str, a)) for a, _ in PLANS])
def test_debug_plan_values(args, want):
    from indexpq_ref import plan

    p = plan(*args)
    assert (p.ranges, p.rows, p.S, p.chunk) == want
    assert p.G == 4


@pytest.mark.parametrize("args,word", [((24, 10, 5, 100), "8, 16, 32, 48, 64"), ((144, 10, 5, 100), "not supported"),
                                       ((8, 0, 5, 100), "k must be in"), ((8, 1025, 5, 100), "k must be in")])
def test_debug_plan_rejects_unsupported_shapes(args, word):
    lib = _lib.load()
    assert lib.ivfpq_pq_debug_plan(*args, None, None, None, None, None) != 0
    assert word in lib.ivfpq_last_error().decode()
    assert lib.ivfpq_pq_debug_plan(8, 10, 5, 100, None, None, None, None, None) == 0  # null outputs are skipped


@pytest.mark.parametrize("kind", [0, 1], ids=["ip", "l2"])
def test_vectorised_tree_equals_the_oracle_bit_for_bit(kind):
    from indexpq_ref import tree_np
    from oracle import oracle as O

    rng = np.random.default_rng(17)
    for d in list(range(1, 34)) + [48, 100, 256]:
        x = rng.standard_normal((3, d)).astype(np.float32)
        y = (rng.standard_normal((5, d)) * 3).astype(np.float32)
        got = tree_np(x[:, None, :], y[None], kind)
        assert got.dtype == np.float32 and got.shape == (3, 5)
        want = np.array([[O.tree(x[i], y[j], kind) for j in range(5)] for i in range(3)], np.float32)
        assert got.tobytes() == want.tobytes(), d


def test_shared_reference_sums_and_order():
    """indexpq_ref's sums and top-k against the plain statements of the same thing."""
    import indexpq_ref as R

    rng = np.random.default_rng(18)
    nq, M, nb = 7, 16, 90
    tab = rng.standard_normal((nq, M, 256)).astype(np.float32)
    codes = rng.integers(0, 4, (nb, M), dtype=np.uint8)  # few distinct codes: ties
    codes[40:] = codes[:50]
    want = np.zeros((nq, nb), np.float32)
    for m in range(M):
        want += tab[:, m, codes[:, m]]
    acc = R.ref_sums(tab, codes)
    assert acc.tobytes() == want.tobytes()
    for metric in (R.L2, R.IP):
        for k in (1, 10, 90, 100):
            D, I = R.ref_topk(acc, k, metric, R.ref_order(acc, 100, metric))
            for q in range(nq):
                order = np.lexsort((np.arange(nb), -acc[q] if metric == R.IP else acc[q]))[:k]
                np.testing.assert_array_equal(I[q, :len(order)], order)
                np.testing.assert_array_equal(D[q, :len(order)], acc[q][order])
                assert (I[q, len(order):] == -1).all()
                assert (D[q, len(order):] == (-R.FMAX if metric == R.IP else R.FMAX)).all()


def test_ixpq_layout_and_round_trip():
    rng = np.random.default_rng(3)
    d, M, n = 24, 8, 13
    cb = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    buf = faiss_io.serialize_pq(d, M, 8, faiss.METRIC_INNER_PRODUCT, cb, codes)
    # fourcc, index header, ProductQuantizer, codes vector, search_type / encode_signs / polysemous_ht
    want = b"".join([
        b"IxPq", struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, 1, 0),
        struct.pack("<QQQ", d, M, 8), struct.pack("<Q", cb.size), cb.tobytes(),
        struct.pack("<Q", codes.size), codes.tobytes(), struct.pack("<iBi", 0, 0, 0)])
    assert buf == want
    z = faiss_io.parse_index(buf)
    assert (z["kind"], z["d"], z["ntotal"], z["M"], z["nbits"], z["metric"], z["is_trained"]) == \
        ("pq", d, n, M, 8, faiss.METRIC_INNER_PRODUCT, True)
    np.testing.assert_array_equal(z["codebook"], cb)
    np.testing.assert_array_equal(z["codes"], codes)
    assert faiss_io.parse_pq(buf)["ntotal"] == n
    with pytest.raises(RuntimeError):
        faiss_io.parse_index(buf[:-3])
    with pytest.raises(RuntimeError):
        faiss_io.parse_index(buf + b"\0")

    # wrapped in an IndexPreTransform
    A = rng.standard_normal((d, 32)).astype(np.float32)
    wrapped = faiss_io.serialize_pretransform(32, faiss.METRIC_INNER_PRODUCT, [(A, None, 32, d, True)], buf, n)
    w = faiss_io.parse_index(wrapped)
    assert w["kind"] == "pretransform" and w["index"]["kind"] == "pq" and w["ntotal"] == n
    np.testing.assert_array_equal(w["chain"][0]["A"], A)
    np.testing.assert_array_equal(w["index"]["codes"], codes)


def test_is_faiss_file_knows_ixpq(tmp_path):
    p = tmp_path / "x.index"
    p.write_bytes(faiss_io.serialize_pq(8, 8, 8, 1, np.zeros((8, 256, 1), np.float32), np.zeros((0, 8), np.uint8)))
    assert faiss_io.is_faiss_file(str(p))


def test_factory_keys():
    assert fidx.parse_pq_factory("PQ96") == (96, 8)
    assert fidx.parse_pq_factory("PQ96x8") == (96, 8)
    assert fidx.parse_pq_factory("OPQ96,PQ96") == (96, 8, 96, -1)
    assert fidx.parse_pq_factory("OPQ96_384,PQ96") == (96, 8, 96, 384)
    assert fidx.parse_pq_factory("IVF1024,PQ16") is None
    assert fidx.parse_pq_factory("PQ") is None
    # the IVF keys are parsed as before
    assert fidx.parse_factory("IVF1024,PQ16") == (1024, 16, 8)
    with pytest.raises(RuntimeError):
        fidx.parse_factory("IVF1024,Flat")
    # index_factory reaches IndexPQ's own argument checks for a flat key
    with pytest.raises(RuntimeError, match="multiple"):
        faiss.index_factory(100, "PQ16")
    with pytest.raises(RuntimeError, match="nbits"):
        faiss.index_factory(128, "PQ16x4")


def test_reconstruct_is_a_numpy_decode():
    rng = np.random.default_rng(4)
    M, dsub, n = 8, 3, 40
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)

    class HostOnly(faiss.IndexPQ):  # the codebook and codes of a handle, without one
        def __init__(self):
            self.d, self.M, self.nbits = M * dsub, M, 8

        def codebook(self):
            return cb

        def _codes(self, i0, n_):
            return codes[i0:i0 + n_]

    ix = HostOnly()
    want = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
    np.testing.assert_array_equal(ix.reconstruct_n(0, n), want)
    np.testing.assert_array_equal(ix.reconstruct_n(7, 9), want[7:16])
    np.testing.assert_array_equal(ix.reconstruct(11), want[11])
    assert ix.reconstruct_n(0, n).dtype == np.float32
