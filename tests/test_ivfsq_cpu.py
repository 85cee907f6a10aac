"""IndexIVFScalarQuantizer without a GPU: the C-ABI symbols, the argument checks made before any
device call, the factory keys, the "IwSq" file layout, the shared reference of the GPU tests
against a float64 brute force, and the kernels' resources read from the built code object."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import faiss_amd as faiss
import ivfsq_ref as R
from faiss_amd import _lib, faiss_io
from faiss_amd import index as fidx

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "ivf_sq.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

SYMBOLS = ["create", "free", "train", "set_trained", "add", "add_device", "add_codes", "reset", "set_nprobe",
           "get_nprobe", "search", "search_preassigned", "search_device", "search_preassigned_device", "ntotal",
           "is_trained", "get_dims", "get_centroids", "get_trained", "get_list_sizes", "get_list"]
QT = {"QT_8bit": 0, "QT_4bit": 1, "QT_8bit_uniform": 2, "QT_4bit_uniform": 3, "QT_fp16": 4, "QT_8bit_direct": 5,
      "QT_6bit": 6}
SUPPORTED = ["QT_fp16", "QT_8bit", "QT_8bit_uniform"]
UNSUPPORTED = ["QT_4bit", "QT_4bit_uniform", "QT_8bit_direct", "QT_6bit"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, "ivfpq_ivfsq_" + n), n
        assert "ivfpq_ivfsq_" + n in _lib.SIGNATURES, n
    assert faiss.IndexIVFScalarQuantizer is fidx.IndexIVFScalarQuantizer
    assert issubclass(faiss.IndexIVFScalarQuantizer, faiss.IndexIVFFlat)  # every method of IndexIVFFlat


@pytest.mark.parametrize("d,nlist,qtype,metric,word",
                         [(6, 8, 4, 1, "multiple of 4"), (0, 8, 4, 1, "multiple of 4"), (2052, 8, 0, 1, "2048"),
                          (32, 0, 4, 1, "nlist"), (32, 8, 4, 7, "metric"), (32, 8, 9, 1, "9")] +
                         [(32, 8, QT[n], 1, n) for n in UNSUPPORTED])
def test_create_rejects_bad_arguments_before_any_device_call(d, nlist, qtype, metric, word):
    lib = _lib.load()
    for by_residual in (0, 1):
        h = ctypes.c_void_p()
        assert lib.ivfpq_ivfsq_create(d, nlist, qtype, metric, by_residual, 0, ctypes.byref(h)) != 0
        assert word in lib.ivfpq_last_error().decode()
        assert not h.value
    with pytest.raises(RuntimeError, match=word):
        faiss.IndexIVFScalarQuantizer(None, d, nlist, qtype, metric)


def test_unsupported_types_get_the_flat_quantizers_messages():
    lib = _lib.load()
    for name in UNSUPPORTED + ["9"]:
        qtype = QT.get(name, 9)
        h = ctypes.c_void_p()
        assert lib.ivfpq_sq_create(32, qtype, 1, 0, ctypes.byref(h)) != 0
        flat = lib.ivfpq_last_error().decode()
        assert lib.ivfpq_ivfsq_create(32, 8, qtype, 1, 1, 0, ctypes.byref(h)) != 0
        assert lib.ivfpq_last_error().decode() == flat


def test_create_without_device_fails_with_a_message():
    lib = _lib.load()
    if lib.ivfpq_device_count() > 0:
        pytest.skip("a device is present")
    h = ctypes.c_void_p()
    assert lib.ivfpq_ivfsq_create(32, 8, QT["QT_fp16"], faiss.METRIC_L2, 1, 0, ctypes.byref(h)) != 0
    assert lib.ivfpq_last_error().decode() != ""
    assert not h.value


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.load()
    assert lib.ivfpq_ivfsq_ntotal(None) == -1
    assert lib.ivfpq_ivfsq_is_trained(None) == 0
    assert lib.ivfpq_ivfsq_get_nprobe(None) == -1
    x = np.zeros((1, 8), np.float32)
    c = np.zeros((1, 16), np.uint8)
    i8 = np.zeros(1, np.int64)
    D, I = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64)
    fp, up, ip = _lib.c_f32p, _lib.c_u8p, _lib.c_i64p
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    calls = [lambda: lib.ivfpq_ivfsq_reset(None), lambda: lib.ivfpq_ivfsq_train(None, 1, p(x, fp), 1, 1),
             lambda: lib.ivfpq_ivfsq_set_trained(None, p(x, fp), p(x, fp), 0),
             lambda: lib.ivfpq_ivfsq_add(None, 1, p(x, fp), None),
             lambda: lib.ivfpq_ivfsq_add_device(None, 1, None, None, None),
             lambda: lib.ivfpq_ivfsq_add_codes(None, 1, p(i8, ip), p(c, up), None),
             lambda: lib.ivfpq_ivfsq_set_nprobe(None, 1),
             lambda: lib.ivfpq_ivfsq_search(None, 1, p(x, fp), 1, p(D, fp), p(I, ip)),
             lambda: lib.ivfpq_ivfsq_search_preassigned(None, 1, p(x, fp), 1, p(i8, ip), None, p(D, fp), p(I, ip)),
             lambda: lib.ivfpq_ivfsq_search_device(None, 1, None, 1, None, None, None),
             lambda: lib.ivfpq_ivfsq_search_preassigned_device(None, 1, None, 1, None, None, None, None, None),
             lambda: lib.ivfpq_ivfsq_get_dims(None, None, None, None, None, None, None),
             lambda: lib.ivfpq_ivfsq_get_centroids(None, p(x, fp)),
             lambda: lib.ivfpq_ivfsq_get_trained(None, None, None),
             lambda: lib.ivfpq_ivfsq_get_list_sizes(None, p(i8, ip)),
             lambda: lib.ivfpq_ivfsq_get_list(None, 0, p(c, up), p(i8, ip))]
    for call in calls:
        assert call() != 0
        assert "null index handle" in lib.ivfpq_last_error().decode()
    assert lib.ivfpq_ivfsq_free(None) == 0


def test_factory_keys():
    assert fidx.parse_ivfsq_factory("IVF8,SQ8") == (8, QT["QT_8bit"])
    assert fidx.parse_ivfsq_factory("IVF1024,SQfp16") == (1024, QT["QT_fp16"])
    assert fidx.parse_ivfsq_factory(" IVF16, SQ8 ") == (16, QT["QT_8bit"])
    for key in ("SQ8", "SQfp16", "IVF8,Flat", "IVF8,PQ4", "PQ16", "Flat", "OPQ16,IVF8,PQ16", "IVF,SQ8", "IVF8,SQ"):
        assert fidx.parse_ivfsq_factory(key) is None, key
    for key in ("IVF8,SQ4", "IVF8,SQ6"):
        with pytest.raises(RuntimeError, match=key):
            fidx.parse_ivfsq_factory(key)
        with pytest.raises(RuntimeError, match=key):
            faiss.index_factory(32, key)
    # the other parsers are unchanged for their keys, and do not take the new ones
    for key in ("IVF8,SQ8", "IVF8,SQfp16"):
        assert fidx.parse_sq_factory(key) is None
        assert fidx.parse_ivfflat_factory(key) is None
        assert fidx.parse_pq_factory(key) is None
        with pytest.raises(RuntimeError):
            fidx.parse_factory(key)
    assert fidx.parse_sq_factory("SQ8") == QT["QT_8bit"] and fidx.parse_sq_factory("SQfp16") == QT["QT_fp16"]
    assert fidx.parse_ivfflat_factory("IVF8,Flat") == 8 and fidx.parse_pq_factory("PQ16") == (16, 8)
    assert fidx.parse_factory("IVF1024,PQ16") == (1024, 16, 8)
    assert fidx.parse_factory("OPQ16_64,IVF256,PQ16x8") == (256, 16, 8, 16, 64)
    assert fidx.parse_pca_front("PCA32,IVF8,SQfp16") == (32, 0.0, False, "IVF8,SQfp16")
    # index_factory reaches IndexIVFScalarQuantizer's own argument checks
    with pytest.raises(RuntimeError, match="multiple of 4"):
        faiss.index_factory(30, "IVF8,SQ8")


def _lists(rng, cs, sizes):
    out, nxt = [], 0
    for n in sizes:
        ids = rng.permutation(1000)[:n].astype(np.int64) + nxt
        out.append((np.sort(ids), rng.integers(0, 256, (n, cs)).astype(np.uint8)))
        nxt += 1000
    return out


@pytest.mark.parametrize("sizes", [(3, 0, 5, 1), (0, 0, 0, 2)], ids=["full", "sprs"])
@pytest.mark.parametrize("by_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("qname", SUPPORTED)
def test_iwsq_layout_and_round_trip(qname, by_residual, sizes):
    rng = np.random.default_rng(5)
    qtype, d, nlist, nprobe = QT[qname], 12, len(sizes), 3
    cs = {"QT_fp16": 2 * d, "QT_8bit": d, "QT_8bit_uniform": d}[qname]
    trained = rng.standard_normal({"QT_fp16": 0, "QT_8bit": 2 * d, "QT_8bit_uniform": 2}[qname]).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    lists = _lists(rng, cs, sizes)
    ntot = sum(sizes)
    buf = faiss_io.serialize_ivfsq(d, nlist, nprobe, qtype, faiss.METRIC_INNER_PRODUCT, by_residual, cent, trained,
                                   lists)
    hdr = lambda dd, n: struct.pack("<iqqqBi", dd, n, 1 << 20, 1 << 20, 1, 0)  # noqa: E731
    nz = [l for l in range(nlist) if sizes[l]]
    if len(nz) > nlist // 2:
        table = b"full" + struct.pack("<Q", nlist) + np.array(sizes, np.uint64).tobytes()
    else:
        table = b"sprs" + struct.pack("<Q", 2 * len(nz)) + b"".join(struct.pack("<QQ", l, sizes[l]) for l in nz)
    want = b"".join([b"IwSq", hdr(d, ntot), struct.pack("<QQ", nlist, nprobe),
                     b"IxFI", hdr(d, nlist), struct.pack("<Q", cent.size), cent.tobytes(),
                     struct.pack("<B", 0), struct.pack("<Q", 0),
                     struct.pack("<i", qtype), struct.pack("<i", 0), struct.pack("<f", 0.0),
                     struct.pack("<Q", d), struct.pack("<Q", cs), struct.pack("<Q", trained.size), trained.tobytes(),
                     struct.pack("<Q", cs), struct.pack("<B", 1 if by_residual else 0),
                     b"ilar", struct.pack("<QQ", nlist, cs), table] +
                    [c.tobytes() + i.tobytes() for i, c in lists if len(i)])
    assert buf == want
    z = faiss_io.parse_index(buf)
    assert (z["kind"], z["d"], z["nlist"], z["nprobe"], z["qtype"], z["metric"], z["by_residual"], z["is_trained"],
            z["code_size"]) == ("ivfsq", d, nlist, nprobe, qtype, faiss.METRIC_INNER_PRODUCT, by_residual, True, cs)
    np.testing.assert_array_equal(z["centroids"], cent)
    assert z["trained"].dtype == np.float32 and z["trained"].tobytes() == trained.tobytes()
    for (ids, codes), (zi, zc) in zip(lists, z["lists"]):
        np.testing.assert_array_equal(zi, ids)
        assert zc.dtype == np.uint8 and zc.shape == codes.shape and zc.tobytes() == codes.tobytes()
    assert faiss_io.serialize_ivfsq(d, nlist, z["nprobe"], z["qtype"], z["metric"], z["by_residual"], z["centroids"],
                                    z["trained"], z["lists"]) == buf
    for cut in range(len(buf)):  # every truncation
        with pytest.raises(RuntimeError):
            faiss_io.parse_index(buf[:cut])
    with pytest.raises(RuntimeError):
        faiss_io.parse_index(buf + b"\0")


def test_iwsq_rejects_other_types_and_a_code_size_that_disagrees():
    d = 8
    empty = [(np.zeros(0, np.int64), np.zeros((0, d), np.uint8))] * 2
    good = faiss_io.serialize_ivfsq(d, 2, 1, QT["QT_8bit"], 1, True, np.zeros((2, d), np.float32),
                                    np.zeros(2 * d, np.float32), empty)
    assert faiss_io.parse_index(good)["kind"] == "ivfsq"
    at = good.index(struct.pack("<iifQQ", QT["QT_8bit"], 0, 0.0, d, d))  # the quantizer block
    for name in UNSUPPORTED:
        bad = good[:at] + struct.pack("<i", QT[name]) + good[at + 4:]
        with pytest.raises(RuntimeError, match="unsupported scalar quantizer"):
            faiss_io.parse_index(bad)
    cs_at = at + struct.calcsize("<iifQQ") + 8 + 4 * 2 * d
    assert good[cs_at:cs_at + 9] == struct.pack("<QB", d, 1)
    bad = good[:cs_at] + struct.pack("<Q", 2 * d) + good[cs_at + 8:]
    with pytest.raises(RuntimeError, match="code size"):
        faiss_io.parse_index(bad)
    with pytest.raises(RuntimeError):
        faiss_io.serialize_ivfsq(d, 2, 1, QT["QT_4bit"], 1, True, np.zeros((2, d), np.float32),
                                 np.zeros(0, np.float32), empty)


def test_is_faiss_file_knows_iwsq(tmp_path):
    p = tmp_path / "x.index"
    p.write_bytes(faiss_io.serialize_ivfsq(4, 2, 1, QT["QT_fp16"], 1, True, np.zeros((2, 4), np.float32),
                                           np.zeros(0, np.float32),
                                           [(np.zeros(0, np.int64), np.zeros((0, 8), np.uint8))] * 2))
    assert faiss_io.is_faiss_file(str(p))


# ------------------------------------------------- the reference against a brute force
def _brute_case(metric):
    rng = np.random.default_rng(21)  # (a seed at which every combination below has the gaps it asserts)
    d, nlist, nb, nq = 12, 4, 200, 3
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, nb)] + 0.5 * rng.standard_normal((nb, d))).astype(np.float32)
    xq = (cent[rng.integers(0, nlist, nq)] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    ids = rng.permutation(nb).astype(np.int64) * 3 + 7
    return cent, xb, xq, ids


@pytest.mark.parametrize("by_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("qtype", [R.QT_FP16, R.QT_8BIT, R.QT_8BIT_UNIFORM], ids=["fp16", "8bit", "uniform"])
@pytest.mark.parametrize("metric", [0, 1], ids=["ip", "l2"])
def test_reference_ranks_like_a_float64_brute_force(metric, qtype, by_residual):
    cent, xb, xq, ids = _brute_case(metric)
    k, nprobe = 5, 2
    ref = R.Ref(xb, cent, qtype, metric, by_residual, ids)
    keys, labels = ref.brute64(xq, k + 1, nprobe)
    D, I = ref.search(xq, k, nprobe)
    for q in range(len(xq)):
        assert len(keys[q]) == k + 1  # (two probed lists hold more than k rows)
        # consecutive float64 keys differ by more than 1e-4 relative, so float32 sums (relative
        # error about d * 2^-24 of the terms' magnitude) cannot change the order
        scale = np.maximum(np.abs(keys[q][1:]), np.abs(keys[q][:-1]))
        assert (np.diff(keys[q]) > 1e-4 * scale).all(), (q, keys[q])
        np.testing.assert_array_equal(I[q], labels[q][:k])
        got = -D[q] if metric == 0 else D[q]
        np.testing.assert_allclose(got, keys[q][:k], rtol=1e-5, atol=1e-5)


def test_reference_lists_residuals_and_preassigned_rules():
    from oracle import oracle as O

    cent, xb, xq, ids = _brute_case(0)
    ref = R.Ref(xb, cent, R.QT_8BIT, 0, True, ids)
    want_list = O.coarse_search(xb, cent, 1, metric=0)[1][:, 0]
    np.testing.assert_array_equal(ref.list_of, want_list)
    res = xb - cent[want_list]
    assert ref.trained.tobytes() == R.S.train(res, R.QT_8BIT).tobytes()
    assert ref.codes.tobytes() == R.S.encode(res, R.QT_8BIT, ref.trained).tobytes()
    for l, (li, lc) in enumerate(ref.lists()):
        assert (np.diff(li) > 0).all()
        sel = [int(np.nonzero(ids == i)[0][0]) for i in li]
        assert (want_list[sel] == l).all()
        np.testing.assert_array_equal(lc, ref.codes[sel])
    # search = search_preassigned with the oracle's probes and coarse values
    Dq, Iq = O.coarse_search(xq, cent, 3, metric=0)
    D0, I0 = ref.search(xq, 5, 3)
    D1, I1 = ref.search(xq, 5, Iq=Iq, Dq=Dq)
    assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes()
    # Dq = None is zeros: the similarities drop by the coarse value of each row's list
    D2, _ = ref.search(xq[:1], 200, Iq=Iq[:1])
    D3, _ = ref.search(xq[:1], 200, Iq=Iq[:1], Dq=np.zeros((1, 3), np.float32))
    assert D2.tobytes() == D3.tobytes() and D2.tobytes() != ref.search(xq[:1], 200, Iq=Iq[:1], Dq=Dq[:1])[0].tobytes()
    # a repeated list is scanned once (with its first column's value), -1 skips a probe
    Ir = np.array([[Iq[0, 0], Iq[0, 0], -1]])
    Da, Ia = ref.search(xq[:1], 200, Iq=Ir, Dq=np.array([[1.5, 99.0, 7.0]], np.float32))
    Db, Ib = ref.search(xq[:1], 200, Iq=np.array([[Iq[0, 0], -1, -1]]), Dq=np.array([[1.5, 0, 0]], np.float32))
    assert Da.tobytes() == Db.tobytes() and Ia.tobytes() == Ib.tobytes()
    n0 = len(ref.rows_of[Iq[0, 0]])
    assert (Ia[0, :n0] >= 0).all() and (Ia[0, n0:] == -1).all() and (Da[0, n0:] == -R.FMAX).all()
    assert len(set(Ia[0, :n0].tolist())) == n0
    # L2 ignores Dq
    ref2 = R.Ref(xb, cent, R.QT_FP16, 1, True, ids)
    Iq2 = O.coarse_search(xq, cent, 3, metric=1)[1]
    a = ref2.search(xq, 5, Iq=Iq2, Dq=np.full((len(xq), 3), 1e9, np.float32))
    b = ref2.search(xq, 5, Iq=Iq2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_reference_training_subsample():
    assert R.train_rows(100000).tolist() == list(range(100000))
    rows = R.train_rows(100500)
    assert rows.shape == (100000,) and len(set(rows.tolist())) == 100000
    assert rows.min() >= 0 and rows.max() < 100500 and (rows != np.arange(100000)).any()


# ---------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Per kernel of lib/ivf_sq.o's gfx950 code object: the compiler's metadata
    (as tests/test_indexsq_cpu.py reads sq_scan.o)."""
    assert os.path.exists(OBJ), f"{OBJ} missing: run __graft_entry__.build() first"
    tmp = tmp_path_factory.mktemp("co")
    fat, co = str(tmp / "fat.bin"), str(tmp / "kernels.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for rec in re.split(r"\n  - \.", notes):
        name = re.search(r"^    \.name:\s+(\S+)\s*$", rec, re.M)
        if not name:
            continue
        f = {}
        for key in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                    "private_segment_fixed_size", "group_segment_fixed_size"):
            v = re.search(rf"^\s+\.?{key}:\s+(\d+)\s*$", rec, re.M)
            f[key] = int(v.group(1)) if v else 0
        out[name.group(1)] = f
    return out


def test_kernels_use_no_scratch_and_spill_nothing_to_memory(kernels):
    """No kernel has a private segment or a VGPR spill.  (sgpr_spill_count is printed, not bounded:
    as in k_ivfflat_scan and k_sq_scan the wave-uniform state of the G pairs is parked in VGPR
    lanes, which costs no memory; only the small kernels are held to none.)"""
    for n, f in sorted(kernels.items()):
        print(n, f)
        assert f["private_segment_fixed_size"] == 0, (n, f)
        assert f["vgpr_spill_count"] == 0, (n, f)
        if "k_ivfsq_scan" not in n:
            assert f["sgpr_spill_count"] == 0, (n, f)
    for n in ("k_ivfsq_scan", "k_ivfsq_encode", "k_ivfsq_residuals"):
        assert any(n in name for name in kernels), n


def test_scan_kernels_cover_every_class_and_keep_their_occupancy(kernels):
    scans = {n: f for n, f in kernels.items() if "k_ivfsq_scan" in n}
    # (metric) x (codec) x (k <= 64, k <= 256, k <= 1024): template arguments <KIND, CODEC, G, R>
    assert len(scans) == 12, sorted(scans)
    classes = {tuple(int(v) for v in re.search(r"k_ivfsq_scanILi(\d)ELi(\d)ELi(\d+)ELi(\d+)E", n).groups()) for n in scans}
    assert classes == {(kind, codec, g, r) for kind in (0, 1) for codec in (0, 1)
                       for g, r in (((8 if codec == 0 else 4), 1), (4, 4), (4, 16))}
    for n, f in scans.items():
        # 160 KiB of LDS and 512 VGPRs per SIMD: two workgroups of four waves per CU up to k = 256,
        # one above (the sixteen top-k rows of four pairs), as the scans this one is built from
        rows = int(re.search(r"ELi(\d+)EEEv", n).group(1))
        assert f["group_segment_fixed_size"] <= 80 * 1024, (n, f)
        assert f["vgpr_count"] <= (256 if rows <= 4 else 512), (n, f)  # VGPRs + AGPRs of a wave
        fp16 = re.search(r"k_ivfsq_scanILi\dELi(\d)E", n).group(1) == "0"
        assert f["group_segment_fixed_size"] >= 256 * (144 if fp16 else 80), (n, f)  # the code tile
