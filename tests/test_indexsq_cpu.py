"""IndexScalarQuantizer without a GPU: the C-ABI symbols, the argument checks made before any
device call, the factory keys, the "IxSQ" file layout, the shared reference of the GPU tests
against itself, and the scan kernels' resources read from the built code object."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import faiss_amd as faiss
import indexsq_ref as R
from faiss_amd import _lib, faiss_io
from faiss_amd import index as fidx

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "csrc")
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "sq_scan.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

SYMBOLS = ["create", "free", "train", "set_trained", "add", "add_device", "add_codes", "reset", "search",
           "search_device", "ntotal", "is_trained", "get_dims", "get_trained", "get_codes", "encode", "decode"]
QT = {"QT_8bit": 0, "QT_4bit": 1, "QT_8bit_uniform": 2, "QT_4bit_uniform": 3, "QT_fp16": 4, "QT_8bit_direct": 5,
      "QT_6bit": 6}
UNSUPPORTED = ["QT_4bit", "QT_4bit_uniform", "QT_8bit_direct", "QT_6bit"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, "ivfpq_sq_" + n), n
        assert "ivfpq_sq_" + n in _lib.SIGNATURES, n
    assert faiss.IndexScalarQuantizer is fidx.IndexScalarQuantizer
    for name, value in QT.items():  # beir looks the type up with getattr: all seven names exist
        assert getattr(faiss.ScalarQuantizer, name) == value


@pytest.mark.parametrize("d,qtype,metric,word", [(6, 4, 1, "multiple of 4"), (0, 4, 1, "multiple of 4"),
                                                 (2052, 0, 1, "2048"), (32, 4, 7, "metric"), (32, 9, 1, "9")] +
                         [(32, QT[n], 1, n) for n in UNSUPPORTED])
def test_create_rejects_bad_arguments_before_any_device_call(d, qtype, metric, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ivfpq_sq_create(d, qtype, metric, 0, ctypes.byref(h)) != 0
    assert word in lib.ivfpq_last_error().decode()
    assert not h.value
    with pytest.raises(RuntimeError, match=word):
        faiss.IndexScalarQuantizer(d, qtype, metric)


def test_create_without_device_fails_with_a_message():
    lib = _lib.load()
    if lib.ivfpq_device_count() > 0:
        pytest.skip("a device is present")
    h = ctypes.c_void_p()
    assert lib.ivfpq_sq_create(32, QT["QT_fp16"], faiss.METRIC_L2, 0, ctypes.byref(h)) != 0
    assert lib.ivfpq_last_error().decode() != ""
    assert not h.value


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.load()
    assert lib.ivfpq_sq_ntotal(None) == -1
    assert lib.ivfpq_sq_is_trained(None) == 0
    x = np.zeros((1, 8), np.float32)
    c = np.zeros((1, 16), np.uint8)
    D, I = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64)
    fp, up, ip = _lib.c_f32p, _lib.c_u8p, _lib.c_i64p
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    calls = [lambda: lib.ivfpq_sq_reset(None), lambda: lib.ivfpq_sq_train(None, 1, p(x, fp)),
             lambda: lib.ivfpq_sq_set_trained(None, p(x, fp), 0), lambda: lib.ivfpq_sq_add(None, 1, p(x, fp)),
             lambda: lib.ivfpq_sq_add_device(None, 1, None, None), lambda: lib.ivfpq_sq_add_codes(None, 1, p(c, up)),
             lambda: lib.ivfpq_sq_search(None, 1, p(x, fp), 1, p(D, fp), p(I, ip)),
             lambda: lib.ivfpq_sq_search_device(None, 1, None, 1, None, None, None),
             lambda: lib.ivfpq_sq_get_dims(None, None, None, None, None),
             lambda: lib.ivfpq_sq_get_trained(None, None, None), lambda: lib.ivfpq_sq_get_codes(None, 0, 0, p(c, up)),
             lambda: lib.ivfpq_sq_encode(None, 1, p(x, fp), p(c, up)),
             lambda: lib.ivfpq_sq_decode(None, 1, p(c, up), p(x, fp))]
    for call in calls:
        assert call() != 0
        assert "null index handle" in lib.ivfpq_last_error().decode()
    assert lib.ivfpq_sq_free(None) == 0


def test_factory_keys():
    assert fidx.parse_sq_factory("SQ8") == QT["QT_8bit"]
    assert fidx.parse_sq_factory("SQfp16") == QT["QT_fp16"]
    assert fidx.parse_sq_factory(" SQ8 ") == QT["QT_8bit"]
    for key in ("PQ16", "IVF8,Flat", "IVF8,SQ8", "Flat", "OPQ16,PQ16", "IVF1024,PQ16"):
        assert fidx.parse_sq_factory(key) is None, key
    for key in ("SQ4", "SQ6"):
        with pytest.raises(RuntimeError, match=key):
            fidx.parse_sq_factory(key)
        with pytest.raises(RuntimeError, match=key):
            faiss.index_factory(32, key)
    # the other parsers are unchanged
    assert fidx.parse_pq_factory("SQ8") is None and fidx.parse_ivfflat_factory("SQ8") is None
    assert fidx.parse_pq_factory("PQ16") == (16, 8) and fidx.parse_ivfflat_factory("IVF8,Flat") == 8
    with pytest.raises(RuntimeError):
        fidx.parse_factory("SQ8")
    # index_factory reaches IndexScalarQuantizer's own argument checks
    with pytest.raises(RuntimeError, match="multiple of 4"):
        faiss.index_factory(30, "SQ8")


@pytest.mark.parametrize("qname", ["QT_fp16", "QT_8bit", "QT_8bit_uniform"])
def test_ixsq_layout_and_round_trip(qname):
    rng = np.random.default_rng(5)
    qtype, d, n = QT[qname], 12, 7
    xb = rng.standard_normal((n, d)).astype(np.float32)
    trained = R.train(xb, qtype)
    codes = R.encode(xb, qtype, trained)
    cs = R.code_size(qtype, d)
    assert codes.shape == (n, cs) and trained.size == {"QT_fp16": 0, "QT_8bit": 2 * d, "QT_8bit_uniform": 2}[qname]
    buf = faiss_io.serialize_sq(d, qtype, faiss.METRIC_INNER_PRODUCT, trained, codes)
    want = b"".join([b"IxSQ", struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, 1, 0),
                     struct.pack("<i", qtype), struct.pack("<i", 0), struct.pack("<f", 0.0),
                     struct.pack("<Q", d), struct.pack("<Q", cs),
                     struct.pack("<Q", trained.size), trained.tobytes(),
                     struct.pack("<Q", n * cs), codes.tobytes()])
    assert buf == want
    z = faiss_io.parse_index(buf)
    assert (z["kind"], z["d"], z["ntotal"], z["qtype"], z["metric"], z["is_trained"], z["code_size"]) == \
        ("sq", d, n, qtype, faiss.METRIC_INNER_PRODUCT, True, cs)
    assert z["trained"].dtype == np.float32 and z["trained"].tobytes() == trained.tobytes()
    np.testing.assert_array_equal(z["codes"], codes)
    assert faiss_io.serialize_sq(d, qtype, z["metric"], z["trained"], z["codes"]) == buf
    for cut in (3, 20, 40, len(buf) // 2, len(buf) - 1):
        with pytest.raises(RuntimeError):
            faiss_io.parse_index(buf[:cut])
    with pytest.raises(RuntimeError):
        faiss_io.parse_index(buf + b"\0")
    # wrapped in an IndexPreTransform
    A = rng.standard_normal((d, 16)).astype(np.float32)
    wrapped = faiss_io.serialize_pretransform(16, 0, [(A, None, 16, d, True)], buf, n)
    zw = faiss_io.parse_index(wrapped)
    assert zw["kind"] == "pretransform" and zw["index"]["kind"] == "sq"
    np.testing.assert_array_equal(zw["index"]["codes"], codes)


def test_ixsq_rejects_other_quantizer_types_and_shapes():
    d = 8
    good = faiss_io.serialize_sq(d, QT["QT_8bit"], 1, np.zeros(2 * d, np.float32), np.zeros((2, d), np.uint8))
    at = 4 + struct.calcsize("<iqqqBi")
    for name in UNSUPPORTED:
        bad = good[:at] + struct.pack("<i", QT[name]) + good[at + 4:]
        with pytest.raises(RuntimeError, match="unsupported scalar quantizer"):
            faiss_io.parse_index(bad)
    bad = good[:at + 4] + struct.pack("<i", 1) + good[at + 8:]  # another range statistic
    with pytest.raises(RuntimeError, match="RS_minmax"):
        faiss_io.parse_index(bad)
    bad = good[:at + 12] + struct.pack("<Q", d + 4) + good[at + 20:]  # the quantizer's own d
    with pytest.raises(RuntimeError, match="shape"):
        faiss_io.parse_index(bad)
    with pytest.raises(RuntimeError):
        faiss_io.serialize_sq(d, QT["QT_4bit"], 1, np.zeros(0, np.float32), np.zeros((0, d), np.uint8))


def test_is_faiss_file_knows_ixsq(tmp_path):
    p = tmp_path / "x.sq"
    p.write_bytes(faiss_io.serialize_sq(4, QT["QT_fp16"], 1, np.zeros(0, np.float32), np.zeros((0, 8), np.uint8)))
    assert faiss_io.is_faiss_file(str(p))


# ------------------------------------------------- the reference against itself
def test_reference_training_is_numpy_min_max():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((300, 12)).astype(np.float32)
    t = R.train(x, R.QT_8BIT)
    assert t.dtype == np.float32 and t[:12].tobytes() == x.min(0).tobytes()
    assert t[12:].tobytes() == (x.max(0) - x.min(0)).astype(np.float32).tobytes()
    u = R.train(x, R.QT_8BIT_UNIFORM)
    assert u.tobytes() == np.array([x.min(), x.max() - x.min()], np.float32).tobytes()
    assert R.train(x, R.QT_FP16).size == 0
    vmin, vdiff = R.expand(u, R.QT_8BIT_UNIFORM, 12)
    assert (vmin == u[0]).all() and (vdiff == u[1]).all() and vmin.shape == (12,)


def test_reference_constant_dimension_and_clamping():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((200, 8)).astype(np.float32)
    x[:, 2] = np.float32(1.75)
    t = R.train(x, R.QT_8BIT)
    codes = R.encode(x, R.QT_8BIT, t)
    assert (codes[:, 2] == 0).all()  # vdiff = 0: code 0 ...
    assert (R.decode(codes, R.QT_8BIT, t, 8)[:, 2] == np.float32(1.75)).all()  # ... and the constant back
    for qtype, tt in ((R.QT_8BIT, t), (R.QT_8BIT_UNIFORM, R.train(x, R.QT_8BIT_UNIFORM))):
        far = np.stack([np.full(8, x.min() - 5, np.float32), np.full(8, x.max() + 5, np.float32)])
        c = R.encode(far, qtype, tt)
        keep = np.arange(8) != 2 if qtype == R.QT_8BIT else np.arange(8) >= 0
        assert (c[0] == 0).all() and (c[1][keep] == 255).all()
    # the extremes of the training set themselves: codes 0 and 255
    c = R.encode(np.stack([x.min(0), x.max(0)]), R.QT_8BIT, t)
    assert (c[0] == 0).all() and (c[1][np.arange(8) != 2] == 255).all()


@pytest.mark.parametrize("qtype", [R.QT_8BIT, R.QT_8BIT_UNIFORM])
def test_reference_8bit_reconstruction_error(qtype):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4000, 16)).astype(np.float32)
    t = R.train(x, qtype)
    _, vdiff = R.expand(t, qtype, 16)
    y = R.decode(R.encode(x, qtype, t), qtype, t, 16)
    err = np.abs(y.astype(np.float64) - x.astype(np.float64))
    # half a quantization step, (vdiff / 255) / 2, plus the roundings
    assert (err <= vdiff.astype(np.float64)[None] / 510 * 1.001).all(), (err / (vdiff / 510)).max()


def test_reference_fp16_round_trips_a_subnormal_and_minus_zero():
    x = np.array([[3e-6, -0.0, -3e-6, 1.0, 65504.0, 0.1, -2.5, 0.0]], np.float32)
    codes = R.encode(x, R.QT_FP16, np.zeros(0, np.float32))
    assert codes.shape == (1, 16)
    y = R.decode(codes, R.QT_FP16, np.zeros(0, np.float32), 8)
    h = x.astype(np.float16)
    assert y.tobytes() == h.astype(np.float32).tobytes()
    assert y[0, 0] != 0 and abs(y[0, 0] - 3e-6) < 3e-8  # a half subnormal (2^-24 steps)
    assert y[0, 1] == 0 and np.signbit(y[0, 1])
    assert R.encode(y, R.QT_FP16, np.zeros(0, np.float32)).tobytes() == codes.tobytes()


@pytest.mark.parametrize("metric", [0, 1], ids=["ip", "l2"])
def test_reference_search_against_the_oracle_entry_by_entry(metric):
    from oracle import oracle as O

    rng = np.random.default_rng(10)
    d, nb, nq, k = 12, 50, 4, 7
    xb = rng.integers(0, 3, (nb, d)).astype(np.float32)  # few values: tied distances
    xq = rng.integers(0, 3, (nq, d)).astype(np.float32)
    ref = R.Ref(xb, R.QT_8BIT, metric)
    D, I = ref.search(xq, k)
    for q in range(nq):
        cand = [(O.tree(xq[q], ref.dec[i], metric), i) for i in range(nb)]
        cand.sort(key=lambda t: (-t[0] if metric == 0 else t[0], t[1]))
        np.testing.assert_array_equal(I[q], [c[1] for c in cand[:k]])
        np.testing.assert_array_equal(D[q], np.array([c[0] for c in cand[:k]], np.float32))
    D, I = ref.search(xq, 64)  # fewer vectors than k: padded
    assert (I[:, nb:] == -1).all() and (D[:, nb:] == (-R.FMAX if metric == 0 else R.FMAX)).all()


def test_range_granule_matches_the_header():
    with open(os.path.join(CSRC, "ivf_flat.h")) as f:
        m = re.search(r"constexpr\s+int\s+kIvfFlatRangeRows\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) == R.RANGE_ROWS


# ---------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Per kernel of lib/sq_scan.o's gfx950 code object: the compiler's metadata
    (as tests/test_ivfflat_cpu.py reads ivf_flat.o)."""
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
        for key in ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                    "group_segment_fixed_size"):
            v = re.search(rf"^\s+\.?{key}:\s+(\d+)\s*$", rec, re.M)
            f[key] = int(v.group(1)) if v else 0
        out[name.group(1)] = f
    return out


def test_scan_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(kernels):
    scans = {n: f for n, f in kernels.items() if "k_sq_scan" in n}
    # (metric) x (codec) x (k <= 64, k <= 256, k <= 1024): template arguments <KIND, CODEC, G, R>
    assert len(scans) == 12, sorted(scans)
    for n, f in scans.items():
        print(n, f)
        assert f["private_segment_fixed_size"] == 0, (n, f)
        assert f["vgpr_spill_count"] == 0, (n, f)
    small = {n: f for n, f in scans.items() if re.search(r"k_sq_scanILi[01]ELi[01]ELi\d+ELi1E", n)}
    assert len(small) == 4, sorted(small)
    for n, f in small.items():
        assert f["group_segment_fixed_size"] <= 80 * 1024, (n, f)
        assert f["vgpr_count"] <= 256, (n, f)  # VGPRs + AGPRs of a wave: two waves per SIMD
    for n in ("k_sq_encode", "k_sq_decode", "k_sq_minmax"):
        assert any(n in name for name in kernels), n
