"""IndexFlat without a GPU: the C-ABI symbols, the argument checks made before any device
call, the factory key, the "IxF2" / "IxFI" file layout, the host role of the index (the IVF
quantizer: no GPU and no library), the growth of its buffer, the shared reference of the GPU
tests against float64, the constants the GPU tests import against csrc/flat_scan.h, and the
scan kernel's resources read from the built code object."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import faiss_amd as faiss
import indexflat_ref as R
from faiss_amd import _lib, faiss_io
from faiss_amd import index as fidx

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "flat_scan.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2

SYMBOLS = ["create", "free", "reset", "add", "add_device", "search", "search_device", "ntotal", "get_dims", "get_rows",
           "get_stats", "set_range_rows", "get_plan"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, "ivfpq_flat_index_" + n), n
        assert "ivfpq_flat_index_" + n in _lib.SIGNATURES, n
    assert hasattr(lib, "ivfpq_flat_search") and "ivfpq_flat_search" in _lib.SIGNATURES  # the stateless call stays
    assert faiss.IndexFlat is fidx.IndexFlat
    assert issubclass(faiss.IndexFlatL2, faiss.IndexFlat) and issubclass(faiss.IndexFlatIP, faiss.IndexFlatL2)


@pytest.mark.parametrize("d,metric,word", [(0, 1, "at least 1"), (-4, 1, "at least 1"), (32, 7, "metric"),
                                           (32, -1, "metric")])
def test_create_rejects_bad_shapes_before_any_device_call(d, metric, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ivfpq_flat_index_create(0, d, metric, ctypes.byref(h)) != 0
    assert word in lib.ivfpq_last_error().decode()
    assert not h.value
    assert lib.ivfpq_flat_index_create(0, 32, 1, None) != 0
    assert "null" in lib.ivfpq_last_error().decode()


def test_python_constructor_rejects_an_unknown_metric():
    with pytest.raises(RuntimeError, match="metric"):
        faiss.IndexFlat(8, 7)


def test_create_without_device_fails_with_a_message():
    lib = _lib.load()
    if lib.ivfpq_device_count() > 0:
        pytest.skip("a device is present")
    h = ctypes.c_void_p()
    assert lib.ivfpq_flat_index_create(0, 32, L2, ctypes.byref(h)) != 0
    assert lib.ivfpq_last_error().decode() != ""
    assert not h.value


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.load()
    x = np.zeros((1, 4), np.float32)
    D, I = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64)
    f32p, i64p = _lib.c_f32p, _lib.c_i64p
    assert lib.ivfpq_flat_index_ntotal(None) == -1
    assert lib.ivfpq_flat_index_free(None) == 0
    for rc in (lib.ivfpq_flat_index_reset(None), lib.ivfpq_flat_index_add(None, 1, x.ctypes.data_as(f32p)),
               lib.ivfpq_flat_index_add_device(None, 1, None, None),
               lib.ivfpq_flat_index_get_dims(None, None, None),
               lib.ivfpq_flat_index_get_rows(None, 0, 1, x.ctypes.data_as(f32p)),
               lib.ivfpq_flat_index_get_stats(None, None, None, None),
               lib.ivfpq_flat_index_set_range_rows(None, 128),
               lib.ivfpq_flat_index_search(None, 1, x.ctypes.data_as(f32p), 1, D.ctypes.data_as(f32p),
                                           I.ctypes.data_as(i64p)),
               lib.ivfpq_flat_index_search_device(None, 1, None, 1, None, None, None)):
        assert rc != 0
        assert lib.ivfpq_last_error().decode() != ""
    assert lib.ivfpq_flat_index_search(None, 1, x.ctypes.data_as(f32p), 1, D.ctypes.data_as(f32p),
                                       I.ctypes.data_as(i64p)) != 0
    assert "null index handle" in lib.ivfpq_last_error().decode()
    # k is checked before the handle, and before any device call
    for k in (0, 1025):
        assert lib.ivfpq_flat_index_search(None, 1, x.ctypes.data_as(f32p), k, D.ctypes.data_as(f32p),
                                           I.ctypes.data_as(i64p)) != 0
        assert "k must be in [1, 1024]" in lib.ivfpq_last_error().decode()


def test_factory_key():
    ix = faiss.index_factory(24, "Flat")
    assert type(ix) is faiss.IndexFlat and ix.metric_type == L2 and ix.d == 24 and ix.ntotal == 0 and ix.is_trained
    iy = faiss.index_factory(24, " Flat", IP)
    assert type(iy) is faiss.IndexFlat and iy.metric_type == IP
    # the other parsers are unchanged
    assert fidx.parse_ivfflat_factory("Flat") is None
    assert fidx.parse_pq_factory("Flat") is None
    assert fidx.parse_sq_factory("Flat") is None
    with pytest.raises(RuntimeError):
        fidx.parse_factory("Flat")
    with pytest.raises(RuntimeError):
        faiss.index_factory(24, "Flat16")
    assert "Flat" in faiss.index_factory.__doc__


def test_plan_is_host_arithmetic():
    p = fidx.flat_search_plan(1024, 1_000_000, 10)
    assert p["tile_q"] == R.TILE_Q and p["range_rows"] % R.RANGE_GRANULE == 0
    assert p["ranges"] == -(-1_000_000 // p["range_rows"]) <= p["S"]
    assert p["ranges"] * -(-1024 // R.TILE_Q) >= 768  # three workgroups for each of 256 CUs
    one = fidx.flat_search_plan(1, 1_000_000, 64)
    assert one["ranges"] >= 768 and one["range_rows"] == R.RANGE_GRANULE and one["tile_q"] == R.TILE_Q_NARROW
    forced = fidx.flat_search_plan(9, 3 * R.RANGE_GRANULE + 5, 10, range_rows=R.TILE_ROWS)
    assert (forced["range_rows"], forced["ranges"], forced["S"], forced["fan"], forced["rounds"]) == (128, 25, 32, 16, 2)
    assert [fidx.flat_search_plan(nq, 5000, 10)["tile_q"] for nq in (1, 16, 17, 1000)] == [16, 16, 64, 64]
    assert fidx.flat_search_plan(100, 5000, R.WIDE_MAX_K)["tile_q"] == R.TILE_Q
    assert fidx.flat_search_plan(100, 5000, R.WIDE_MAX_K + 1)["tile_q"] == R.TILE_Q_NARROW
    big = fidx.flat_search_plan(1024, 1_000_000, 1000)
    assert big["ranges"] * -(-1024 // R.TILE_Q_NARROW) >= 768 and big["fan"] == 2
    with pytest.raises(RuntimeError, match="k must be"):
        fidx.flat_search_plan(9, 5000, 1025)


# ------------------------------------------------------------------ file layout
def hand_assembled(d, metric, xb):
    """Faiss's write_index of an IndexFlat: fourcc, write_index_header, xb as a vector."""
    b = (b"IxF2" if metric == L2 else b"IxFI")
    b += struct.pack("<i", d) + struct.pack("<q", xb.shape[0]) + struct.pack("<qq", 1 << 20, 1 << 20)
    b += struct.pack("<B", 1) + struct.pack("<i", metric)
    return b + struct.pack("<Q", xb.size) + xb.tobytes()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_file_layout_and_roundtrip_without_a_gpu(tmp_path, metric, n):
    d = 12
    xb = np.random.default_rng(n + metric).standard_normal((n, d)).astype(np.float32)
    buf = hand_assembled(d, metric, xb)
    z = faiss_io.parse_index(buf)
    assert (z["kind"], z["d"], z["ntotal"], z["metric"], z["is_trained"]) == ("flat", d, n, metric, True)
    np.testing.assert_array_equal(z["xb"], xb)
    ix = faiss.IndexFlat(d, metric)
    for lo in range(0, n, 300):
        ix.add(xb[lo:lo + 300])
    p = str(tmp_path / "flat.index")
    faiss.write_index(ix, p)
    assert open(p, "rb").read() == buf
    assert faiss_io.is_faiss_file(p)
    iy = faiss.read_index(p, device=0)
    assert type(iy) is (faiss.IndexFlatL2 if metric == L2 else faiss.IndexFlatIP)
    assert iy.d == d and iy.ntotal == n and iy.metric_type == metric
    np.testing.assert_array_equal(iy.xb, xb.reshape(-1))
    assert ix._h is None and iy._h is None  # no device image was made
    with pytest.raises(RuntimeError, match="Faiss layout"):
        faiss.write_index(ix, p, fmt="native")


def test_file_errors_name_the_problem(tmp_path):
    xb = np.arange(40, dtype=np.float32).reshape(5, 8)
    buf = hand_assembled(8, L2, xb)
    with pytest.raises(RuntimeError, match="truncated"):
        faiss_io.parse_index(buf[:-3])
    with pytest.raises(RuntimeError, match="truncated"):
        faiss_io.parse_index(buf[:20])
    with pytest.raises(RuntimeError, match="trailing"):
        faiss_io.parse_index(buf + b"\0")
    with pytest.raises(RuntimeError, match="ntotal"):
        faiss_io.parse_index(buf[:4] + struct.pack("<i", 8) + struct.pack("<q", 6) + buf[16:])
    with pytest.raises(RuntimeError, match="metric"):
        faiss_io.parse_index(b"IxFI" + buf[4:])
    with pytest.raises(RuntimeError, match="fourcc"):
        faiss_io.parse_ivfpq(buf)  # the IVF-PQ parser keeps rejecting a flat file
    p = tmp_path / "flat.index"
    p.write_bytes(buf)
    with pytest.raises(RuntimeError, match="IxF2"):
        faiss.read_index_binary(str(p))
    p.write_bytes(buf[:-3])
    with pytest.raises(RuntimeError, match="truncated"):
        faiss.read_index(str(p), device=0)


# ------------------------------------------------------------------ the host role
@pytest.mark.parametrize("cls", [faiss.IndexFlatL2, faiss.IndexFlatIP])
def test_host_surface_needs_no_library(cls, monkeypatch):
    def no_library():
        raise AssertionError("the host role must not load the library")

    monkeypatch.setattr(_lib, "load", no_library)
    rng = np.random.default_rng(5)
    d = 7
    ix = cls(d, device=0)
    assert ix.ntotal == 0 and ix.xb.shape == (0,) and ix.metric_type == cls.metric_type
    parts = [rng.standard_normal((n, d)).astype(np.float32) for n in rng.integers(1, 90, 20)]
    for part in parts:
        ix.add(part)
    xb = np.concatenate(parts)
    assert ix.ntotal == len(xb)
    np.testing.assert_array_equal(ix.xb, xb.reshape(-1))
    np.testing.assert_array_equal(ix.reconstruct(17), xb[17])
    np.testing.assert_array_equal(ix.reconstruct_n(30, 50), xb[30:80])
    with pytest.raises(RuntimeError):
        ix.reconstruct(len(xb))
    with pytest.raises(RuntimeError):
        ix.add(np.zeros((3, d + 1), np.float32))
    ix.train(xb)
    ix.reset()
    assert ix.ntotal == 0 and ix.xb.shape == (0,)
    ix.add(parts[0])
    np.testing.assert_array_equal(ix.xb, parts[0].reshape(-1))
    assert ix._h is None and ix.uploaded_rows() == 0


def test_add_is_linear_the_buffer_grows_geometrically():
    ix = faiss.IndexFlatIP(16)
    block = np.random.default_rng(7).standard_normal((500, 16)).astype(np.float32)
    caps = set()
    for i in range(200):
        ix.add(block + i)
        caps.add(ix.capacity)
        assert ix.capacity >= ix.ntotal
    assert ix.ntotal == 100_000
    assert len(caps) <= 10  # 500 -> 1000 -> ... -> 128000: log2(200) + 1 reallocations, not 200
    assert ix.capacity < 2 * ix.ntotal + 64
    np.testing.assert_array_equal(ix.reconstruct_n(99_500, 500), block + 199)
    np.testing.assert_array_equal(ix.reconstruct_n(0, 500), block)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_equals_float64_on_integer_data(metric):
    rng = np.random.default_rng(11)
    xb = rng.integers(0, 20, (700, 24)).astype(np.float32)
    xb[100:160] = xb[100]  # a block of exact ties
    xq = rng.integers(0, 20, (9, 24)).astype(np.float32)
    xq[0] = xb[100]
    for k in (1, 12, 100):
        D, I = R.search(xq, xb, k, metric)
        D64, I64 = R.search64(xq, xb, k, metric)
        np.testing.assert_array_equal(I, I64)
        np.testing.assert_array_equal(D, D64)
    if metric == L2:
        D, I = R.search(xq[:1], xb, 60, metric)
        assert (I[0] == np.arange(100, 160)).all() and (D[0] == 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_pads_and_handles_an_empty_base(metric):
    xq = np.ones((3, 5), np.float32)
    D, I = R.search(xq, np.zeros((0, 5), np.float32), 4, metric)
    assert (I == -1).all() and (D == R.pad(metric)).all() and D.dtype == np.float32 and I.dtype == np.int64
    D, I = R.search(xq, np.eye(5, dtype=np.float32)[:2], 4, metric)
    assert (I[:, 2:] == -1).all() and (D[:, 2:] == R.pad(metric)).all() and (I[:, :2] >= 0).all()
    assert R.pad(L2) == np.finfo(np.float32).max and R.pad(IP) == -np.finfo(np.float32).max


def test_constants_match_the_header():
    assert R.header_constant("kFlatTileQ") == R.TILE_Q
    assert R.header_constant("kFlatTileRows") == R.TILE_ROWS
    assert R.header_constant("kFlatKc") == R.K_CHUNK
    assert R.header_constant("kFlatRangeGranule") == R.RANGE_GRANULE
    assert R.header_constant("kFlatTileQNarrow") == R.TILE_Q_NARROW
    assert R.header_constant("kFlatWideMaxK") == R.WIDE_MAX_K
    assert R.RANGE_GRANULE % R.TILE_ROWS == 0


# ------------------------------------------------------------------ kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Per kernel of lib/flat_scan.o's gfx950 code object: the compiler's metadata (as
    tests/test_ivfflat_cpu.py reads ivf_flat.o)."""
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


def test_scan_uses_no_scratch_and_fits_the_stated_workgroups_per_cu(kernels):
    """DESIGN.md section 4f's table: workgroups of 256 threads per CU (= waves per SIMD) of
    every instantiation <R, VEC, TQ> (rows of 64 per list, aligned rows, query tile).  A SIMD
    has 512 registers per lane (VGPRs and AGPRs are one file on gfx950: vgpr_count is their
    sum), a CU 160 KiB of LDS."""
    scans = {n: f for n, f in kernels.items() if "k_flat_scan" in n}
    assert len(scans) == 10, sorted(scans)
    stated = {("1", "1", "64"): 3, ("1", "0", "64"): 2, ("4", "1", "64"): 1, ("4", "0", "64"): 1,
              ("1", "1", "16"): 3, ("1", "0", "16"): 2, ("4", "1", "16"): 2, ("4", "0", "16"): 2,
              ("16", "1", "16"): 1, ("16", "0", "16"): 1}
    for n, f in scans.items():
        print(n, f)
        assert f["private_segment_fixed_size"] == 0, (n, f)
        assert f["vgpr_spill_count"] == 0, (n, f)
        m = re.search(r"k_flat_scanILi(\d+)ELb([01])ELi(\d+)E", n)
        assert m, n
        wgs = stated[m.groups()]
        assert f["vgpr_count"] <= 512 // wgs // 8 * 8, (n, f, wgs)
        assert f["group_segment_fixed_size"] <= 160 * 1024 // wgs, (n, f, wgs)
