"""IndexIVFFlat without a GPU: the C-ABI symbols, the argument checks made before any
device call, the "IwFl" file layout, the factory key, the shared reference of the GPU tests
against the oracle, and the scan kernel's resources read from the built code object."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib, faiss_io
from faiss_amd import index as fidx

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "csrc")
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "ivf_flat.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

SYMBOLS = ["create", "free", "train", "set_trained", "add", "add_device", "reset", "set_nprobe", "get_nprobe",
           "search", "search_device", "search_preassigned", "search_preassigned_device", "ntotal", "is_trained",
           "get_dims", "get_centroids", "get_list_sizes", "get_list"]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, "ivfpq_ivfflat_" + n), n
        assert "ivfpq_ivfflat_" + n in _lib.SIGNATURES, n
    assert faiss.IndexIVFFlat is fidx.IndexIVFFlat


@pytest.mark.parametrize("d,nlist,metric,word", [(6, 8, 1, "multiple of 4"), (0, 8, 1, "multiple of 4"),
                                                 (2052, 8, 1, "2048"), (32, 0, 1, "nlist"), (32, 8, 7, "metric")])
def test_create_rejects_bad_shapes_before_any_device_call(d, nlist, metric, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ivfpq_ivfflat_create(d, nlist, metric, 0, ctypes.byref(h)) != 0
    assert word in lib.ivfpq_last_error().decode()
    assert not h.value
    with pytest.raises(RuntimeError, match=word):
        faiss.IndexIVFFlat(None, d, nlist, metric)


def test_create_without_device_fails_with_a_message():
    lib = _lib.load()
    if lib.ivfpq_device_count() > 0:
        pytest.skip("a device is present")
    h = ctypes.c_void_p()
    assert lib.ivfpq_ivfflat_create(32, 8, faiss.METRIC_L2, 0, ctypes.byref(h)) != 0
    assert lib.ivfpq_last_error().decode() != ""
    assert not h.value


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.load()
    assert lib.ivfpq_ivfflat_ntotal(None) == -1
    assert lib.ivfpq_ivfflat_is_trained(None) == 0
    assert lib.ivfpq_ivfflat_get_nprobe(None) == -1
    assert lib.ivfpq_ivfflat_reset(None) != 0
    assert lib.ivfpq_ivfflat_free(None) == 0


def test_factory_keys():
    assert fidx.parse_ivfflat_factory("IVF1024,Flat") == 1024
    assert fidx.parse_ivfflat_factory("IVF1,Flat") == 1
    assert fidx.parse_ivfflat_factory(" IVF8, Flat") == 8
    for key in ("IVF1024,PQ16", "PQ16", "Flat", "IVF,Flat", "IVF8,Flat16", "OPQ16,IVF8,Flat"):
        assert fidx.parse_ivfflat_factory(key) is None, key
    with pytest.raises(RuntimeError):
        fidx.parse_factory("IVF8,Flat")  # the IVF-PQ parser itself is unchanged
    # index_factory reaches IndexIVFFlat's own argument checks
    with pytest.raises(RuntimeError, match="multiple of 4"):
        faiss.index_factory(30, "IVF8,Flat")


def _lists(rng, d, sizes):
    out, nxt = [], 0
    for n in sizes:
        ids = rng.permutation(1000)[:n].astype(np.int64) + nxt
        out.append((np.sort(ids), rng.standard_normal((n, d)).astype(np.float32)))
        nxt += 1000
    return out


@pytest.mark.parametrize("sizes", [(3, 0, 5, 1), (0, 0, 0, 2)], ids=["full", "sprs"])
def test_iwfl_layout_and_round_trip(sizes):
    rng = np.random.default_rng(5)
    d, nlist, nprobe = 12, len(sizes), 3
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    lists = _lists(rng, d, sizes)
    ntot = sum(sizes)
    buf = faiss_io.serialize_ivfflat(d, nlist, nprobe, faiss.METRIC_L2, cent, lists)
    hdr = lambda dd, n: struct.pack("<iqqqBi", dd, n, 1 << 20, 1 << 20, 1, 1)  # noqa: E731
    nz = [l for l in range(nlist) if sizes[l]]
    if len(nz) > nlist // 2:
        table = b"full" + struct.pack("<Q", nlist) + np.array(sizes, np.uint64).tobytes()
    else:
        table = b"sprs" + struct.pack("<Q", 2 * len(nz)) + b"".join(struct.pack("<QQ", l, sizes[l]) for l in nz)
    want = b"".join([b"IwFl", hdr(d, ntot), struct.pack("<QQ", nlist, nprobe),
                     b"IxF2", hdr(d, nlist), struct.pack("<Q", cent.size), cent.tobytes(),
                     struct.pack("<B", 0), struct.pack("<Q", 0),
                     b"ilar", struct.pack("<QQ", nlist, 4 * d), table] +
                    [v.tobytes() + i.tobytes() for i, v in lists if len(i)])
    assert buf == want
    z = faiss_io.parse_index(buf)
    assert (z["kind"], z["d"], z["nlist"], z["nprobe"], z["metric"], z["is_trained"]) == \
        ("ivfflat", d, nlist, nprobe, faiss.METRIC_L2, True)
    np.testing.assert_array_equal(z["centroids"], cent)
    for (ids, vecs), (zi, zv) in zip(lists, z["lists"]):
        np.testing.assert_array_equal(zi, ids)
        assert zv.dtype == np.float32 and zv.shape == vecs.shape
        assert zv.tobytes() == vecs.tobytes()
    for cut in (3, 40, len(buf) // 2, len(buf) - 1):
        with pytest.raises(RuntimeError):
            faiss_io.parse_index(buf[:cut])
    with pytest.raises(RuntimeError):
        faiss_io.parse_index(buf + b"\0")


def test_is_faiss_file_knows_iwfl(tmp_path):
    p = tmp_path / "x.index"
    p.write_bytes(faiss_io.serialize_ivfflat(4, 2, 1, 1, np.zeros((2, 4), np.float32),
                                             [(np.zeros(0, np.int64), np.zeros((0, 4), np.float32))] * 2))
    assert faiss_io.is_faiss_file(str(p))


@pytest.mark.parametrize("metric", [0, 1], ids=["ip", "l2"])
def test_shared_reference_against_the_oracle_entry_by_entry(metric):
    import ivfflat_ref as R
    from oracle import oracle as O

    rng = np.random.default_rng(6)
    d, nlist, nb, nq, nprobe, k = 12, 4, 60, 5, 2, 7
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    xb = rng.integers(0, 3, (nb, d)).astype(np.float32)  # few values: tied distances
    xq = rng.integers(0, 3, (nq, d)).astype(np.float32)
    ids = rng.permutation(nb).astype(np.int64) + 100
    ref = R.Ref(xb, cent, metric, ids)
    want_list = np.array([O.coarse_search(xb[i:i + 1], cent, 1, metric=metric)[1][0, 0] for i in range(nb)])
    np.testing.assert_array_equal(ref.list_of, want_list)
    for l, (li, lv) in enumerate(ref.lists()):
        assert (np.diff(li) > 0).all()
        sel = [int(np.nonzero(ids == i)[0][0]) for i in li]
        assert (want_list[sel] == l).all()
        np.testing.assert_array_equal(lv, xb[sel])
    Iq = O.coarse_search(xq, cent, nprobe, metric=metric)[1]
    Iq[0, 1] = -1       # a skipped probe
    Iq[1, 1] = Iq[1, 0]  # a repeated list
    for probes in (None, Iq):
        D, I = ref.search(xq, k, nprobe=nprobe, Iq=probes)
        P = R.probes(xq, cent, nprobe, metric) if probes is None else probes
        for q in range(nq):
            cand = [(O.tree(xq[q], xb[i], metric), int(ids[i])) for i in range(nb) if want_list[i] in set(P[q])]
            cand.sort(key=lambda t: (-t[0] if metric == 0 else t[0], t[1]))
            cand = cand[:k]
            np.testing.assert_array_equal(I[q, :len(cand)], [c[1] for c in cand])
            np.testing.assert_array_equal(D[q, :len(cand)], np.array([c[0] for c in cand], np.float32))
            assert (I[q, len(cand):] == -1).all()
            assert (D[q, len(cand):] == (-R.FMAX if metric == 0 else R.FMAX)).all()
    # a query whose probes hold fewer than k vectors is padded
    D, I = ref.search(xq[:1], 64, Iq=np.array([[int(np.argmin(np.bincount(want_list, minlength=nlist))), -1]]))
    assert (I[0] == -1).any()


def test_range_granule_matches_the_header():
    import ivfflat_ref as R

    with open(os.path.join(CSRC, "ivf_flat.h")) as f:
        m = re.search(r"constexpr\s+int\s+kIvfFlatRangeRows\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) == R.RANGE_ROWS


# ---------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Per kernel of lib/ivf_flat.o's gfx950 code object: the compiler's metadata
    (as tests/test_scan_resources.py reads ivfpq_kernels.o)."""
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


def test_scan_uses_no_scratch_and_fits_two_workgroups_per_cu(kernels):
    scans = {n: f for n, f in kernels.items() if "k_ivfflat_scan" in n}
    # (metric) x (k <= 64, k <= 256, k <= 1024): template arguments <KIND, G, R>
    assert len(scans) == 6, sorted(scans)
    for n, f in scans.items():
        print(n, f)
        assert f["private_segment_fixed_size"] == 0, (n, f)
        assert f["vgpr_spill_count"] == 0, (n, f)
    small = {n: f for n, f in scans.items() if re.search(r"k_ivfflat_scanILi[01]ELi\d+ELi1E", n)}
    assert len(small) == 2, sorted(small)
    for n, f in small.items():
        assert f["group_segment_fixed_size"] <= 80 * 1024, (n, f)
        assert f["vgpr_count"] <= 256, (n, f)  # VGPRs + AGPRs of a wave: two waves per SIMD
