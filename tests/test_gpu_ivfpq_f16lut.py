"""IVF-PQ with float16 lookup tables (GpuClonerOptions.useFloat16 -> k_scan_lists_h): labels and distances
bit for bit against tests/ivfpq_f16lut_ref.py, for every pairs-per-item class of (M, k), both metrics, the
saturating clamp, non-fused planning, repaired probes and batches in flight; and the Faiss-GPU surface
(GpuClonerOptions, index_cpu_to_gpu, setNumProbes) that bench_gpu_sift1m.py's approximate section uses."""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfpq_f16lut_ref as ref

NQ, NPROBE, N = 37, 4, 6000  # 37 queries: no multiple of any pairs-per-item count


@functools.lru_cache(maxsize=None)
def case(M, ip=False, scale=1.0, nlist=16):
    """Quantizers, lists and queries of one shape, and the reference's 1000 best of every query (a prefix
    of it is the answer for a smaller k).  List 0 holds 1700 codes (more than JB x 256: the super-batch
    loop repeats), list 1 none, list 2 exactly one; queries 0..2 sit on those lists' centroids."""
    rng = np.random.default_rng(1000 * M + nlist + int(ip))
    d = 2 * M
    cent = (rng.standard_normal((nlist, d)) * 2 * scale).astype(np.float32)
    cb = (rng.standard_normal((M, 256, 2)) * scale).astype(np.float32)
    list_no = np.concatenate([np.zeros(1700, np.int64), [2], rng.integers(3, nlist, N - 1701)])
    codes = rng.integers(0, 256, (N, M), dtype=np.uint8)
    ids = rng.permutation(N).astype(np.int64)
    xq = (rng.standard_normal((NQ, d)) * 2 * scale).astype(np.float32)
    xq[:3] += cent[:3]
    lists = [np.sort(ids[list_no == l]) for l in range(nlist)]  # device lists are label-sorted
    by_id = np.argsort(ids)
    lcodes = [codes[by_id[l]] for l in lists]
    stats = {}
    D, I = ref.search(xq, 1000, cent, cb, lcodes, lists, NPROBE, ip, stats=stats)
    D32, I32 = ref.search(xq, 1000, cent, cb, lcodes, lists, NPROBE, ip, half=False)
    return dict(d=d, cent=cent, cb=cb, list_no=list_no, codes=codes, ids=ids, xq=xq, D=D, I=I, D32=D32, I32=I32,
                saturated=stats["saturated"])


def gpu_index(c, M, ip=False, nlist=16, on=True):
    co = faiss.GpuClonerOptions()
    co.useFloat16 = on
    metric = faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2
    ix = faiss.index_cpu_to_gpu(None, 0, faiss.IndexIVFPQ(None, c["d"], nlist, M, 8, metric, device=0), co)
    ix.set_trained(c["cent"], c["cb"])
    ix.add_preencoded(c["list_no"], c["codes"], c["ids"])
    ix.setNumProbes(NPROBE)
    return ix


def check(got, c, k):
    D, I = got
    np.testing.assert_array_equal(I, c["I"][:, :k])
    np.testing.assert_array_equal(D.view(np.uint32), c["D"][:, :k].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("k", [10, 100, 200, 1000])  # 1, 2, 4, 16 top-k rows: every value of G_h
@pytest.mark.parametrize("M", [8, 16, 32, 48, 64])
def test_matches_reference(M, k, ip):
    c = case(M, ip)
    assert not np.array_equal(c["D"][:, :k], c["D32"][:, :k])  # the case tells the half LUT from the fp32 one
    ix = gpu_index(c, M, ip)
    assert ix.use_float16_lut
    check(ix.search(c["xq"], k), c, k)


@pytest.mark.gpu
def test_saturating_entries():
    """Entries beyond +-65504 clamp to it instead of becoming inf: every key stays finite and ordered."""
    c = case(16, scale=120.0)
    assert c["saturated"] > 0 and np.isfinite(c["D"][c["I"] >= 0]).all()
    assert not np.array_equal(c["I"][:, :10], c["I32"][:, :10])
    check(gpu_index(c, 16).search(c["xq"], 10), c, 10)


@pytest.mark.gpu
def test_non_fused_planning():
    c = case(32, nlist=1100)  # more lists than the scan plans by itself: k_plan_items writes the records
    check(gpu_index(c, 32, nlist=1100).search(c["xq"], 10), c, 10)


@pytest.mark.gpu
def test_lost_partial_lists_are_repaired_with_half_entries():
    c = case(64)
    ix = gpu_index(c, 64)
    before = ix.repair_stats()[1]
    ix.set_fault_injection(3)  # the hook skips partial-list stores; the merge rescans those probes
    try:
        got = ix.search(c["xq"], 10)
    finally:
        ix.set_fault_injection(0)
    check(got, c, 10)
    assert ix.repair_stats()[1] > before


@pytest.mark.gpu
def test_lost_partial_lists_of_a_first_batch_are_not_read_from_a_freed_handle():
    """A new handle's first batch has the epoch, and so the tags, of every earlier handle's first batch.  The
    workspace of an inner-product handle of the same shape is freed just before, so that the allocator may hand
    the same block to the L2 handle: its lost slots must not be taken from the records left there (negated
    similarities, far below every L2 key), which the workspace clears when it allocates."""
    import gc

    c_ip, c = case(64, True), case(64)
    for _ in range(3):
        old = gpu_index(c_ip, 64, True)
        old.search(c_ip["xq"], 10)
        del old
        gc.collect()
        ix = gpu_index(c, 64)
        before = ix.repair_stats()[1]
        ix.set_fault_injection(3)
        try:
            got = ix.search(c["xq"], 10)
        finally:
            ix.set_fault_injection(0)
        check(got, c, 10)
        assert ix.repair_stats()[1] > before
        del ix
        gc.collect()


@pytest.mark.gpu
def test_batches_in_flight():
    import torch

    c = case(32)
    ix = gpu_index(c, 32)
    ix.inflight = True
    x = torch.from_numpy(c["xq"]).cuda()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [slice(0, 20), slice(20, NQ)]
    out = []
    for s, h in zip(streams, halves):
        with torch.cuda.stream(s):
            out.append(ix.search_device(x[h].contiguous(), 100, stream=s.cuda_stream))
    torch.cuda.synchronize()
    D = np.concatenate([o[0].cpu().numpy() for o in out])
    I = np.concatenate([o[1].cpu().numpy() for o in out])
    check((D, I), c, 100)


@pytest.mark.gpu
def test_flag_off_is_the_fp32_scan():
    c = case(32)
    ix = gpu_index(c, 32, on=False)
    D0, I0 = ix.search(c["xq"], 100)
    ix.use_float16_lut = True
    check(ix.search(c["xq"], 100), c, 100)
    ix.use_float16_lut = False
    D1, I1 = ix.search(c["xq"], 100)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    assert np.array_equal(I0, c["I32"][:, :100]) and np.array_equal(D0, c["D32"][:, :100])


@pytest.mark.gpu
def test_sift1m_approximate_section():
    """bench_gpu_sift1m.py:71-95 as written, on 4000 random rows."""
    rng = np.random.default_rng(5)
    d = 128
    xb = rng.random((4000, d), dtype=np.float32)
    xt, xq = xb[:3000], rng.random((NQ, d), dtype=np.float32)
    res = faiss.StandardGpuResources()
    index = faiss.index_factory(d, "IVF16,PQ64")
    co = faiss.GpuClonerOptions()
    co.useFloat16 = True
    index = faiss.index_cpu_to_gpu(res, 0, index, co)
    index.train(xt)
    index.add(xb)
    index.search(xq, 123)
    index.setNumProbes(4)
    D, I = index.search(xq, 100)
    list_no, codes, ids = index.invlists.export()
    lists = [ids[list_no == l] for l in range(16)]
    lcodes = [codes[list_no == l] for l in range(16)]
    Dr, Ir = ref.search(xq, 100, index.centroids(), index.codebook(), lcodes, lists, 4)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


def test_cloner_options_defaults():
    co = faiss.GpuClonerOptions()
    assert (co.useFloat16, co.useFloat16CoarseQuantizer, co.usePrecomputed, co.indicesOptions, co.reserveVecs,
            co.verbose) == (False, False, False, 0, 0, False)


def test_index_cpu_to_gpu_mapping(monkeypatch):
    """The type mapping and its errors, with the constructors that would create device handles stubbed out."""
    from faiss_amd import gpu

    made = []
    for cls in (gpu.GpuIndexIVFPQ, gpu.GpuIndexIVFFlat, gpu.GpuIndexFlat):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _n=cls.__name__: made.append((_n, a)))
    monkeypatch.setattr(gpu, "_clone_ivf", lambda src, dst: dst)
    monkeypatch.setattr(gpu.GpuIndexIVFPQ, "use_float16_lut", None)
    co = faiss.GpuClonerOptions()
    co.useFloat16 = True
    pq = object.__new__(faiss.IndexIVFPQ)
    pq.d, pq.nlist, pq.M, pq.nbits, pq.metric_type, pq.niter_pq = 32, 4, 16, 8, faiss.METRIC_L2, 25
    out = faiss.index_cpu_to_gpu(None, 0, pq, co)
    assert type(out) is gpu.GpuIndexIVFPQ and out.use_float16_lut is True
    assert made[-1] == ("GpuIndexIVFPQ", (None, 32, 4, 16, 8, faiss.METRIC_L2, 0))
    flat = object.__new__(faiss.IndexIVFFlat)
    flat.d, flat.nlist, flat.metric_type = 32, 4, faiss.METRIC_L2
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer"):
        faiss.index_cpu_to_gpu(None, 0, flat, co)
    assert type(faiss.index_cpu_to_gpu(None, 0, flat)) is gpu.GpuIndexIVFFlat
    exact = faiss.IndexFlatL2(32, device=0)
    assert type(faiss.index_cpu_to_gpu(None, 0, exact, co)) is gpu.GpuIndexFlat and made[-1][1][3].useFloat16
    other = object.__new__(faiss.IndexPQ)
    other.device = 0
    assert faiss.index_cpu_to_gpu(None, 0, other, co) is other
    with pytest.raises(RuntimeError, match="not copied"):
        faiss.index_cpu_to_gpu(None, 1, other, co)
    co.useFloat16CoarseQuantizer = True
    with pytest.raises(RuntimeError, match="useFloat16CoarseQuantizer"):
        faiss.index_cpu_to_gpu(None, 0, pq, co)


def test_flag_through_the_c_abi_without_a_handle():
    lib = faiss.index._lib.load()
    assert lib.ivfpq_get_float16_lut(None) == -1
    assert lib.ivfpq_set_float16_lut(None, 1) != 0 and len(lib.ivfpq_last_error()) > 0
