"""Item composition of the list scan under float16 lookup tables: tests/test_gpu_plan_fill.py's scenarios
with the flag on, so that the planning and the record prefetch of k_scan_lists_h run at the pairs per item
that only the half scan has:

    (M = 32, k = 10)   G = 4 (the fp32 scan has 2)
    (M = 64, k = 10)   G = 2 (the fp32 scan has 1)
    (M = 8, k = 100)   G = 2

A list with c0 first-probe pairs and c1 others forms ceil((c0 + c1) / G) items, the first ceil(c0 / G) of them
lead items; hdr[0] / hdr[1] must hold those sums for scenarios "c0_0to5" and "c0_1" (rows, -1 entries and
the empty list as in the fp32 file).  The tables are small integers (|T1| + 2 |T3| < 2048, asserted), which
half holds exactly, so the half keys are the fp32 keys and the CPU oracle is the reference, bit for bit.

The "range" scenario is a rejection here: a list-range shard has no float16 lookup tables, in whichever
order the two are asked for, and the handle stays usable after the error."""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfpq_f16lut_ref as RH
import test_gpu_plan_fill as PF
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NLIST = PF.NLIST
SHAPES = {"d64_m32_k10": (64, 32, 10, 4), "d128_m64_k10": (128, 64, 10, 2), "d32_m8_k100": (32, 8, 100, 2)}  # d, M, k, G


def tables(d, M, ip, seed, nq):
    rng = np.random.default_rng(seed)
    cent = rng.integers(-3, 4, size=(NLIST, d)).astype(np.float32)
    cb = rng.integers(-2, 3, size=(M, 256, d // M)).astype(np.float32)
    xq = rng.integers(-3, 4, size=(nq, d)).astype(np.float32)
    return rng, cent, cb, xq


def assert_half_is_exact(cent, cb, xq, ip):
    """Every LUT entry of every (query, list) pair is an integer below 2048: h16 changes none."""
    T3 = O.ip_table(xq, cb)
    T1 = np.zeros(1, np.float32) if ip else O.precompute_T1(cent, cb)
    assert (T3 == np.round(T3)).all() and (T1 == np.round(T1)).all()
    assert np.abs(T1).max() + 2 * np.abs(T3).max() < 2048
    lut = RH.lut32(T3[0], None if ip else T1[0], ip)
    np.testing.assert_array_equal(RH.entries(lut), lut)


@functools.lru_cache(maxsize=None)
def make_pair(shape, metric, lo=0, hi=NLIST, flag=True):
    """GpuIndexIVFPQ (flag on) and oracle on the same integer-valued tables and codes."""
    d, M, _, _ = SHAPES[shape]
    ip = metric == "ip"
    rng, cent, cb, xq = tables(d, M, ip, 5100 + 10 * list(SHAPES).index(shape) + ip, 16)
    assert_half_is_exact(cent, cb, xq, ip)
    sizes = [s if lo <= l < hi else 0 for l, s in enumerate(PF.SIZES)]
    n = int(np.sum(sizes))
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.arange(NLIST, dtype=np.int64), sizes)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    mt = faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2
    ix = faiss.GpuIndexIVFPQ(None, d, NLIST, M, 8, mt, 0)
    ix.set_trained(cent, cb)
    if (lo, hi) != (0, NLIST):
        ix.set_list_range(lo, hi)
    ix.add_preencoded(list_no, codes, ids)
    if flag:
        ix.use_float16_lut = True
    ox = O.OracleIVFPQ(d, NLIST, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    return ix, ox, xq


def scenario_rows(name, lo=0, hi=NLIST):
    (slo, shi), nprobe, spec = PF.SCENARIOS[name]
    assert (slo, shi) == (lo, hi)
    unusable = [3] + [l for l in range(NLIST) if not lo <= l < hi]
    rows = PF.make_rows(spec, nprobe, unusable, seed=len(name))
    c = PF.pair_counts(rows, lo, hi)
    for l in range(NLIST):  # the rows give every list the counts the scenario names
        assert tuple(c[l]) == spec.get(l, (0, 0)), (l, tuple(c[l]))
    return rows


@pytest.mark.parametrize("name", ["c0_0to5", "c0_1"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_preassigned_rows_match_oracle(shape, metric, name):
    import torch

    _, _, k, g = SHAPES[shape]
    ix, ox, xq = make_pair(shape, metric)
    assert ix.use_float16_lut
    rows = scenario_rows(name)
    xq = xq[np.arange(rows.shape[0]) % xq.shape[0]]
    dq = None if metric == "ip" else np.random.default_rng(5).integers(0, 5, size=rows.shape).astype(np.float32)
    ix.nprobe = rows.shape[1]
    e0, rs0 = ix.error_count(), ix.repair_stats()
    want = PF.expected_items(rows, 0, NLIST, g)
    for other in (g // 2, 2 * g):  # the counts tell this G from the fp32 scan's
        assert want != PF.expected_items(rows, 0, NLIST, other)
    ref = ox.search_preassigned(xq, k, rows, dq)
    ep = PF.epochs(ix)
    PF.check(ix.search_preassigned(xq, k, rows, dq), ref, f"k={k}")
    got = PF.item_counts(ix, ep)
    print(f"{shape} {metric} {name}: items (all, lead) {got}, expected {want} at G = {g}")
    assert got == want
    xd, rd = torch.from_numpy(xq).cuda(), torch.from_numpy(rows).cuda()
    dd = torch.from_numpy(dq).cuda() if dq is not None else None
    D, I = ix.search_preassigned_device(xd, k, rd, dd)
    torch.cuda.synchronize()
    PF.check((D.cpu().numpy(), I.cpu().numpy()), ref, "device")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_list_range_shard_rejects_the_flag(metric):
    """The "range" scenario: lists [1, 7) of the 8."""
    shape = "d32_m8_k100"
    d, M, k, _ = SHAPES[shape]
    (lo, hi), _, _ = PF.SCENARIOS["range"]
    # the flag first: the range is refused, the handle keeps all its lists and the half scan
    ix, ox, xq = make_pair(shape, metric)
    rows = scenario_rows("c0_1")
    xq_r = xq[np.arange(rows.shape[0]) % xq.shape[0]]
    dq = None if metric == "ip" else np.zeros(rows.shape, np.float32)
    probe = faiss.GpuIndexIVFPQ(None, d, NLIST, M, 8, faiss.METRIC_INNER_PRODUCT if metric == "ip" else faiss.METRIC_L2, 0)
    probe.set_trained(ix.centroids(), ix.codebook())
    probe.use_float16_lut = True
    with pytest.raises(RuntimeError, match="list-range shard"):
        probe.set_list_range(lo, hi)
    assert probe.use_float16_lut
    probe.add_preencoded(*ix.invlists.export())
    probe.nprobe = rows.shape[1]
    PF.check(probe.search_preassigned(xq_r, k, rows, dq), ox.search_preassigned(xq_r, k, rows, dq), "flag, then range")
    assert probe.error_count() == 0
    # the range first: the flag is refused, the shard goes on with the fp32 scan over its own lists
    sh, osh, xq = make_pair(shape, metric, lo, hi, flag=False)
    with pytest.raises(RuntimeError, match="list-range shard"):
        sh.use_float16_lut = True
    assert not sh.use_float16_lut
    rows = scenario_rows("range", lo, hi)
    xq_r = xq[np.arange(rows.shape[0]) % xq.shape[0]]
    dq = None if metric == "ip" else np.zeros(rows.shape, np.float32)
    sh.nprobe = rows.shape[1]
    PF.check(sh.search_preassigned(xq_r, k, rows, dq), osh.search_preassigned(xq_r, k, rows, dq), "range, then flag")
    assert sh.error_count() == 0
