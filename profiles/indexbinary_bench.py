#!/usr/bin/env python3
"""IndexBinaryFlat throughput on one MI355X beside the library's exact inner-product search
over the +-1 float expansion of the same codes and queries, and beside its two floors.

    python profiles/indexbinary_bench.py [--out profiles/indexbinary_bench.json] [--nb 1000000]

Shapes: nb random codes, 1024 queries, d = 256 and 768 bits, k = 10 and 1000 (beir's
binary_k).  Since ip = d - 2 * hamming, the float search gives the same ranking.  Two
comparators hold the expansion:
  IndexFlatIP  the flat float index a caller would otherwise build.  Its base lives on the host, so every search call
               uploads it; timed with the host clock around the (synchronous) call.
  IVF1,Flat    the same exact scan with the vectors resident in HBM (inner product, one list):
               the stricter comparator, timed like the binary index.
Every GPU step runs in a child process of its own under ``timeout``; the first step that fails
ends the run (nothing else is started on the GPU) and no JSON is written.

Times: device events around whole ``search_device`` calls after a warm-up, over windows of at
least a second; the indexes are timed in turn, three rounds of turns per k; median and
max - min spread.  ``faster`` is true where the binary median is below the comparator's median
by more than the comparator's own spread.  Floors:
  valu_floor_ms  2 * stride / 4 lane-operations per distance (xor, bit count), two passes, over
                 256 CUs x 128 lanes x 2.4 GHz
  byte_floor_ms  the codes read 2 * ceil(nq / QB) times (QB queries per work item, two passes)
                 over the HBM read rate measured here by csrc/hbm_stream.hip
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd"), os.path.join(REPO, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ivfflat_bench import VALU_LANE_OPS_PER_S, hbm_read_rate, timed  # noqa: E402

NQ, KS, ROUNDS, DS = 1024, (10, 1000), 3, (256, 768)
STEP_TIMEOUT = 560


def timed_host(fn, min_seconds=1.0):
    """ms per synchronous call by the host clock: one warm-up, then a window of >= min_seconds."""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = int(min(2000, max(2, min_seconds / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def expand(t, torch):
    """uint8 [n][cs] -> float32 [n][8 * cs] of +-1, bit order of np.unpackbits."""
    shifts = torch.arange(7, -1, -1, device=t.device, dtype=torch.uint8)
    bits = (t.unsqueeze(-1) >> shifts) & 1
    return (bits.reshape(t.shape[0], -1).to(torch.float32) * 2 - 1).contiguous()


def step_shape(d, nb):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import _lib

    g = torch.Generator(device="cuda").manual_seed(1234)
    cb = torch.randint(0, 256, (nb, d // 8), generator=g, device="cuda", dtype=torch.uint8)
    cq = torch.randint(0, 256, (NQ, d // 8), generator=g, device="cuda", dtype=torch.uint8)
    binary = faiss.IndexBinaryFlat(d)
    flat_dev = faiss.index_factory(d, "IVF1,Flat", faiss.METRIC_INNER_PRODUCT)
    flat_dev.set_trained(np.zeros((1, d), np.float32))
    flat_host = faiss.IndexFlatIP(d)
    for i0 in range(0, nb, 250_000):
        binary.add_device(cb[i0:i0 + 250_000])
        x = expand(cb[i0:i0 + 250_000], torch)
        flat_dev.add_device(x)
        flat_host.add(x.cpu().numpy())
        del x
    fq = expand(cq, torch)
    fq_host = fq.cpu().numpy()
    read_rate = hbm_read_rate(torch)
    stride, qb, sg, rows, qc = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64())
    _lib.check(_lib.load().ivfpq_bin_get_plan(d, nb, NQ, 10, *[ctypes.byref(v) for v in (stride, qb, sg, rows, qc)]))
    out = dict(d=d, nb=nb, nq=NQ, rounds=ROUNDS, hbm_read_bytes_per_s=read_rate, stride=stride.value,
               query_block=qb.value, segments=sg.value, segment_rows=rows.value, by_k={})
    valu_floor = 2 * (stride.value // 4) * 2 * nb * NQ / VALU_LANE_OPS_PER_S * 1e3
    byte_floor = 2 * -(-NQ // qb.value) * stride.value * nb / read_rate * 1e3
    for k in KS:
        Db = torch.empty((NQ, k), dtype=torch.int32, device="cuda")
        Ib = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
        Df = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
        If = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
        runs = {"IndexBinaryFlat": [], "IVF1,Flat": [], "IndexFlatIP": []}
        host = {}
        for _ in range(ROUNDS):  # in turn: one window of every index per round
            runs["IndexBinaryFlat"].append(timed(lambda: binary.search_device(cq, k, Db, Ib), torch)[0])
            runs["IVF1,Flat"].append(timed(lambda: flat_dev.search_device(fq, k, Df, If), torch)[0])
            runs["IndexFlatIP"].append(timed_host(lambda: host.update(r=flat_host.search(fq_host, k))))
        # the same ranking: ip = d - 2 * hamming, exactly
        same_d = bool(torch.equal(Df, (d - 2 * Db).to(torch.float32)))
        same_d_host = bool(np.array_equal(host["r"][0], (d - 2 * Db.cpu().numpy()).astype(np.float32)))
        res = {}
        for key, r in runs.items():
            res[key] = dict(ms_runs=r, ms_per_batch=statistics.median(r), spread_ms=max(r) - min(r))
        b = res["IndexBinaryFlat"]
        b.update(valu_floor_ms=valu_floor, byte_floor_ms=byte_floor, queries_per_s=NQ / b["ms_per_batch"] * 1e3,
                 distances_equal_ivf1flat=same_d, distances_equal_indexflatip=same_d_host)
        for key in ("IVF1,Flat", "IndexFlatIP"):
            c = res[key]
            c["ratio_binary_to_this"] = b["ms_per_batch"] / c["ms_per_batch"]
            c["faster"] = bool(b["ms_per_batch"] < c["ms_per_batch"] - c["spread_ms"])
        out["by_k"][str(k)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexbinary_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--ds", default=",".join(str(d) for d in DS))
    ap.add_argument("--step", type=int)
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_shape(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S, "shapes": {}}
    for d in a.ds.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", d,
               "--nb", str(a.nb)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:])
            sys.stderr.write(f"\nstep d={d} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print("d=" + d, json.dumps(r), flush=True)
        result["shapes"]["d" + d] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
