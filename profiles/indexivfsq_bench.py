#!/usr/bin/env python3
"""IndexIVFScalarQuantizer throughput on one MI355X beside IndexIVFFlat over the same vectors,
lists and probes (fp32 rows), and beside the HBM bound of the bytes it scans.

    python profiles/indexivfsq_bench.py [--out profiles/indexivfsq_bench.json] [--nb 1000000]

Shapes: 1024 queries, k = 10 and k = 100, nb vectors, IVF1024:
  sift128  d = 128, clustered data (datasets.synthetic_sift_like), L2, nprobe 16 and 64 -- the
           shape of profiles/ivfflat_bench.py
  beir768  d = 768, unit-norm rows, inner product, nprobe 16
For each shape five indexes hold the same vectors on the same centroids (every index runs the
same coarse k-means: same rows, iterations and seed; asserted): fp16 and 8-bit codes, each with
by_residual (the factory's default; "_res") and without, and the comparator "IVF1024,Flat".
Every GPU step runs in a child process of its own under ``timeout``; the first step that fails
ends the run (nothing else is started on the GPU) and no JSON is written.

Times: device events around whole ``search_device`` calls (coarse quantizer, planning, residual
queries where there are any, scan and merge) after a warm-up, over windows of at least a second.
The indexes are timed in turn, three rounds of turns per (nprobe, k), so that drift of the machine
shows as spread inside every index's runs, not as a difference between indexes.  ``not_slower``
compares the medians, allowing the spread (max - min) of the comparator's own runs.
  hbm_floor_ms        row bytes fetched once per work item -- per list, ceil(pairs / G) groups x
                      the list's rows x the code size -- over the HBM read rate measured here by
                      csrc/hbm_stream.hip, as bench.py measures it
  residual_over_plain by_residual = True over False on the same codec: what the residual
                      queries (L2: a kernel and [pairs][d] floats) or the added coarse value (IP) cost
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd"), os.path.join(REPO, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

from indexsq_bench import make_data  # noqa: E402
from ivfflat_bench import hbm_read_rate, timed  # noqa: E402

NQ, KS, ROUNDS, NLIST, NITER = 1024, (10, 100), 3, 1024, 5
SHAPES = {"sift128": dict(d=128, metric="l2", nprobes=(16, 64)), "beir768": dict(d=768, metric="ip", nprobes=(16,))}
# label -> (quantizer type name or None for fp32 rows, by_residual, bytes per dimension)
INDEXES = {"SQfp16_res": ("QT_fp16", True, 2), "SQfp16": ("QT_fp16", False, 2), "SQ8_res": ("QT_8bit", True, 1),
           "SQ8": ("QT_8bit", False, 1), "Flat": (None, False, 4)}
STEP_TIMEOUT = 560


def build_indexes(name, txb):
    import numpy as np

    import faiss_amd as faiss

    s = SHAPES[name]
    d, nb = s["d"], txb.shape[0]
    metric = faiss.METRIC_L2 if s["metric"] == "l2" else faiss.METRIC_INNER_PRODUCT
    xt = txb[:100_000].cpu().numpy()
    index = {}
    for label, (qname, by_residual, _) in INDEXES.items():
        if qname is None:
            ix = faiss.IndexIVFFlat(None, d, NLIST, metric)
        else:
            ix = faiss.IndexIVFScalarQuantizer(None, d, NLIST, getattr(faiss.ScalarQuantizer, qname), metric,
                                               by_residual)
        ix.niter_coarse = NITER
        ix.train(xt)
        for i0 in range(0, nb, 250_000):
            ix.add_device(txb[i0:i0 + 250_000])
        index[label] = ix
    for ix in index.values():
        assert np.array_equal(ix.centroids(), index["Flat"].centroids())
        assert np.array_equal(ix.invlists.list_sizes(), index["Flat"].invlists.list_sizes())
    return index


def scanned_rows(sizes, probes, G):
    """Rows fetched by the scan's work items: per list, ceil(pairs / G) groups x its rows."""
    import numpy as np

    pairs = np.bincount(probes.reshape(-1), minlength=len(sizes))
    return int(((pairs + G - 1) // G * sizes).sum())


def step_shape(name, nb):
    import numpy as np
    import torch

    s = SHAPES[name]
    d = s["d"]
    txb, txq = make_data(name, nb)
    index = build_indexes(name, txb)
    del txb
    read_rate = hbm_read_rate(torch)
    sizes = index["Flat"].invlists.list_sizes()
    xq = txq.cpu().numpy()
    out = dict(shape=name, d=d, nb=nb, nq=NQ, nlist=NLIST, metric=s["metric"], rounds=ROUNDS,
               hbm_read_bytes_per_s=read_rate, code_bytes={l: v[2] * d * nb for l, v in INDEXES.items()}, runs={})
    for nprobe in s["nprobes"]:
        for ix in index.values():
            ix.nprobe = nprobe
        probes = index["Flat"].quantizer.search(xq, nprobe)[1]
        for k in KS:
            Dd = {l: torch.empty((NQ, k), dtype=torch.float32, device="cuda") for l in INDEXES}
            Id = {l: torch.empty((NQ, k), dtype=torch.int64, device="cuda") for l in INDEXES}
            runs = {l: [] for l in INDEXES}
            for _ in range(ROUNDS):
                for l in INDEXES:  # in turn: one window of every index per round
                    ms, _reps = timed(lambda: index[l].search_device(txq, k, Dd[l], Id[l]), torch)
                    runs[l].append(ms)
            flat_I = Id["Flat"].cpu().numpy()
            res = {}
            for l, (qname, _, elem) in INDEXES.items():
                G = 8 if k <= 64 and qname != "QT_8bit" else 4  # pairs per work item
                med = statistics.median(runs[l])
                got = Id[l].cpu().numpy()
                same = np.mean([len(np.intersect1d(got[q], flat_I[q])) / k for q in range(NQ)])
                scanned = scanned_rows(sizes, probes, G) * elem * d
                res[l] = dict(ms_runs=runs[l], ms_per_batch=med, spread_ms=max(runs[l]) - min(runs[l]),
                              queries_per_s=NQ / med * 1e3, scanned_bytes=scanned,
                              hbm_floor_ms=scanned / read_rate * 1e3, recall_at_k_vs_fp32=float(same))
            cmp_ = res["Flat"]
            for l in INDEXES:
                if l == "Flat":
                    continue
                res[l]["ratio_to_ivfflat"] = res[l]["ms_per_batch"] / cmp_["ms_per_batch"]
                res[l]["not_slower"] = bool(res[l]["ms_per_batch"] <= cmp_["ms_per_batch"] + cmp_["spread_ms"])
            for codec in ("SQfp16", "SQ8"):
                res[codec + "_res"]["residual_over_plain"] = res[codec + "_res"]["ms_per_batch"] / res[codec]["ms_per_batch"]
            out["runs"][f"nprobe{nprobe}_k{k}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexivfsq_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_shape(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "shapes": {}}
    for step in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", step,
               "--nb", str(a.nb)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:])
            sys.stderr.write(f"\nstep {step} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print(step, json.dumps(r), flush=True)
        result["shapes"][step] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
