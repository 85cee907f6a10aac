#!/usr/bin/env python3
"""IndexScalarQuantizer throughput on one MI355X beside the library's exact scan over the
same vectors in fp32 (IVF1,Flat), and beside its two bounds.

    python profiles/indexsq_bench.py [--out profiles/indexsq_bench.json] [--nb 1000000]

Shapes: 1024 queries, k = 10 and k = 100, nb vectors:
  sift128  d = 128, clustered data (datasets.synthetic_sift_like), L2 -- the shape of
           profiles/ivfflat_bench.py
  beir768  d = 768, unit-norm rows, inner product -- the BEIR dense-retrieval shape
For each shape three indexes hold the same vectors: "SQfp16", "SQ8" and the comparator
"IVF1,Flat".  Every GPU step runs in a child process of its own under ``timeout``; the first
step that fails ends the run (nothing else is started on the GPU) and no JSON is written.

Times: device events around whole ``search_device`` calls (scan and merge; the comparator
also its coarse quantizer and planning) after a warm-up, over windows of at least a second.
The three indexes are timed in turn, three rounds of turns per k, so that drift of the
machine shows as spread inside every index's runs, not as a difference between indexes.
``not_slower`` compares the medians, allowing the spread (max - min) of the comparator's own
runs.  Bounds, as profiles/ivfflat_bench.py computes them:
  valu_floor_ms   (3 for L2: subtract, multiply, add; 2 for inner product) x d x nb x nq
                  lane-operations over 256 CUs x 128 lanes x 2.4 GHz; the decode is not counted
  hbm_floor_ms    code bytes fetched once per (row range, group of G queries) over the HBM
                  read rate measured here by csrc/hbm_stream.hip, as bench.py measures it
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

from ivfflat_bench import VALU_LANE_OPS_PER_S, hbm_read_rate, timed  # noqa: E402

NQ, KS, ROUNDS = 1024, (10, 100), 3
SHAPES = {"sift128": dict(d=128, metric="l2"), "beir768": dict(d=768, metric="ip")}
KEYS = ("SQfp16", "SQ8", "IVF1,Flat")
STEP_TIMEOUT = 560


def make_data(name, nb):
    """(base, queries) of a shape as CUDA tensors."""
    import torch

    from faiss_amd import datasets

    d = SHAPES[name]["d"]
    if name == "sift128":
        return (torch.from_numpy(datasets.synthetic_sift_like(nb, d, seed=1234)).cuda(),
                torch.from_numpy(datasets.synthetic_sift_like(NQ, d, seed=123)).cuda())
    g = torch.Generator(device="cuda").manual_seed(1234)
    return (torch.nn.functional.normalize(torch.randn((nb, d), generator=g, device="cuda"), dim=1).contiguous(),
            torch.nn.functional.normalize(torch.randn((NQ, d), generator=g, device="cuda"), dim=1).contiguous())


def build_indexes(name, txb, keys):
    import numpy as np

    import faiss_amd as faiss

    s = SHAPES[name]
    d, nb = s["d"], txb.shape[0]
    metric = faiss.METRIC_L2 if s["metric"] == "l2" else faiss.METRIC_INNER_PRODUCT
    index = {}
    for key in keys:
        ix = faiss.index_factory(d, key, metric)
        if key == "IVF1,Flat":
            ix.set_trained(np.zeros((1, d), np.float32))
        else:
            ix.train(txb[:100_000].cpu().numpy())
        for i0 in range(0, nb, 250_000):
            ix.add_device(txb[i0:i0 + 250_000])
        index[key] = ix
    return index


def step_shape(name, nb):
    import numpy as np
    import torch

    s = SHAPES[name]
    d = s["d"]
    txb, txq = make_data(name, nb)
    index = build_indexes(name, txb, KEYS)
    del txb
    read_rate = hbm_read_rate(torch)
    code_size = {"SQfp16": 2 * d, "SQ8": d, "IVF1,Flat": 4 * d}
    out = dict(shape=name, d=d, nb=nb, nq=NQ, metric=s["metric"], rounds=ROUNDS, hbm_read_bytes_per_s=read_rate,
               code_bytes={k_: code_size[k_] * nb for k_ in KEYS}, by_k={})
    for k in KS:
        Dd = {key: torch.empty((NQ, k), dtype=torch.float32, device="cuda") for key in KEYS}
        Id = {key: torch.empty((NQ, k), dtype=torch.int64, device="cuda") for key in KEYS}
        runs = {key: [] for key in KEYS}
        for _ in range(ROUNDS):
            for key in KEYS:  # in turn: one window of every index per round
                ms, _reps = timed(lambda: index[key].search_device(txq, k, Dd[key], Id[key]), torch)
                runs[key].append(ms)
        # queries per work item: 8 at k <= 64 (4 for the 8-bit codec), 4 above
        groups = {key: -(-NQ // (8 if k <= 64 and key != "SQ8" else 4)) for key in KEYS}
        ops = 3 if s["metric"] == "l2" else 2
        valu_floor = ops * d * nb * NQ / VALU_LANE_OPS_PER_S * 1e3
        flat_I = Id["IVF1,Flat"].cpu().numpy()
        res = {}
        for key in KEYS:
            med = statistics.median(runs[key])
            got = Id[key].cpu().numpy()
            same = np.mean([len(np.intersect1d(got[q], flat_I[q])) / k for q in range(NQ)])
            res[key] = dict(ms_runs=runs[key], ms_per_batch=med, spread_ms=max(runs[key]) - min(runs[key]),
                            queries_per_s=NQ / med * 1e3, valu_floor_ms=valu_floor,
                            hbm_floor_ms=groups[key] * code_size[key] * nb / read_rate * 1e3,
                            recall_at_k_vs_fp32=float(same))
        cmp_ = res["IVF1,Flat"]
        for key in KEYS[:2]:
            res[key]["ratio_to_ivf1flat"] = res[key]["ms_per_batch"] / cmp_["ms_per_batch"]
            res[key]["not_slower"] = bool(res[key]["ms_per_batch"] <= cmp_["ms_per_batch"] + cmp_["spread_ms"])
        out["by_k"][str(k)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexsq_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_shape(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S, "shapes": {}}
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
