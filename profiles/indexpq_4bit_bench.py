#!/usr/bin/env python3
"""IndexPQ at 4 bits against 8 bits on one MI355X: the question of the reference's
nbits_experiments_fix_bytes_per_vec.py ("16 bytes per vector = 16 x 8 bits = 32 x 4 bits"),
and the 8-bit scan at equal M as the yardstick.

    python profiles/indexpq_4bit_bench.py [--out profiles/indexpq_4bit_bench.json] [--nb 1000000]

Cells: d = 128 (k = 10, 100): PQ32x4 against PQ32x8 (same look-up count, twice the code bytes,
16 x the table) and PQ16x8 (same 16 bytes per vector, half the look-ups); d = 768 (k = 10, 1000):
PQ192x4 against PQ96x8 (same 96 bytes).  nb clustered vectors (SIFT-like: uniform centres,
Gaussian blobs, rounded and clipped to [0, 255], made on the GPU), 1024 queries of the same
distribution, L2.  Every index of a cell is trained on the same rows (the first --train of
the base, --niter Lloyd iterations) and holds the same base.  Times are device events around
whole ``search_device`` calls (table build + scan + merge) after a warm-up, over windows of
at least a second, in rounds that alternate between the indexes of a cell; every round is
reported.  recall@k is the mean fraction of IndexFlatL2's k labels that a search returns.

Each d runs in a child process of its own under ``timeout``; the first that fails ends the
run (nothing else is started on the GPU) and no JSON is written.  The kernels' registers, LDS and
workgroups per CU are in DESIGN.md ("IndexPQ at 4 bits"), from the compiler's resource report.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from indexpq_bench import timed  # noqa: E402  (profiles/ is the script's directory)

CELLS = {
    128: dict(ks=(10, 100), keys=("PQ32x4", "PQ32x8", "PQ16x8"), same_M=("PQ32x4", "PQ32x8"),
              same_bytes=("PQ32x4", "PQ16x8")),
    768: dict(ks=(10, 1000), keys=("PQ192x4", "PQ96x8"), same_M=None, same_bytes=("PQ192x4", "PQ96x8")),
}
NQ, ROUNDS, STEP_TIMEOUT = 1024, 3, 540


def clustered(torch, n, d, seed, n_centres=20_000, sigma=16.0):
    g = torch.Generator(device="cuda").manual_seed(20251015)
    centres = torch.rand((n_centres, d), generator=g, device="cuda") * 128.0
    g.manual_seed(seed)
    which = torch.randint(0, n_centres, (n,), generator=g, device="cuda")
    out = torch.empty((n, d), device="cuda")
    for i0 in range(0, n, 1 << 17):
        w = which[i0:i0 + (1 << 17)]
        out[i0:i0 + len(w)] = (centres[w] + sigma * torch.randn((len(w), d), generator=g, device="cuda")).round_()
    return out.clamp_(0, 255)


def step(d, nb, ntrain, niter):
    import torch

    import faiss_amd as faiss

    cell = CELLS[d]
    xb = clustered(torch, nb, d, 1)
    xq = clustered(torch, NQ, d, 2)
    xt = xb[:ntrain].cpu().numpy()
    flat = faiss.IndexFlatL2(d)
    flat.add_device(xb)
    kmax = max(cell["ks"])
    gt = flat.search_device(xq, kmax)[1].cpu().numpy()
    del flat
    idx = {}
    for key in cell["keys"]:
        ix = faiss.index_factory(d, key)
        ix.niter_pq = niter
        ix.train(xt)
        ix.add_device(xb)
        idx[key] = ix
    out = {"d": d, "nb": nb, "nq": NQ, "train_rows": ntrain, "niter_pq": niter, "cells": {}}
    for k in cell["ks"]:
        D = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
        I = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
        c = {"recall_at_k": {}, "code_bytes": {key: idx[key].code_size for key in cell["keys"]}, "rounds": []}
        for key, ix in idx.items():
            ix.search_device(xq, k, D, I)
            got = I.cpu().numpy()
            c["recall_at_k"][key] = float(sum(len(set(a) & set(b)) for a, b in zip(got, gt[:, :k]))) / (NQ * k)
        for _ in range(ROUNDS):
            c["rounds"].append({key: timed(lambda ix=ix: ix.search_device(xq, k, D, I), torch)[0]
                                for key, ix in idx.items()})
        if cell["same_M"]:
            a, b = cell["same_M"]
            c["x8_over_x4_same_M"] = [r[b] / r[a] for r in c["rounds"]]
            c["x4_no_slower_than_x8_same_M_in_every_round"] = all(r[a] <= r[b] for r in c["rounds"])
        a, b = cell["same_bytes"]
        c["x8_over_x4_same_bytes"] = [r[b] / r[a] for r in c["rounds"]]
        c["recall_x4_minus_x8_same_bytes"] = c["recall_at_k"][a] - c["recall_at_k"][b]
        R = 1 if k <= 64 else 4 if k <= 256 else 16
        c["x4_kernel"] = f"k_pq_scan4<{R}>"
        out["cells"][f"k{k}"] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexpq_4bit_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--step", type=int)
    a = ap.parse_args()
    if a.step:  # child: one d, one JSON line
        print("RESULT " + json.dumps(step(a.step, a.nb, a.train, a.niter)), flush=True)
        return 0
    result = {"ms_per_search_of_1024_queries": "rounds[i][key]", "shapes": {}}
    for d in CELLS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(d),
               "--nb", str(a.nb), "--train", str(a.train), "--niter", str(a.niter)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:])
            sys.stderr.write(f"\nstep d={d} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print(d, json.dumps(r), flush=True)
        result["shapes"][f"d{d}"] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
