#!/usr/bin/env python3
"""Kmeans.train (Lloyd iterations resident on the GPU, csrc/clustering.cpp) beside the trainer
behind every index's ``train`` (KMeans of csrc/kmeans.h: distance matrix, assignments to the
host, update on one host thread), on one MI355X.

    python profiles/kmeans_bench.py [--out profiles/kmeans_bench.json] [--rounds 5] [--only SHAPE]

Shapes (clustered rows: 4 k centres plus unit noise):
  coarse1024   n = 1 000 000, d = 128, k = 1024     the C2 coarse trainer
  pq256        n = 1 000 000, d = 8,   k = 256      one PQ sub-quantizer
  coarse16384  n = 4 000 000, d = 128, k = 16 384

Per shape, in one child process: ``--rounds`` alternating pairs of ``Kmeans.train(x)`` and
``IndexIVFFlat.train(x)`` on the same host rows with the same seed and NITER iterations, each
timed with the wall clock (both copy the rows in and the centroids out), and their centroids
asserted equal.  ``iter_ms`` is the resident trainer's time per iteration from device events
around synchronised ``train_device`` calls on rows already in HBM: (NITER + 1 iterations minus
1 iteration) / NITER, so allocation, the row norms and the initial centroids cancel.  The
accumulate kernel's time comes from a separate child under ``rocprofv3 --kernel-trace`` (one
``train_device`` call); its bytes are n d 4, each row read once.
Every GPU step is a child process under ``timeout``; the first that fails ends the run and no
JSON is written.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

NITER = 3
SEED = 1234
SHAPES = {
    "coarse1024": dict(n=1_000_000, d=128, k=1024),
    "pq256": dict(n=1_000_000, d=8, k=256),
    "coarse16384": dict(n=4_000_000, d=128, k=16384),
}
STEP_TIMEOUT = 900


def rows(n, d, k):
    import numpy as np

    rng = np.random.default_rng(7)
    centres = (rng.random((4 * k, d), dtype=np.float32) * 16.0).astype(np.float32)
    x = centres[rng.integers(0, 4 * k, size=n)]
    x += rng.standard_normal((n, d), dtype=np.float32)
    return np.ascontiguousarray(x)


def new_kmeans(faiss, d, k, niter):
    return faiss.Kmeans(d, k, niter=niter, seed=SEED, max_points_per_centroid=1 << 30)


def child_pairs(name, rounds):
    import numpy as np
    import torch

    import faiss_amd as faiss

    sh = SHAPES[name]
    n, d, k = sh["n"], sh["d"], sh["k"]
    x = rows(n, d, k)
    new_s, old_s = [], []
    for r in range(rounds + 1):  # round 0 warms both sides up and is not reported
        t0 = time.perf_counter()
        km = new_kmeans(faiss, d, k, NITER)
        km.train(x)
        t1 = time.perf_counter()
        ix = faiss.IndexIVFFlat(None, d, k, faiss.METRIC_L2)
        ix.niter_coarse, ix.seed = NITER, SEED
        ix.train(x)
        t2 = time.perf_counter()
        assert np.array_equal(km.centroids, ix.centroids()), "the two trainers disagree"
        if r:
            new_s.append(t1 - t0)
            old_s.append(t2 - t1)
        del ix
    objective, nsplit = float(km.obj[-1]), [s["nsplit"] for s in km.iteration_stats]
    xd = torch.from_numpy(x).cuda()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev = {}
    for niter in (1, NITER + 1):
        ms = []
        for r in range(rounds + 1):
            km = new_kmeans(faiss, d, k, niter)
            torch.cuda.synchronize()
            a.record()
            km.train_device(xd)
            b.record()
            b.synchronize()
            if r:
                ms.append(a.elapsed_time(b))
        ev[niter] = ms
    iter_ms = [(hi - lo) / NITER for lo, hi in zip(ev[1], ev[NITER + 1])]
    print("RESULT " + json.dumps(dict(shape=name, n=n, d=d, k=k, niter=NITER, rounds=rounds,
                                      new_train_s=new_s, parent_train_s=old_s, centroids_equal=True,
                                      new_faster_every_round=max(new_s) < min(old_s),
                                      iter_ms=iter_ms, objective=objective, nsplit=nsplit)))


def child_trace(name):
    import torch

    import faiss_amd as faiss

    sh = SHAPES[name]
    xd = torch.from_numpy(rows(sh["n"], sh["d"], sh["k"])).cuda()
    new_kmeans(faiss, sh["d"], sh["k"], NITER).train_device(xd)
    torch.cuda.synchronize()


def run_child(args, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, cwd=REPO)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"step {' '.join(args)} failed with status {p.returncode}; nothing else is started")
    return p.stdout


def accumulate_from_trace(name):
    """ns of every k_km_accumulate launch of one train_device call (NITER launches), and the
    eight kernels with the largest total time in that call (us)."""
    with tempfile.TemporaryDirectory() as tmp:
        run_child(["--trace-child", name],
                  prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"])
        out, total = [], {}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    kname = row.get("Kernel_Name", "")
                    ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    if "k_km_accumulate" in kname:
                        out.append(ns)
                    short = re.sub(r"^void |\(anonymous namespace\)::|chivf::|[<(].*", "", kname)
                    total[short] = total.get(short, 0) + ns
        top = sorted(total.items(), key=lambda kv: -kv[1])[:8]
        return out, {k: v / 1e3 for k, v in top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kmeans_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--pairs-child")
    ap.add_argument("--trace-child")
    a = ap.parse_args()
    if a.pairs_child:
        return child_pairs(a.pairs_child, a.rounds)
    if a.trace_child:
        return child_trace(a.trace_child)
    results = []
    for name in ([a.only] if a.only else list(SHAPES)):
        out = run_child(["--pairs-child", name, "--rounds", str(a.rounds)])
        res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        ns, top = accumulate_from_trace(name)
        if not ns:
            raise SystemExit("no k_km_accumulate launch in the kernel trace")
        nbytes = res["n"] * res["d"] * 4
        res["accumulate_us"] = [t / 1e3 for t in ns]
        res["accumulate_bytes"] = nbytes
        res["accumulate_GBps"] = [nbytes / t for t in ns]
        res["kernel_total_us"] = top
        print(json.dumps(res))
        results.append(res)
    with open(a.out, "w") as fh:
        json.dump(dict(niter=NITER, seed=SEED, shapes=results), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
