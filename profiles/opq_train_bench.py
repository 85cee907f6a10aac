#!/usr/bin/env python3
"""OPQMatrix.train_device (rows resident on one MI355X) beside the host OPQMatrix.train.

    python profiles/opq_train_bench.py [--out profiles/opq_train_bench.json]

Shapes: d = 128, M = 16 (the "OPQ16" front of bench_gpu_1bn.py) and d = 768 -> 384, M = 96 (beir's
OPQMatrix(768, 96, 384)).  Both trainers get the same rows, seed and settings, so they start from
the same matrix and the same initial codebooks.  The settings are cut so that the host trainer
finishes in about a minute per run: n = 16384 rows, niter = 3, niter_pq_0 = 6, niter_pq = 2 (10
Lloyd iterations of every sub-quantizer, 3 SVDs; Faiss's defaults are 65536 rows and 236 + 50).
Rows: 32 latent Gaussian factors of decaying scale mixed into d dimensions plus noise, seeded.

Times: the host clock around whole (synchronous) calls; train_device ends in a device
synchronise.  One short device training first (code objects loaded), then the two trainers in
turn, ROUNDS rounds; median and max - min spread.  ``device_s`` / ``svd_s`` split train_device's
time into the rounds on the GPU and the float64 SVDs on the host (OPQMatrix.timing).  ``pq_mse`` is
the PQ reconstruction error of the rotated, centred training set under each trainer's matrix,
measured with the host _pq_kmeans / _pq_recons (5 iterations, seed 5).  No speed-up is promised:
``ratio_device_to_host`` is reported as measured.
Every GPU step runs in a child process of its own under ``timeout``; the first step that fails
ends the run (nothing else is started on the GPU) and no JSON is written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"d128_M16": (128, 16, 128), "d768_d384_M96": (768, 96, 384)}
N, NITER, NITER_PQ_0, NITER_PQ, ROUNDS = 16384, 3, 6, 2, 2
STEP_TIMEOUT = 540


def rows(n, d):
    import numpy as np

    rng = np.random.default_rng(2)
    z = rng.standard_normal((n, 32)).astype(np.float32) * np.linspace(8, 1, 32, dtype=np.float32)
    return (z @ rng.standard_normal((32, d)).astype(np.float32)
            + 0.05 * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def step_shape(name):
    import numpy as np
    import torch

    from faiss_amd.transform import OPQMatrix, opq_plan

    d, M, d2 = SHAPES[name]
    x = rows(N, d)
    xd = torch.from_numpy(x).cuda()

    def make(niter=NITER):
        o = OPQMatrix(d, M, d2)
        o.niter, o.niter_pq_0, o.niter_pq = niter, NITER_PQ_0, NITER_PQ
        return o

    make(1).train_device(xd)  # warm-up
    runs = {"device": [], "host": []}
    split = {"device_s": [], "svd_s": []}
    mats = {}
    for _ in range(ROUNDS):
        o = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o.train_device(xd)
        runs["device"].append(time.perf_counter() - t0)
        for k in split:
            split[k].append(o.timing[k])
        mats["device"] = o.A
        o = make()
        t0 = time.perf_counter()
        o.train(x)
        runs["host"].append(time.perf_counter() - t0)
        mats["host"] = o.A
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    out = dict(d=d, d2=d2, M=M, n=N, niter=NITER, niter_pq_0=NITER_PQ_0, niter_pq=NITER_PQ, rounds=ROUNDS,
               cross_plan=opq_plan(N, d, d2))
    for key, A in mats.items():
        xp = xc @ A.astype(np.float64).T
        cb = OPQMatrix._pq_kmeans(xp, M, [None] * M, 5, np.random.default_rng(5))
        mse = float(((xp - OPQMatrix._pq_recons(xp, M, cb)) ** 2).sum(1).mean())
        r = runs[key]
        out[key] = dict(s_runs=r, s=statistics.median(r), spread_s=max(r) - min(r), pq_mse=mse)
    for k, v in split.items():
        out["device"][k] = statistics.median(v)
    out["ratio_device_to_host"] = out["device"]["s"] / out["host"]["s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "opq_train_bench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_shape(a.step)), flush=True)
        return 0
    result = {"shapes": {}}
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:])
            sys.stderr.write(f"\nstep {name} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print(name, json.dumps(r), flush=True)
        result["shapes"][name] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
