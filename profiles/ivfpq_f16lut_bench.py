#!/usr/bin/env python3
"""IVF-PQ search with float16 lookup tables (GpuClonerOptions.useFloat16, k_scan_lists_h) beside the
fp32 tables of the same index on one MI355X.

    python profiles/ivfpq_f16lut_bench.py [--out profiles/ivfpq_f16lut_bench.json] [--nb 1000000]

Data: clustered vectors from datasets.synthetic_sift_like, d = 128, 1 M base rows, 1024 queries, L2.
Indexes: IVF4096,PQ64 and IVF1024,PQ32 at k = 100, IVF1024,PQ16 at k = 10; nprobe 1, 16, 64.
One child process per index under ``timeout``; the first step that fails ends the run (nothing else is
started on the GPU; the JSON keeps the steps that finished).

Per (index, nprobe), three alternating rounds of
  half_device_ms   search_device with use_float16_lut on: device events around whole calls (coarse
                   step, tables, list scan, merge), a window of at least a second after a warm-up
  fp32_device_ms   the same index and call with the flag off
``half_faster_in_every_pair`` compares the two of every round.  ``recall_half`` / ``recall_fp32``: the share
of IndexFlatL2's k nearest that each setting returns (recall@k); ``labels_equal_fp32`` the share of equal labels.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd"), os.path.join(REPO, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

NQ, D = 1024, 128
STEP_TIMEOUT = 420
INDEXES = {"IVF4096,PQ64": 100, "IVF1024,PQ32": 100, "IVF1024,PQ16": 10}
NPROBES = (1, 16, 64)


def step_index(key, nb):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import datasets
    from ivfflat_bench import timed

    k = INDEXES[key]
    xb = datasets.synthetic_sift_like(nb, D, seed=1234)
    xq = datasets.synthetic_sift_like(NQ, D, seed=123)
    exact = faiss.IndexFlatL2(D)
    co = faiss.GpuClonerOptions()
    co.useFloat16 = True
    index = faiss.index_cpu_to_gpu(faiss.StandardGpuResources(), 0, faiss.index_factory(D, key), co)
    index.niter_coarse = index.niter_pq = 10
    index.train(xb[:200_000])
    for lo in range(0, nb, 100_000):
        index.add(xb[lo:lo + 100_000])
        exact.add(xb[lo:lo + 100_000])
    _, It = exact.search(xq, k)
    del xb, exact
    txq = torch.from_numpy(xq).cuda()
    Dh = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
    Ih = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
    Df, If = torch.empty_like(Dh), torch.empty_like(Ih)

    def recall(I):
        I = I.cpu().numpy()
        return float(np.mean([len(np.intersect1d(I[q], It[q])) for q in range(NQ)]) / k)

    results = []
    for nprobe in NPROBES:
        index.setNumProbes(nprobe)
        rounds = []
        for _ in range(3):
            index.use_float16_lut = True
            h_ms, h_reps = timed(lambda: index.search_device(txq, k, Dh, Ih), torch)
            index.use_float16_lut = False
            f_ms, f_reps = timed(lambda: index.search_device(txq, k, Df, If), torch)
            rounds.append(dict(half_device_ms=h_ms, half_calls=h_reps, fp32_device_ms=f_ms, fp32_calls=f_reps))
        hs, fs = sorted(r["half_device_ms"] for r in rounds), sorted(r["fp32_device_ms"] for r in rounds)
        results.append(dict(
            index=key, nb=nb, nq=NQ, k=k, nprobe=nprobe, rounds=rounds, half_device_ms=hs[1], fp32_device_ms=fs[1],
            half_min_max_ms=[hs[0], hs[2]], fp32_min_max_ms=[fs[0], fs[2]], speedup=fs[1] / hs[1],
            half_faster_in_every_pair=all(r["half_device_ms"] < r["fp32_device_ms"] for r in rounds),
            recall_half=recall(Ih), recall_fp32=recall(If), labels_equal_fp32=float((Ih == If).float().mean().item())))
        print("SHAPE " + json.dumps(results[-1]), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivfpq_f16lut_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:  # child: one index, one JSON line
        print("RESULT " + json.dumps(step_index(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "nq": NQ, "d": D, "indexes": {}}
    for key in INDEXES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", key,
               "--nb", str(a.nb)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines, tail = [], []
        for ln in p.stdout:  # a line per finished setting, as it comes
            tail = (tail + [ln])[-60:]
            if ln.startswith("RESULT "):
                lines.append(ln)
            elif ln.startswith("SHAPE "):
                s = json.loads(ln[6:])
                print(f"{key} nprobe={s['nprobe']} k={s['k']}: half {s['half_device_ms']:.3f} ms, fp32 "
                      f"{s['fp32_device_ms']:.3f} ms ({s['speedup']:.2f}x), recall@k {s['recall_half']:.4f} / "
                      f"{s['recall_fp32']:.4f}", flush=True)
        p.wait()
        if p.returncode != 0 or not lines:
            sys.stderr.write("".join(tail))
            sys.stderr.write(f"\nstep {key} failed (exit {p.returncode}); stopping\n")
            return 1
        result["indexes"][key] = json.loads(lines[-1][7:])
        with open(a.out, "w") as f:  # (rewritten after every step: a later step's failure keeps the earlier numbers)
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
