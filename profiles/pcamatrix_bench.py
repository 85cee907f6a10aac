#!/usr/bin/env python3
"""PCAMatrix training on one MI355X beside the host code it replaces.

    python profiles/pcamatrix_bench.py [--out profiles/pcamatrix_bench.json] [--dims 128,768]

Shapes: d = 128 and d = 768, n = 1000 d rows (Faiss's max_points_per_d cap, the most train
ever keeps), d_out = d / 2; standard normal rows with per-column scales and an offset, from a
seed.  One child process per d under ``timeout``; the first step that fails ends the run
(nothing else is started on the GPU; the JSON keeps the steps that finished).

Per shape, three alternating rounds of
  moments_ms        ivfpq_pca_moments_device on resident rows (mean + scatter + reduce; the call
                    returns after a stream synchronise), host clock over a window of calls of at
                    least a second after a warm-up
  train_device_ms   PCAMatrix.train_device on resident rows: moments, the copy of mean and scatter
                    to the host, numpy.linalg.eigh in float64, prepare_Ab
  upload_ms         the rows from pageable host memory to the device, synchronised
  train_ms          PCAMatrix.train on the numpy rows (upload + train_device's work)
  host_ms           the host alternative: float32 numpy column mean, centring and xc.T @ xc,
                    numpy at the machine's thread setting (the moments only, no eigh)
  eigh_ms           numpy.linalg.eigh of the d x d float64 scatter alone
Computed: mfma_tile_flop = 2 n 64 64 tiles (what the upper-triangle tiles execute) and
mfma_fraction = mfma_tile_flop / moments time / the 155 TF measured for v_mfma_f32_16x16x4_f32
(the moments time includes the mean and the reduce, so this is a whole-call rate, not the
scatter kernel's share of peak); full_product_tflops = 2 n d d / moments time.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MFMA_F32_FLOPS = 155e12
STEP_TIMEOUT = 500


def step_d(d, n):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import transform as T

    rng = np.random.default_rng(d)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= (1.0 + 4.0 * rng.random(d, dtype=np.float32))[None, :]
    x += (10.0 * rng.standard_normal(d, dtype=np.float32))[None, :]
    plan = T.pca_plan(n, d)

    def sync():
        torch.cuda.synchronize()

    def wall(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    xd = torch.from_numpy(x).cuda()
    T.pca_moments_device(xd)  # warm-up: code objects, allocator
    one, _ = wall(lambda: T.pca_moments_device(xd))
    reps = max(3, int(1000.0 / max(one, 1e-3)) + 1)

    def moments_window():
        for _ in range(reps):
            out = T.pca_moments_device(xd)
        return out

    def host_moments():
        m = x.mean(0, dtype=np.float32)
        xc = x - m[None, :]
        return m, xc.T @ xc

    rounds = []
    for _ in range(3):
        t_mom, (mean_d, S_d) = wall(moments_window)
        pd = faiss.PCAMatrix(d, d // 2)
        t_dev, _ = wall(lambda: pd.train_device(xd))
        t_up, xu = wall(lambda: torch.from_numpy(x).cuda())
        del xu
        ph = faiss.PCAMatrix(d, d // 2)
        t_train, _ = wall(lambda: ph.train(x))
        t_host, (mean_h, S_h) = wall(host_moments)
        S64 = S_d.cpu().numpy().astype(np.float64)
        t_eigh, _ = wall(lambda: np.linalg.eigh(S64))
        rounds.append(dict(moments_ms=t_mom / reps, moments_calls=reps, train_device_ms=t_dev, upload_ms=t_up,
                           train_ms=t_train, host_ms=t_host, eigh_ms=t_eigh))
        print("ROUND " + json.dumps(rounds[-1]), flush=True)
    S_g = S_d.cpu().numpy()
    scale = np.sqrt(np.outer(np.diag(S_g), np.diag(S_g)))
    med = lambda key: sorted(r[key] for r in rounds)[1]  # noqa: E731
    tile_flop = 2.0 * n * 64 * 64 * plan["tiles"]
    mom = med("moments_ms")
    return dict(d=d, n=n, d_out=d // 2, plan=plan, rounds=rounds, moments_ms=mom, train_device_ms=med("train_device_ms"),
                upload_ms=med("upload_ms"), train_ms=med("train_ms"), host_ms=med("host_ms"), eigh_ms=med("eigh_ms"),
                mfma_tile_flop=tile_flop, mfma_fraction=tile_flop / (mom * 1e-3) / MFMA_F32_FLOPS,
                full_product_tflops=2.0 * n * d * d / (mom * 1e-3) / 1e12,
                upload_share_of_train=med("upload_ms") / med("train_ms"),
                train_faster_than_host_in_every_round=all(r["train_ms"] < r["host_ms"] + r["eigh_ms"] for r in rounds),
                train_device_faster_than_host_in_every_round=all(r["train_device_ms"] < r["host_ms"] + r["eigh_ms"]
                                                                 for r in rounds),
                same_A_train_and_train_device=bool(np.array_equal(pd.A, ph.A)),
                max_scatter_difference_from_host_over_scale=float((np.abs(S_g - S_h) / scale).max()),
                numpy_threads=os.environ.get("OMP_NUM_THREADS", "unset"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcamatrix_bench.json"))
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--rows-per-d", type=int, default=1000)
    ap.add_argument("--step", type=int)
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_d(a.step, a.rows_per_d * a.step)), flush=True)
        return 0
    result = {"mfma_f32_flops": MFMA_F32_FLOPS, "rows_per_d": a.rows_per_d, "dims": {}}
    for d in [int(v) for v in a.dims.split(",")]:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(d),
               "--rows-per-d", str(a.rows_per_d)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines, tail = [], []
        for ln in p.stdout:
            tail = (tail + [ln])[-60:]
            if ln.startswith("RESULT "):
                lines.append(ln)
            elif ln.startswith("ROUND "):
                print(f"  d={d} {ln.strip()}", flush=True)
        p.wait()
        if p.returncode != 0 or not lines:
            sys.stderr.write("".join(tail))
            sys.stderr.write(f"\nstep d={d} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print(f"d={d} n={r['n']}: moments {r['moments_ms']:.3f} ms ({r['mfma_fraction']:.3f} of the fp32 MFMA rate), "
              f"train_device {r['train_device_ms']:.1f} ms, upload {r['upload_ms']:.1f} ms, train {r['train_ms']:.1f} ms, "
              f"host moments {r['host_ms']:.1f} ms + eigh {r['eigh_ms']:.1f} ms", flush=True)
        result["dims"][str(d)] = r
        with open(a.out, "w") as f:  # (rewritten after every step: a later step's failure keeps the earlier numbers)
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
