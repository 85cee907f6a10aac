#!/usr/bin/env python3
"""A/B runs of k_sq_scan's two build choices on one MI355X:

    step   dimensions per staged step (-DSQ_SCAN_STEP_DIMS=32 | 64)
    group  queries per work item at k <= 64: 8, two workgroups per CU, or 4, three workgroups
           per CU at twice the code bytes (-DSQ_SCAN_GROUP_SMALL_K=8 | 4 for both codecs,
           -DSQ_SCAN_GROUP_SMALL_K_8BIT=8 | 4 for the 8-bit codec alone)

    python profiles/indexsq_variants.py --lib <name>=chameleon-rag-acceleration_amd/lib/libivfpq.so \\
        --lib <name>=<a libivfpq.so linked with sq_scan.o built with other switches> ... --out <json>

The two runs behind the shipped choice are profiles/indexsq_variants_step.json (step 32 against
64 and G = 8 against 4, from the 32-dimension build) and profiles/indexsq_variants_group.json
(G = 4 for the 8-bit codec alone, from the 64-dimension build); their "libraries" entry maps the
labels to the names the runs were given.

Each library is loaded by a child process of its own (IVFPQ_LIB) under ``timeout``; the
children alternate, three rounds of every library, and a child that fails ends the run.  A
child times SQfp16 and SQ8 over both shapes of profiles/indexsq_bench.py at k = 10 and 100,
device events around whole search_device calls over windows of at least a second."""
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

ROUNDS, STEP_TIMEOUT = 3, 300


def child(nb):
    import torch

    from indexsq_bench import KEYS, KS, NQ, SHAPES, build_indexes, make_data
    from ivfflat_bench import timed

    out = {}
    for name in SHAPES:
        txb, txq = make_data(name, nb)
        index = build_indexes(name, txb, KEYS[:2])
        del txb
        for key, ix in index.items():
            for k in KS:
                Dd = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
                Id = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
                out[f"{name} {key} k={k}"] = timed(lambda: ix.search_device(txq, k, Dd, Id), torch)[0]
        del index
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="name=path of a libivfpq.so")
    ap.add_argument("--out", required=True)
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.nb)), flush=True)
        return 0
    libs = [spec.split("=", 1) for spec in a.lib]
    runs = {name: {} for name, _ in libs}
    for _ in range(ROUNDS):
        for name, path in libs:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child",
                   "--nb", str(a.nb)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               env=dict(os.environ, IVFPQ_LIB=os.path.abspath(path)))
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.stderr.write(p.stdout[-4000:])
                sys.stderr.write(f"\nlibrary {name} failed (exit {p.returncode}); stopping\n")
                return 1
            r = json.loads(lines[-1][7:])
            print(name, json.dumps(r), flush=True)
            for case, ms in r.items():
                runs[name].setdefault(case, []).append(ms)
    result = {"nb": a.nb, "rounds": ROUNDS,
              "ms_per_batch": {name: {case: dict(runs=v, median=statistics.median(v)) for case, v in cases.items()}
                               for name, cases in runs.items()}}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
