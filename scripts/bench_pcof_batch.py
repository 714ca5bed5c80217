"""Batches of control vectors (jq_traceobjgrad_batch) against the same vectors evaluated one call at a time.

    python3 scripts/bench_pcof_batch.py [--cases cnot3,cnot2] [--sizes 1,8,64,256] [--reps 5] [--seq-max 8] [--out profiles/pcof_batch.txt]

For every case and every batch size G: one warm-up, then `reps` timed batches of G perturbed control vectors, and -- in the same process
and run -- `reps` timed loops of G sequential traceobjgrad calls on the same handle (G <= --seq-max; beyond that the loop of --seq-max
calls is scaled, and the line says so: 256 sequential cnot3 evaluations take 40 s each time).  Wall time around the calls (they return
after their stream synchronisation); median and min .. max of the repetitions.  Two conditions are checked and reported, not tuned:
the G = 8 batch beats 8 sequential calls, and G = 1 costs no more than a single call beyond the spread of the repetitions.

Every (case, G) step is a child process under its own time limit; the parent stops at the first step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step(case, G, reps, seq_max):
    sys.path.insert(0, ROOT)
    import numpy as np
    import juqbox_jl_amd as jq
    params, info = jq.cases.BUILDERS[case]()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", info["golden"] + ".json"))) if info.get("golden") else {}
    pcof = np.array(golden["pcof0"]) if "pcof0" in golden else np.asarray(info["pcof0"], dtype=np.float64)
    rng = np.random.default_rng(1000 + G)
    amp = 0.05 * max(1.0, float(np.max(np.abs(pcof))))
    vecs = [pcof] + [pcof + amp * rng.standard_normal(pcof.size) for _ in range(G - 1)]
    wa = jq.Working_Arrays_HIP(params, pcof.size)

    def timed(f, n):
        f()      # warm-up
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return ts

    tb = timed(lambda: jq.traceobjgrad_batch(vecs, params, wa, True), reps)
    pb = wa.plan_info()["pcof_batch"]
    fam = wa.last_timing()["kernel_family"]
    nseq = min(G, seq_max)
    tsq = timed(lambda: [jq.traceobjgrad(v, params, wa, False, True) for v in vecs[:nseq]], reps)
    fam1 = wa.last_timing()["kernel_family"], wa.last_timing()["kernel_variant"]
    wa.close()
    scale = G / nseq
    print(json.dumps(dict(case=case, G=G, mode=pb["mode"], per_launch=pb["vectors_per_launch"], family=fam, single_family_variant=fam1,
                          batch_s=tb, seq_s=[t * scale for t in tsq], seq_measured_calls=nseq, version=jq._lib.load().jq_version().decode())))


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cnot3,cnot2")
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seq-max", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcof_batch.txt"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.reps, a.seq_max)
        return 0
    lines, rows = [], {}
    for case in a.cases.split(","):
        for G in [int(g) for g in a.sizes.split(",")]:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", case, str(G),
                   "--reps", str(a.reps), "--seq-max", str(a.seq_max)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                print(r.stdout)
                print("step %s G=%d ended with status %d: stopping" % (case, G, r.returncode))
                return 1
            d = json.loads(r.stdout.strip().splitlines()[-1])
            rows[(case, G)] = d
            b, s = d["batch_s"], d["seq_s"]
            note = "" if d["seq_measured_calls"] == G else "  (sequential: %d calls measured, scaled)" % d["seq_measured_calls"]
            line = ("%-6s G %3d  %-10s family %d, %3d per launch | batch median %8.4f s (%.4f .. %.4f) | %3d sequential calls median %8.4f s (%.4f .. %.4f) | "
                    "sequential / batch %6.2f%s" % (case, G, d["mode"], d["family"], d["per_launch"], med(b), min(b), max(b), G, med(s), min(s), max(s), med(s) / med(b), note))
            print(line, flush=True)
            lines.append(line)
        if (case, 8) in rows:
            d = rows[(case, 8)]
            lines.append("%-6s condition: the G = 8 batch is faster than 8 sequential calls: %s" % (case, "MET" if med(d["batch_s"]) < med(d["seq_s"]) else "NOT MET"))
        if (case, 1) in rows:
            d = rows[(case, 1)]
            spread = max(max(d["seq_s"]) - min(d["seq_s"]), max(d["batch_s"]) - min(d["batch_s"]))
            ok = med(d["batch_s"]) <= med(d["seq_s"]) + spread
            lines.append("%-6s condition: G = 1 costs no more than a single call beyond the spread of the repetitions (%.4f s): %s" % (case, spread, "MET" if ok else "NOT MET"))
        print("\n".join(lines[-2:]), flush=True)
    head = ["jq_traceobjgrad_batch against sequential jq_traceobjgrad calls (scripts/bench_pcof_batch.py; wall time, median of %d after one warm-up)" % a.reps,
            "library: %s" % next(iter(rows.values()))["version"], ""]
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
