"""Control vectors x ensemble nodes in one call (jq_eval_f_g_grad_batch) against the same work as G consecutive jq_eval_f_g_grad calls on
ANOTHER build of the library (the parent commit's, which has no batch entry).

    python3 scripts/measure_nodes_batch.py --parent-lib PATH/libjuqbox_hip.so [--reps 7] [--out profiles/nodes_batch_ab.txt]

Shapes: SWAP-02 risk-neutral x 512 nodes with G = 1, 2, 4 control vectors; cnot3 (full length) x 9 nodes with G = 1, 4, 16.  Per shape
two worker processes stay alive on the one GPU -- this build (one batch call per repetition) and the parent build (G single calls per
repetition) -- each after one warm-up; the driver ALTERNATES them repetition by repetition, so drift of the machine hits both alike.
Wall time around the calls (they return after their stream synchronisation); median and min .. max of the repetitions.  A grouped shape
counts as faster only when its median is below the sequential one by more than the larger of the two spreads (max - min).

Every worker runs under its own time limit; the driver stops at the first worker that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("swap02_rn", 512, 1), ("swap02_rn", 512, 2), ("swap02_rn", 512, 4), ("cnot3", 9, 1), ("cnot3", 9, 4), ("cnot3", 9, 16)]


def worker(case, nq, G, batch):
    """stdin: one line per repetition; stdout: one JSON line per repetition (seconds), a first one after set-up and warm-up"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib
    if not batch:      # (the parent build does not export the batch entry: bind the table without it)
        _lib.SYMBOLS.pop("jq_eval_f_g_grad_batch", None)
    params, info = jq.cases.BUILDERS[case]()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", info["golden"] + ".json"))) if info.get("golden") else {}
    pcof = np.array(golden["pcof0"]) if "pcof0" in golden else np.asarray(info["pcof0"], dtype=np.float64)
    if case == "cnot3":
        nodes, weights, shift = jq.cases.cnot3_ensemble(nq)
    else:
        nodes, weights, shift = info["nodes"][:nq], info["weights"][:nq], params.shift_weights_reference()
    rng = np.random.default_rng(1000 + G)
    amp = 0.05 * max(1.0, float(np.max(np.abs(pcof))))
    vecs = [pcof] + [pcof + amp * rng.standard_normal(pcof.size) for _ in range(G - 1)]
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    if batch:
        run = lambda: jq.eval_f_g_grad_batch(vecs, params, wa, nodes, weights, True, shift=shift)
    else:
        run = lambda: [jq.eval_f_g_grad(v, params, wa, nodes, weights, True, shift=shift) for v in vecs]
    run()      # warm-up
    t = wa.last_timing()
    ready = dict(ready=True, family=t["kernel_family"], variant=t["kernel_variant"], version=_lib.load().jq_version().decode())
    if batch:
        ready["pcof_batch"] = wa.plan_info()["pcof_batch"]
    print(json.dumps(ready), flush=True)
    for _ in sys.stdin:
        t0 = time.perf_counter()
        run()
        print(json.dumps(dict(s=time.perf_counter() - t0)), flush=True)
    wa.close()


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libjuqbox_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodes_batch_ab.txt"))
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.worker[3] == "batch")
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        print("need --parent-lib: the library built from the parent commit")
        return 2
    if a.reps < 5:
        print("need at least five repetitions")
        return 2

    def start(case, nq, G, kind):
        env = dict(os.environ)
        if kind == "seq":
            env["JQ_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("JQ_LIB", None)
        cmd = ["timeout", "-k", "10", str(a.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", case, str(nq), str(G), kind]
        p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        line = p.stdout.readline()
        return (p, json.loads(line)) if line.strip() else (p, None)

    def stop(p):
        try:
            p.stdin.close()
        except OSError:
            pass
        return p.wait()

    lines, versions = [], {}
    for case, nq, G in SHAPES:
        pb, rb = start(case, nq, G, "batch")
        if rb is None:
            print("%s x %d nodes, G = %d: the batch worker ended with status %d: stopping" % (case, nq, G, stop(pb)))
            return 1
        ps, rs = start(case, nq, G, "seq")
        if rs is None:
            stop(pb)
            print("%s x %d nodes, G = %d: the sequential worker ended with status %d: stopping" % (case, nq, G, stop(ps)))
            return 1
        versions = dict(batch=rb["version"], parent=rs["version"])
        tb, ts, ok = [], [], True
        for _ in range(a.reps):      # alternate: batch, sequential, batch, sequential ...
            for p, acc in ((pb, tb), (ps, ts)):
                p.stdin.write("go\n")
                p.stdin.flush()
                line = p.stdout.readline()
                if not line.strip():
                    ok = False
                    break
                acc.append(json.loads(line)["s"])
            if not ok:
                break
        st = stop(pb), stop(ps)
        if not ok or st != (0, 0):
            print("%s x %d nodes, G = %d: a worker ended early (status %r): stopping" % (case, nq, G, st))
            return 1
        spread = max(max(tb) - min(tb), max(ts) - min(ts))
        verdict = "FASTER" if med(tb) < med(ts) - spread else "SLOWER" if med(tb) > med(ts) + spread else "within the spread"
        info = rb["pcof_batch"]
        line = ("%-9s x %3d nodes, G %2d  %-10s family %d, %2d per launch | one batch call median %9.5f s (%.5f .. %.5f) | %2d single calls, "
                "parent build (family %d, variant %d) median %9.5f s (%.5f .. %.5f) | sequential / batch %5.2f | spread %.5f s: batch %s"
                % (case, nq, G, info["mode"], rb["family"], info["vectors_per_launch"], med(tb), min(tb), max(tb), G, rs["family"], rs["variant"],
                   med(ts), min(ts), max(ts), med(ts) / med(tb), spread, verdict))
        print(line, flush=True)
        lines.append(line)
    head = ["jq_eval_f_g_grad_batch (this build) against G consecutive jq_eval_f_g_grad calls (parent build), alternating in one job on one GPU",
            "(scripts/measure_nodes_batch.py; wall time, median and min .. max of %d repetitions each after one warm-up)" % a.reps,
            "this build:   %s" % versions["batch"], "parent build: %s" % versions["parent"], ""]
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
