"""One control vector over an ensemble of drift Hamiltonians in one call (jq_traceobjgrad_drifts) against the loop jq_update_hconst +
jq_traceobjgrad over the same members on ANOTHER build of the library (the parent commit's, which has no such entry).

    python3 scripts/measure_drift_batch.py --parent-lib PATH/libjuqbox_hip.so [--reps 5] [--out profiles/drift_batch_ab.txt]

Shapes: SWAP-02 with 64 and 512 members (Hconst + 1e-2 |Hconst|_max R, R seeded random symmetric); cnot3 at full length with 16 and 64
structure-preserving members (every stored nonzero scaled by 1 + 1e-2 r_ij, plus a random diagonal: the 4 x 4 x n plan holds them all).
Both sides go through the C ABI directly with preallocated outputs, gradients included.  Per shape two worker processes stay alive on the
one GPU -- this build (one call per repetition) and the parent build (ndrift x two calls per repetition) -- each after one warm-up; the
driver ALTERNATES them repetition by repetition, so drift of the machine hits both alike.  Wall time around the calls (they return after
their stream synchronisation); median and min .. max of the repetitions.  A shape counts as faster only when its median is below the
loop's by more than the larger of the two spreads (max - min).

Every worker runs under its own time limit; the driver stops at the first worker that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("swap02", 64), ("swap02", 512), ("cnot3", 16), ("cnot3", 64)]
NEW = ("jq_traceobjgrad_drifts", "jq_eval_f_g_grad_drifts")


def members_of(case, H0, n):
    import numpy as np
    rng = np.random.default_rng(7000 + n)
    amp = 1e-2 * float(np.max(np.abs(H0)))
    out = []
    for _ in range(n):
        r = rng.standard_normal(H0.shape)
        r = 0.5 * (r + r.T)
        if case == "cnot3":
            out.append(H0 * (1.0 + 1e-2 * r) + np.diag(amp * rng.standard_normal(H0.shape[0])))
        else:
            out.append(H0 + amp * r)
    return out


def worker(case, n, batch):
    """stdin: one line per repetition; stdout: one JSON line per repetition (seconds), a first one after set-up and warm-up"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib
    if not batch:      # (the parent build does not export the new entries: bind the table without them)
        for name in NEW:
            _lib.SYMBOLS.pop(name, None)
    L = _lib.load()
    params, info = jq.cases.BUILDERS[case]()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", info["golden"] + ".json"))) if info.get("golden") else {}
    pcof = np.ascontiguousarray(golden["pcof0"] if "pcof0" in golden else info["pcof0"], dtype=np.float64)
    nc = pcof.size
    H0 = np.asarray(params.Hconst, dtype=np.float64)
    H = np.ascontiguousarray(np.stack([M.ravel(order="F") for M in members_of(case, H0, n)]))
    wa = jq.Working_Arrays_HIP(params, nc)
    wa.sync_params()
    h = wa.handle
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    out4, tg, ig, lg = np.zeros((n, 4)), np.zeros((n, nc)), np.zeros((n, nc)), np.zeros((n, nc))
    own = np.ascontiguousarray(H0.ravel(order="F"))

    def run_batch():
        _lib.check(L.jq_traceobjgrad_drifts(h, ptr(pcof), nc, ptr(H), n, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)), h)

    def run_loop():
        for i in range(n):
            _lib.check(L.jq_update_hconst(h, ptr(H[i])), h)
            _lib.check(L.jq_traceobjgrad(h, ptr(pcof), nc, 1, ptr(out4[i]), ptr(tg[i]), ptr(ig[i]), ptr(lg[i])), h)
        _lib.check(L.jq_update_hconst(h, ptr(own)), h)      # (the batch call leaves the handle's drift as it was, too)

    run = run_batch if batch else run_loop
    run()      # warm-up
    t = wa.last_timing()
    ready = dict(ready=True, family=t["kernel_family"], variant=t["kernel_variant"], version=L.jq_version().decode(),
                 checksum=float(np.sum(out4[:, 0])))
    if batch:
        ready["drift_batch"] = wa.plan_info()["drift_batch"]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_batch_ab.txt"))
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--worker", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], int(a.worker[1]), a.worker[2] == "batch")
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        print("need --parent-lib: the library built from the parent commit")
        return 2
    if a.reps < 5:
        print("need at least five repetitions")
        return 2

    def start(case, n, kind):
        env = dict(os.environ)
        if kind == "seq":
            env["JQ_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("JQ_LIB", None)
        cmd = ["timeout", "-k", "10", str(a.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", case, str(n), kind]
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
    for case, n in SHAPES:
        pb, rb = start(case, n, "batch")
        if rb is None:
            print("%s x %d members: the batch worker ended with status %d: stopping" % (case, n, stop(pb)))
            return 1
        ps, rs = start(case, n, "seq")
        if rs is None:
            stop(pb)
            print("%s x %d members: the loop worker ended with status %d: stopping" % (case, n, stop(ps)))
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
            print("%s x %d members: a worker ended early (status %r): stopping" % (case, n, st))
            return 1
        spread = max(max(tb) - min(tb), max(ts) - min(ts))
        verdict = "FASTER" if med(tb) < med(ts) - spread else "SLOWER" if med(tb) > med(ts) + spread else "within the spread"
        info = rb["drift_batch"]
        line = ("%-7s x %3d members  %-10s family %d, %3d per launch | one call median %9.5f s (%.5f .. %.5f) | loop of %3d x (jq_update_hconst + "
                "jq_traceobjgrad), parent build (family %d, variant %d) median %9.5f s (%.5f .. %.5f) | loop / one call %5.2f | spread %.5f s: one call %s"
                " | sum of objfv %.12e vs %.12e"
                % (case, n, info["mode"], rb["family"], info["members_per_launch"], med(tb), min(tb), max(tb), n, rs["family"], rs["variant"],
                   med(ts), min(ts), max(ts), med(ts) / med(tb), spread, verdict, rb["checksum"], rs["checksum"]))
        print(line, flush=True)
        lines.append(line)
    head = ["jq_traceobjgrad_drifts (this build) against the loop jq_update_hconst + jq_traceobjgrad over the same members (parent build), alternating in one job on one GPU",
            "(scripts/measure_drift_batch.py; wall time with gradients, median and min .. max of %d repetitions each after one warm-up)" % a.reps,
            "this build:   %s" % versions["batch"], "parent build: %s" % versions["parent"], ""]
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
