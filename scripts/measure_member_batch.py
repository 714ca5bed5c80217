"""One control vector over an ensemble of miscalibrated control amplitudes in one call (jq_traceobjgrad_members) against the two
alternatives, all on THIS build:

    python3 scripts/measure_member_batch.py [--reps 5] [--members 64] [--out profiles/member_batch_ab.txt]

  (a) members  jq_traceobjgrad_members with ctrl_mix = diag(1 + 0.05 r_i), one call per repetition;
  (b) drifts   jq_traceobjgrad_drifts with the same member count, every member the handle's own drift, one call per repetition -- the
               grouped launches without a mix: what the mix costs on top of a drift ensemble;
  (c) handles  a loop of jq_traceobjgrad over one handle PER MEMBER, each created beforehand (outside the timing) with that member's scaled
               operators Hsym_k (1 + 0.05 r_ik), Hanti_k likewise -- the only way a caller has without the call.
Shapes: SWAP-02 at full length and cnot3 shortened to 2 000 steps.  All three go through the C ABI directly with preallocated outputs,
gradients included.  Per shape three worker processes stay alive on the one GPU, each after one warm-up; the driver ALTERNATES them
repetition by repetition, so drift of the machine hits all alike.  Wall time around the calls (they return after their stream
synchronisation); median and min .. max of the repetitions.  No ratio is a pass / fail gate: the record says what was measured.

Every worker runs under its own time limit; the driver stops at the first worker that fails."""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("swap02", None), ("cnot3", 2000)]
KINDS = ("members", "drifts", "handles")


def worker(case, nsteps, n, kind):
    """stdin: one line per repetition; stdout: one JSON line per repetition (seconds), a first one after set-up and warm-up"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info = jq.cases.BUILDERS[case]()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", info["golden"] + ".json"))) if info.get("golden") else {}
    pcof = np.ascontiguousarray(golden["pcof0"] if "pcof0" in golden else info["pcof0"], dtype=np.float64)
    if nsteps:
        params.T = params.T * nsteps / params.nsteps
        params.nsteps = nsteps
    nc, Nc = pcof.size, params.Ncoupled
    scales = 1.0 + 0.05 * np.random.default_rng(8000 + n).standard_normal((n, Nc))
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    out4, tg, ig, lg = np.zeros((n, 4)), np.zeros((n, nc)), np.zeros((n, nc)), np.zeros((n, nc))
    handles = []
    if kind == "handles":
        for i in range(n):
            p = copy.copy(params)
            p.Hsym_ops = [scales[i, k] * np.asarray(params.Hsym_ops[k], dtype=np.float64) for k in range(Nc)]
            p.Hanti_ops = [scales[i, k] * np.asarray(params.Hanti_ops[k], dtype=np.float64) for k in range(Nc)]
            w = jq.Working_Arrays_HIP(p, nc)
            w.sync_params()
            handles.append(w)
        wa = handles[0]
    else:
        wa = jq.Working_Arrays_HIP(params, nc)
        wa.sync_params()
    h = wa.handle
    C = np.ascontiguousarray(np.stack([M.ravel(order="F") for M in np.moveaxis(jq.amplitude_mix(scales), 2, 0)]))
    H = np.ascontiguousarray(np.tile(np.asarray(params.Hconst, dtype=np.float64).ravel(order="F"), (n, 1)))

    def run_members():
        _lib.check(L.jq_traceobjgrad_members(h, ptr(pcof), nc, None, ptr(C), n, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)), h)

    def run_drifts():
        _lib.check(L.jq_traceobjgrad_drifts(h, ptr(pcof), nc, ptr(H), n, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)), h)

    def run_handles():
        for i, w in enumerate(handles):
            _lib.check(L.jq_traceobjgrad(w.handle, ptr(pcof), nc, 1, ptr(out4[i]), ptr(tg[i]), ptr(ig[i]), ptr(lg[i])), w.handle)

    run = dict(members=run_members, drifts=run_drifts, handles=run_handles)[kind]
    run()      # warm-up
    t = wa.last_timing()
    ready = dict(ready=True, family=t["kernel_family"], variant=t["kernel_variant"], version=L.jq_version().decode(),
                 checksum=float(np.sum(out4[:, 0])))
    if kind != "handles":
        ready["member_batch"] = wa.plan_info()["member_batch"]
    print(json.dumps(ready), flush=True)
    for _ in sys.stdin:
        t0 = time.perf_counter()
        run()
        print(json.dumps(dict(s=time.perf_counter() - t0)), flush=True)
    for w in handles or [wa]:
        w.close()


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_batch_ab.txt"))
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.worker[3])
        return 0
    if a.reps < 5:
        print("need at least five repetitions")
        return 2

    def start(case, nsteps, kind):
        cmd = ["timeout", "-k", "10", str(a.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", case, str(nsteps or 0),
               str(a.members), kind]
        p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = p.stdout.readline()
        return (p, json.loads(line)) if line.strip() else (p, None)

    def stop(p):
        try:
            p.stdin.close()
        except OSError:
            pass
        return p.wait()

    lines, version = [], ""
    for case, nsteps in SHAPES:
        procs, ready = [], []
        for kind in KINDS:
            p, r = start(case, nsteps, kind)
            procs.append(p)
            if r is None:
                print("%s: the %s worker ended with status %r: stopping" % (case, kind, [stop(q) for q in procs][-1]))
                return 1
            ready.append(r)
        version = ready[0]["version"]
        times, ok = [[] for _ in KINDS], True
        for _ in range(a.reps):      # alternate: members, drifts, handles, members ...
            for p, acc in zip(procs, times):
                p.stdin.write("go\n")
                p.stdin.flush()
                line = p.stdout.readline()
                if not line.strip():
                    ok = False
                    break
                acc.append(json.loads(line)["s"])
            if not ok:
                break
        st = [stop(p) for p in procs]
        if not ok or any(st):
            print("%s: a worker ended early (status %r): stopping" % (case, st))
            return 1
        ta, tb, tc = times
        info = ready[0]["member_batch"]
        line = ("%-7s %s x %d amplitude members  %-10s family %d, %3d per launch | (a) jq_traceobjgrad_members median %9.5f s (%.5f .. %.5f) | "
                "(b) jq_traceobjgrad_drifts (%s) median %9.5f s (%.5f .. %.5f) | (c) %d handles x jq_traceobjgrad (family %d, variant %d) median %9.5f s "
                "(%.5f .. %.5f) | a / b %5.3f | c / a %5.2f | sum of objfv (a) %.12e (c) %.12e"
                % (case, "%d steps" % nsteps if nsteps else "full length", a.members, info["mode"], ready[0]["family"], info["members_per_launch"],
                   med(ta), min(ta), max(ta), ready[1]["member_batch"]["mode"], med(tb), min(tb), max(tb), a.members, ready[2]["family"],
                   ready[2]["variant"], med(tc), min(tc), max(tc), med(ta) / med(tb), med(tc) / med(ta), ready[0]["checksum"], ready[2]["checksum"]))
        print(line, flush=True)
        lines.append(line)
    head = ["(a) jq_traceobjgrad_members with diagonal mixes, (b) jq_traceobjgrad_drifts with the same member count, (c) one handle per member x jq_traceobjgrad:",
            "one build, alternating in one job on one GPU (scripts/measure_member_batch.py; wall time with gradients, median and min .. max of %d" % a.reps,
            "repetitions each after one warm-up; (c)'s handles are created outside the timing)", "build: %s" % version, ""]
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
