"""Records what the three-slab quad-layout kernels (k_forward / k_backward<6, 7, 3, ...>) return for the cases of
tests/test_gpu_step_trim.py: infidelity, leak and both gradients as float.hex() strings, one JSON file per case.

    python3 scripts/record_step_trim.py [DIR]          (default: tests/golden/step_trim; needs a GPU; library: JQ_LIB or the built one)

The committed files were written by the build BEFORE the per-step trims (LKC, CWH, PK in csrc/jq_kernels.h): the trims keep every
floating-point operation, its operands and its order, so the kernels must reproduce these files bit for bit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NS = 3072
CASES = ("a_300_perturbed", "b_23_chunk7", "c_300_unperturbed", "d_two_controls", "e_nonuniform_s")


def build_case(jq, name):
    """(params, pcof, options, nodes, weights, shift) of a case"""
    params, info = jq.cases.cnot3()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    nsteps = 23 if name == "b_23_chunk7" else 300
    params.T, params.nsteps = params.T * nsteps / params.nsteps, nsteps
    opts = {"chunk_steps": 7} if name == "b_23_chunk7" else None
    nodes, weights, shift = jq.cases.cnot3_ensemble(NS)
    if name == "c_300_unperturbed":      # the use_shift == 0 path
        nodes, weights, shift = np.zeros(NS), np.full(NS, 1.0 / NS), np.zeros(params.Ntot)
    if name == "d_two_controls":         # the third control dropped: Ncoupled = 2 (same B-spline count per control and frequency)
        params.Hsym_ops, params.Hanti_ops = params.Hsym_ops[:2], params.Hanti_ops[:2]
        params.Ncoupled, params.Cfreq = 2, np.asfortranarray(params.Cfreq[:2])
        pcof = pcof[:pcof.size * 2 // 3].copy()
    if name == "e_nonuniform_s":         # one Hanti entry x 1.01 (tests/test_gpu_s_compact.py): the kernels with the full S operand
        H = params.Hanti_ops[0]
        H[21, 20] *= 1.01
        H[20, 21] = -H[21, 20]
    return params, pcof, opts, nodes, weights, shift


def run_case(jq, name):
    params, pcof, opts, nodes, weights, shift = build_case(jq, name)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    plan = wa.plan_info()
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    t = wa.last_timing()
    wa.close()
    res = {"infidelity": float(params.last_infidelity).hex(), "leak": float(params.last_leak).hex(),
           "infidelity_grad": [float(x).hex() for x in np.asarray(params.last_infidelity_grad).ravel()],
           "leak_grad": [float(x).hex() for x in np.asarray(params.last_leak_grad).ravel()]}
    return res, t, plan


def main():
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_trim")
    os.makedirs(out, exist_ok=True)
    print("library:", _lib.load().jq_version().decode())
    for name in CASES:
        res, t, plan = run_case(jq, name)
        assert t["kernel_family"] == 6 and t["kernel_band"] == 7, (name, t)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(res, f, indent=0)
            f.write("\n")
        print("%s: s_uniform %s, infidelity %s leak %s, %d + %d gradient entries" % (
            name, plan.get("s_uniform"), res["infidelity"], res["leak"], len(res["infidelity_grad"]), len(res["leak_grad"])))


if __name__ == "__main__":
    main()
