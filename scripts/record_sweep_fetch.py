"""Records what the three-slab quad-layout kernels (k_forward / k_backward<6, 7, 3, ..., SC>) return for the cases of
tests/test_gpu_sweep_fetch.py: infidelity, leak and both gradients as float.hex() strings, one JSON file per case.

    python3 scripts/record_sweep_fetch.py [DIR]        (default: tests/golden/sweep_fetch; needs a GPU; library: JQ_LIB or the built one)

The committed files were written by the build of src:f27de3bb5068, BEFORE any change around the products of these kernels (the Horner
chain with its odd product in front of the pair loop, a lane's leak weights in registers, one wait per operand block:
profiles/sweep_fetch_ab.txt).  Such changes keep every floating-point operation, its operands and its order, so the kernels must
reproduce these files bit for bit.

Every case has 3 072 samples (one full round of the three-slab kernels): DISTINCT Gauss-Legendre nodes of the cnot3 detuning
ensemble, each repeated 3 072 / DISTINCT times with its weight divided likewise -- the CPU oracle evaluates the DISTINCT nodes
with the undivided weights (oracle_inputs) and the test holds the kernels to it at the reference's tolerance."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NS = 3072
DISTINCT = 8
# With cnot3's own step and golden control vector S = h/2 Hanti(t) is so small that every term of the Neumann series beyond the
# second is below rounding: results with m = 3 ... 7 are the same bits, and a product too few or too many would go unseen.  The
# cases take steps eight times as long with 300 times the control amplitudes: each further term up to the eighth then moves the
# infidelity by 1e-7 ... 1e-12 (CPU oracle), and the integration is still stable.
DT_FACTOR = 8
PCOF_SCALE = 300.0
# name: (Neumann terms m, time steps, chunk_steps or None)
#   m1 ... m7: the Horner chain with the final product alone (1), without pair loop (2, 3), with the odd product in front of the
#              pair loop (5, 7) and without it (6); 60 steps each
#   odd_chunk: one chunk with an odd number of steps, and an odd m
#   short_chunks: chunks of 3 steps and a remainder of 2 -- shorter than the five time points of the operator ring
#   two_controls: the third control dropped (Ncoupled = 2), m = 5
#   no_shift: unperturbed samples (use_shift == 0), m = 3
CASES = {
    "m1": (1, 60, None), "m2": (2, 60, None), "m3": (3, 60, None), "m5": (5, 60, None), "m6": (6, 60, None), "m7": (7, 60, None),
    "odd_chunk": (5, 151, None), "short_chunks": (6, 41, 3), "two_controls": (5, 60, None), "no_shift": (3, 60, None),
}


def build_case(jq, name):
    """(params, pcof, options, nodes, weights, shift) of a case"""
    m, nsteps, chunk = CASES[name]
    params, info = jq.cases.cnot3()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    params.T, params.nsteps = DT_FACTOR * params.T * nsteps / params.nsteps, nsteps
    pcof = PCOF_SCALE * pcof
    params.linear_solver.max_iter = m
    opts = {"chunk_steps": chunk} if chunk else None
    x, w, shift = jq.cases.cnot3_ensemble(DISTINCT)
    if name == "no_shift":
        x, shift = np.zeros(DISTINCT), np.zeros(params.Ntot)
    nodes, weights = np.tile(x, NS // DISTINCT), np.tile(w / (NS // DISTINCT), NS // DISTINCT)
    if name == "two_controls":           # (same B-spline count per control and frequency)
        params.Hsym_ops, params.Hanti_ops = params.Hsym_ops[:2], params.Hanti_ops[:2]
        params.Ncoupled, params.Cfreq = 2, np.asfortranarray(params.Cfreq[:2])
        pcof = pcof[:pcof.size * 2 // 3].copy()
    return params, pcof, opts, nodes, weights, shift


def oracle_inputs(jq, name):
    """(params, pcof, nodes, weights, shift) of the same ensemble with every distinct node once"""
    params, pcof, opts, nodes, weights, shift = build_case(jq, name)
    return params, pcof, nodes[:DISTINCT].copy(), weights[:DISTINCT] * (NS // DISTINCT), shift


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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sweep_fetch")
    os.makedirs(out, exist_ok=True)
    print("library:", _lib.load().jq_version().decode())
    for name in CASES:
        res, t, plan = run_case(jq, name)
        assert t["kernel_family"] == 6 and t["kernel_band"] == 7 and plan["s_uniform"] is True, (name, t, plan)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(res, f, indent=0)
            f.write("\n")
        print("%s: infidelity %s leak %s, %d + %d gradient entries" % (
            name, res["infidelity"], res["leak"], len(res["infidelity_grad"]), len(res["leak_grad"])))


if __name__ == "__main__":
    main()
