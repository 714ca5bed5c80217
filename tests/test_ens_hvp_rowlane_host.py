"""CPU: what the row-lane route of jq_eval_f_g_grad_hvp adds outside the device -- the tangent-linear row-lane kernels in the list of
instantiations (jq_inst_list.h) and in the build manifest (no scratch), and the route's name on every surface that documents the call.
The device side is tests/test_gpu_ens_hvp_rowlane.py."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "juqbox.jl_amd", "csrc")
KERNELS = ("k_forward_rowlane_tl", "k_backward_rowlane_tl")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _macro(text, name):
    """the replacement text of #define <name>(...) with its continuation lines joined"""
    m = re.search(r"^#define %s\([^)]*\)((?:.*\\\n)*.*)$" % re.escape(name), text, re.M)
    assert m, name
    return m.group(1).replace("\\\n", " ")


def test_the_instantiation_list_names_the_kernels_under_the_r_family():
    text = _read("juqbox.jl_amd", "csrc", "jq_inst_list.h")
    inst = _macro(text, "JQ_INST_R_TL")
    for k in KERNELS:
        assert re.search(r"X\(%s, np\)" % k, inst), (k, inst)
    sizes = [int(x) for x in re.findall(r"L\(A, (\d+)\)", _macro(text, "JQ_SIZES_ROWLANE_TL"))]
    assert sizes == [12, 16]
    families = _macro(text, "JQ_OBJECT_FAMILIES")
    assert re.search(r"Y\(r, JQ_SIZES_ROWLANE_TL, JQ_INST_R_TL\)", families), families
    # ... and the r_ variant of the one instantiation file applies the list, for the sizes of the list only
    unit = _read("juqbox.jl_amd", "csrc", "jq_kernel_inst.hip")
    assert '#include "jq_rowlane_tl_kernels.h"' in unit and "JQ_INST_R_TL(JQ_DEF, JQ_NT)" in unit
    rule = re.search(r"^\$\(OBJDIR\)/r_%\.o:(.*)$", _read("juqbox.jl_amd", "csrc", "Makefile"), re.M).group(1)
    assert "jq_rowlane_tl_kernels.h" in rule and "check_dpp_hazard.py" in rule


def test_the_build_manifest_shows_the_kernels_without_scratch():
    path = os.path.join(CSRC, "build", "manifest.json")
    if not os.path.exists(path):
        pytest.skip("no build directory here (the library was built elsewhere)")
    man = json.load(open(path))["objects"]
    for npj in (12, 16):
        kernels = {k["name"]: k for k in man["r_%d" % npj]["kernels"]}
        for name in KERNELS:
            hits = [k for n, k in kernels.items() if "%sILi%dEE" % (name, npj) in n]
            assert len(hits) == 1, (name, npj, sorted(kernels))
            print("r_%d %s: %d VGPRs, %d AGPRs, scratch %d bytes" % (npj, name, hits[0]["vgprs"], hits[0]["agprs"], hits[0]["scratch_bytes"]))
            assert hits[0]["scratch_bytes"] == 0 and hits[0]["vgpr_spills"] == 0, hits[0]
    for npj in (2, 4, 6, 8):      # no tangent kernels below NPJ 12: Ntot <= 6 has the lane kernels' twins, Ntot 7 and 8 stay sequential
        assert not [k for k in man["r_%d" % npj]["kernels"] if "rowlane_tl" in k["name"]]


def test_the_route_is_named_where_the_call_is_documented():
    header = _read("include", "juqbox_hip.h")
    i = header.index("int jq_eval_f_g_grad_hvp(")
    comment = header[header.rindex("/*", 0, i):i]
    assert "Row-lane route" in comment and '"rowlane"' in comment and "Ntot 9 .. 16" in comment
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "rowlane" in text and re.search(r"Ntot 9 … 16", text), doc
    design = _read("DESIGN.md")
    not_built = design[design.index("Hessian-vector products of the risk-neutral ensemble (`jq_eval_f_g_grad_hvp`; `eval_f_g_grad_hvp`"):]
    not_built = not_built[not_built.index("Not built:"):not_built.index("\n\n")]
    assert "row-lane family" not in not_built and "NP = 8" in not_built, not_built
    assert "k_backward_rowlane_tl" in design and "jq_rowlane_tl_kernels.h" in design
    py = _read("juqbox.jl_amd", "ipopt_interface.py")
    for fn in ("eval_f_g_grad_hvp", "eval_hessvec_par", "setup_ipopt_problem"):
        j = py.index("def %s(" % fn)
        doc = py[j:py.index('"""', py.index('"""', j) + 3)]
        assert "row-lane" in doc, fn
    assert "row-lane" in _read("julia", "hip_backend.jl").split("function eval_f_g_grad_hvp")[0][-900:]
    assert "ens_hvp_rowlane_timing.txt" in _read("profiles", "README.md")
