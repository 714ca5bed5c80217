"""CPU: what the quad route of jq_eval_f_g_grad_hvp adds outside the device -- the tangent-linear quad-layout kernels in the list of
instantiations (jq_inst_list.h) for the shipped block counts and no other, the list and the Makefile in agreement, the build manifest
(no scratch), and the route's name on every surface that documents the call.  The device side is tests/test_gpu_ens_hvp_quad.py."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "juqbox.jl_amd", "csrc")
KERNELS = ("k_forward_quad_tl", "k_backward_quad_tl")
SHIPPED = (2, 3, 4, 5, 6)      # NT; 7 and 8 need scratch in the backward kernel and stay on the sequential route


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _macro(text, name):
    """the replacement text of #define <name>(...) with its continuation lines joined"""
    m = re.search(r"^#define %s\([^)]*\)((?:.*\\\n)*.*)$" % re.escape(name), text, re.M)
    assert m, name
    return m.group(1).replace("\\\n", " ")


def test_the_instantiation_list_names_the_kernels_for_the_shipped_block_counts_only():
    text = _read("juqbox.jl_amd", "csrc", "jq_inst_list.h")
    inst = _macro(text, "JQ_INST_T_TL")
    for k in KERNELS:
        assert re.search(r"X\(%s, nt\)" % k, inst), (k, inst)
    assert len(re.findall(r"X\(", inst)) == len(KERNELS)
    sizes = [(int(a), int(b)) for a, b in re.findall(r"L\(A, (\d+), (\d+)\)", _macro(text, "JQ_SIZES_QUAD_TL"))]
    assert sizes == [(nt, 7) for nt in SHIPPED]
    # the t_ objects stand over the Makefile's QUAD list (NT 1 .. 6) and hold nothing but these kernels: t_1_7 is empty
    assert not _macro(text, "JQ_INST_T").strip()
    families = _macro(text, "JQ_OBJECT_FAMILIES")
    assert re.search(r"Y\(t, JQ_SIZES_QUAD, JQ_INST_T\) Y\(t, JQ_SIZES_QUAD_TL, JQ_INST_T_TL\)", families), families
    assert len(re.findall(r"Y\(t,", families)) == 2 and len(re.findall(r"JQ_INST_T_TL", families)) == 1
    # ... and the variant of the one instantiation file that applies the list, for the sizes of the list only
    unit = _read("juqbox.jl_amd", "csrc", "jq_kernel_inst.hip")
    assert '#include "jq_quad_tl_kernels.h"' in unit and re.search(r"#if JQ_NT >= 2 .*\nJQ_INST_T_TL\(JQ_DEF, JQ_NT, JQ_BW\)\n#endif", unit)
    # the host declares the templates it does not include and routes by the layout record
    assert "k_backward_quad_tl" in _read("juqbox.jl_amd", "csrc", "jq_host_select.h")
    host = _read("juqbox.jl_amd", "csrc", "jq_host_ens_hvp.h")
    assert "ens_hvp_layout_quad" in host and "h->quad_max_slabs > 0" in host and "h->BW == JQ_BW_T4" in host


def test_the_list_and_the_makefile_agree():
    mk = _read("juqbox.jl_amd", "csrc", "Makefile")
    tags = re.search(r"^QUAD = (.*)$", mk, re.M).group(1).split()
    assert tags == ["1_7"] + ["%d_7" % nt for nt in SHIPPED]
    assert "$(QUAD:%=$(OBJDIR)/t_%.o)" in re.search(r"^KOBJS = (.*)$", mk, re.M).group(1)
    rule = re.search(r"^\$\(OBJDIR\)/t_%\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "jq_quad_tl_kernels.h" in rule.group(1) and "-DJQ_VARIANT=14" in rule.group(2) and "KCC" in rule.group(2)


def test_the_build_manifest_shows_the_kernels_without_scratch():
    path = os.path.join(CSRC, "build", "manifest.json")
    if not os.path.exists(path):
        pytest.skip("no build directory here (the library was built elsewhere)")
    man = json.load(open(path))["objects"]
    for nt in SHIPPED:
        kernels = {k["name"]: k for k in man["t_%d_7" % nt]["kernels"]}
        assert len(kernels) == len(KERNELS), sorted(kernels)
        for name in KERNELS:
            hits = [k for n, k in kernels.items() if "%sILi%dEE" % (name, nt) in n]
            assert len(hits) == 1, (name, nt, sorted(kernels))
            print("t_%d_7 %s: %d VGPRs, %d AGPRs, scratch %d bytes" % (nt, name, hits[0]["vgprs"], hits[0]["agprs"], hits[0]["scratch_bytes"]))
            assert hits[0]["scratch_bytes"] == 0 and hits[0]["vgpr_spills"] == 0, hits[0]
    assert not man["t_1_7"]["kernels"]      # (NT = 1 is Ntot <= 16: the lane and row-lane routes)
    assert not [t for t in man if t.startswith("t_") and t not in ["t_%d_7" % nt for nt in (1,) + SHIPPED]]
    assert not [t for t, e in man.items() if not t.startswith("t_") and any("quad_tl" in k["name"] for k in e["kernels"])]


def test_the_route_is_named_where_the_call_is_documented():
    header = _read("include", "juqbox_hip.h")
    i = header.index("int jq_eval_f_g_grad_hvp(")
    comment = header[header.rindex("/*", 0, i):i]
    assert "Quad route" in comment and '"quad"' in comment and "4 x 4 x n" in comment
    assert '"quad"' in _read("juqbox.jl_amd", "csrc", "jq_host_info.h")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert '"quad"' in _read(doc), doc
    design = _read("DESIGN.md")
    assert "k_backward_quad_tl" in design and "jq_quad_tl_kernels.h" in design and "*Quad route*" in design
    not_built = design[design.index("Hessian-vector products of the risk-neutral ensemble (`jq_eval_f_g_grad_hvp`; `eval_f_g_grad_hvp`"):]
    not_built = not_built[not_built.index("Not built:"):not_built.index("\n\n")]
    assert "the structured\nfamilies" not in not_built and "NT = 7" in not_built, not_built
    py = _read("juqbox.jl_amd", "ipopt_interface.py")
    for fn in ("eval_f_g_grad_hvp", "eval_hessvec_par", "setup_ipopt_problem"):
        j = py.index("def %s(" % fn)
        doc = py[j:py.index('"""', py.index('"""', j) + 3)]
        assert "quad" in doc, fn
    assert '"quad"' in _read("julia", "hip_backend.jl").split("function eval_f_g_grad_hvp")[0][-1200:]
    assert "ens_hvp_quad_timing.txt" in _read("profiles", "README.md")
