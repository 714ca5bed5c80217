"""CPU: which instantiation a batch runs is data.  csrc/jq_inst_list.h names every instantiation of the propagator kernels once;
build/dump_selection (csrc/jq_dump_selection.h: the host code with a main(), no HIP call) calls every select_* function of
csrc/jq_host_select.h with every combination of its inputs and prints the object, the instantiation and the KernelSel record it picks.
Its output must equal profiles/selection_table.txt, which was recorded from the select_* functions of the commit BEFORE the list existed
(profiles/README.md) -- a change of the selection is a diff of that file.  Plus the completeness checks of the list:
  (a) its size lists and csrc/Makefile name the same objects;
  (b) jq_kernel_inst.hip and jq_host_select.h spell no instantiation of their own;
  (c) the host translation unit instantiates no propagator kernel: one that the list does not declare would be compiled into host.o with
      host.o's flags -- no register form, no scheduler option, outside the build manifest -- while "last_kernels" names an object."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "juqbox.jl_amd", "csrc")
DUMP = os.path.join(CSRC, "build", "dump_selection")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def dump(*args):
    assert os.path.exists(DUMP), "csrc/build/dump_selection is missing: `make` in juqbox.jl_amd/csrc builds it with the library"
    r = subprocess.run([DUMP, *args], capture_output=True, text=True)
    assert r.returncode == 0, "dump_selection exited with %d: %s" % (r.returncode, r.stderr)
    return r.stdout.splitlines()


def test_selection_equals_the_recorded_table():
    got = dump()
    want = open(os.path.join(ROOT, "profiles", "selection_table.txt")).read().splitlines()
    assert not [ln for ln in got if "UNLISTED" in ln]
    assert len(got) > 1000 and len({ln.split()[0] for ln in got if not ln.startswith("#")}) == 13      # (thirteen select_* functions)
    for n, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, "line %d differs from profiles/selection_table.txt" % n
    assert len(got) == len(want)


def makefile_objects():
    """the tags of KOBJS, from the size lists and the loose objects of csrc/Makefile"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+) = (.*)$", text, re.M)}
    lists = {name: var[name].split() for name in ("INST", "QUAD", "QUADBIG", "BIG", "LANE", "ROWLANE")}
    m = re.fullmatch(r"\$\(filter-out ([\d_ ]+),\$\(INST\)\)", var["COOP"].strip())
    assert m, var["COOP"]
    lists["COOP"] = [x for x in lists["INST"] if x not in m.group(1).split()]
    tags, rest = set(), var["KOBJS"]
    for name, prefix in re.findall(r"\$\((\w+):%=\$\(OBJDIR\)/(\w)_%\.o\)", rest):
        tags |= {"%s_%s" % (prefix, size) for size in lists[name]}
    rest = re.sub(r"\$\(\w+:%=\$\(OBJDIR\)/\w_%\.o\)", "", rest)
    loose = set(re.findall(r"\$\(OBJDIR\)/(\w+)\.o", rest))
    assert loose == {"w_1_0", "w_6_5", "x_1_0", "x_6_5", "u_7_7", "v_7_7", "i_1_0"} and not re.sub(r"\$\(OBJDIR\)/\w+\.o", "", rest).strip()
    return tags | loose


def test_the_size_lists_and_the_makefile_name_the_same_objects():
    listed, built = set(dump("--objects")), makefile_objects()
    assert len(built) > 230
    for letter in sorted({t[0] for t in listed | built}):
        a, b = {t for t in listed if t[0] == letter}, {t for t in built if t[0] == letter}
        assert a == b, "%s_ objects: jq_inst_list.h only %s, csrc/Makefile only %s" % (letter, sorted(a - b), sorted(b - a))


def test_no_instantiation_is_spelled_outside_the_list():
    for f in ("jq_kernel_inst.hip", "jq_host_select.h"):
        stray = [ln for ln in open(os.path.join(CSRC, f)) if re.search(r"\btemplate\s+__global__", ln) and not ln.startswith("#define JQ_")]
        assert not stray, "%s: %s" % (f, stray)
        assert len(re.findall(r"^#define JQ_\w+\(name, \.\.\.\) (?:extern )?template __global__ void name<__VA_ARGS__>", open(os.path.join(CSRC, f)).read(), re.M)) == 1


def test_the_host_object_holds_no_propagator_kernel_of_its_own():
    host = os.path.join(CSRC, "build", "host.o")
    assert os.path.exists(host)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, host, os.path.join(tmp, "unused.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", co], check=True, capture_output=True, text=True).stdout
    kernels = set()      # (a kernel has a descriptor <symbol>.kd; _Z<n><name>...: the name of a mangled symbol)
    for sym in re.findall(r"(\S+)\.kd$", syms, re.M):
        m = re.match(r"_Z(\d+)", sym)
        kernels.add(sym[m.end():m.end() + int(m.group(1))] if m else sym)
    assert {"k_stream", "k_gradacc", "k_forward_huge"} <= kernels, sorted(kernels)
    text = open(os.path.join(CSRC, "jq_inst_list.h")).read().replace("\\\n", " ")
    allowed = set(re.findall(r"X\((\w+)", re.search(r"^#define JQ_INST_HOST\(X\)(.*)$", text, re.M).group(1))) | {"k_forward_huge", "k_backward_huge"}
    prop = {k for k in kernels if re.match(r"k_(forward|backward)", k)}
    assert prop <= allowed, "propagator kernels instantiated into host.o: %s" % sorted(prop - allowed)
