"""GPU (-m gpu): long-lived handles.  Every other GPU test builds a handle, puts it in one state, evaluates and closes it; here ONE handle is
driven through a seeded sequence of setter actions and evaluator calls (tests/handle_sequence.py; tests/test_handle_sequence.py pins what
the generator promises), through the Python mirror, so sync_params is under test too.  Three criteria per step and no others:

  (a) oracle: the result agrees with the CPU oracle for the state the handle is in -- conftest.reference_pass (atol 1e-14 or rtol 1e-10),
      1e-11 absolute for histories, the criterion of tests/test_gpu_imr.py for the implicit-midpoint problems; sv_type 4 and the pair
      "type 2, type 3" through the constructions of tests/test_svtype_host.py; the batch, drift and member calls under sv_type != 1
      column by column against single calls on the replay handle;
  (b) replay: the result is bit-identical to the same call on a handle freshly created from the problem's initial parameters that got the
      setter actions of all steps so far (sync_params where the long-lived handle evaluated) and no earlier evaluation -- an evaluation
      leaves nothing behind, the state is the setters' alone;
  (c) refusal: a call the library refuses in the handle's state returns JQ_EUNSUPPORTED on both handles and writes nothing to its output
      arrays; the next step still meets (a) and (b).

After the last step both handles report the same plan.  Next to the sequences: a refused SETTER leaves the handle as it was."""
import numpy as np
import pytest

import handle_sequence as HS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", HS.IDS)
def test_sequence(jq, key):
    name, seed = key.rsplit("-", 1)
    families = HS.run_sequence(jq, name, int(seed))
    print("  kernel families:", sorted(families))
    if HS.SPECS[name].families == 2:      # two state layouts in one handle: single evaluations and the large ensemble
        assert len(families) >= 2, families


# ---- a refused setter leaves the handle as it was ---------------------------------------------------------------------------------------------
def _lib():
    from juqbox_jl_amd import _lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(_lib().c_dp)


def _update_wmat(m, hermitian):
    p = m.params
    rng = np.random.default_rng(31)
    A = rng.standard_normal((p.Ntot, p.Ntot))
    Wr = np.ascontiguousarray(A + A.T if hermitian else A + A.T + np.triu(np.ones((p.Ntot, p.Ntot)), 1))
    Wi = np.zeros_like(Wr)
    return _lib().load().jq_update_wmat(m.wa.handle, _ptr(Wr), _ptr(Wi))


def _sv2(m):
    HS.apply_setter(m, ("sv_type", "pair-2", 17))


REFUSED_SETTERS = {
    # name: (problem, preparation or None, the refused call -> its return code, expected code)
    "non-hermitian-wmat": ("rowlane12", None, lambda m: _update_wmat(m, False), "JQ_EUNSUPPORTED"),
    "wmat-under-implicit-midpoint": ("imr-rowlane", None, lambda m: _update_wmat(m, True), "JQ_EUNSUPPORTED"),
    "sv_type-2-under-implicit-midpoint": ("imr-rowlane", None, lambda m: _lib().load().jq_set_sv_type(m.wa.handle, 2), "JQ_EUNSUPPORTED"),
    "implicit-midpoint-under-sv_type-2": ("rowlane12", _sv2, lambda m: _lib().load().jq_set_integrator(m.wa.handle, 2, 60, 1e-11), "JQ_EUNSUPPORTED"),
    "sv_type-0": ("rowlane12", None, lambda m: _lib().load().jq_set_sv_type(m.wa.handle, 0), "JQ_EINVAL"),
    "sv_type-5": ("rowlane12", None, lambda m: _lib().load().jq_set_sv_type(m.wa.handle, 5), "JQ_EINVAL"),
    "unknown-option": ("rowlane12", None, lambda m: _lib().load().jq_set_option(m.wa.handle, b"no_such_option", 1), "JQ_EINVAL"),
    "wlr_sc-1": ("t4", None, lambda m: _lib().load().jq_set_option(m.wa.handle, b"wlr_sc", 1), "JQ_EUNSUPPORTED"),
    "debug-1": ("t4", None, lambda m: _lib().load().jq_set_option(m.wa.handle, b"debug", 1), "JQ_EUNSUPPORTED"),
    "multi_same_device-0": ("multi", None, lambda m: _lib().load().jq_set_option(m.wa.handle, b"multi_same_device", 0), "JQ_EINVAL"),
}
GETTERS = ("wlr_sc", "debug", "multi_same_device", "chunk_steps", "cq3")


def _reported(m):
    info = m.wa.plan_info()
    out = {k: info[k] for k in HS.PLAN_KEYS + ("integrator", "neumann_terms_or_max_iter", "chunk_steps")}
    out["jq_get_sv_type"] = _lib().load().jq_get_sv_type(m.wa.handle)
    out.update({"option " + o: m.wa.get_option(o) for o in GETTERS})
    return out


@pytest.mark.parametrize("case", sorted(REFUSED_SETTERS))
def test_a_refused_setter_leaves_the_handle_as_it_was(jq, case):
    name, prepare, call, code = REFUSED_SETTERS[case]
    m = HS.Model(jq, name).open()
    try:
        if prepare:
            prepare(m)
        before = HS.evaluate(m, "gradient", 0)
        assert "refused" not in before, before
        HS.check_oracle(m, "gradient", {"pcof": m.pcof}, before, case)
        reported = _reported(m)
        rc = call(m)
        assert rc == getattr(_lib(), code), (case, rc)
        assert _reported(m) == reported, (case, _reported(m), reported)
        HS.same_bits(case + ": the evaluation after the refusal", HS.evaluate(m, "gradient", 0), before)
    finally:
        m.close()
