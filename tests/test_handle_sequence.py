"""CPU: what the generator of tests/handle_sequence.py promises the GPU test (tests/test_gpu_handle_sequence.py), checked with the
generator and the CPU oracle alone.

* Coverage: over all sequences together every setter kind is directly followed by every evaluator kind in a step that is SERVED, every
  form of every setter occurs, every refusal rule the ten problems can reach occurs (the uncoupled gradient under implicit midpoint has no
  problem in the table), no sequence holds more than MAX_REFUSED refused steps, and the sequences of "twin" and "multi" hold every setter
  form that exists for them.  Each problem meets the needs the generator dealt to it (handle_sequence.needs).
* Discrimination: for every setter action other than the options the oracle's objective and total gradient after the action differ from
  those before it by more than 1e-6 relative -- a setter that never reached the device cannot meet the oracle criterion.  The type
  setters leave the objective alone by construction (it is taken against the target in every type): the gradient alone is held to the
  figure there, types 2 / 3 through the pair's sum (tests/test_svtype_host.py).  The drift ensemble that re-plans the handle changes the
  plan and nothing the oracle sees: it is drawn under sv_type 1 only, where the GPU test holds its columns to the oracle, and to the replay handle.
* Determinism: building the sequences twice gives equal lists."""
import numpy as np
import pytest

import handle_sequence as HS


@pytest.fixture(scope="module")
def sequences(jq):
    return HS.all_sequences(jq)


def test_every_problem_has_its_sequences(sequences):
    assert list(sequences) == [(n, s) for n in HS.SPECS for s in HS.SEEDS_PER_PROBLEM] and len(sequences) == 20
    for steps in sequences.values():
        assert len(steps) == HS.STEPS
        for st in steps:
            assert len(st["setters"]) <= 2 and st["evaluator"] in HS.EVALUATORS


def test_coverage(jq, sequences):
    """a pair counts only where the evaluator is SERVED (a refused call says nothing about the state its setter left); the refusals are
    counted through their rules"""
    pairs, forms, rules = set(), set(), set()
    per_problem = {n: {"pairs": set(), "rules": set(), "forms": set()} for n in HS.SPECS}
    for (name, seed), steps in sequences.items():
        refused = [st["refused"] for st in steps if st["refused"]]
        assert len(refused) <= HS.MAX_REFUSED, (name, seed, refused)
        mine = per_problem[name]
        mine["rules"].update(refused)
        for st in steps:
            mine["forms"].update(a[:2] for a in st["setters"])
            if st["setters"] and not st["refused"]:
                mine["pairs"].add((st["setters"][-1][0], st["evaluator"]))
            if HS.SPECS[name].imr and any(a[0] == "weights" and a[1].startswith("full") for a in st["setters"]):
                mine["rules"].add("imr-full-weights")
    for name, mine in per_problem.items():      # what the generator dealt to each problem
        need = HS.needs(jq, name)
        for k in need:
            assert need[k] <= mine[k], (name, k, sorted(need[k] - mine[k]))
        pairs |= mine["pairs"]
        forms |= mine["forms"]
        rules |= mine["rules"]
    missing = {(k, e) for k in HS.SETTER_KINDS for e in HS.EVALUATORS} - pairs
    assert not missing, sorted(missing)
    assert rules == set(HS.REACHABLE_RULES), set(HS.REACHABLE_RULES) ^ rules
    want = {("drift", f) for f in ("diagonal", "pattern", "outside", "original", "ensemble-outside")} | {("target", "new")} | \
        {("sv_type", f) for f in ("1", "4", "pair-2", "pair-3")} | \
        {("weights", f) for f in ("diagonal", "full-real-2", "full-complex-3", "full-20", "back-to-diagonal")} | \
        {("solver", f) for f in ("neumann-0", "neumann-1", "neumann-3", "neumann-4", "jacobi")} | \
        {("options", "%s=%s" % (o, v)) for o, off in (("chunk_steps", 3), ("cq3", 0), ("t4", 0), ("quad", 0), ("lane", 0), ("dq", 0)) for v in (off, "unset")}
    assert want <= forms, sorted(want - forms)
    # every setter must reach the embedded twin and go through multi_forall: every kind and every form that exists for the problem
    for name in HS.EVERY_FORM:
        have = per_problem[name]["forms"]
        assert {k for k, _ in have} == set(HS.SETTER_KINDS), (name, have)
        named = {("weights", f) for f in ("diagonal", "full-real-2", "full-complex-3", "back-to-diagonal")} | \
            {("solver", f) for f in ("neumann-0", "neumann-1", "neumann-3", "neumann-4", "jacobi")} | \
            {("drift", f) for f in ("diagonal", "pattern", "outside", "original")}
        assert named <= have, (name, sorted(named - have))
    assert ("weights", "full-20") in per_problem["multi"]["forms"]


def test_every_pair_and_rule_is_dealt_to_a_problem(jq):
    dealt = [HS.needs(jq, n) for n in HS.SPECS]
    assert set().union(*[d["pairs"] for d in dealt]) == {(k, e) for k in HS.SETTER_KINDS for e in HS.EVALUATORS}
    assert set().union(*[d["rules"] for d in dealt]) == set(HS.REACHABLE_RULES)


def test_the_predicate_names_every_rule(jq):
    """refusal() in the states the rules are about (the one rule no problem of the table reaches included)"""
    m = HS.Model(jq, "imr-t4")
    assert HS.refusal(m, "gradient") is None and HS.refusal(m, "hvp") == "tl-imr" and HS.refusal(m, "jvp") == "tl-imr"
    m.params.sv_type = 4
    assert HS.refusal(m, "forward") == "imr-sv_type"
    m.params.sv_type = 1
    m.spec = m.spec._replace(uncoupled=True)
    assert HS.refusal(m, "gradient") == "imr-uncoupled-gradient" and HS.refusal(m, "forward") is None and HS.refusal(m, "history") is None
    m = HS.Model(jq, "uncoupled")
    assert HS.refusal(m, "jvp") is None and HS.refusal(m, "hvp") == "tl-uncoupled" and HS.refusal(m, "gradient") is None
    m.params.sv_type = 2
    assert HS.refusal(m, "jvp") is None and HS.refusal(m, "ens_hvp") == "tl-sv_type" and HS.refusal(m, "drifts") is None
    HS.apply_setter(m, ("weights", "full-real-2", 5))
    assert HS.refusal(m, "jvp") == "tl-full-weights"
    HS.apply_setter(m, ("solver", "jacobi", 5))
    assert HS.refusal(m, "drifts_hvp") == "tl-jacobi" and HS.refusal(m, "ens13") is None


def _relative(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("key", HS.IDS)
def test_discrimination(jq, sequences, key):
    name, seed = key.rsplit("-", 1)
    steps = sequences[(name, int(seed))]
    m = HS.Model(jq, name)
    for i, st in enumerate(steps):
        for a in st["setters"]:
            if a[0] == "options" or a[1] == "ensemble-outside" or (m.spec.imr and a[0] == "weights" and a[1].startswith("full")):
                HS.apply_setter(m, a)
                continue
            if m.spec.imr and a[0] == "sv_type":      # refused by the library: nothing to tell apart
                HS.apply_setter(m, a)
                continue
            f0, g0 = HS.oracle_state(m)
            HS.apply_setter(m, a)
            f1, g1 = HS.oracle_state(m)
            df, dg = _relative(f1, f0), _relative(g1, g0)
            print("%s step %d %-28s objective %.2e gradient %.2e" % (key, i, a[:2], df, dg))
            assert dg > HS.DISCRIMINATION, (key, i, a, dg)
            if a[0] != "sv_type":
                assert df > HS.DISCRIMINATION, (key, i, a, df)
        HS.after_refusal(m, st["refused"])


def test_determinism(jq, sequences):
    again = HS.all_sequences(jq, fresh=True)
    assert again == sequences
    # a sequence is a function of (problem name, seed): built on its own it is what it is in the table
    assert HS.sequence(jq, "t4", 1, fresh=True) == sequences[("t4", 1)] and HS.sequence(jq, "twin", 0, fresh=True) == sequences[("twin", 0)]
