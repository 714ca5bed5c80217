"""Long-lived handles: seeded sequences of setter actions and evaluator calls (tests/test_handle_sequence.py on the CPU,
tests/test_gpu_handle_sequence.py on the GPU).

A sequence belongs to a problem and a seed and is a list of STEPS steps; a step is zero to two setter actions followed by one evaluator
call.  Everything goes through the Python mirror: a setter mutates `params` (or calls wa.set_option), the evaluator's sync_params pushes
it.  An action is a tuple (kind, form, seed) -- its data are drawn from default_rng(seed) when it is applied, so a sequence is a plain
list of tuples and a pure function of (problem name, seed).

The generator works on the CPU with the problem's params alone (no handle): it applies the setters to them as it goes, asks refusal() --
the refusal rules of tl_refuse (jq_host_tl.h) and plan_batch (jq_host_plan.h) restated -- what the library will say to the evaluator,
and fills what needs() deals to the problem -- its share of the (setter kind, evaluator kind) pairs, each in a step that is SERVED, its
refusal rules, for "twin" and "multi" every setter form -- greedily over the problem's seeds in their
fixed order.  The runner (run_sequence) drives a handle through a sequence and holds every step to three criteria: (a) the CPU oracle
for the state the handle is in, (b) the bits of the same call on a replay handle that got the setter actions only, (c) refusals."""
import collections
import copy
import time
import zlib

import numpy as np

from conftest import reference_pass

STEPS = 12
MAX_REFUSED = 4
DISCRIMINATION = 1e-6      # tests/test_gpu_ens_hvp_quad.py: "a dropped shift cannot pass"
SEEDS_PER_PROBLEM = (0, 1)
# the large ensemble: samples x Ntot^2 x N x steps at most (the CPU oracle takes about 70 ns per unit and up to four passes per call; beyond
# this the oracle of that one call takes longer than the rest of the sequence: "parts", whose next family starts at 129 samples of 20 columns)
LARGE_MAX = 25e6

# ---- the problems ---------------------------------------------------------------------------------------------------------------------
# plan_opt: the plan-shaping option the "options" setter switches off and on again; t4: the problem has the 4 x 4 x n structure (the (1, 7)
# entry leaves it; the others take a dense symmetric perturbation as the drift outside the plan); families: kernel families a sequence of
# the problem must have run on at least (jq_last_timing)
Spec = collections.namedtuple("Spec", "name base imr uncoupled devices options plan_opt t4 families")
SPECS = collections.OrderedDict((s.name, s) for s in (
    Spec("lanes", "lanes", False, False, None, {}, "lane", False, 2),
    Spec("rowlane12", "rowlane12", False, False, None, {}, "lane", False, 1),
    Spec("t4", "t4", False, False, None, {}, "t4", True, 2),
    Spec("twin", "twin", False, False, None, {"embed": 2}, "quad", False, 1),
    Spec("dense29", "dense29", False, False, None, {}, "dq", False, 2),
    Spec("parts", "parts", False, False, None, {}, "t4", False, 1),
    Spec("uncoupled", "t4", False, True, None, {}, "t4", True, 1),
    Spec("multi", "t4", False, False, 2, {"multi_same_device": 1}, "t4", True, 1),
    Spec("imr-rowlane", "rowlane12", True, False, None, {}, "t4", False, 1),
    Spec("imr-t4", "t4", True, False, None, {}, "t4", True, 1),
))
# (problem, seed) whose default generator seed left one of the problem's needs (needs(): a pair, a rule, a form) open, or gave a setter
# action below DISCRIMINATION on the oracle: the generator seed used instead
SEEDS = {("twin", 0): 100, ("twin", 1): 301, ("multi", 0): 100, ("multi", 1): 501}

SETTER_KINDS = ("drift", "target", "sv_type", "weights", "solver", "options")
EVALUATORS = ("forward", "gradient", "history", "ens1", "ens3", "ens13", "ens_large", "batch", "ens_batch", "drifts", "members",
              "jvp", "hvp", "ens_hvp", "drifts_hvp")
TANGENT_LINEAR = ("jvp", "hvp", "ens_hvp", "drifts_hvp")
RULES = ("tl-imr", "tl-jacobi", "tl-full-weights", "tl-sv_type", "tl-uncoupled", "imr-sv_type", "imr-full-weights", "imr-uncoupled-gradient")
# rules the ten problems can reach (there is no uncoupled implicit-midpoint problem among them: tests/test_gpu_uncoupled.py provokes that
# refusal on every implicit-midpoint cell of its matrix)
REACHABLE_RULES = RULES[:-1]


def _base_problem(jq, base):
    from block_band_problem import block_band_problem
    from kronecker_problem import random_kronecker_problem
    from subsystem_problem import subsystem_problem
    from test_gpu_random import random_problem
    if base == "lanes":
        return random_problem(jq, np.random.default_rng(9101), 6, 2, 2, 2, 9, 3, 2, False)
    if base == "rowlane12":
        return random_problem(jq, np.random.default_rng(9102), 10, 3, 2, 2, 9, 3, 2, False)
    if base == "t4":
        return subsystem_problem(jq, np.random.default_rng(9103), 2, 29, 4, 3, 3, "varied", 11, 2)
    if base == "twin":
        return random_kronecker_problem(jq, (3, 3, 2), 4)[:2]
    if base == "dense29":
        return random_problem(jq, np.random.default_rng(9105), 29, 4, 2, 2, 9, 3, 2, False)
    if base == "parts":
        return block_band_problem(jq, np.random.default_rng(9106), 45, 20, 1, (1, 1), 9, 3, 2)
    raise KeyError(base)


class Model:
    """One problem in its current state: the live params a handle mirrors, and what the generator needs to know about the handle"""

    def __init__(self, jq, name):
        self.jq, self.spec = jq, SPECS[name]
        s = self.spec
        p, pcof = _base_problem(jq, s.base)
        if s.uncoupled:
            from uncoupled_problem import to_uncoupled
            p = to_uncoupled(jq, p, "sas", np.random.default_rng(9107))
        if s.imr:
            import block_band_matrix as B
            p = B.with_solver(jq, p, "imr")
        self.params, self.pcof = p, np.array(pcof, dtype=np.float64)
        self.H0 = np.array(p.Hconst, dtype=np.float64)
        self.wimag0 = copy.copy(p.wmat_imag)
        self.opts = dict(s.options)
        self.drift = "original"      # the form of the last drift action
        self.wa = None

    # -- what the refusal rules and the generator's eligibility tests read
    @property
    def sv_type(self):
        return int(self.params.sv_type)

    @property
    def full_weights(self):
        return np.ndim(self.params.wmat_real) == 2

    @property
    def jacobi(self):
        return self.params.linear_solver.solver_id == self.jq.JACOBI_SOLVER

    def open(self):
        jq, s = self.jq, self.spec
        make = jq.Working_Arrays_M_HIP if s.imr else jq.Working_Arrays_HIP
        self.wa = make(self.params, self.pcof.size, devices=s.devices, options=dict(s.options))
        return self

    def close(self):
        if self.wa is not None:
            self.wa.close()
            self.wa = None


# ---- the refusal rules ------------------------------------------------------------------------------------------------------------------
def refusal(model, evaluator):
    """None, or the rule by which the library refuses this evaluator in the handle's state (every rule answers JQ_EUNSUPPORTED).
    tl_refuse (jq_host_tl.h) in its order: integrator, solver, full weights, then -- the calls with an adjoint sweep -- sv_type and
    uncoupled controls; plan_batch (jq_host_plan.h): an uncoupled gradient, sv_type != 1 and full weights under implicit midpoint.
    Through the mirror sv_type != 1 under implicit midpoint is refused earlier, by jq_set_sv_type in sync_params, for every evaluator."""
    s = model.spec
    gradient = evaluator not in ("forward", "history", "jvp")
    if s.imr:
        if model.sv_type != 1:
            return "imr-sv_type"
        if evaluator in TANGENT_LINEAR:
            return "tl-imr"
        if s.uncoupled and gradient:
            return "imr-uncoupled-gradient"
        return None
    if evaluator in TANGENT_LINEAR:
        if model.jacobi:
            return "tl-jacobi"
        if model.full_weights:
            return "tl-full-weights"
        if evaluator != "jvp" and model.sv_type != 1:
            return "tl-sv_type"
        if evaluator != "jvp" and s.uncoupled:
            return "tl-uncoupled"
    return None


# ---- setter actions -----------------------------------------------------------------------------------------------------------------------
def _outside(model, rng_seed):
    """a drift outside the planned structure: the (1, 7) construction of tests/test_gpu_drift_batch.py for 4 x 4 x n, a dense symmetric
    perturbation elsewhere"""
    from test_gpu_drift_batch import dense_members, pattern_members
    if not model.spec.t4:
        return dense_members(model.H0, 1, rng_seed)[0]
    M = pattern_members(model.H0, 1, rng_seed)[0]
    assert M[1, 7] == 0.0
    M[1, 7] = M[7, 1] = 1e-2 * float(np.max(np.abs(model.H0)))
    return M


def setter_forms(model, step):
    """the (kind, form) pairs that change the state the model is in (an action that changes nothing could not be told from a lost one)"""
    s, p = model.spec, model.params
    forms = [("drift", "diagonal"), ("drift", "pattern"), ("drift", "outside"), ("target", "new")]
    if not np.array_equal(np.asarray(p.Hconst), model.H0):
        forms.append(("drift", "original"))
    if s.t4 and not s.imr and not s.devices and model.sv_type == 1:      # (sv_type 1: its columns are held to the oracle)
        forms.append(("drift", "ensemble-outside"))
    if model.sv_type != 1:
        forms.append(("sv_type", "1"))
    forms.append(("sv_type", "4"))      # (implicit midpoint: the evaluator is refused and the type put back)
    if not s.imr and step + 2 <= STEPS - 1:
        forms.append(("sv_type", "pair"))
    forms.append(("weights", "diagonal"))
    forms += [("weights", "full-real-2"), ("weights", "full-complex-3")]      # (implicit midpoint: jq_update_wmat itself, refused)
    if not s.imr:
        if p.Ntot >= 29:
            forms.append(("weights", "full-20"))
        if model.full_weights:
            forms.append(("weights", "back-to-diagonal"))
        # (two solvers that both carry the series beyond order 0 differ by its second term or less, which moves the objective of the
        #  shortest steps here by 6e-7, below DISCRIMINATION: a solver action has order 0 on one of its two sides)
        order = 99 if model.jacobi else int(p.linear_solver.max_iter)
        forms += [("solver", "neumann-%d" % m) for m in (0, 1, 3, 4) if m != order and min(m, order) == 0]
        if order == 0:
            forms.append(("solver", "jacobi"))
    for name, off in (("chunk_steps", 3), ("cq3", 0), (s.plan_opt, 0)):
        forms.append(("options", "%s=%d" % (name, off)) if name not in model.opts else ("options", "%s=unset" % name))
    # quad=0 and full weights exclude each other on a 4 x 4 x n plan (here the embedded twin's; plan_batch: "the quad-layout kernels are
    # disabled ... and the JQ_BW_T4 slab kernels have no low-rank terms"): a refusal outside the rules these sequences are about
    if s.plan_opt == "quad":
        if model.full_weights:
            forms = [f for f in forms if f != ("options", "quad=0")]
        if model.opts.get("quad") == 0:
            forms = [f for f in forms if not f[1].startswith("full")]
    return forms


def apply_setter(model, action):
    """apply one setter action to the model's params (and, with a handle, to the handle where the mirror has no field for it).
    Returns None, or for the drift ensemble with a member outside the plan -- the one evaluator that counts as a setter -- its result."""
    kind, form, seed = action
    jq, p, s = model.jq, model.params, model.spec
    rng = np.random.default_rng(seed)
    if kind == "drift":
        from test_gpu_drift_batch import pattern_members
        if form != "ensemble-outside":
            model.drift = form
        if form == "diagonal":
            p.Hconst = model.H0 + np.diag(5e-2 * float(np.max(np.abs(model.H0))) * rng.standard_normal(p.Ntot))
        elif form == "pattern":
            p.Hconst = pattern_members(model.H0, 1, seed)[0]
        elif form == "outside":
            p.Hconst = _outside(model, seed)
        elif form == "original":
            p.Hconst = model.H0.copy()
        else:      # the ensemble re-plans the handle for the union of the patterns and puts its own drift back
            members = pattern_members(model.H0, 3, seed)
            members[1] = _outside(model, seed + 1)
            if model.wa is not None:
                return evaluate(model, "drifts", seed, members=members)
    elif kind == "target":
        X = np.linalg.qr(rng.standard_normal((p.Ntot, p.N)) + 1j * rng.standard_normal((p.Ntot, p.N)))[0]
        jq.change_target(p, X)
    elif kind == "sv_type":
        if form == "1":
            p.sv_type = 1
        elif form == "pair-3":
            p.sv_type = 3
        else:
            D = rng.standard_normal((p.Ntot, p.N)) + 1j * rng.standard_normal((p.Ntot, p.N))
            if form == "pair-2":      # phase-aligned with the state the handle is in: the oracle then knows type 2 and type 3 each on its own
                from test_svtype_host import align
                D = align(plain(p), model.pcof, D)[0]
            p.dVds_r, p.dVds_i = np.asfortranarray(D.real.copy()), np.asfortranarray(D.imag.copy())
            p.sv_type = 4 if form == "4" else 2
    elif kind == "weights":
        if form in ("diagonal", "back-to-diagonal"):
            w = (0.2 + rng.random(p.Ntot)) * (np.arange(p.Ntot) >= p.N)
            p.wmat_real, p.wmat_imag = w, copy.copy(model.wimag0)
            if s.imr:
                p.wmat = w.copy()
        elif s.imr:      # the mirror of this integrator has no field for full weights: the library call itself, which must refuse
            if model.wa is not None:
                return refused_update_wmat(model, rng, int(form.split("-")[-1]), "complex" in form)
        else:
            from test_gpu_dense_wmat import set_forbidden
            set_forbidden(p, rng, int(form.split("-")[-1]), complex_states="real" not in form)
    elif kind == "solver":
        if form == "jacobi":
            p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=60, tol=1e-12)
        else:
            p.linear_solver = jq.lsolver_object(max_iter=int(form.split("-")[1]))
    elif kind == "options":
        name, value = form.split("=")
        if value == "unset":
            model.opts.pop(name)
        else:
            model.opts[name] = int(value)
        if model.wa is not None:
            model.wa.set_option(name, None if value == "unset" else int(value))
    else:
        raise KeyError(kind)
    return None


def refused_update_wmat(model, rng, nforb, complex_states):
    """jq_update_wmat on an implicit-midpoint handle: JQ_EUNSUPPORTED, and the handle is what it was (the caller's next evaluation)"""
    from juqbox_jl_amd import _lib
    from test_gpu_dense_wmat import set_forbidden
    q = copy.copy(model.params)
    set_forbidden(q, rng, nforb, complex_states)
    wr, wi = np.ascontiguousarray(q.wmat_real.ravel(order="F")), np.ascontiguousarray(q.wmat_imag.ravel(order="F"))
    rc = _lib.load().jq_update_wmat(model.wa.handle, wr.ctypes.data_as(_lib.c_dp), wi.ctypes.data_as(_lib.c_dp))
    assert rc == _lib.JQ_EUNSUPPORTED, rc
    assert model.wa.plan_info()["full_weight_rank"] == 0
    return None


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def _seed_of(name, seed):
    return SEEDS.get((name, seed), zlib.crc32(name.encode()) % 100000 + 7919 * seed)


def servable(spec, kind, evaluator):
    """can a problem's sequences hold a SERVED `evaluator` directly after a setter of this kind?"""
    if spec.imr:      # no tangent-linear sweeps, no solver action; a type action is refused
        return evaluator not in TANGENT_LINEAR and kind not in ("solver", "sv_type")
    if spec.uncoupled and evaluator in ("hvp", "ens_hvp", "drifts_hvp"):
        return False
    return True


RULE_PROBLEMS = {"tl-imr": ("imr-rowlane", "imr-t4"), "imr-sv_type": ("imr-rowlane", "imr-t4"), "imr-full-weights": ("imr-rowlane", "imr-t4"),
                 "tl-uncoupled": ("uncoupled",), "tl-jacobi": ("lanes", "parts"), "tl-full-weights": ("rowlane12", "twin"),
                 "tl-sv_type": ("t4", "dense29", "multi")}
# problems whose sequences must hold every form of every setter that exists for them: every setter must reach the embedded twin, and
# every setter must go through multi_forall
EVERY_FORM = ("twin", "multi")


def needs(jq, name):
    """what the sequences of ONE problem must hold (the two seeds together): the (setter kind, evaluator) pairs dealt to it -- every pair of
    the table goes round-robin to the problems that can serve it --, its refusal rules, and for EVERY_FORM problems every setter form"""
    pairs = set()
    for ki, k in enumerate(SETTER_KINDS):
        for ei, e in enumerate(EVALUATORS):      # (dealt along the diagonals: the pairs of one evaluator go to different problems)
            able = [s.name for s in SPECS.values() if servable(s, k, e)]
            if able[(ki + ei) % len(able)] == name:
                pairs.add((k, e))
    rules = {r for r, names in RULE_PROBLEMS.items() if name in names}
    forms = set()
    if name in EVERY_FORM:
        m = Model(jq, name)
        forms = {(k, "pair-2" if f == "pair" else f) for k, f in setter_forms(m, 0)} | {("drift", "original"), ("sv_type", "1"), ("sv_type", "pair-3"),
                                                                                         ("weights", "back-to-diagonal")}
        forms |= {("options", "%s=unset" % o) for o in ("chunk_steps", "cq3", m.spec.plan_opt)} | {("solver", f) for f in ("neumann-1", "neumann-3", "neumann-4", "jacobi")}
        if m.spec.devices:
            forms.discard(("drift", "ensemble-outside"))      # (not drawn for the multi-device handle)
    return {"pairs": pairs, "rules": rules, "forms": forms}


def _generate_problem(jq, name):
    need = needs(jq, name)
    return [_generate(jq, name, seed, need) for seed in SEEDS_PER_PROBLEM]


ORACLE_SV4 = ("gradient", "ens1", "ens3", "ens13")      # the calls that have an oracle under sv_type 4


def _form(kf):
    return (kf[0], "pair-2" if kf[1] == "pair" else kf[1])


def _score(kf, evaluator, rule, need):
    """the greedy choice: a needed pair that is SERVED, a needed refusal rule, a needed form; an unneeded refusal costs"""
    pair = (5 if evaluator == "ens_large" else 4) if rule is None and (kf[0], evaluator) in need["pairs"] else 0      # (one large ensemble per sequence)
    wanted_rule = 6 if rule in need["rules"] else 0
    form = 5 if _form(kf) in need["forms"] else 0
    if kf == ("solver", "neumann-0") and any(k == "solver" for k, _ in need["forms"]):
        form = 2      # (the other solver forms are offered from order 0 only)
    wasted = -4 if rule is not None and rule not in need["rules"] else 0
    return pair + wanted_rule + form + wasted


def _generate(jq, name, seed, need):
    """one sequence; `need` (what the problem's sequences still lack) shrinks as it goes, so seed s builds on seeds 0 .. s - 1 of the SAME
    problem and on nothing else"""
    model = Model(jq, name)
    spec = model.spec
    rng = np.random.default_rng(_seed_of(name, seed))
    steps, refused, pending = [], 0, None
    # problems that hold two kernel families in one handle: one large ensemble and one single evaluation on the Neumann solver with
    # Diagonal weights (the Jacobi solver and full weights send every batch size to the same family)
    force = ["ens_large", "gradient"] if spec.families == 2 else []
    # every Stormer-Verlet sequence: a re-plan (a drift out of the plan, or back into it) while sv_type 4 is in force and has been pushed
    # by an earlier step -- within one step sync_params pushes the drift before the type -- followed by a call whose gradient has an oracle
    if not spec.imr:
        force += ["sv_type-4", "re-plan"]
    sub = lambda: int(rng.integers(1, 1 << 30))
    normal = lambda f: not _peek(model, f).jacobi and not _peek(model, f).full_weights
    while len(steps) < STEPS:
        i = len(steps)
        if pending is not None:      # second half of "type 2, evaluate, type 3 with the same dVds, evaluate"
            setters, ev, pending = [("sv_type", "pair-3", 0)], "gradient", None
        else:
            forms = setter_forms(model, i)
            after_pair = model.sv_type == 3      # types 2 / 3 have an oracle only while their dVds is aligned: the next action ends the pair
            if after_pair:
                forms = [f for f in forms if f[0] == "sv_type" and f[1] in ("1", "4")]
            forced, prefix = None, []
            if force and i >= 3 and not after_pair:
                what = force.pop(0)
                norm = ([("solver", "neumann-0")] if model.jacobi else []) + ([("weights", "back-to-diagonal")] if model.full_weights else [])
                if what == "sv_type-4":
                    forced = ORACLE_SV4
                    forms = [("sv_type", "4")] if model.sv_type != 4 else [f for f in forms if f[0] in ("target", "weights", "solver")]
                elif what == "re-plan":
                    forced = ORACLE_SV4
                    if spec.t4:
                        forms = [("drift", "original" if model.drift == "outside" else "outside")]
                    else:      # (no structure a drift could leave: the plan-shaping option re-plans, the embedded twin included)
                        forms = [f for f in forms if f[0] == "options" and f[1].startswith(spec.plan_opt + "=")] or \
                            [("weights", "back-to-diagonal")]      # (the twin: quad=0 is not offered under full weights)
                elif norm:
                    forced, forms, prefix = (what,), norm[-1:], [(a[0], a[1], sub()) for a in norm[:-1]]
                else:
                    forced = (what,)
                    forms = [f for f in forms if normal(f) and f[1] not in ("outside", "ensemble-outside", "pair")]
            cands = []
            for kf in forms:
                for e in (forced or EVALUATORS):
                    if kf[1] == "pair" and e != "gradient":
                        continue
                    # one large ensemble per sequence (its oracle takes seconds): the forced one where there is one
                    if e == "ens_large" and not forced and (spec.families == 2 or any(st["evaluator"] == e for st in steps)):
                        continue
                    rule = refusal(_peek(model, kf), e)
                    if rule is not None and refused >= MAX_REFUSED:
                        continue
                    cands.append((_score(kf, e, rule, need), kf, e))
            best = max(c[0] for c in cands)
            pick = [c for c in cands if c[0] == best]
            _, kf, ev = pick[int(rng.integers(len(pick)))]
            setters = [(kf[0], _form(kf)[1], sub())]
            if kf[1] == "pair":
                pending = True
            r = rng.random()
            # a second setter of another kind in front of it: a form the problem still needs, else one in three steps a random one
            others = [f for f in forms if f[0] != kf[0] and f[1] not in ("pair", "ensemble-outside") and
                      refusal(_peek(_peek(model, f), kf), ev) == refusal(_peek(model, kf), ev)]
            if spec.imr:
                others = [f for f in others if f[0] != "sv_type" and not f[1].startswith("full")]
            wanted = [f for f in others if _form(f) in need["forms"]]
            if forced:
                setters = prefix + setters
            elif after_pair or kf[1] in ("pair", "ensemble-outside"):
                pass
            elif wanted:
                o = wanted[int(rng.integers(len(wanted)))]
                setters.insert(0, (o[0], o[1], sub()))
            elif best <= 0 and r < 0.2:
                setters = []      # an evaluation after no setter at all
            elif r < 0.35 and others:
                o = others[int(rng.integers(len(others)))]
                setters.insert(0, (o[0], o[1], sub()))
        for a in setters:
            apply_setter(model, a)
            need["forms"].discard((a[0], a[1]))
            if spec.imr and a[0] == "weights" and a[1].startswith("full"):
                need["rules"].discard("imr-full-weights")
        rule = refusal(model, ev)
        if rule is not None:
            refused += 1
            need["rules"].discard(rule)
        elif setters:      # (a refused call says nothing about the state the setter left: only a served one covers the pair)
            need["pairs"].discard((setters[-1][0], ev))
        steps.append({"setters": setters, "evaluator": ev, "seed": sub(), "refused": rule})
        after_refusal(model, rule)
    return steps


def _peek(model, kf):
    """a cheap stand-in of the model after a setter of this (kind, form): only what refusal() reads"""
    t = copy.copy(model)
    t.params = copy.copy(model.params)
    kind, form = kf
    if kind == "sv_type":
        t.params.sv_type = {"1": 1, "4": 4, "pair": 2}[form]
    elif kind == "weights" and not model.spec.imr:
        t.params.wmat_real = np.zeros((1, 1)) if form.startswith("full") else np.zeros(1)
    elif kind == "solver":
        t.params.linear_solver = model.jq.lsolver_object(solver=model.jq.JACOBI_SOLVER, tol=1e-12) if form == "jacobi" else model.jq.lsolver_object()
    return t


def after_refusal(model, rule):
    """sv_type != 1 under implicit midpoint: jq_set_sv_type refused it and the handle kept type 1; the script puts its params back"""
    if rule == "imr-sv_type":
        model.params.sv_type = 1


_CACHE = {}


def sequence(jq, name, seed, fresh=False):
    """the sequence of (problem name, seed): a function of the two alone (the other problems' sequences play no part)"""
    if fresh:
        return _generate_problem(jq, name)[SEEDS_PER_PROBLEM.index(seed)]
    if name not in _CACHE:
        _CACHE[name] = _generate_problem(jq, name)
    return _CACHE[name][SEEDS_PER_PROBLEM.index(seed)]


def all_sequences(jq, fresh=False):
    return collections.OrderedDict(((n, sd), sequence(jq, n, sd, fresh)) for n in SPECS for sd in SEEDS_PER_PROBLEM)


IDS = ["%s-%d" % (n, s) for n in SPECS for s in SEEDS_PER_PROBLEM]


# ---- evaluator calls ------------------------------------------------------------------------------------------------------------------------
def large_count(info, N, cost=1):
    """the smallest ensemble size beyond the kernel family that serves 13 samples, from jq_plan_info's thresholds (None: the last family
    of the list serves it, or the next one starts beyond what LARGE_MAX allows the oracle: the call then takes 14)"""
    def capacity(f):      # samples a family takes
        if "max_columns" in f:
            return f["max_columns"] // N
        if "max_quads" in f:
            return 4 * f["max_quads"] // N
        return f["max_slabs"] * (16 // N) if N <= 16 else f["max_slabs"] // ((N + 15) // 16)
    for f in info["families"]:
        c = capacity(f)
        if c >= 13:
            return c + 1 if (c + 1) * cost <= LARGE_MAX else None
    return None


def call_data(model, evaluator, seed, members=None):
    """the seeded arguments of an evaluator call"""
    from test_gpu_drift_batch import pattern_members
    from test_gpu_member_batch import amplitude_mixes, full_mixes
    from test_gpu_pcof_batch import vectors
    p = model.params
    rng = np.random.default_rng(seed)
    d = {"pcof": model.pcof}
    if evaluator.startswith("ens"):
        n = {"ens1": 1, "ens3": 3, "ens13": 13, "ens_batch": 3, "ens_hvp": 3}.get(evaluator)
        if evaluator == "ens_large":
            n = large_count(model.wa.plan_info(), p.N, p.Ntot * p.Ntot * p.N * p.nsteps) if model.wa is not None else 14
            n = 14 if n is None else n
        d["nodes"], d["weights"] = 0.05 * rng.standard_normal(n), rng.random(n)
        d["shift"] = 0.05 * rng.standard_normal(p.Ntot)
        d["shift"][0] = 0.0
    if evaluator in ("batch", "ens_batch"):
        d["pcofs"] = vectors(model.pcof, 3, seed)
    if evaluator in ("drifts", "drifts_hvp"):
        d["members"] = members if members is not None else pattern_members(model.H0, 3, seed)
        d["weights"] = rng.random(3)
    if evaluator == "members":
        nc = max(p.Ncoupled, p.Nunc)
        d["mixes"] = amplitude_mixes(model.jq, nc, 3, seed) if p.Nunc else full_mixes(nc, 3, seed)
    if evaluator in TANGENT_LINEAR:
        d["dirs"] = rng.standard_normal((model.pcof.size, 2))
    return d


NAMES7 = ("objfv", "totalgrad", "primaryobjf", "secondaryobjf", "traceInfidelity", "infidelgrad", "leakgrad")


def evaluate(model, evaluator, seed, members=None, data=None):
    """one evaluator call through the mirror -> dict of everything it returned; a library refusal -> {"refused": code}"""
    from juqbox_jl_amd import _lib
    jq, p, wa = model.jq, model.params, model.wa
    d = data or call_data(model, evaluator, seed, members)
    pcof = d["pcof"]
    try:
        if evaluator == "forward":
            r = dict(zip(("objfv", "primaryobjf", "secondaryobjf"), jq.traceobjgrad(pcof, p, wa, False, False)))
        elif evaluator == "gradient":
            r = dict(zip(NAMES7, jq.traceobjgrad(pcof, p, wa, False, True)))
        elif evaluator == "history":
            r = dict(zip(("objfv", "history", "fidelity"), jq.traceobjgrad(pcof, p, wa, True, False)))
        elif evaluator in ("ens1", "ens3", "ens13", "ens_large"):
            inf, leak = jq.eval_f_g_grad(pcof, p, wa, d["nodes"], d["weights"], True, shift=d["shift"])
            r = dict(infidelity=inf, leak=leak, infid_grad=p.last_infidelity_grad.copy(), leak_grad=p.last_leak_grad.copy())
        elif evaluator == "batch":
            r = dict(zip(NAMES7, jq.traceobjgrad_batch(d["pcofs"], p, wa, True)))
        elif evaluator == "ens_batch":
            r = dict(zip(("infidelity", "leak", "infid_grad", "leak_grad"),
                         jq.eval_f_g_grad_batch(d["pcofs"], p, wa, d["nodes"], d["weights"], True, shift=d["shift"])))
        elif evaluator == "drifts":
            r = dict(zip(NAMES7, jq.traceobjgrad_drifts(pcof, p, wa, d["members"], True)))
        elif evaluator == "members":
            r = dict(zip(NAMES7, jq.traceobjgrad_members(pcof, p, wa, ctrl_mix=d["mixes"], evaladjoint=True)))
        elif evaluator == "jvp":
            r = jq.traceobj_jvp(pcof, d["dirs"], p, wa, final=True)
        elif evaluator == "hvp":
            r = jq.traceobjgrad_hvp(pcof, d["dirs"], p, wa)
        elif evaluator == "ens_hvp":
            r = jq.eval_f_g_grad_hvp(pcof, d["dirs"], p, wa, d["nodes"], d["weights"], shift=d["shift"])
        elif evaluator == "drifts_hvp":
            r = jq.eval_f_g_grad_drifts_hvp(pcof, d["dirs"], p, wa, d["members"], d["weights"])
        else:
            raise KeyError(evaluator)
    except _lib.JuqboxHipError as e:
        return {"refused": e.code}
    r["kernel_family"] = wa.last_timing()["kernel_family"]
    return r


def same_bits(tag, a, b):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        if k == "kernel_family":
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (tag, k, a[k], b[k])


# ---- criterion (a): the CPU oracle for the state the handle is in ----------------------------------------------------------------------------
def oracle_single(params, pcof, history=False):
    """the oracle's traceobjgrad of a problem in its integrator (sv_type 1)"""
    from oracle.oracle import Oracle
    orc = Oracle(params, use_sparse=False)
    if params.Integrator_id == 2:
        return orc.traceobjgrad_imr(pcof, int(params.linear_solver.max_iter), float(params.linear_solver.tol), history=history)
    return orc.traceobjgrad(pcof, history=history)


def oracle_ensemble(params, pcof, nodes, weights, shift):
    """dict(infidelity, leak, infid_grad, leak_grad, totalgrad) of the risk-neutral ensemble (implicit midpoint: the weighted sum of the
    samples' evaluations, as tests/test_gpu_imr.py _random_checks)"""
    from oracle.oracle import Oracle
    if params.Integrator_id != 2:
        r = Oracle(params, use_sparse=False).eval_f_g_grad(pcof, nodes, weights, shift)
        return dict(infidelity=r["last_infidelity"], leak=r["last_leak"], infid_grad=r["last_infidelity_grad"], leak_grad=r["last_leak_grad"],
                    totalgrad=r["last_infidelity_grad"] + r["last_leak_grad"])
    out = dict(infidelity=0.0, leak=0.0, infid_grad=np.zeros(pcof.size), leak_grad=np.zeros(pcof.size))
    q = copy.copy(params)
    for ep, w in zip(nodes, weights):
        q.Hconst = np.asarray(params.Hconst, dtype=np.float64) + np.diag(ep * shift)
        r = oracle_single(q, pcof)
        out["infidelity"] += w * r["primaryobjf"]
        out["leak"] += w * r["secondaryobjf"]
        out["infid_grad"] += w * r["infidelgrad"]
        out["leak_grad"] += w * r["leakgrad"]
    out["totalgrad"] = out["infid_grad"] + out["leak_grad"]
    return out


def plain(params):
    """a copy of the params with sv_type 1: what the oracle knows"""
    q = copy.copy(params)
    q.sv_type = 1
    return q


def oracle_state(model, pcof=None):
    """(objfv, totalgrad) of the single evaluation for the state the model is in: type 1 as it is, type 4 polarisation term + leak part,
    types 2 / 3 -- whose dVds the pair action has phase-aligned -- the aligned constructions (tests/test_svtype_host.py)"""
    from test_svtype_host import leak_part, ref_polar
    p, pcof = plain(model.params), model.pcof if pcof is None else pcof
    ev = lambda q: oracle_single(q, pcof)
    r = ev(p)
    if model.sv_type == 1:
        return r["objfv"], r["totalgrad"]
    D = np.asarray(model.params.dVds_r) + 1j * np.asarray(model.params.dVds_i)
    if model.sv_type == 4:
        return r["objfv"], ref_polar(p, ev, D) + leak_part(p, ev)
    return r["objfv"], aligned_reference(p, pcof, D, model.sv_type, ev)["totalgrad"]


def aligned_reference(q, pcof, D, sv_type, ev):
    """the oracle's type 2 / type 3 evaluation for a dVds that is phase-aligned at pcof (s_T / s_D = rho > 0, asserted)"""
    from test_svtype_host import ref_type2, ref_type3, traces
    sT, sD = traces(q, pcof, D)
    ratio = sT / sD
    assert abs(ratio.imag) <= 1e-9 * abs(ratio) and ratio.real > 0, ("dVds is not phase-aligned in this state", ratio)
    return ref_type2(q, ev, D, abs(ratio)) if sv_type == 2 else ref_type3(q, ev, abs(ratio))


OBJECTIVE_PARTS = ("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity", "fidelity", "infidelity", "leak")


def close(tag, value, ref, imr=False):
    value, ref = np.atleast_1d(np.asarray(value, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    d, n = np.linalg.norm(value - ref), np.linalg.norm(ref)
    print("    %-52s |diff| %.3e  |ref| %.3e" % (tag, d, n))
    if imr:      # the criterion of tests/test_gpu_imr.py (_random_checks): 1e-9 relative; the parts of the objective with its floor of 1e-3
        floor = 1e-3 if tag.split()[-1] in OBJECTIVE_PARTS else 0.0
        assert d <= 1e-9 * max(n, floor), tag
    else:
        assert reference_pass(value, ref), tag


def check_oracle(model, evaluator, data, r, tag, pair=None):
    """criterion (a) for one served call.  sv_type != 1: the single and ensemble gradients through the constructions of
    tests/test_svtype_host.py (types 2 / 3: the sum identity once both halves of the pair are in, `pair` = the first half's result); the
    batch, drift and member calls have no oracle helper there (the caller compares their columns with single calls on the replay handle)."""
    from test_svtype_host import leak_part, oracle_ensemble_eval, ref_polar
    p, pcof, imr = model.params, data["pcof"], model.spec.imr
    q = plain(p)
    sv = model.sv_type
    two = p.objFuncType != 1
    D = np.asarray(p.dVds_r) + 1j * np.asarray(p.dVds_i)
    cl = lambda name, v, w: close("%s %s" % (tag, name), v, w, imr)
    if evaluator in ("forward", "gradient", "history"):
        o = oracle_single(q, pcof, history=evaluator == "history")
        for k in ("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity"):
            if k in r:
                cl(k, r[k], o[k])
        if evaluator == "history":
            from uncoupled_problem import HISTORY_ATOL
            err = float(np.max(np.abs(r["history"] - o["history"])))
            print("    %-52s max |diff| %.3e" % (tag + " history", err))
            assert err < HISTORY_ATOL
            cl("fidelity", r["fidelity"], 1.0 - o["traceInfidelity"])
        if evaluator == "gradient":
            ev = lambda x: oracle_single(x, pcof)
            if sv == 1:
                for k in ("totalgrad", "infidelgrad") + (("leakgrad",) if two else ()):
                    cl(k, r[k], o[k])
            elif sv == 4:
                cl("totalgrad (type 4)", r["totalgrad"], ref_polar(q, ev, D) + leak_part(q, ev))
                if two:
                    cl("infidelgrad (type 4)", r["infidelgrad"], ref_polar(q, ev, D))
            else:
                a = aligned_reference(q, pcof, D, sv, ev)
                cl("totalgrad (type %d, aligned)" % sv, r["totalgrad"], a["totalgrad"])
                cl("infidelgrad (type %d, aligned)" % sv, r["infidelgrad"], a["infidelgrad"])
            if sv == 3 and pair is not None:
                cl("totalgrad (types 2 + 3)", pair["totalgrad"] + r["totalgrad"], ref_polar(q, ev, D) + 2.0 * leak_part(q, ev))
                if two:
                    cl("infidelgrad (types 2 + 3)", pair["infidelgrad"] + r["infidelgrad"], ref_polar(q, ev, D))
            if two and sv != 1:
                cl("leakgrad", r["leakgrad"], o["leakgrad"])
    elif evaluator in ("ens1", "ens3", "ens13", "ens_large"):
        o = oracle_ensemble(q, pcof, data["nodes"], data["weights"], data["shift"])
        cl("infidelity", r["infidelity"], o["infidelity"])
        cl("leak", r["leak"], o["leak"])
        if sv == 1:
            cl("infid_grad", r["infid_grad"], o["infid_grad"] if two else o["totalgrad"])
            if two:
                cl("leak_grad", r["leak_grad"], o["leak_grad"])
        elif sv == 4:
            ev = oracle_ensemble_eval(pcof, data["nodes"], data["weights"], data["shift"])
            total = r["infid_grad"] + (r["leak_grad"] if two else 0.0)
            cl("total gradient (type 4)", total, ref_polar(q, ev, D) + leak_part(q, ev))
    elif sv != 1 and evaluator in ("batch", "ens_batch", "drifts", "members"):
        pass
    elif evaluator == "batch":
        for i, v in enumerate(data["pcofs"]):
            o = oracle_single(q, v)
            for k in NAMES7:
                if k != "leakgrad" or two:
                    cl("vector %d %s" % (i, k), r[k][i] if r[k].ndim == 1 else r[k][:, i], o[k])
    elif evaluator == "ens_batch":
        for i, v in enumerate(data["pcofs"]):
            o = oracle_ensemble(q, v, data["nodes"], data["weights"], data["shift"])
            cl("vector %d infidelity" % i, r["infidelity"][i], o["infidelity"])
            cl("vector %d leak" % i, r["leak"][i], o["leak"])
            cl("vector %d infid_grad" % i, r["infid_grad"][:, i], o["infid_grad"] if two else o["totalgrad"])
            if two:
                cl("vector %d leak_grad" % i, r["leak_grad"][:, i], o["leak_grad"])
    elif evaluator in ("drifts", "members"):
        import test_gpu_drift_batch as DB
        import test_gpu_member_batch as MB
        from test_gpu_pcof_batch import column
        nc = max(p.Ncoupled, p.Nunc)
        for i in range(3):
            col = column(r, i)
            if evaluator == "drifts" and not imr:
                DB.check_oracle("%s member %d" % (tag, i), q, pcof, data["members"][i], col)
            elif evaluator == "drifts":
                MB.check_oracle("%s member %d" % (tag, i), q, pcof, np.eye(nc), data["members"][i], col)
            else:
                MB.check_oracle("%s member %d" % (tag, i), q, pcof, data["mixes"][i], None, col)
    elif evaluator == "jvp":
        from tangent_reference import TangentReference
        ref = TangentReference(q)
        ts = [ref.tangent(pcof, data["dirs"][:, j]) for j in range(data["dirs"].shape[1])]
        cl("primaryobjf", r["primaryobjf"], ts[0]["primaryobjf"])
        cl("d_primary", r["d_primary"], [t["d_primary"] for t in ts])
        cl("d_secondary", r["d_secondary"], [t["d_secondary"] for t in ts])
        for j, t in enumerate(ts):
            W = r["W"][:, :, j]
            cl("W %d" % j, np.concatenate([W.real.ravel(), W.imag.ravel()]), np.concatenate([t["W"].real.ravel(), t["W"].imag.ravel()]))
    elif evaluator == "hvp":
        from hessian_reference import HessianReference
        ref, o = HessianReference(q), oracle_single(q, pcof)
        cl("totalgrad", r["totalgrad"], o["totalgrad"])
        for j in range(data["dirs"].shape[1]):
            t = ref.hvp(pcof, data["dirs"][:, j])
            cl("hv %d" % j, r["hv"][:, j], t["hv"])
            if two:
                cl("hv_infid %d" % j, r["hv_infid"][:, j], t["hv_infid"])
    elif evaluator in ("ens_hvp", "drifts_hvp"):
        if evaluator == "ens_hvp":
            from ensemble_hessian_reference import EnsembleHessianReference
            ref = EnsembleHessianReference(q, data["nodes"], data["weights"], data["shift"])
            o = oracle_ensemble(q, pcof, data["nodes"], data["weights"], data["shift"])
        else:
            from drift_hessian_reference import DriftHessianReference, weighted_oracle
            stack = np.stack(data["members"], axis=2)
            ref = DriftHessianReference(q, stack, data["weights"])
            w = weighted_oracle(q, pcof, stack, data["weights"])
            o = dict(infidelity=w["infidelity"], leak=w["leak"], infid_grad=w["infidelgrad"], totalgrad=w["totalgrad"])
        cl("infidelity", r["infidelity"], o["infidelity"])
        cl("leak", r["leak"], o["leak"])
        cl("infid_grad", r["infid_grad"], o["infid_grad"] if two else o["totalgrad"])
        for j in range(data["dirs"].shape[1]):
            t = ref.hvp(pcof, data["dirs"][:, j])
            cl("hv_infid %d" % j, r["hv_infid"][:, j], t["hv_infid"])
            cl("hv_leak %d" % j, r["hv_leak"][:, j], t["hv_leak"])
    else:
        raise KeyError(evaluator)


# ---- criterion (c): what a refused call leaves of its output arrays ----------------------------------------------------------------------------
def refused_call_writes_nothing(model, evaluator, data):
    """the refused evaluator once more through the C ABI itself, its output arrays pre-filled with NaN: the expected code, nothing written"""
    from juqbox_jl_amd import _lib
    L, h, p = _lib.load(), model.wa.handle, model.params
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F"))
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    nan = lambda *shape: np.full(shape, np.nan)
    pcof = f(data["pcof"])
    n = pcof.size
    if evaluator in TANGENT_LINEAR:
        D = np.ascontiguousarray(data["dirs"].T)
        nd = D.shape[0]
    if evaluator == "jvp":
        outs = [nan(4), nan(nd, 3), nan(p.Ntot * p.N * nd), nan(p.Ntot * p.N * nd)]
        rc = L.jq_traceobj_jvp(h, ptr(pcof), n, ptr(D), nd, *[ptr(o) for o in outs])
    elif evaluator == "hvp":
        outs = [nan(4), nan(n), nan(nd, n), nan(nd, n)]
        rc = L.jq_traceobjgrad_hvp(h, ptr(pcof), n, ptr(D), nd, *[ptr(o) for o in outs])
    elif evaluator == "ens_hvp":
        nodes, weights, sh = f(data["nodes"]), f(data["weights"]), f(data["shift"])
        outs = [nan(2), nan(n), nan(n), nan(nd, n), nan(nd, n)]
        rc = L.jq_eval_f_g_grad_hvp(h, ptr(pcof), n, ptr(D), nd, ptr(nodes), ptr(weights), nodes.size, ptr(sh), *[ptr(o) for o in outs])
    elif evaluator == "drifts_hvp":
        H = np.ascontiguousarray(np.stack([f(M) for M in data["members"]]))
        w = f(data["weights"])
        outs = [nan(2), nan(n), nan(n), nan(nd, n), nan(nd, n)]
        rc = L.jq_eval_f_g_grad_drifts_hvp(h, ptr(pcof), n, ptr(D), nd, ptr(H), ptr(w), H.shape[0], *[ptr(o) for o in outs])
    else:      # (sv_type != 1 under implicit midpoint is refused by the setter inside sync_params: no output array is involved)
        return
    assert rc == _lib.JQ_EUNSUPPORTED, (evaluator, rc)
    for o in outs:
        assert np.all(np.isnan(o)), (evaluator, "a refused call wrote to an output array")


# ---- the runner ---------------------------------------------------------------------------------------------------------------------------
PLAN_KEYS = ("structure", "sv_type", "full_weight_rank", "linear_solver", "options", "embedded_twin_Ntot", "replanned")


def replay_handle(jq, name, steps, upto):
    """a fresh handle that gets the setter actions of steps[0 .. upto] -- sync_params where the long-lived handle evaluated, no evaluation"""
    from juqbox_jl_amd import _lib
    m = Model(jq, name).open()
    try:
        for j in range(upto + 1):
            m.side = [apply_setter(m, a) for a in steps[j]["setters"]]
            if j < upto:
                try:
                    m.wa.sync_params()
                except _lib.JuqboxHipError as e:
                    assert steps[j]["refused"] == "imr-sv_type" and e.code == _lib.JQ_EUNSUPPORTED, (j, steps[j], e)
                after_refusal(m, steps[j]["refused"])
    except Exception:
        m.close()
        raise
    return m


def columns_against_single_calls(replay, evaluator, data, r):
    """sv_type != 1: the columns of a batch / drift call bit for bit against the single call, both on the replay handle with cq3=0 as in
    tests/test_gpu_drift_batch.py -- the one-workgroup backward kernel a grouped launch runs (after criterion (b): that handle is thrown away)"""
    from test_gpu_pcof_batch import column
    p = replay.params
    replay.wa.set_option("cq3", 0)
    # ... for the call itself too: once more on this handle, which must give the long-lived handle's bits again
    again = evaluate(replay, evaluator, 0, data=dict(data))
    same_bits("the call with cq3=0", again, r)
    r = again
    if evaluator == "batch":
        for i, v in enumerate(data["pcofs"]):
            s = evaluate(replay, "gradient", 0, data={"pcof": v})
            same_bits("vector %d against the single call" % i, {k: s[k] for k in NAMES7}, column(r, i))
    elif evaluator == "ens_batch":
        for i, v in enumerate(data["pcofs"]):
            s = evaluate(replay, "ens3", 0, data=dict(data, pcof=v))
            for k in ("infidelity", "leak", "infid_grad", "leak_grad"):
                col = r[k][i] if r[k].ndim == 1 else r[k][:, i]
                if replay.spec.devices:
                    # a multi-device handle shards the VECTORS of a batch (a vector's nodes are summed on one device, the bits of a
                    # single-device handle: tests/test_gpu_nodes_batch.py) but the NODES of the single call (summed across devices in
                    # another order): the same numbers to the reference's criterion, not the same bits
                    assert reference_pass(col, s[k]), ("vector %d against eval_f_g_grad" % i, k)
                else:
                    assert np.array_equal(np.asarray(s[k]), col), ("vector %d against eval_f_g_grad" % i, k)
    elif evaluator == "drifts":
        H = np.array(p.Hconst, dtype=np.float64)
        structure = replay.wa.plan_info()["structure"]
        for i, M in enumerate(data["members"]):
            p.Hconst = np.array(M, dtype=np.float64)
            s = evaluate(replay, "gradient", 0, data={"pcof": data["pcof"]})
            if replay.wa.plan_info()["structure"] == structure:
                same_bits("member %d against the single call" % i, {k: s[k] for k in NAMES7}, column(r, i))
            else:
                # a handle that was re-planned out of its structure plans back when a member with that structure becomes ITS drift
                # (jq_update_hconst), while the ensemble ran the member on the general plan: other kernels, the reference's criterion
                for k in NAMES7:
                    assert reference_pass(column(r, i)[k], s[k]), ("member %d against the single call on the plan it plans back to" % i, k)
        p.Hconst = H
    # (members: a member's single call needs a handle of the mixed operators, whose plan is its own -- criterion (b) alone)


def run_sequence(jq, name, seed, replay_every=1):
    """drive one handle through the sequence; returns the kernel families its evaluations ran on"""
    from juqbox_jl_amd import _lib
    steps = sequence(jq, name, seed)
    long = Model(jq, name).open()
    families, pair, replay = set(), None, None
    try:
        for i, st in enumerate(steps):
            tag = "%s-%d step %d %s" % (name, seed, i, st["evaluator"])
            print("  %s after %s%s" % (tag, [a[:2] for a in st["setters"]], " (refused: %s)" % st["refused"] if st["refused"] else ""))
            t0 = time.time()
            side = [apply_setter(long, a) for a in st["setters"]]
            assert refusal(long, st["evaluator"]) == st["refused"], (tag, "the generator's model and the runner's disagree")
            data = call_data(long, st["evaluator"], st["seed"])
            r = evaluate(long, st["evaluator"], st["seed"], data=data)
            replayed = bool(st["setters"]) or i % replay_every == 0 or i == len(steps) - 1
            if replayed:
                replay = replay_handle(jq, name, steps, i)
                for res, res2 in zip(side, replay.side):      # the drift ensemble that re-planned the handle: a setter action on both
                    if res is not None:
                        same_bits(tag + " re-planning ensemble against the replay handle", res, res2)
                rr = evaluate(replay, st["evaluator"], st["seed"], data=dict(data))
            if st["refused"]:
                assert r == {"refused": _lib.JQ_EUNSUPPORTED}, (tag, r)
                refused_call_writes_nothing(long, st["evaluator"], data)
                if replayed:
                    assert rr == r, (tag, rr)
            else:
                assert "refused" not in r, (tag, r, st)
                families.add(r["kernel_family"])
                failed = []      # both criteria are evaluated before either fails the test
                for what, crit in (("(a) oracle", lambda: check_oracle(long, st["evaluator"], data, r, tag, pair)),
                                   ("(b) replay", lambda: same_bits(tag + " against the replay handle", r, rr) if replayed else None)):
                    try:
                        crit()
                    except AssertionError as e:
                        failed.append("%s: %s" % (what, str(e)[:300]))
                assert not failed, (tag, failed)
            if i == len(steps) - 1:      # after the last step both handles report the same plan
                a, b = long.wa.plan_info(), replay.wa.plan_info()
                for k in PLAN_KEYS:
                    assert a[k] == b[k], (name, seed, k, a[k], b[k])
            if replayed and not st["refused"] and long.sv_type != 1 and st["evaluator"] in ("batch", "ens_batch", "drifts"):
                columns_against_single_calls(replay, st["evaluator"], data, r)      # (the replay handle is thrown away after this)
            for a, res in zip(st["setters"], side):      # the drift ensemble with a member outside the plan: held to the oracle too
                if res is not None and long.sv_type == 1:
                    from test_gpu_drift_batch import pattern_members
                    members = pattern_members(long.H0, 3, a[2])
                    members[1] = _outside(long, a[2] + 1)
                    check_oracle(long, "drifts", {"pcof": long.pcof, "members": members}, res, tag + " (re-planning ensemble)")
            pair = r if (st["evaluator"] == "gradient" and long.sv_type == 2) else None
            after_refusal(long, st["refused"])
            if replayed:
                replay.close()
                replay = None
            print("    (step %d: %.2f s%s)" % (i, time.time() - t0, ", %d samples" % len(data["nodes"]) if "nodes" in data else ""))
        return families
    finally:
        long.close()
        if replay is not None:
            replay.close()
