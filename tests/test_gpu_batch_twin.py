"""GPU (-m gpu): a grouped batch of control vectors that reaches its kernels through the embedded twin.

A random 3 x 3 x 2 Kronecker problem (18 levels: no row-lane kernels; the twin has 4 x 4 x 2 = 32) with option embed=2: every batch of the
handle is evaluated by the twin, so the request of a grouped launch -- its vectors, the padding of a vector's column quads, its nodes --
crosses from one handle to the other, and a caller's shift is remapped to the twin's rows on the way.
  (a) jq_traceobjgrad_batch: every column bit-identical to traceobjgrad on the same handle, and against the CPU oracle;
  (b) jq_eval_f_g_grad_batch with a caller's shift and unequal weights: per vector bit-identical to eval_f_g_grad and traceobj_sweep, and
      against the oracle's ensemble;
  (c) afterwards a plain ensemble evaluation on the same handle equals that of a fresh handle bit for bit: nothing of a request
      outlives its call.
Oracle criterion: conftest.reference_pass (atol 1e-14 or rtol 1e-10 in the 2-norm)."""
import numpy as np
import pytest

import test_gpu_nodes_batch as nb
import test_gpu_pcof_batch as pb
from kronecker_problem import random_kronecker_problem

pytestmark = pytest.mark.gpu

OPTIONS = {"embed": 2, "cq3": 0}


def test_grouped_batches_through_the_embedded_twin(jq):
    params, pcof, _ = random_kronecker_problem(jq, (3, 3, 2), 4)
    assert params.Ntot == 18
    vecs = pb.vectors(pcof, 3, 301)
    shift = nb.small_shift(params, 33)      # (random per level, nothing on the first one: the oracle's ensemble perturbs the levels from the second on)
    nodes, weights = nb.ensemble(3, 31)
    nodes5, weights5 = nb.ensemble(5, 32)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=OPTIONS)
    try:
        assert wa.plan_info()["embedded_twin_Ntot"] == 32
        # (a)
        b = pb.batch(jq, vecs, params, wa)
        info = wa.plan_info()["pcof_batch"]
        print("  pcof_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == "grouped" and info["nodes_per_vector"] == 1, info
        assert wa.last_timing()["kernel_family"] == 8, wa.last_timing()
        for i, v in enumerate(vecs):
            pb.same_bits("column %d against the single call" % i, pb.column(b, i), pb.single(jq, v, params, wa))
            pb.check_oracle("column %d" % i, params, v, pb.column(b, i))
        # (b)
        e = nb.batch(jq, vecs, params, wa, nodes, weights, shift)
        info = wa.plan_info()["pcof_batch"]
        print("  pcof_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == "grouped" and info["nodes_per_vector"] == 3, info
        assert wa.last_timing()["kernel_family"] == 8, wa.last_timing()
        for i, v in enumerate(vecs):
            nb.same_bits("column %d against the single calls" % i, nb.column(e, i), nb.single(jq, v, params, wa, nodes, weights, shift))
            nb.check_oracle("column %d" % i, params, nb.column(e, i), nb.oracle_ref(params, v, nodes, weights, shift))
        nb.batch(jq, vecs, params, wa, nodes, weights, shift)      # (the last call before (c) is a grouped one)
        # (c)
        after = nb.single(jq, pcof, params, wa, nodes5, weights5, shift)
        fresh_wa = jq.Working_Arrays_HIP(params, pcof.size, options=OPTIONS)
        try:
            fresh = nb.single(jq, pcof, params, fresh_wa, nodes5, weights5, shift)
        finally:
            fresh_wa.close()
        nb.same_bits("after the batches against a fresh handle", after, fresh)
    finally:
        wa.close()
