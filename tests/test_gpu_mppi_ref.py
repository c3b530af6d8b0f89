"""GPU against tests/mppi_ref.py, the restatement of MPPIUtils.jl written from the Julia text -- not against
oracle/or_mppi.c.  The oracle package appears only as the source of the libm routines and of the Philox stream
(this project's own noise, a given input).

Cases (tests/mppi_ref_cases.py), the smallest shapes at which the plan kernel can still go wrong:
  generic-ref / -A / -B   S = 2, K = 70, H = 5, external noise, three circles and a grid, the reference's Σ and
                          the two correlated ones (A: inverse and Cholesky factor differ when divided instead of
                          scaled by LAPACK's reciprocal; B: getrf swaps the rows).
  lpr1                    S = 2, K = 300, H = 7, one rollout per lane (MPGPU_LPR=1), the lean instance and the
                          generic one (MPGPU_PLAN_LEAN=0), Philox noise, grid, control cost, Σ = A; the
                          FeasibilityCount prefix ends inside the partial block of both scenes.

Per scene:
  * the whole TrajectoryCollection -- sampled controls, states, costs, feasibility flags of all K rollouts -- bit
    for bit, RolloutCount and FeasibleTrajCount exactly;
  * the final rollout given the device's own MPPICtrl: TrajectoryRollout(U_device) by the restatement equals the
    device's Traj, cost and Feasibility bit for bit (no tolerance: the input is the device's);
  * MPPICtrl against its exact value, per entry within the forward error bound derived in
    tests/mppi_ref_cases.py's docstring (the reference's own sequential fold is held to the same bound in
    tests/test_mppi_ref.py).  Measured error / bound: DESIGN.md, next to the tolerance table.
"""
import numpy as np
import pytest

from motionplanning_amd.mppi import mppi_plan_batch

import mppi_ref
import mppi_ref_cases as cases

pytestmark = pytest.mark.gpu

PARAMS = [(n, i) for n in cases.NAMES for i in range(len(cases.build(n)["envs"]))]


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name,ienv", PARAMS, ids=["%s-env%d" % (n, i) for n, i in PARAMS])
def test_device_equals_restatement(ctx, name, ienv):
    c = cases.build(name)
    p, S = c["p"], c["S"]
    with cases.env(c["envs"][ienv]):
        gpu = mppi_plan_batch(p, c["X0"], c["goal"], c["unom"], c["obs"], c["grid"], c["z"], collect=True, ctx=ctx)
    assert not gpu["nan"]
    for s in range(S):
        ref = cases.restatement(c, s)
        coll = ref["arrays"]
        # the collection, all K rollouts
        assert _same(gpu["coll"]["ctrl"][s], coll["ctrl"]), (s, "sampled controls")
        assert _same(gpu["coll"]["traj"][s], coll["traj"]), (s, "states")
        assert _same(gpu["coll"]["cost"][s], coll["cost"]), (s, "costs")
        assert np.array_equal(gpu["coll"]["feas"][s], coll["feas"]), (s, "feasibility")
        assert int(gpu["rollout_count"][s]) == ref["rollout_count"]
        assert int(gpu["feasible_count"][s]) == ref["feasible_count"]
        if name == "lpr1":
            assert 257 < ref["rollout_count"] < p.K + 1  # the prefix ends inside the partial block
        else:
            assert 0 < coll["feas"].sum() < p.K
        # the final rollout, from the device's own MPPICtrl
        U = gpu["U"][s]
        st = cases.setting(c, s)
        traj, _, feas, cost = mppi_ref.TrajectoryRollout(st, [[float(a), float(b)] for a, b in U])
        assert _same(gpu["traj"][s], np.array(traj)), (s, "final trajectory")
        assert _same(gpu["cost"][s], cost), (s, "final cost")
        assert bool(gpu["feasible"][s]) == feas
        # MPPICtrl against the exact value
        m = ref["rollout_count"] - 1
        Ustar, bound = cases.exact_mppictrl(coll["cost"][:m], coll["ctrl"][:m], p.lambda_)
        ratio = cases.error_ratio(U, Ustar, bound)
        seq = cases.error_ratio(ref["U"], Ustar, bound)
        print("%s env %d scene %d: m = %d, MPPICtrl error / bound: device %.4f, sequential fold %.4f"
              % (name, ienv, s, m, ratio, seq))
        assert ratio <= 1.0, (s, ratio)
