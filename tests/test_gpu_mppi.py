"""GPU parity: libmpgpu's MPPI / rollout / plant kernels vs the CPU oracle and the golden fixtures.

Tolerances (floating point, fp64 like the reference):
  * rollout costs, trajectories, feasibility flags, RolloutCount: BIT-EXACT vs the oracle
    (same FDLIBM libm, no FMA contraction, same evaluation order);
  * MPPICtrl (weighted control): rtol 1e-9 / atol 1e-12 — the device combines
    per-block online-softmax partials (exp(a)·exp(b) vs exp(a+b), tree sums) where the
    reference sums sequentially ("<= 1e-9 for weighted controls");
  * final trajectory / cost (rolled out from MPPICtrl): rtol 1e-9.

mp_rollout and mp_vehicle_euler appear here only through the two CSV replays (DWAPlan's one call shape, the
100-step plant); their direct parity with the oracle -- per-step and batched controls, ragged K, every output,
the argmin's ties and NaN order, the plant's partial blocks -- lives in tests/test_gpu_rollout.py.
"""
import os

import numpy as np
import pytest

import oracle
from motionplanning_amd import configs
from motionplanning_amd.abi import MP_NOISE_PHILOX
from motionplanning_amd.mppi import mppi_plan_batch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _check_plan(gpu, ref, s=0, coll=True):
    if coll:
        assert np.array_equal(gpu["coll"]["cost"][s], ref["coll"]["cost"])
        assert np.array_equal(gpu["coll"]["feas"][s], ref["coll"]["feas"])
        assert np.array_equal(gpu["coll"]["ctrl"][s], ref["coll"]["ctrl"])
        assert np.array_equal(gpu["coll"]["traj"][s], ref["coll"]["traj"])
    assert int(gpu["rollout_count"][s]) == ref["rollout_count"]
    assert int(gpu["feasible_count"][s]) == ref["feasible_count"]
    np.testing.assert_allclose(gpu["U"][s], ref["U"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gpu["traj"][s], ref["traj"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(gpu["cost"][s], ref["cost"], rtol=1e-9)
    assert bool(gpu["feasible"][s]) == ref["feasible"]


def test_cfg1_external_noise(ctx):
    c = configs.cfg1()
    p = c["params"]
    z = configs.standard_noise(p.K, p.H)
    gpu = mppi_plan_batch(p, c["X0"][None], c["goal"][None], c["unom"][None], c["obstacles"][None], None, z[None],
                          collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, c["X0"], c["goal"], c["unom"], c["obstacles"], None, z, collect=True)
    _check_plan(gpu, ref)


def test_reference_defaults_nonzero_nominal(ctx):
    """MPPI/main.jl settings (K=1500, N=20, 3 circles) with a non-zero nominal control,
    exercising the λ u_nomᵀΣ⁻¹(u−u_nom) term and K not a multiple of the block size."""
    p = configs.mppi_params(K=1500, H=20, T=3.0, n_obs=3)
    r = np.random.default_rng(11)
    unom = np.c_[r.uniform(-0.2, 0.2, 20), r.uniform(-1, 1, 20)]
    X0 = np.array([3.0, 0.5, 0.1, 0.02, 0.05, 6.0, 0.01])
    z = r.standard_normal((1500, 20, 2))
    obs = np.array(configs.OBSTACLES_REF)
    gpu = mppi_plan_batch(p, X0[None], np.array(configs.GOAL_REF)[None], unom[None], obs[None], None, z[None],
                          collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, X0, np.array(configs.GOAL_REF), unom, obs, None, z, collect=True)
    _check_plan(gpu, ref)


@pytest.mark.parametrize("fc", [0, 7, 300, 1299])
def test_feasibility_count_prefix(ctx, fc):
    """MPPIUtils.jl:175 early stop: only the first m rollouts enter the weights."""
    p = configs.mppi_params(K=1500, H=20, T=3.0, n_obs=3, feasibility_count=fc)
    z = configs.standard_noise(1500, 20, seed=5)
    obs = np.array(configs.OBSTACLES_REF)
    X0, goal, un = np.array(configs.X0_REF), np.array(configs.GOAL_REF), np.zeros((20, 2))
    gpu = mppi_plan_batch(p, X0[None], goal[None], un[None], obs[None], None, z[None], collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, X0, goal, un, obs, None, z, collect=True)
    assert ref["rollout_count"] - 1 < 1500 or fc >= 1300
    _check_plan(gpu, ref)


@pytest.mark.parametrize("fc", [0, 300])
def test_philox_feasibility_prefix(ctx, fc):
    """Device Philox noise drawn inside the rollout loop + the FeasibilityCount boundary block
    (whose controls phase 2 regenerates from the same counters)."""
    p = configs.mppi_params(K=1500, H=21, T=3.0, n_obs=3, feasibility_count=fc, noise_mode=MP_NOISE_PHILOX,
                            seed=99, offset=4)
    obs = np.array(configs.OBSTACLES_REF)
    X0, goal, un = np.array(configs.X0_REF), np.array(configs.GOAL_REF), np.zeros((21, 2))
    gpu = mppi_plan_batch(p, X0[None], goal[None], un[None], obs[None], None, None, collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, X0, goal, un, obs, None, None, collect=True)
    _check_plan(gpu, ref)


def test_philox_mode_matches_oracle(ctx):
    c = configs.cfg1()
    p = c["params"]
    p.seed, p.offset = 1234567, 3
    gpu = mppi_plan_batch(p, c["X0"][None], c["goal"][None], c["unom"][None], c["obstacles"][None], None, None,
                          collect=True, ctx=ctx)
    assert p.noise_mode == MP_NOISE_PHILOX
    ref = oracle.mppi_plan(p, c["X0"], c["goal"], c["unom"], c["obstacles"], None, None, collect=True)
    _check_plan(gpu, ref)
    # the draws are standard normal
    z = np.array([oracle.philox_normal2(7, 0, 0, k, h) for k in range(200) for h in range(20)]).ravel()
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05


def test_multi_scene(ctx):
    p = configs.mppi_params(K=300, H=25, T=3.75, n_obs=5)
    r = np.random.default_rng(2)
    S = 4
    X0 = np.tile(configs.X0_REF, (S, 1))
    X0[:, 0] = [0, 10, 25, 40]
    X0[:, 1] = r.uniform(-1, 1, S)
    goal = np.tile(configs.GOAL_REF, (S, 1))
    un = r.uniform(-0.1, 0.1, (S, 25, 2))
    obs = np.stack([np.array(configs.OBSTACLES_CFG1) + [[r.uniform(-2, 2), 0, 0]] for _ in range(S)])
    z = r.standard_normal((S, 300, 25, 2))
    gpu = mppi_plan_batch(p, X0, goal, un, obs, None, z, collect=True, ctx=ctx)
    for s in range(S):
        ref = oracle.mppi_plan(p, X0[s], goal[s], un[s], obs[s], None, z[s], collect=True)
        _check_plan(gpu, ref, s)


def test_cfg2_grid_full_size(ctx):
    """BASELINE configs[1]: K=8192, H=50, occupancy grid — full-size parity."""
    c = configs.cfg2()
    p = c["params"]
    z = configs.standard_noise(p.K, p.H)
    gpu = mppi_plan_batch(p, c["X0"][None], c["goal"][None], c["unom"][None], None, c["grid"][None], z[None],
                          collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, c["X0"], c["goal"], c["unom"], None, c["grid"], z, collect=True)
    _check_plan(gpu, ref)
    # size-independent properties: controls inside [CL, CU] hull, determinism
    U = gpu["U"][0]
    assert (U[:, 0] >= p.CL[0] - 1e-12).all() and (U[:, 0] <= p.CU[0] + 1e-12).all()
    again = mppi_plan_batch(p, c["X0"][None], c["goal"][None], c["unom"][None], None, c["grid"][None], z[None],
                            collect=False, ctx=ctx)
    assert np.array_equal(again["U"], gpu["U"]) and np.array_equal(again["cost"], gpu["cost"])


def test_dwa_closed_loop_matches_reference_csv(ctx):
    """The whole DynamicWindow/main.jl closed loop on the device (rollout kernel + argmin +
    Euler plant kernel) reproduces DWATrajectory.csv bit for bit."""
    from motionplanning_amd.dwa import run_dwa_closed_loop

    g = np.load(os.path.join(GOLD, "dwa_closed_loop.npz"))
    rows, picks = run_dwa_closed_loop(ctx=ctx)
    assert rows.shape[0] == int(g["n_rows"])
    assert np.array_equal(picks // 41 + 1, g["i_sr"]) and np.array_equal(picks % 41 + 1, g["i_ax"])
    assert np.array_equal(rows[g["step_index"]], g["rows"])


def test_plant_replay_mppi_csv(ctx):
    from motionplanning_amd.rollout import vehicle_euler

    g = np.load(os.path.join(GOLD, "mppi_plant.npz"))
    ctrl = g["block_ctrl"]
    starts = g["replan_states"]
    n = 100
    s, his = vehicle_euler(starts[:-1], ctrl[:-1], 1e-3, n, ctx=ctx)
    for b in range(len(ctrl) - 1):
        _, ref = oracle.vehicle_euler(starts[b], ctrl[b], 1e-3, n)
        assert np.array_equal(his[b], ref)
    # and against the CSV rows at block ends
    idx = g["step_index"]
    rows = g["rows"]
    for b in range(len(ctrl) - 1):
        j = np.where(idx == (b + 1) * 100)[0]
        if len(j):
            assert np.abs(his[b, -1] - rows[j[0], 1:]).max() < 1e-12


EXP_EDGES = np.array([0.34657359027997264, 0.3465735902799727, 1.0397207708399179, 1.039720770839918, 7.450580596923828e-09,
                      3.725290298461914e-09, 703.9, -703.9, 704.0, -708.4, 709.78, -745.2, 800.0, np.inf, -np.inf,
                      0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 5.23, -10.47])
TAN_EDGES = np.array([0.6743884, 0.67438866, -0.67438866, 0.7853981633974483, -0.7853981633974483,
                      0.7853981633974484, 1e-9, -1e-9, 0.5235987755982988, -0.5235987755982988, 1.2, -3.0])
ATAN2_EDGES = np.array([(0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (2.0, 1.0), (1e-300, 1e300),
                        (1e300, 1e-300), (np.inf, 1.0), (1.0, np.inf), (np.inf, -np.inf), (3.0, 3.0), (-2.0, 2.0),
                        (1e-17, -1.0), (-1e-17, -1.0), (1.0, 1e-17), (-3.0, -3.0)])


def test_jlmath_bitexact(ctx):
    """Every device libm routine (exact FDLIBM restatements and the branch-free variants of the hot
    kernels) equals the CPU build bit for bit, incl. range edges and the kπ/2 Cody-Waite points."""
    from motionplanning_amd.abi import ptr

    r = np.random.default_rng(0)
    ranges = {0: (-30, 30), 1: (-30, 30), 2: (-1.5, 1.5), 3: (-60, 60), 4: (-5, 5), 5: (-1, 1), 6: (-1, 1),
              7: (-700, 700), 8: (1e-300, 1e4), 9: (-40, 40), 10: (0, 1e6), 11: (-15, 15), 12: (-60, 60),
              13: (-60, 60), 14: (-10, 10), 15: (-10, 10), 16: (-720, 720), 17: (-1.0, 1.0), 18: (-5, 5),
              19: (-1e6, 1e6), 20: (-12, 12), 21: (-12, 12), 22: (-2.3, 2.3), 23: (1e-17, 1.0)}
    names = {0: "sin", 1: "cos", 2: "tan", 3: "atan", 4: "atan2", 5: "asin", 6: "acos", 7: "exp", 8: "log",
             9: "modpi", 11: "modpi", 12: "atan", 13: "atan", 14: "sin", 15: "cos", 16: "exp_fdlibm", 17: "tan",
             18: "atan2", 19: "sin", 20: "cos", 21: "tan", 22: "sin", 23: "log"}
    edges = np.array([0.0, -0.0, 1e-300, -1e-300, 0.4375, 0.6875, 1.1875, 2.4375, np.pi / 4, np.pi / 2, np.pi,
                      2 * np.pi, 3 * np.pi / 4, 4 * np.pi, -4 * np.pi, 1e5, -1e5] +  # |x| < 2^20 pi/2 (Cody-Waite domain)
                     [np.nextafter(k * np.pi / 2, d) for k in range(-6, 7) for d in (-np.inf, np.inf)])
    for fn, (lo, hi) in ranges.items():
        x = np.r_[r.uniform(lo, hi, 20000), edges if fn in (11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22) else [],
                  EXP_EDGES if fn == 16 else [], TAN_EDGES if fn in (17, 21) else []]
        y = r.uniform(-5, 5, len(x))
        if fn == 18:
            y[:len(ATAN2_EDGES)] = ATAN2_EDGES[:, 1]
            x[:len(ATAN2_EDGES)] = ATAN2_EDGES[:, 0]
        out = np.zeros_like(x)
        ctx.check(ctx.lib.mp_math_eval(ctx.handle, fn, len(x), ptr(x), ptr(y), ptr(out)))
        if fn == 10:
            assert np.array_equal(out, np.sqrt(x))
            continue
        cpu = np.array([oracle.m(names[fn], a, b) if fn in (4, 18) else oracle.m(names[fn], a) for a, b in zip(x, y)])
        assert np.array_equal(out.view(np.int64), cpu.view(np.int64)), (fn, names[fn], x[out.view(np.int64) != cpu.view(np.int64)][:5])


@pytest.mark.parametrize("base", [0, 8, 16, 24, 32, 40, 48, 56])
def test_bench_workload_full_size_bitexact(ctx, base):
    """The headline bench workload itself (bench.py run(): configs[4] per-GPU shard = 8 of the 64 scenes,
    each configs[1], K=8192, H=50, its own X0 and its own occupancy grid from obstacle_field.mat field g+1
    (every rank's shard of the world-8 job: fields base+1..base+8), device Philox noise seeded 20260415, step offset 3,
    final rollout on the side stream) vs 8 oracle MPPIPlan solves with the same Philox stream (threaded):
    every rollout's cost, feasibility, controls and states bit for bit, MPPICtrl / final trajectory within
    the stated tolerance."""
    from concurrent.futures import ThreadPoolExecutor

    from motionplanning_amd.abi import MP_NOISE_PHILOX

    S = 8
    c = configs.cfg5_shard(base, S, noise_mode=MP_NOISE_PHILOX, seed=20260415)
    p = c["params"]
    p.offset = 3
    p.final_stream = 1
    X0, goal, grid = c["X0"], c["goal"], c["grid"]
    assert len({g.tobytes() for g in grid}) == S, "every scene has its own obstacle set"
    gpu = mppi_plan_batch(p, X0, goal, np.zeros((S, p.H, 2)), None, grid, None, collect=True, ctx=ctx)

    def ref(s):
        return oracle.mppi_plan(p, X0[s], goal[s], np.zeros((p.H, 2)), None, grid[s], None, scene=s, collect=True)

    with ThreadPoolExecutor(8) as ex:
        refs = list(ex.map(ref, range(S)))
    for s in range(S):
        _check_plan(gpu, refs[s], s=s)


@pytest.mark.parametrize("base", [0, 56])
def test_bench_workload_in_flight_bitexact(ctx, base):
    """The headline workload as bench.py runs it with two calls in flight (calls_in_flight = 2: the launch takes
    the one-rollout-per-lane layout whose waves share the CUs with the other call's) -- the same checks against
    the oracle as test_bench_workload_full_size_bitexact."""
    from concurrent.futures import ThreadPoolExecutor

    from motionplanning_amd.abi import MP_NOISE_PHILOX

    S = 8
    c = configs.cfg5_shard(base, S, noise_mode=MP_NOISE_PHILOX, seed=20260415)
    p = c["params"]
    p.calls_in_flight = 2
    p.offset = 5
    p.final_stream = 1
    X0, goal, grid = c["X0"], c["goal"], c["grid"]
    gpu = mppi_plan_batch(p, X0, goal, np.zeros((S, p.H, 2)), None, grid, None, collect=True, ctx=ctx)

    def ref(s):
        return oracle.mppi_plan(p, X0[s], goal[s], np.zeros((p.H, 2)), None, grid[s], None, scene=s, collect=True)

    with ThreadPoolExecutor(8) as ex:
        refs = list(ex.map(ref, range(S)))
    for s in range(S):
        _check_plan(gpu, refs[s], s=s)


def test_scene_batching_invariance(ctx):
    """Sharding correctness on the device: a scene planned inside an 8-scene launch equals the same scene
    planned alone with scene_base = its global index (the Philox counter word a rank of a sharded job
    passes), bit for bit, while both launches use the same layout (here K=1024: lane pairs, 256-thread
    blocks).  Across layouts see test_scene_batching_across_layouts."""
    import ctypes as _ct

    from motionplanning_amd.abi import MP_NOISE_PHILOX, MPPIParams

    S = 8
    c = configs.cfg2(noise_mode=MP_NOISE_PHILOX, seed=77)
    p = c["params"]
    p.K = 1024
    X0 = np.tile(c["X0"], (S, 1))
    X0[:, 1] = np.linspace(-0.5, 0.5, S)
    goal = np.tile(c["goal"], (S, 1))
    grid = np.tile(c["grid"], (S, 1, 1))
    whole = mppi_plan_batch(p, X0, goal, np.zeros((S, p.H, 2)), None, grid, None, collect=True, ctx=ctx)
    for s in (0, 3, 7):
        q = MPPIParams()
        _ct.pointer(q)[0] = p
        q.scene_base = s
        one = mppi_plan_batch(q, X0[s:s + 1], goal[s:s + 1], np.zeros((1, p.H, 2)), None, grid[s:s + 1], None,
                              collect=True, ctx=ctx)
        for key in ("cost", "feas", "ctrl", "traj"):
            assert np.array_equal(one["coll"][key][0], whole["coll"][key][s]), (s, key)
        assert np.array_equal(one["U"][0], whole["U"][s]) and one["cost"][0] == whole["cost"][s]


def test_scene_batching_across_layouts(ctx):
    """configs[4] at full size: the 64 scenes planned as eight 8-scene launches (each rank's shard:
    lane pairs, 512-thread blocks) and as one 64-scene launch (one rollout per lane).  The launch layout
    follows S*K (mppi.hip plan_launch), and the log-sum-exp combine of MPPICtrl sums block partials whose
    grouping follows the layout, so:
      * every rollout (noise, costs, feasibility flags) and the counts are bit-identical;
      * MPPICtrl, the final trajectory and its cost agree within the stated tolerance (rtol 1e-9), not
        bit for bit."""
    from motionplanning_amd.abi import MP_NOISE_PHILOX

    c = configs.cfg5_shard(0, 64, noise_mode=MP_NOISE_PHILOX, seed=20260415)
    p = c["params"]
    p.offset = 5
    X0, goal, grid = c["X0"], c["goal"], c["grid"]
    un = np.zeros((64, p.H, 2))
    whole = mppi_plan_batch(p, X0, goal, un, None, grid, None, collect="costs", ctx=ctx)
    base0 = p.scene_base
    for a in range(0, 64, 8):
        p.scene_base = base0 + a
        part = mppi_plan_batch(p, X0[a:a + 8], goal[a:a + 8], un[a:a + 8], None, grid[a:a + 8], None,
                               collect="costs", ctx=ctx)
        sl = slice(a, a + 8)
        assert np.array_equal(part["coll"]["cost"], whole["coll"]["cost"][sl]), a
        assert np.array_equal(part["coll"]["feas"], whole["coll"]["feas"][sl]), a
        assert np.array_equal(part["rollout_count"], whole["rollout_count"][sl])
        assert np.array_equal(part["feasible_count"], whole["feasible_count"][sl])
        np.testing.assert_allclose(part["U"], whole["U"][sl], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(part["traj"], whole["traj"][sl], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(part["cost"], whole["cost"][sl], rtol=1e-9)
        assert np.array_equal(part["feasible"], whole["feasible"][sl])
    p.scene_base = base0


def test_cfg2_default_feasibility_count_full_size(ctx):
    """configs[1] at full size (K=8192, H=50, grid) with the reference's default FeasibilityCount = 1300
    (types.jl:24, MPPIUtils.jl:175): the prefix stops at the 1301st feasible rollout, so only the first m
    rollouts enter the weights and RolloutCount = m + 1 -- bit-exact collection, exact counts."""
    c = configs.cfg2(feasibility_count=configs.FEASIBILITY_COUNT_REF)
    p = c["params"]
    assert p.feasibility_count == 1300
    z = configs.standard_noise(p.K, p.H, seed=8)
    gpu = mppi_plan_batch(p, c["X0"][None], c["goal"][None], c["unom"][None], None, c["grid"][None], z[None],
                          collect=True, ctx=ctx)
    ref = oracle.mppi_plan(p, c["X0"], c["goal"], c["unom"], None, c["grid"], z, collect=True)
    assert ref["feasible_count"] == 1301 and ref["rollout_count"] - 1 < p.K, (ref["feasible_count"],
                                                                             ref["rollout_count"])
    _check_plan(gpu, ref)


def test_ctx_destroy_refused_inside_communicator():
    """mp_ctx_destroy refuses a context that still belongs to an RCCL communicator (a dangling
    rank otherwise); after mp_comm_destroy the same context closes normally."""
    from motionplanning_amd.abi import MPGPUError
    from motionplanning_amd.context import CommGroup

    g = CommGroup([0])
    try:
        with pytest.raises(MPGPUError, match="mp_comm_destroy"):
            g.ctxs[0].close()
        assert g.ctxs[0].handle  # still valid
    finally:
        g.close()
    assert g.ctxs[0].handle is None


def test_sharded_plan_one_gpu_equals_plan(ctx):
    """mp_comm_init + mp_mppi_plan_sharded over a one-GPU communicator (RCCL all-gather with one rank)
    equals mp_mppi_plan of the same scenes bit for bit (U, final trajectory, cost, flags, counts).
    n > 1 needs a multi-GPU box (not available to these tests)."""
    from motionplanning_amd.context import CommGroup
    from motionplanning_amd.mppi import mppi_plan_sharded

    S = 3
    c = configs.cfg5_shard(5, S, noise_mode=MP_NOISE_PHILOX, seed=31)
    p = c["params"]
    p.K = 2048
    g = CommGroup([0])
    try:
        for fs in (0, 1):
            p.final_stream = fs
            sh = mppi_plan_sharded(g, p, c["X0"], c["goal"], c["unom"], None, c["grid"])
            one = mppi_plan_batch(p, c["X0"], c["goal"], c["unom"], None, c["grid"], None, ctx=ctx)
            for k in ("U", "traj", "cost", "feasible", "rollout_count", "feasible_count"):
                assert np.array_equal(sh[k], one[k]), (fs, k)
    finally:
        g.close()


def test_searcher_object_api(ctx):
    """The drop-in searcher surface (MPPIUtils.jl:169-203, types.jl:3-8): MPPIPlan(mppi) mutates mppi.r
    (Control, Traj, Feasibility, cost, RolloutCount, FeasibleTrajCount) and mppi.p.TrajectoryCollection[1:m];
    TrajectoryRollout(mppi, ctrl) returns (states_his, ctrl, constraint, cost); MPPIClosedLoop(mppi) leaves
    the last plan in mppi.r -- each checked field by field against the oracle on the same noise."""
    from motionplanning_amd import mppi

    m = mppi.reference_searcher(K=1500, N=20)
    m.s.FeasibilityCount = 700  # a prefix that stops early: TrajectoryCollection has m < K holders
    r = np.random.default_rng(4)
    un = np.c_[r.uniform(-0.1, 0.1, 20), r.uniform(-0.5, 0.5, 20)]
    mppi.defineMPPINominalControl_(m, un)
    z = r.standard_normal((1500, 20, 2))
    p = mppi.params_of(m, 0)
    ref = oracle.mppi_plan(p, m.s.X0, m.s.goal, un, np.array(m.s.obstacle_list), None, z, collect=True)
    assert mppi.MPPIPlan(m, noise=z, ctx=ctx) is None
    mm = ref["rollout_count"] - 1
    assert m.r.RolloutCount == ref["rollout_count"] and m.r.FeasibleTrajCount == ref["feasible_count"]
    assert m.r.Feasibility == ("Feasible" if ref["feasible"] else "InFeasible")
    np.testing.assert_allclose(m.r.Control, ref["U"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(m.r.Traj, ref["traj"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(m.r.cost, ref["cost"], rtol=1e-9)
    assert len(m.p.TrajectoryCollection) == mm < 1500
    for i in (0, 1, mm // 2, mm - 1):
        h = m.p.TrajectoryCollection[i]
        assert np.array_equal(h.Trajectory, ref["coll"]["traj"][i])
        assert np.array_equal(h.Control, ref["coll"]["ctrl"][i])
        assert h.Feasibility == bool(ref["coll"]["feas"][i]) and h.cost == ref["coll"]["cost"][i]
    # TrajectoryRollout(mppi, ctrl) of one control list (MPPIUtils.jl:31-57): the collection's holder i
    i = mm // 3
    sh, cl, feas, cost = mppi.TrajectoryRollout(m, ref["coll"]["ctrl"][i], ctx=ctx)
    assert np.array_equal(sh, ref["coll"]["traj"][i]) and np.array_equal(cl, ref["coll"]["ctrl"][i])
    assert feas == bool(ref["coll"]["feas"][i]) and cost == ref["coll"]["cost"][i]
    # MPPIClosedLoop(mppi): 0.3 s of main.jl's loop (3 replans) with given noise, last plan in mppi.r
    m2 = mppi.reference_searcher(K=1500, N=20)
    zz = r.standard_normal((3, 1500, 20, 2))
    his = mppi.MPPIClosedLoop(m2, sim_time=0.3, noise=zz, ctx=ctx)
    upd, hold = configs.mppi_hold_index(3.0, 20)
    p2 = mppi.params_of(m2, 0)
    o = oracle.mppi_closed_loop(p2, np.array(configs.X0_REF), np.array(configs.GOAL_REF), np.zeros((20, 2)), hold,
                                upd, 300, 1e-3, 6.0, obstacles=np.array(configs.OBSTACLES_REF), noise=zz)
    assert his.shape == (301, 8) and o["n_replans"] == 3
    np.testing.assert_allclose(his, o["his"], rtol=0, atol=1e-9)
    assert m2.r.RolloutCount == o["rollout_count"][-1]
    np.testing.assert_allclose(m2.r.Control, m2.r.log["Control"][-1], rtol=0, atol=0)
