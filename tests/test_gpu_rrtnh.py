"""GPU parity of the car-like RRT / RRT* kernel (motionplanning_amd/csrc/rrtnh.hip: mp_rrtnh_plan) against the CPU
restatement tests/rrtnh_ref.py -- BIT-EXACT tree (state, cost, parent), node counts, status, best node and cost,
path and the eight branch counters.  Each test is one or two calls of at most 600 iterations; before comparing,
each asserts on the reference's counters that the branch it is about was taken."""
import functools
import os

import numpy as np
import pytest

import rrt_ref
import rrtnh_ref as R
from motionplanning_amd import abi, rrt_nonholonomic as nh
from motionplanning_amd.abi import RRTParams, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "obstacle_fields_64.npz")
BOUND = [0.0, 120.0, 0.0, 120.0]
BLOCK_ALL = [60.0, 60.0, 1e3]  # a circle over the whole field: padding that must not be read
LDS_SET = 256                  # rrtnh.hip NH_SET: in-disk candidates the kernel keeps in LDS
REJ_BOUND, REJ_KIN, REJ_CIRCLE, REWIRED, CAPPED, IN_RANGE, DREW, SMALL_R = range(8)


@functools.lru_cache(maxsize=None)
def fields():
    z = np.load(GOLD)
    return z["circles"], z["count"]


def field(k):
    return rrt_ref.field(*fields(), k)


def uniforms(seed, n_iter):
    return np.random.default_rng(seed).random((n_iter, 6))


def params(n_iter, buffer_size, rrt_star, bias_rate=0.2, grow=(1.0, 3.0), tol=1.0):
    return RRTParams(n_iter=n_iter, buffer_size=buffer_size, rrt_star=int(rrt_star), reserved=0, bias_rate=bias_rate,
                     grow_min=grow[0], grow_max=grow[1], goal_tolerance=tol)


def gpu_plan(ctx, p, scenes, use_count=True, check=True):
    """mp_rrtnh_plan; scenes = [(bound, start pose, goal, obstacles, uniforms [n_iter][6])].  Obstacle lists are
    padded to the longest with BLOCK_ALL and go with obs_count (use_count=False: every list has the same length)."""
    B, cap = len(scenes), p.n_iter + 1
    bound = np.ascontiguousarray([s[0] for s in scenes], np.float64)
    start = np.ascontiguousarray([s[1] for s in scenes], np.float64)
    goal = np.ascontiguousarray([s[2] for s in scenes], np.float64)
    count = np.array([len(s[3]) for s in scenes], np.int32)
    n_obs = int(count.max())
    obs = np.tile(np.array(BLOCK_ALL), (B, max(n_obs, 1), 1))[:, :n_obs].copy()
    for b, s in enumerate(scenes):
        if count[b]:
            obs[b, : count[b]] = np.asarray(s[3], np.float64)
    assert use_count or (count == n_obs).all()
    uni = np.ascontiguousarray([s[4] for s in scenes], np.float64).reshape(B, max(p.n_iter, 0), 6)
    out = dict(n_nodes=np.zeros(B, np.int32), status=np.zeros(B, np.int32), best_idx=np.zeros(B, np.int32),
               best_cost=np.zeros(B), state=np.zeros((B, max(cap, 1), 3)), cost=np.zeros((B, max(cap, 1))),
               parent=np.zeros((B, max(cap, 1)), np.int32), path_idx=np.zeros((B, max(cap, 1)), np.int32),
               path_n=np.zeros(B, np.int32), counters=np.zeros((B, 8), np.int32))
    st = ctx.lib.mp_rrtnh_plan(ctx.handle, p, B, ptr(bound), ptr(start), ptr(goal), n_obs,
                               ptr(count) if use_count else None, ptr(obs) if n_obs else None, ptr(uni),
                               ptr(out["n_nodes"]), ptr(out["status"]), ptr(out["best_idx"]), ptr(out["best_cost"]),
                               ptr(out["state"]), ptr(out["cost"]), ptr(out["parent"]), ptr(out["path_idx"]),
                               ptr(out["path_n"]), ptr(out["counters"]))
    if check:
        ctx.check(st)
    out["st"] = st
    return out


def ref_plan(p, scene):
    b, s, g, obs, U = scene
    return R.plan(b, s, g, obs, U, p.buffer_size, bool(p.rrt_star), p.bias_rate, p.grow_min, p.grow_max,
                  p.goal_tolerance)


def check_against_ref(out, b, ref):
    n = ref["n_nodes"]
    assert out["n_nodes"][b] == n, (b, out["n_nodes"][b], n)
    assert list(out["counters"][b]) == list(ref["counters"]), (b, out["counters"][b], ref["counters"])
    assert (out["parent"][b] == ref["parent"]).all(), b
    assert out["state"][b].tobytes() == ref["state"].tobytes(), b
    assert out["cost"][b].tobytes() == ref["cost"].tobytes(), b
    assert out["status"][b] == ref["status"] and out["best_idx"][b] == ref["best_idx"], b
    assert out["best_cost"][b].tobytes() == np.float64(ref["best_cost"]).tobytes(), b
    k = len(ref["path_idx"])
    assert out["path_n"][b] == k and list(out["path_idx"][b, :k]) == list(ref["path_idx"]), b
    assert (out["path_idx"][b, k:] == 0).all(), b


# ---- the main batch: B = 4 different fields, seeds, start headings and goals; a fifth scene with buffer_size = 13
# is its own call
def main_scenes():
    return [(BOUND, [0.0, 0.0, 0.0], [30.0, 10.0], field(53), uniforms(1, 600)),
            (BOUND, [0.0, 0.0, 0.0], [25.0, 10.0], field(4), uniforms(1, 600)),
            (BOUND, [0.0, 0.0, 0.7], [20.0, 20.0], field(17), uniforms(1, 600)),
            (BOUND, [0.0, 0.0, 0.7], [15.0, 25.0], field(9), uniforms(1, 600))]


def buf13_scene():
    return (BOUND, [0.0, 0.0, 0.0], [35.0, 5.0], field(53), uniforms(5, 600))


# plain RRT: the same shapes on other seeds.  Poses do not depend on costs, so on the star batch's seeds a read of a
# stale workspace slot would return the expected value
def plain_scenes():
    return [s[:4] + (uniforms(seed, 600),) for s, seed in zip(main_scenes(), (101, 101, 101, 101))]


def plain_buf13_scene():
    return buf13_scene()[:4] + (uniforms(101, 600),)


@functools.lru_cache(maxsize=None)
def main_refs(rrt_star):
    scenes, s13 = (main_scenes(), buf13_scene()) if rrt_star else (plain_scenes(), plain_buf13_scene())
    return [ref_plan(params(600, 7, rrt_star), s) for s in scenes], ref_plan(params(600, 13, rrt_star), s13)


def main_conditions():
    refs, ref13 = main_refs(True)
    for r in refs + [ref13]:  # the reference takes every branch in every scene
        c, near_sets = r["counters"], r["n_nodes"] - 1
        assert c[REWIRED] >= 1 and c[CAPPED] >= 1 and near_sets - c[CAPPED] >= 1 and c[REJ_KIN] >= 1, c
        assert c[IN_RANGE] >= 1 and c[DREW] >= 1 and 600 - c[DREW] >= 1, c
        assert c[CAPPED] >= 1 and 30 <= r["max_disk"] <= LDS_SET, r["max_disk"]  # ranked in LDS
    assert sum(r["status"] for r in refs + [ref13]) >= 2
    return refs, ref13


def test_rrt_star_main_batch_bitexact(ctx):
    refs, ref13 = main_conditions()
    out = gpu_plan(ctx, params(600, 7, True), main_scenes())
    for b, r in enumerate(refs):
        check_against_ref(out, b, r)
    out = gpu_plan(ctx, params(600, 13, True), [buf13_scene()])
    check_against_ref(out, 0, ref13)


def plain_conditions():
    refs, ref13 = main_refs(False)
    for r in refs + [ref13]:
        c = r["counters"]
        assert c[REWIRED] == 0 and c[CAPPED] == 0 and c[SMALL_R] == 0 and r["n_nodes"] > 100 and c[REJ_KIN] >= 1, c
    return refs, ref13


def test_plain_rrt_bitexact(ctx):
    refs, ref13 = plain_conditions()
    # the tree workspace is first filled by other trees of the same shape: nothing of them may show below
    gpu_plan(ctx, params(600, 7, True), main_scenes())
    out = gpu_plan(ctx, params(600, 7, False), plain_scenes())
    for b, r in enumerate(refs):
        check_against_ref(out, b, r)
    assert (out["counters"][:, [REWIRED, CAPPED, SMALL_R]] == 0).all()
    gpu_plan(ctx, params(600, 13, True), [buf13_scene()])
    out = gpu_plan(ctx, params(600, 13, False), [plain_buf13_scene()])
    check_against_ref(out, 0, ref13)


@functools.lru_cache(maxsize=None)
def circle_case():
    # circles 4 to 8 m ahead of the start pose: the first steps forward end inside them
    p = params(600, 7, True)
    s = (BOUND, [10.0, 10.0, 0.0], [40.0, 20.0], [(16.0, 10.0, 2.0), (10.0, 18.0, 2.5), (22.0, 4.0, 1.5)],
         uniforms(13, 600))
    ref = ref_plan(p, s)
    assert ref["counters"][REJ_CIRCLE] >= 10 and ref["n_nodes"] >= 20, (ref["counters"], ref["n_nodes"])
    return p, s, ref


def test_circle_rejections_bitexact(ctx):
    p, s, ref = circle_case()
    check_against_ref(gpu_plan(ctx, p, [s]), 0, ref)


@functools.lru_cache(maxsize=None)
def small_radius_case():
    # a 4 m x 4 m bound: gamma * log(n) / n falls below the cap of 24 once the tree has a few hundred nodes
    p = params(600, 7, True)
    s = ([0.0, 4.0, 0.0, 4.0], [0.5, 2.0, 0.0], [3.5, 2.0], [], uniforms(21, 600))
    ref = ref_plan(p, s)
    assert ref["counters"][SMALL_R] >= 10 and ref["counters"][REWIRED] >= 1, ref["counters"]
    return p, s, ref


def test_radius_below_the_cap_bitexact(ctx):
    p, s, ref = small_radius_case()
    check_against_ref(gpu_plan(ctx, p, [s]), 0, ref)


@functools.lru_cache(maxsize=None)
def wide_case():
    # an empty 20 m x 20 m field: the in-disk set outgrows the candidates the kernel keeps in LDS, and the 30
    # smallest come from its threshold search over the stored metric values
    p = params(600, 7, True)
    s = ([0.0, 20.0, 0.0, 20.0], [1.0, 10.0, 0.0], [18.0, 10.0], [], uniforms(32, 600))
    ref = ref_plan(p, s)
    assert ref["max_disk"] > LDS_SET and ref["counters"][CAPPED] > 200 and ref["counters"][REWIRED] >= 1
    return p, s, ref


def test_candidate_set_larger_than_lds_bitexact(ctx):
    p, s, ref = wide_case()
    check_against_ref(gpu_plan(ctx, p, [s]), 0, ref)


@functools.lru_cache(maxsize=None)
def pile_case():
    # bias 1.0: every sample is the goal under another heading, and the tree piles up around it
    p = params(600, 7, True, bias_rate=1.0)
    s = (BOUND, [0.0, 0.0, 0.0], [15.0, 3.0], [], uniforms(31, 600))
    ref = ref_plan(p, s)
    assert ref["status"] == 1 and ref["counters"][REWIRED] >= 100 and ref["counters"][CAPPED] >= 300, ref["counters"]
    assert ref["max_disk"] > LDS_SET  # the search beyond LDS a second time, on a crowded disk
    return p, s, ref


def test_goal_pile_bitexact(ctx):
    p, s, ref = pile_case()
    check_against_ref(gpu_plan(ctx, p, [s]), 0, ref)


# ---- edges: each its own small call
def run_edge(ctx, p, scenes, use_count=True):
    refs = edge_refs(p, scenes)
    out = gpu_plan(ctx, p, scenes, use_count)
    for b, r in enumerate(refs):
        check_against_ref(out, b, r)
    return out, refs


def edge_refs(p, scenes):
    return [ref_plan(p, s) for s in scenes]


def no_obstacle_scenes():
    return params(64, 3, True), [(BOUND, [1.0, 1.0, 0.5], [8.0, 9.0], [], uniforms(21, 64)),
                                 (BOUND, [60.0, 60.0, -2.0], [70.0, 65.0], [], uniforms(22, 64))]


def test_edge_no_obstacles(ctx):
    p, scenes = no_obstacle_scenes()
    assert all(r["n_nodes"] > 20 for r in edge_refs(p, scenes))
    run_edge(ctx, p, scenes, use_count=False)


def obs_count_scenes():
    return params(64, 3, True), [(BOUND, [0.0, 0.0, 0.3], [12.0, 9.0], field(53), uniforms(23, 64)),
                                 (BOUND, [0.0, 0.0, 0.3], [12.0, 9.0], field(4)[:2], uniforms(24, 64)),
                                 (BOUND, [0.0, 0.0, 0.3], [12.0, 9.0], [], uniforms(25, 64))]


def test_edge_obs_count_varies_and_padding_is_not_read(ctx):
    p, scenes = obs_count_scenes()
    # a padded circle that was read would reject every sample that passes the kinematics
    assert all(r["n_nodes"] > 15 for r in edge_refs(p, scenes))
    run_edge(ctx, p, scenes)


def inside_circle_scene():
    return params(48, 3, True), [(BOUND, [10.0, 10.0, 0.0], [20.0, 20.0], [(10.5, 10.0, 2.0)], uniforms(26, 48))]


def test_edge_start_inside_a_circle(ctx):
    p, scenes = inside_circle_scene()
    r = edge_refs(p, scenes)[0]
    assert r["n_nodes"] == 1 and r["status"] == 0 and sum(r["counters"][:3]) == 48 and r["counters"][REJ_CIRCLE] >= 1
    out, _ = run_edge(ctx, p, scenes)
    assert out["best_idx"][0] == 0 and out["best_cost"][0] == 0.0 and out["path_n"][0] == 0


def start_outside_scene():
    # heading down and to the right from just left of the field: some first steps land inside the bound, others
    # below it; only the second pose of an edge is tested against the bound
    return params(64, 3, True), [(BOUND, [-1.0, 3.0, -0.8], [10.0, 12.0], [], uniforms(33, 64))]


def test_edge_start_outside_the_bound(ctx):
    p, scenes = start_outside_scene()
    r = edge_refs(p, scenes)[0]
    assert r["n_nodes"] >= 5 and r["counters"][REJ_BOUND] >= 1, (r["n_nodes"], r["counters"])
    run_edge(ctx, p, scenes)


def goal_outside_scene():
    return params(64, 3, True, bias_rate=0.5), [(BOUND, [114.0, 60.0, 0.0], [121.5, 60.0], field(53),
                                                 uniforms(27, 64))]


def test_edge_goal_outside_the_bound(ctx):
    p, scenes = goal_outside_scene()
    r = edge_refs(p, scenes)[0]
    assert r["counters"][REJ_BOUND] >= 5 and r["status"] == 0 and r["n_nodes"] >= 2, (r["n_nodes"], r["counters"])
    run_edge(ctx, p, scenes)


def buffer_scene(buffer_size):
    return params(64, buffer_size, True), [(BOUND, [0.0, 0.0, 0.4], [10.0, 10.0], field(4), uniforms(29, 64))]


@pytest.mark.parametrize("buffer_size", [1, 65])
def test_edge_buffer_sizes(ctx, buffer_size):
    p, scenes = buffer_scene(buffer_size)
    r = edge_refs(p, scenes)[0]
    assert r["n_nodes"] > 5
    if buffer_size > 64:  # never rebuilt: every node hangs off node 1
        assert (r["parent"][1: r["n_nodes"]] == 1).all()
    else:
        assert (r["parent"][1: r["n_nodes"]] != 1).any()
    run_edge(ctx, p, scenes)


def one_iteration_scene():
    return params(1, 1, True, bias_rate=1.0), [(BOUND, [0.0, 0.0, 0.0], [2.0, 0.0], [], uniforms(30, 1))]


def test_edge_one_iteration(ctx):
    p, scenes = one_iteration_scene()
    r = edge_refs(p, scenes)[0]
    assert r["n_nodes"] == 2 and r["status"] == 1 and list(r["path_idx"]) == [2, 1]
    out, _ = run_edge(ctx, p, scenes)
    assert list(out["path_idx"][0]) == [2, 1]


def identical_scene():
    return params(64, 3, True), (BOUND, [0.0, 0.0, 0.3], [12.0, 9.0], field(53), uniforms(31, 64))


def test_edge_seventy_identical_scenes(ctx):
    p, s = identical_scene()
    ref = ref_plan(p, s)
    assert ref["n_nodes"] > 15
    out = gpu_plan(ctx, p, [s] * 70, use_count=False)
    for b in range(70):
        check_against_ref(out, b, ref)
    one = gpu_plan(ctx, p, [s], use_count=False)  # B = 1
    check_against_ref(one, 0, ref)


# ---- the Python surface
def test_python_api(ctx):
    specs = [(53, 1, 0.0, [30.0, 10.0]), (4, 1, 0.0, [25.0, 10.0]), (17, 1, 0.7, [20.0, 20.0])]

    def make(k, seed, psi, goal):
        a = nh.defineRRT(600, [0.0, 0.0], psi, goal, 0.0, 7, BOUND, True, 0.2, seed=seed)
        nh.defineRRTobs_(a, field(k))
        return a

    refs, _ = main_conditions()
    singles = [make(*s) for s in specs]
    for a in singles:
        nh.planRRT_(a, ctx=ctx)
    batch = nh.plan_batch([make(*s) for s in specs], ctx=ctx)
    for a, bt, ref in zip(singles, batch, refs):
        r = a.r
        assert r.status == ("Solved" if ref["status"] else "NotSolved") and r.n_nodes == ref["n_nodes"]
        assert r.states.tobytes() == ref["state"][: r.n_nodes].tobytes()
        assert r.costs.tobytes() == ref["cost"][: r.n_nodes].tobytes()
        assert (r.parents == ref["parent"][: r.n_nodes]).all() and list(r.counters) == list(ref["counters"])
        seg = r.tree_segments()
        assert seg.shape == (3, 2 * (r.n_nodes - 1))
        assert tuple(seg[:, 0]) == tuple(r.states[1]) and tuple(seg[:, 1]) == tuple(r.states[r.parents[1] - 1])
        if ref["status"]:
            assert list(r.resultIdxs) == list(ref["path_idx"]) and r.cost == ref["best_cost"]
            assert r.Path.shape == (2, len(r.resultIdxs))
            assert tuple(r.Path[:, 0]) == tuple(ref["state"][ref["best_idx"] - 1][:2])
            assert tuple(r.Path[:, -1]) == (0.0, 0.0)
        fields_ = ["states", "costs", "parents", "counters"] + (["Path", "resultIdxs"] if ref["status"] else [])
        for f in fields_:
            assert getattr(bt.r, f).tobytes() == getattr(r, f).tobytes(), f
        assert bt.r.status == r.status and bt.r.cost == r.cost and bt.r.n_nodes == r.n_nodes
    assert sum(ref["status"] for ref in refs[:3]) >= 1
    # given uniforms replace the seeded ones
    a = make(53, 99, 0.0, [30.0, 10.0])
    nh.planRRT_(a, ctx=ctx, uniforms=uniforms(1, 600))
    assert a.r.states.tobytes() == singles[0].r.states.tobytes()
    with pytest.raises(ValueError):
        nh.plan_batch([make(53, 1, 0.0, [30.0, 10.0]),
                       nh.defineRRT(600, [0.0, 0.0], 0.0, [30.0, 10.0], 0.0, 9, BOUND, True)], ctx=ctx)


# ---- error paths: nothing is launched
@pytest.mark.parametrize("n_iter,buffer_size", [(0, 7), (64, 0), (abi.MP_RRT_MAX_ITER + 1, 7)])
def test_invalid_sizes(ctx, n_iter, buffer_size):
    p = params(n_iter, buffer_size, True)
    B = 1
    bound, start, goal = np.array([BOUND]), np.zeros((B, 3)), np.ones((B, 2))
    uni = np.zeros((B, 1, 6))  # never read: the sizes are refused first
    nn = np.full(B, -7, np.int32)
    st, bi = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    bc = np.full(B, -7.0)
    rc = ctx.lib.mp_rrtnh_plan(ctx.handle, p, B, ptr(bound), ptr(start), ptr(goal), 0, None, None, ptr(uni), ptr(nn),
                               ptr(st), ptr(bi), ptr(bc), None, None, None, None, None, None)
    assert rc == abi.MP_ERR_INVALID
    assert nn[0] == -7 and st[0] == -7 and bi[0] == -7 and bc[0] == -7.0  # nothing ran, nothing was written
    with pytest.raises(abi.MPGPUError):
        ctx.check(rc)


def test_non_finite_start_is_refused(ctx):
    p = params(8, 2, True)
    bound, start, goal = np.array([BOUND]), np.array([[0.0, 0.0, np.nan]]), np.ones((1, 2))
    nn = np.full(1, -7, np.int32)
    st, bi = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    bc = np.full(1, -7.0)
    rc = ctx.lib.mp_rrtnh_plan(ctx.handle, p, 1, ptr(bound), ptr(start), ptr(goal), 0, None, None,
                               ptr(uniforms(1, 8)), ptr(nn), ptr(st), ptr(bi), ptr(bc), None, None, None, None, None,
                               None)
    assert rc == abi.MP_ERR_INVALID and nn[0] == -7 and bc[0] == -7.0
