"""motionplanning_amd/_rrt.py: pack_scenes, the arrays both RRT wrappers hand to the library (no GPU, no library
call)."""
import numpy as np
import pytest

from motionplanning_amd import _rrt, rrt, rrt_nonholonomic as nh

CIRCLES = [[1.0, 2.0, 0.5], [3.0, 4.0, 0.25], [5.0, 6.0, 1.0]]
BOUND = [[0.0, 10.0, 0.0, 20.0], [-5.0, 5.0, -1.0, 1.0]]


def searchers(mod, buffer_sizes=(7, 7)):
    if mod is rrt:
        ss = [rrt.defineRRT(16, [1.0, 2.0], [8.0, 9.0], buffer_sizes[0], BOUND[0], True, 0.3, seed=11),
              rrt.defineRRT(16, [-3.0, 0.5], [4.0, 0.0], buffer_sizes[1], BOUND[1], True, 0.3, seed=12)]
    else:
        ss = [nh.defineRRT(16, [1.0, 2.0], 0.4, [8.0, 9.0], 0.0, buffer_sizes[0], BOUND[0], True, 0.3, seed=11),
              nh.defineRRT(16, [-3.0, 0.5], -1.2, [4.0, 0.0], 0.0, buffer_sizes[1], BOUND[1], True, 0.3, seed=12)]
    mod.defineRRTobs_(ss[0], CIRCLES)
    mod.defineRRTobs_(ss[1], [])
    return ss


@pytest.mark.parametrize("mod,width,n_uni,third", [(rrt, 2, 3, None), (nh, 3, 6, [0.4, -1.2])])
def test_pack_scenes(mod, width, n_uni, third):
    ss = searchers(mod)
    p, bound, start, goal, count, obs, uni = mod._pack(ss)
    assert (p.n_iter, p.buffer_size, p.rrt_star, p.reserved) == (16, 7, 1, 0)
    assert (p.bias_rate, p.grow_min, p.grow_max, p.goal_tolerance) == (0.3, *ss[0].s.grow_dist, 1.0)
    assert bound.tolist() == BOUND and goal.tolist() == [[8.0, 9.0], [4.0, 0.0]]
    assert start.shape == (2, width) and start[:, :2].tolist() == [[1.0, 2.0], [-3.0, 0.5]]
    if third is not None:
        assert start[:, 2].tolist() == third  # starting_ang
    assert count.dtype == np.int32 and count.tolist() == [3, 0]
    assert obs.shape == (2, 3, 3) and obs[0].tolist() == CIRCLES and not obs[1].any()
    assert uni.shape == (2, 16, n_uni)
    for b, a in enumerate(ss):
        assert uni[b].tobytes() == np.random.default_rng(a.s.seed).random((16, n_uni)).tobytes()
    for a in (bound, start, goal, obs, uni):
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    # given uniforms replace the seeded ones; the wrapper's packing is pack_scenes on its start rows
    given = np.arange(2 * 16 * n_uni, dtype=np.float64).reshape(2, 16, n_uni) / 1000.0
    assert mod._pack(ss, given)[6].tobytes() == given.tobytes()
    direct = _rrt.pack_scenes(ss, start.tolist(), n_uni, given)
    assert direct[2].tobytes() == start.tobytes() and direct[6].tobytes() == given.tobytes()


@pytest.mark.parametrize("mod", [rrt, nh])
def test_unequal_settings_raise(mod):
    with pytest.raises(ValueError):
        mod._pack(searchers(mod, buffer_sizes=(7, 9)))
