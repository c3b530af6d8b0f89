"""GPU parity for the batched iLQR (mp_ilqr_*) vs the CPU oracle: BIT-EXACT.

Same FDLIBM libm (include/mp_jlmath.h), same evaluation order, no FMA contraction;
the device hoists control-only terms (tan δ, β, cos β, sigmoid barriers), which are
pure functions of identical bits, so derivatives, gains, line-search decisions and
iteration counts are identical.  Parity against Julia itself is unpinned.
"""
import numpy as np
import pytest

import oracle
from motionplanning_amd import ilqr

pytestmark = pytest.mark.gpu


def _instances(B, N, seed=3):
    return ilqr.cfg3_instances(B, N, seed)


# N-1 = 19, 29, 2, 4, 20, 22: every residue mod 4 of the forward trial's last 4-knot store group
@pytest.mark.parametrize("variant,N", [(ilqr.MP_ILQR_OPTIMALCONTROL, 20), (ilqr.MP_ILQR_PARKING, 30),
                                       (ilqr.MP_ILQR_OPTIMALCONTROL, 3), (ilqr.MP_ILQR_OPTIMALCONTROL, 5),
                                       (ilqr.MP_ILQR_OPTIMALCONTROL, 21), (ilqr.MP_ILQR_PARKING, 23)])
def test_rollout_backward_forward_bitexact(ctx, variant, N):
    p = ilqr.params(N=N, variant=variant)
    x0, U = _instances(48, N)
    X, J = ilqr.ilqr_rollout(p, x0, U, ctx=ctx)
    k, K = ilqr.ilqr_backward(p, X, U, ctx=ctx)
    alphas = np.where(np.arange(48) % 2 == 0, 1.0, 0.25)
    Xn, Un, Jn = ilqr.ilqr_forward(p, X, U, k, K, alphas, ctx=ctx)
    for b in range(48):
        Xo, Jo = oracle.ilqr_rollout(p, x0[b], U[b])
        assert np.array_equal(X[b], Xo) and J[b] == Jo
        ko, Ko = oracle.ilqr_backward(p, Xo, U[b])
        assert np.array_equal(k[b], ko) and np.array_equal(K[b], Ko)
        Xno, Uno, Jno = oracle.ilqr_forward(p, Xo, U[b], ko, Ko, alphas[b])
        assert np.array_equal(Xn[b], Xno) and np.array_equal(Un[b], Uno) and Jn[b] == Jno


@pytest.mark.parametrize("variant,N,max_iter", [(ilqr.MP_ILQR_OPTIMALCONTROL, 20, 1000),
                                                (ilqr.MP_ILQR_PARKING, 30, 40),
                                                (ilqr.MP_ILQR_OPTIMALCONTROL, 23, 60)])
def test_solve_bitexact(ctx, variant, N, max_iter):
    p = ilqr.params(N=N, variant=variant, max_iter=max_iter)
    x0, U0 = _instances(24, N, seed=7)
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)
    for b in range(24):
        Xo, Uo, Jo, ito, flags = oracle.ilqr_solve(p, X0[b], U0[b])
        assert it[b] == ito, (b, it[b], ito)
        assert J[b] == Jo and np.array_equal(X[b], Xo) and np.array_equal(U[b], Uo)
    if variant == ilqr.MP_ILQR_OPTIMALCONTROL and N == 20:
        # x0 of ILQR.jl:12 (its N = 20) converges (restatement value 10093.67); other random instances may stall
        # at a stationary point where the reference's unbounded halving would spin (max_ls flag),
        # identically in the oracle (compared above).
        assert 10080 < J[0] < 10100 and it[0] == 13


def test_solve_under_workspace_limit():
    """mp_ilqr_solve keeps its results when its optional line-search slots cannot be allocated: a
    context capped below the all-trials-at-once slots falls back to the multi-round 16-wide search,
    a tighter cap to the 4-wide one; a cap below the base buffers is MP_ERR_NOMEM, and the context
    works again after mp_ctx_trim + lifting the cap (no hard failure where the old
    search fit)."""
    from motionplanning_amd.abi import MP_ERR_NOMEM, MPGPUError
    from motionplanning_amd.context import Context

    p = ilqr.params(N=20, max_iter=60)
    x0, U0 = _instances(24, 20, seed=7)  # includes instances that stall (max_ls trials)
    c = Context(0)
    try:
        X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=c)
        ref = ilqr.ilqr_solve(p, X0, U0, ctx=c)  # no cap: rest slots (2.8 MB) in use
        # 1 MB: the 16-wide slots (245 KB) fit, the rest slots (2.8 MB) do not; 230 KB: the
        # 4-wide slots (61 KB) and the derivative records (212 KB) only
        for cap in (1 << 20, 230 << 10):
            c.trim()
            c.set_workspace_limit(cap)
            got = ilqr.ilqr_solve(p, X0, U0, ctx=c)
            for a, b in zip(got[:4], ref[:4]):
                assert np.array_equal(a, b), cap
        c.trim()  # the cap applies when a workspace grows: cached buffers are kept until trimmed
        c.set_workspace_limit(1024)
        with pytest.raises(MPGPUError) as e:
            ilqr.ilqr_solve(p, X0, U0, ctx=c)
        assert e.value.status == MP_ERR_NOMEM
        c.set_workspace_limit(0)
        c.trim()
        got = ilqr.ilqr_solve(p, X0, U0, ctx=c)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    finally:
        c.close()


def test_cfg3_full_size_one_pass(ctx):
    """BASELINE configs[2]: H=100 knots x 4096 initial states, rollout + one backward pass + one
    forward trial (alpha 2^-(b%16), the line search's first 16 steps); EVERY instance bit-exact vs the
    oracle (threaded, ~1 s)."""
    from concurrent.futures import ThreadPoolExecutor

    B, N = 4096, 100
    p = ilqr.params(N=N)
    x0, U = _instances(B, N)
    X, J = ilqr.ilqr_rollout(p, x0, U, ctx=ctx)
    k, K = ilqr.ilqr_backward(p, X, U, ctx=ctx)
    alphas = np.ldexp(1.0, -(np.arange(B) % 16))
    Xn, Un, Jn = ilqr.ilqr_forward(p, X, U, k, K, alphas, ctx=ctx)
    assert np.isfinite(k).all() and np.isfinite(K).all() and np.isfinite(Jn).all()

    def ref(b):
        Xo, Jo = oracle.ilqr_rollout(p, x0[b], U[b])
        ko, Ko = oracle.ilqr_backward(p, Xo, U[b])
        return (Xo, Jo, ko, Ko) + tuple(oracle.ilqr_forward(p, Xo, U[b], ko, Ko, alphas[b]))

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(B)))
    for b, (Xo, Jo, ko, Ko, Xno, Uno, Jno) in enumerate(refs):
        assert np.array_equal(X[b], Xo) and J[b] == Jo, b
        assert np.array_equal(k[b], ko) and np.array_equal(K[b], Ko), b
        assert np.array_equal(Xn[b], Xno) and np.array_equal(Un[b], Uno) and Jn[b] == Jno, b


def test_dev_entry_points_match_host(ctx):
    """mp_ilqr_{backward,forward}_dev on HBM-resident tensors == the host-pointer calls (bit-exact)."""
    import ctypes

    import torch

    from motionplanning_amd.abi import ptr

    p = ilqr.params(N=30)
    x0, U = ilqr.cfg3_instances(96, 30, seed=8)
    X, _ = ilqr.ilqr_rollout(p, x0, U, ctx=ctx)
    k, K = ilqr.ilqr_backward(p, X, U, ctx=ctx)
    Xn, Un, Jn = ilqr.ilqr_forward(p, X, U, k, K, np.full(96, 0.5), ctx=ctx)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
    with torch.cuda.stream(stream):
        dX, dU = torch.as_tensor(X, device=dev), torch.as_tensor(U, device=dev)
        dk, dK = torch.empty((96, 29, 2), dtype=torch.float64, device=dev), torch.empty(
            (96, 29, 4, 2), dtype=torch.float64, device=dev)
        dXn, dUn, dJn = torch.empty_like(dX), torch.empty_like(dU), torch.empty(96, dtype=torch.float64, device=dev)
        dal = torch.full((96,), 0.5, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.mp_ilqr_backward_dev(ctx.handle, ctypes.byref(p), 96, ptr(dX), ptr(dU), ptr(dk), ptr(dK)))
        ctx.check(ctx.lib.mp_ilqr_forward_dev(ctx.handle, ctypes.byref(p), 96, ptr(dX), ptr(dU), ptr(dk), ptr(dK),
                                              ptr(dal), ptr(dXn), ptr(dUn), ptr(dJn)))
        ctx.synchronize()
    assert np.array_equal(dk.cpu().numpy(), k) and np.array_equal(dK.cpu().numpy(), K)
    assert np.array_equal(dXn.cpu().numpy(), Xn) and np.array_equal(dUn.cpu().numpy(), Un)
    assert np.array_equal(dJn.cpu().numpy(), Jn)


def test_solve_configs2_horizon_bitexact(ctx):
    """mp_ilqr_solve at configs[2]'s horizon (H=100, max_iter 60 as in the bench) on 640 of its instances
    vs the oracle's sequential loop (threaded): iteration counts, costs, states and controls bit for bit
    -- the 16-wide quad round 0 + remaining-trials pass while more than 512 instances are active, the
    one-pass search after, the trial-fixpoint cutoff and the max_ls stops included."""
    from concurrent.futures import ThreadPoolExecutor

    B, N = 640, 100
    p = ilqr.params(N=N, max_iter=60)
    x0, U0 = ilqr.cfg3_instances(B, N, seed=3)
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)

    def ref(b):
        return oracle.ilqr_solve(p, X0[b], U0[b])

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(B)))
    stalled = 0
    for b, (Xo, Uo, Jo, ito, flags) in enumerate(refs):
        assert it[b] == ito and J[b] == Jo, (b, it[b], ito)
        assert np.array_equal(X[b], Xo) and np.array_equal(U[b], Uo)
        stalled += bool(flags & 1)
    assert stalled > 0  # the rest pass (trials 16..max_ls) was exercised


def test_solve_dev_matches_host_api(ctx):
    """mp_ilqr_solve_dev (device buffers, solved in place -- the form the bench times) gives the host API's
    results bit for bit: states, controls, costs, iteration counts and the status, on the bench's instances."""
    import torch

    B, N = 1024, 100
    p = ilqr.params(N=N, max_iter=60)
    x0, U0 = ilqr.cfg3_instances(B, N, seed=3)
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)
    dev = torch.device("cuda", 0)
    dX, dU = torch.as_tensor(X0, device=dev).clone(), torch.as_tensor(U0, device=dev).clone()
    dJ = torch.empty(B, dtype=torch.float64, device=dev)
    dit = torch.empty(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (torch's copies ran on its own stream, the solve runs on the context's)
    ok_dev = ilqr.ilqr_solve_dev(p, dX, dU, dJ, dit, ctx=ctx)
    torch.cuda.synchronize()
    assert ok_dev == ok
    assert np.array_equal(dX.cpu().numpy(), X) and np.array_equal(dU.cpu().numpy(), U)
    assert np.array_equal(dJ.cpu().numpy(), J) and np.array_equal(dit.cpu().numpy(), it)


def test_solve_bench_workload_full_size_bitexact(ctx):
    """The bench's own configs[2] solve (bench.py bench_ilqr: 4,096 instances x H=100 from
    cfg3_instances(seed=3), rolled out, then mp_ilqr_solve with max_iter 60; ILQR.jl:44-88) vs the
    oracle's sequential loop for EVERY instance (threaded): iteration counts, J, X and U bit for bit.
    Covers the pipelined search at full activity, the switch to the one-pass search with instances
    still pending, the trial-fixpoint cutoff and the max_ls stops."""
    from concurrent.futures import ThreadPoolExecutor

    B, N = 4096, 100
    p = ilqr.params(N=N, max_iter=60)
    x0, U0 = ilqr.cfg3_instances(B, N, seed=3)
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)

    def ref(b):
        return oracle.ilqr_solve(p, X0[b], U0[b])

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(B)))
    bad = [b for b, (Xo, Uo, Jo, ito, flags) in enumerate(refs)
           if not (it[b] == ito and J[b] == Jo and np.array_equal(X[b], Xo) and np.array_equal(U[b], Uo))]
    assert not bad, (len(bad), bad[:8])
    stalled = sum(bool(r[4] & 1) for r in refs)
    assert stalled > 0 and int(it.max()) > 20  # max_ls stops and long searches were exercised


# N-1 = 19, 20, 21, 22: every residue of the trial's last 4-knot store group in round 0
@pytest.mark.parametrize("B,N", [(2048, 20), (768, 21), (768, 22), (768, 23)])
def test_solve_pipelined_search_bitexact(ctx, B, N):
    """mp_ilqr_solve's pipelined line search on a batch large enough to stay in it for many
    iterations (2048 instances: > 512 active): each iteration's rest pass runs in the next launch
    beside round 0, the instances it holds sit one backward pass out, and the switch to the one-pass
    search happens while some are still pending.  Every instance's iteration count, cost, states and
    controls must equal the oracle's sequential loop."""
    from concurrent.futures import ThreadPoolExecutor

    p = ilqr.params(N=N, max_iter=60)
    x0, U0 = ilqr.cfg3_instances(B, N, seed=11)
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)

    def ref(b):
        return oracle.ilqr_solve(p, X0[b], U0[b])

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(B)))
    stalled = 0
    for b, (Xo, Uo, Jo, ito, flags) in enumerate(refs):
        assert it[b] == ito and (J[b] == Jo or (J[b] != J[b] and Jo != Jo)), (b, it[b], ito)
        assert np.array_equal(X[b], Xo) and np.array_equal(U[b], Uo)
        stalled += bool(flags & 1)
    assert stalled > 0 and int(it.max()) > 10


def test_solve_context_reused_across_strategies():
    """One context, five solves in a row that take different search strategies and shapes, so each finds the
    workspace, the list buffers and the pinned and mapped count words as the one before left them: 24 x 20
    (one-pass from the first iteration, with stalling instances), 600 x 21 (more than 512 active: pipelined, then
    the switch to one-pass with instances pending), 24 x 20 again, the same under a 1 MiB cap after a trim (the
    16-wide search without rest slots), and 600 x 21 once more with the cap lifted.  Each result -- X, U, J,
    iteration counts, status -- equals, bit for bit, that of the same solve on a fresh context of its own."""
    from motionplanning_amd.context import Context

    def problem(B, N, seed):
        p = ilqr.params(N=N, max_iter=60)
        x0, U0 = ilqr.cfg3_instances(B, N, seed)
        return p, x0, U0

    def solve(c, prob, cap=0):
        p, x0, U0 = prob
        if cap:
            c.trim()
            c.set_workspace_limit(cap)
        X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=c)
        return ilqr.ilqr_solve(p, X0, U0, ctx=c)

    def fresh(prob, cap=0):
        c = Context(0)
        try:
            return solve(c, prob, cap)
        finally:
            c.close()

    small, big = problem(24, 20, 7), problem(600, 21, 11)
    want_small, want_capped, want_big = fresh(small), fresh(small, 1 << 20), fresh(big)
    assert int(want_big[3].max()) > 10  # the big solve does stay pipelined for many iterations
    c = Context(0)
    try:
        got = [solve(c, small), solve(c, big), solve(c, small), solve(c, small, 1 << 20)]
        c.set_workspace_limit(0)
        got.append(solve(c, big))
    finally:
        c.close()
    for i, (g, w) in enumerate(zip(got, (want_small, want_big, want_small, want_capped, want_big))):
        for a, b in zip(g, w):
            assert np.array_equal(a, b, equal_nan=True), i


# ------------------------------------------------------------------ knots off the pinv's generic path
# tests/ilqr_rare_cases.py: at rest (diagonal Quu at every knot), creeping (dbdsqr splits), braking to rest (one
# sweep crosses from diagonal to generic knots), a NaN state, ax = 80 (the barrier's exp far branch), headings at
# the Cody-Waite edges.  tests/test_ilqr_rare_cases.py asserts on the CPU which knots are rare and in which class.
import ilqr_rare_cases as rc  # noqa: E402


def _one_pass_vs_oracle(ctx, p, x0, U, what):
    """ilqr_rollout + ilqr_backward + ilqr_forward (alpha 1 / 0.25 alternating) for the batch; EVERY instance bit
    for bit against the oracle (NaN by mask).  Returns the device results."""
    from concurrent.futures import ThreadPoolExecutor

    B = len(x0)
    X, J = ilqr.ilqr_rollout(p, x0, U, ctx=ctx)
    k, K = ilqr.ilqr_backward(p, X, U, ctx=ctx)
    alphas = np.where(np.arange(B) % 2 == 0, 1.0, 0.25)
    Xn, Un, Jn = ilqr.ilqr_forward(p, X, U, k, K, alphas, ctx=ctx)

    def ref(b):
        Xo, Jo = oracle.ilqr_rollout(p, x0[b], U[b])
        ko, Ko = oracle.ilqr_backward(p, Xo, U[b])
        return (Xo, Jo, ko, Ko) + tuple(oracle.ilqr_forward(p, Xo, U[b], ko, Ko, alphas[b]))

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(B)))
    for b, r in enumerate(refs):
        for name, got, want in zip(("X", "J", "k", "K", "Xn", "Un", "Jn"), (X[b], J[b], k[b], K[b], Xn[b], Un[b], Jn[b]), r):
            rc.assert_bits(got, want, "%s, instance %d, %s" % (what, b, name))
    return X, k, K, alphas, Xn, Un, Jn


@pytest.mark.parametrize("cfg", (0, 1))
@pytest.mark.parametrize("N", (2, 3, 6))
@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_rare_family_one_pass_bitexact(ctx, variant, N, cfg):
    """The whole family as one batch (40 instances: a partial wave, rare quads next to generic ones and to dead
    lanes), both variants, the script's (dT, eps) and another."""
    x0, U = rc.family_batch(N, cfg)
    _one_pass_vs_oracle(ctx, rc.params(N, variant, cfg), x0, U, "family")


@pytest.mark.parametrize("slots", [(0,), (7,), (15,), (0, 7, 15)])
@pytest.mark.parametrize("N", (3, 6))
@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_rare_instance_among_cfg3_quads(ctx, variant, N, slots):
    """One compute wave of the sweep (16 instances on lane quads): rare instances at quad 0, 7, 15 among cfg3
    instances.  The wave takes mpj_pinv2_bl's exact fallback for the rare quads' knots; the generic quads beside
    them must keep the bits the straight-line path gives them.  All 16 are checked.  Alone, slot 0 holds the
    vehicle at rest (diagonal), slot 7 the creeping one (split), slot 15 the one that brakes to rest."""
    x0, U = rc.wave_batch(N, 0, 16, slots, start=rc.QUAD_START[slots])
    _one_pass_vs_oracle(ctx, rc.params(N, variant), x0, U, "slots %s" % (slots,))


@pytest.mark.parametrize("B,slots", [(1, (0,)), (17, (0, 16)), (17, (3,)), (48, (5, 16, 31, 47, 32, 1, 20, 40))])
def test_rare_partial_waves(ctx, B, slots):
    """Partial waves: dead quads (which recompute the last column) next to rare quads; B = 48 is the split
    deriv4 + quad path of run_backward with three blocks."""
    for variant in rc.VARIANTS:
        x0, U = rc.wave_batch(3, 0, B, slots)
        _one_pass_vs_oracle(ctx, rc.params(3, variant), x0, U, "B=%d" % B)


def test_rare_fused_backward_path(ctx):
    """B = 2064 > kDeriv4Max: run_backward takes ilqr_backward_fused_kernel.  Rare instances scattered through
    the batch (every 97th slot and the last); the same batch cut to 48 instances takes the deriv4 + quad path, and
    both agree with the oracle, hence with each other."""
    B, N = 2064, 3
    slots = tuple(range(3, B, 97)) + (B - 1,)
    x0, U = rc.wave_batch(N, 0, B, slots)
    p = rc.params(N, ilqr.MP_ILQR_OPTIMALCONTROL)
    X, k, K = _one_pass_vs_oracle(ctx, p, x0, U, "fused")[:3]
    k48, K48 = ilqr.ilqr_backward(p, X[:48], U[:48], ctx=ctx)
    rc.assert_bits(k48, k[:48], "split path vs fused path, k")
    rc.assert_bits(K48, K[:48], "split path vs fused path, K")


def _solve_mix(N, cfg=0):
    """64 instances: the family without the NaN state, then cfg3 instances.  (With J = NaN on entry the reference
    loop skips its line search and copies trial buffers that no trial wrote, and pinv(Quu) throws in Julia: nothing
    to be exact against.  NaN costs that arise during a solve are covered by test_solve_pipelined_search_bitexact.)"""
    x0, U = rc.family_batch(N, cfg, pad_to=65)
    keep = [i for i, (n, _, _) in enumerate(rc.family(N, cfg)) if n != "NaN state"] + list(range(len(rc.family(N, cfg)), 65))
    return x0[keep], U[keep]


@pytest.mark.parametrize("ls", [None, (0.25, 3)])
@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_solve_rare_mix_bitexact(ctx, variant, ls):
    """mp_ilqr_solve on the 64-instance mix (N = 12, max_iter = 30): iteration counts, J, X and U against the
    oracle's sequential loop.  The Parking variant's instances that start at rest 0.5 m from the origin approach
    rest through the solve.  ls = (alpha_floor, max_ls) = (0.25, 3): the floor and the cap decide ls_cap and stop
    searches early."""
    from concurrent.futures import ThreadPoolExecutor

    N = 12
    kw = {} if ls is None else dict(alpha_floor=ls[0], max_ls=ls[1])
    p = rc.params(N, variant, 0, max_iter=30, **kw)
    x0, U0 = _solve_mix(N)
    assert len(x0) == 64
    X0, _ = ilqr.ilqr_rollout(p, x0, U0, ctx=ctx)
    X, U, J, it, ok = ilqr.ilqr_solve(p, X0, U0, ctx=ctx)
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda b: oracle.ilqr_solve(p, X0[b], U0[b]), range(64)))
    for b, (Xo, Uo, Jo, ito, flags) in enumerate(refs):
        assert it[b] == ito, (b, it[b], ito)
        rc.assert_bits(J[b], Jo, "J, instance %d" % b)
        rc.assert_bits(X[b], Xo, "X, instance %d" % b)
        rc.assert_bits(U[b], Uo, "U, instance %d" % b)
    assert ok == all(r[4] == 0 for r in refs)
    assert len({r[3] for r in refs}) > 2  # instances stop at different iterations


def test_rare_dev_entry_points_match_host(ctx):
    """mp_ilqr_{backward,forward}_dev on the rare family batch in HBM == the host-pointer calls (NaN by mask)."""
    import ctypes

    import torch

    from motionplanning_amd.abi import ptr

    N = 6
    p = rc.params(N, ilqr.MP_ILQR_PARKING)
    x0, U = rc.family_batch(N, 0, pad_to=48)
    B = len(x0)
    X, _ = ilqr.ilqr_rollout(p, x0, U, ctx=ctx)
    k, K = ilqr.ilqr_backward(p, X, U, ctx=ctx)
    Xn, Un, Jn = ilqr.ilqr_forward(p, X, U, k, K, np.full(B, 0.5), ctx=ctx)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
    with torch.cuda.stream(stream):
        dX, dU = torch.as_tensor(X, device=dev), torch.as_tensor(U, device=dev)
        dk = torch.empty((B, N - 1, 2), dtype=torch.float64, device=dev)
        dK = torch.empty((B, N - 1, 4, 2), dtype=torch.float64, device=dev)
        dXn, dUn, dJn = torch.empty_like(dX), torch.empty_like(dU), torch.empty(B, dtype=torch.float64, device=dev)
        dal = torch.full((B,), 0.5, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.mp_ilqr_backward_dev(ctx.handle, ctypes.byref(p), B, ptr(dX), ptr(dU), ptr(dk), ptr(dK)))
        ctx.check(ctx.lib.mp_ilqr_forward_dev(ctx.handle, ctypes.byref(p), B, ptr(dX), ptr(dU), ptr(dk), ptr(dK),
                                              ptr(dal), ptr(dXn), ptr(dUn), ptr(dJn)))
        ctx.synchronize()
    for name, got, want in (("k", dk, k), ("K", dK, K), ("Xn", dXn, Xn), ("Un", dUn, Un), ("Jn", dJn, Jn)):
        rc.assert_bits(got.cpu().numpy(), want, name)
    # and the device solve on the solve mix == the host solve
    ps = rc.params(12, ilqr.MP_ILQR_PARKING, 0, max_iter=30)
    x0, U0 = _solve_mix(12)
    X0, _ = ilqr.ilqr_rollout(ps, x0, U0, ctx=ctx)
    Xs, Us, Js, its, ok = ilqr.ilqr_solve(ps, X0, U0, ctx=ctx)
    dX, dU = torch.as_tensor(X0, device=dev).clone(), torch.as_tensor(U0, device=dev).clone()
    dJ = torch.empty(64, dtype=torch.float64, device=dev)
    dit = torch.empty(64, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert ilqr.ilqr_solve_dev(ps, dX, dU, dJ, dit, ctx=ctx) == ok
    torch.cuda.synchronize()
    rc.assert_bits(dX.cpu().numpy(), Xs, "solve_dev X")
    rc.assert_bits(dU.cpu().numpy(), Us, "solve_dev U")
    rc.assert_bits(dJ.cpu().numpy(), Js, "solve_dev J")
    assert np.array_equal(dit.cpu().numpy(), its)
