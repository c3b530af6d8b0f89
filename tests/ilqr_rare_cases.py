"""iLQR instances whose knots leave the generic path of the Riccati sweep's 2x2 pinv (mpj_pinv2_bl), shared by
tests/test_ilqr_rare_cases.py (CPU: which knots are rare, and in which class) and tests/test_gpu_ilqr.py (GPU:
bit-exact against the oracle) -- test infrastructure only.

A vehicle at rest with a zero control guess has an exactly diagonal Quu at every knot: at ux = 0 the steering
column of B is exactly 0, and the mixed second difference luu[0][1] at u = (0, 0) is f + f - f - f = 0 because
sigmoid_boundary is symmetric.  cfg3_instances and the fuzz's moving instances never get there.
"""
import functools

import numpy as np

import oracle
from motionplanning_amd import ilqr

VARIANTS = (ilqr.MP_ILQR_OPTIMALCONTROL, ilqr.MP_ILQR_PARKING)
CONFIGS = ((0.05, 1e-3), (0.1, 2e-3))  # (dT, eps): the script's, and another


def params(N, variant, cfg=0, **kw):
    dT, eps = CONFIGS[cfg]
    return ilqr.params(N=N, variant=variant, dT=dT, eps=eps, **kw)


def _ux_step(ax, dT):
    """What one RK4 step adds to ux (Dynamics.jl:18-28: every stage's d ux = ax), as the oracle rounds it."""
    return 1.0 / 6 * (ax + 2 * ax + 2 * ax + ax) * dT


def brake_to_rest(m, dT, ax=-2.0):
    """(ux0, [ax_0 .. ax_{m-1}]): m braking steps that end at exactly ux = 0.0.  Built backwards from 0: each
    earlier speed is a double whose step lands on the next one exactly, with the step's ax moved a few ulps off
    the nominal value where no such double exists for it."""
    u, axs = 0.0, []
    for _ in range(m):
        for i in range(200):
            a = ax + (i // 2) * (1 if i % 2 else -1) * np.spacing(ax)
            c = _ux_step(a, dT)
            t = u - c
            hit = [float(v) for v in (t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)) if c + v == u]
            if hit:
                break
        u = hit[0]
        axs.insert(0, float(a))
    return u, axs


def family(N, cfg=0):
    """[(name, x0 (4,), U (N, 2))] for horizon N: U[N-1] = 0 as in ilqr.initial_controls."""
    dT = CONFIGS[cfg][0]

    def ctrl(ax=0.0, dl=0.0, upto=None):
        U = np.zeros((N, 2))
        U[: N - 1 if upto is None else upto] = [ax, dl]
        return U

    out = [("rest at origin", [0.0, 0.0, 0.0, 0.0], ctrl()), ("rest", [1.0, 2.0, 0.0, 0.1], ctrl()),
           ("rest, ax 0.5", [1.0, 2.0, 0.0, 0.1], ctrl(0.5)), ("rest, ax -1", [1.0, 2.0, 0.0, 0.1], ctrl(-1.0)),
           ("rest, ax 2 first knot", [-0.5, 0.25, 0.0, -0.3], ctrl(2.0, upto=1))]
    for v in (1e-12, 1e-11, 1e-10, 1e-9, 1e-6, 1e-3):
        out.append(("creep %g" % v, [1.0, 2.0, v, 0.1], ctrl()))
        out.append(("creep %g, ax 0.5" % -v, [1.0, 2.0, -v, 0.1], ctrl(0.5)))
    m = max(1, (N - 1) // 2)  # knots 0..m-1 moving, m..N-1 at rest
    ux0, axs = brake_to_rest(m, dT)
    Ub = ctrl()
    Ub[:m, 0] = axs
    out.append(("brake to rest", [0.3, 0.2, ux0, 0.05], Ub))
    # Parking: starts 0.5 m from the origin, at rest or rolling towards it
    out += [("park 0.5 m, rest", [0.5, 0.0, 0.0, 0.0], ctrl()), ("park 0.5 m, rest, turned", [-0.3, 0.4, 0.0, 0.2], ctrl()),
            ("park 0.5 m, rolling", [0.5, 0.0, -0.2, 0.0], ctrl())]
    u0 = ilqr.U_INIT_REF
    out.append(("NaN state", [np.nan, 3.6, 5.0, 0.0], ctrl(*u0)))
    out.append(("ax 80", list(ilqr.X0_REF), ctrl(80.0, 0.01)))  # the barrier's exp argument passes +-708.39
    for k in (1, 2, 3, 4, -1, -2, -3, -4):  # Cody-Waite edges of the exact sincos
        for d in (np.inf, -np.inf):
            out.append(("heading next%s(%d pi/2)" % ("up" if d > 0 else "down", k),
                        [0.0, 3.6, 5.0, float(np.nextafter(k * np.pi / 2, d))], ctrl(*u0)))
    out.append(("heading 1e5", [0.0, 3.6, 5.0, 1e5], ctrl(*u0)))
    return [(n, np.array(x, np.float64), U) for n, x, U in out]


def classify(p, x0, U):
    """Roll out and sweep on the oracle: (X, Quu (N-1, 2, 2), mask (N-1,)), mask the rare disjuncts per knot
    (oracle.RARE_DISJUNCTS), 0 = generic."""
    X, _ = oracle.ilqr_rollout(p, x0, U)
    _, _, Quu = oracle.ilqr_backward(p, X, U, want_quu=True)
    with np.errstate(all="ignore"):
        _, _, mask = oracle.pinv2_fast_batch(Quu, want_mask=True)
    return X, Quu, mask


def knot_class(Quu, mask):
    """The branch of mpj_pinv2_bl a knot takes: generic, diagonal (mpj_pinv2's isdiag), nan, or the names of
    the disjuncts set."""
    if mask == 0:
        return "generic"
    if np.isnan(Quu).any():
        return "nan"
    if Quu[0, 1] == 0 and Quu[1, 0] == 0:
        return "diagonal"
    return " + ".join(n for b, n in enumerate(oracle.RARE_DISJUNCTS) if mask >> b & 1)


# diagonal at every knot; split (dbdsqr) at every knot under CONFIGS[0]; split at knot 1 for N = 3, CONFIGS[0],
# OptimalControl (generic at N = 6); split at the last knot under CONFIGS[1], OptimalControl; diagonal from
# mid-horizon on; diagonal at every knot
RARE_NAMES = ("rest at origin", "creep 1e-12", "rest, ax 2 first knot", "creep 1e-06", "brake to rest", "park 0.5 m, rest")


QUAD_START = {(0,): 0, (7,): 1, (15,): 4, (0, 7, 15): 0}  # slots of a 16-instance wave -> first RARE_NAMES entry


@functools.lru_cache(maxsize=None)
def wave_batch(N, cfg, B, slots, start=0, seed=5):
    """B cfg3 instances with family members at the given slots (cycled through RARE_NAMES, NaN state, ax 80, from
    entry `start` on);
    slots a tuple; returns (x0 (B, 4), U (B, N, 2)), read-only."""
    x0, U = ilqr.cfg3_instances(B, N, seed)
    fam = dict((n, (x, u)) for n, x, u in family(N, cfg))
    names = RARE_NAMES + ("NaN state", "ax 80")
    for i, s in enumerate(slots):
        x0[s], U[s] = fam[names[(start + i) % len(names)]]
    x0.setflags(write=False)
    U.setflags(write=False)
    return x0, U


def family_batch(N, cfg, pad_to=None, seed=9):
    """The whole family as one batch, then cfg3 instances up to pad_to."""
    fam = family(N, cfg)
    x0 = np.stack([x for _, x, _ in fam])
    U = np.stack([u for _, _, u in fam])
    if pad_to is not None and pad_to > len(fam):
        cx, cu = ilqr.cfg3_instances(pad_to - len(fam), N, seed)
        x0, U = np.concatenate([x0, cx]), np.concatenate([U, cu])
    return x0, U


def assert_bits(got, ref, what=""):
    """Bit-for-bit equality; where the oracle has NaN only the NaN mask is compared."""
    got, ref = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(ref, np.float64)
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(np.int64) != ref.view(np.int64)))
    assert not bad.any(), "%s: %d entries differ, first at %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
