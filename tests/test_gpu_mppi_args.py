"""Argument checks of the MPPI entry points, through the C ABI directly: mp_mppi_plan_dev, mp_mppi_plan,
mp_mppi_closed_loop and mp_mppi_plan_sharded (one context) share one set of checks in mppi.hip, and the status and
message of each rejection are part of the interface.  A rejected call launches nothing; after each one a valid small
call (S 1, K 64, H 6, an 11 x 11 grid) must succeed on the same context.  The one check that depends on the launch
shape is here too: a horizon whose dynamic LDS cannot fit is refused before any launch, with the byte count."""
import ctypes

import numpy as np
import pytest
import torch

from motionplanning_amd import configs
from motionplanning_amd.abi import MP_ERR_INVALID, MP_NOISE_EXTERNAL, MP_NOISE_PHILOX, MP_OK, MPPILoopParams, ptr

pytestmark = pytest.mark.gpu

S, K, H, NG = 1, 64, 6, 11
SPEC = configs.grid_spec(nx=NG, ny=NG)
ENTRIES = ("plan_dev", "plan", "closed_loop", "sharded")

# the messages of mppi.hip's checks, as the library has always worded them
MSG_S = "S (0) must be >= 1"
MSG_REQUIRED = "required pointer is NULL"
MSG_NOISE = "noise is NULL in MP_NOISE_EXTERNAL mode"
MSG_OBS = "obstacles NULL with n_obs > 0"
MSG_GRID = "grid NULL with grid_nx > 0"
MSG_FINAL = "final_stream (2) must be 0 or 1"
MSG_IN_FLIGHT = "calls_in_flight (65) must be in [0, 64]"
MSG_SIGMA = "Σ must be positive definite"
MSG_UPDATE = "update_steps (0) must be >= 1"
MSG_HOLD = "hold_idx[0] = 6 outside [0, H=6)"
MSG_LDS = "K/H/obstacles too large for one scene (dynamic LDS 196616 B)"


def _params(**kw):
    p = configs.mppi_params(K=K, H=H, T=H * 0.15, n_obs=0, feasibility_count=K, grid=SPEC, noise_mode=MP_NOISE_PHILOX,
                            seed=5)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _loop_params(**kw):
    lp = MPPILoopParams(update_steps=2, max_steps=4, plant_dt=0.001, goal_radius=0.5, poll_every=0)
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


def _host_args(s=S, k=K, h=H, ng=NG):
    r = np.random.default_rng(3)
    return dict(X0=np.tile(configs.X0_REF, (s, 1)), goal=np.tile(configs.GOAL_REF, (s, 1)),
                unom=r.uniform(-0.1, 0.1, (s, h, 2)), obstacles=np.tile(configs.OBSTACLES_REF, (s, 1, 1)),
                grid=np.zeros((s, ng, ng), np.uint8), noise=np.zeros((s, k, h, 2)),
                U=np.zeros((s, h, 2)), traj=np.zeros((s, h + 1, 7)), cost=np.zeros(s), feasible=np.zeros(s, np.int32),
                rc=np.zeros(s, np.int32), fc=np.zeros(s, np.int32))


PLAN_ORDER = ("X0", "goal", "unom", "obstacles", "grid", "noise", "U", "traj", "cost", "feasible", "rc", "fc")


class Caller:
    """One entry point with a full set of valid arguments; call(p, ...) names what to leave out (NULL)."""

    def __init__(self, entry, ctx, group):
        self.entry = entry
        self.lib = ctx.lib
        self.ctx = group.ctxs[0] if entry == "sharded" else ctx
        self.group = group
        self.a = _host_args()
        if entry == "plan_dev":
            self.a = {k: torch.as_tensor(v, device="cuda") for k, v in self.a.items()}
            torch.cuda.synchronize()
        self.hold = np.zeros(2, np.int32)
        self.his = np.zeros((S, 5, 8))
        self.n_rows = np.zeros(S, np.int32)
        self.n_replans = np.zeros(S, np.int32)

    def call(self, p, s=S, null=(), lp=None, hold=None):
        a = {k: (None if k in null else ptr(v)) for k, v in self.a.items()}
        plan = [a[k] for k in PLAN_ORDER]
        h = self.ctx.handle
        if self.entry == "plan_dev":
            return self.lib.mp_mppi_plan_dev(h, ctypes.byref(p), s, *plan, None, None, None, None)
        if self.entry == "plan":
            return self.lib.mp_mppi_plan(h, ctypes.byref(p), s, *plan, None, None, None, None)
        if self.entry == "sharded":
            return self.lib.mp_mppi_plan_sharded(self.group.array, 1, ctypes.byref(p), s, *plan)
        lp = lp or _loop_params()
        hold = self.hold if hold is None else hold
        return self.lib.mp_mppi_closed_loop(h, ctypes.byref(p), ctypes.byref(lp), s, a["X0"], a["goal"], a["unom"],
                                            a["obstacles"], a["grid"], ptr(hold), a["noise"], ptr(self.his),
                                            ptr(self.n_rows), ptr(self.n_replans), None, None, None, None, None)

    def message(self):
        return self.lib.mp_last_error(self.ctx.handle).decode()

    def valid_call_succeeds(self):
        st = self.call(_params())
        assert st == MP_OK, self.message()
        if self.entry == "closed_loop":
            assert self.n_replans[0] >= 1 and self.n_rows[0] >= 2
            return
        if self.entry == "plan_dev":
            self.ctx.synchronize()
        rc = self.a["rc"].cpu().numpy() if self.entry == "plan_dev" else self.a["rc"]
        cost = self.a["cost"].cpu().numpy() if self.entry == "plan_dev" else self.a["cost"]
        assert 1 <= int(rc[0]) <= K + 1 and np.isfinite(cost[0])


@pytest.fixture(scope="module")
def group():
    from motionplanning_amd.context import CommGroup

    g = CommGroup([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def callers(ctx, group):
    return {e: Caller(e, ctx, group) for e in ENTRIES}


# (id, parameter overrides, call overrides, message); every entry point unless `only` names some
SHARED = [
    ("S0", {}, dict(s=0), MSG_S, ENTRIES),
    ("null_required", {}, dict(null=("goal",)), MSG_REQUIRED, ENTRIES),
    ("null_noise_external", dict(noise_mode=MP_NOISE_EXTERNAL), dict(null=("noise",)), MSG_NOISE, ENTRIES),
    ("null_obstacles", dict(n_obs=3), dict(null=("obstacles",)), MSG_OBS, ENTRIES),
    ("null_grid", {}, dict(null=("grid",)), MSG_GRID, ENTRIES),
    ("final_stream_2", dict(final_stream=2), {}, MSG_FINAL, ("plan_dev", "plan", "sharded")),
    ("calls_in_flight_65", dict(calls_in_flight=65), {}, MSG_IN_FLIGHT, ENTRIES),
]
CASES = [pytest.param(e, pk, ck, msg, id=f"{e}-{cid}") for cid, pk, ck, msg, only in SHARED for e in only]


@pytest.mark.parametrize("entry,pkw,ckw,msg", CASES)
def test_rejected_with_message(callers, entry, pkw, ckw, msg):
    c = callers[entry]
    assert c.call(_params(**pkw), **ckw) == MP_ERR_INVALID
    assert c.message() == msg
    c.valid_call_succeeds()


@pytest.mark.parametrize("entry", ENTRIES)
def test_sigma_not_positive_definite(callers, entry):
    c = callers[entry]
    p = _params()
    for i, v in enumerate((1.0, 0.0, 0.0, -1.0)):
        p.sigma[i] = v
    assert c.call(p) == MP_ERR_INVALID
    assert c.message() == MSG_SIGMA
    c.valid_call_succeeds()


def test_closed_loop_update_steps_and_hold(callers):
    c = callers["closed_loop"]
    assert c.call(_params(), lp=_loop_params(update_steps=0)) == MP_ERR_INVALID
    assert c.message() == MSG_UPDATE
    c.valid_call_succeeds()
    assert c.call(_params(), hold=np.array([H, 0], np.int32)) == MP_ERR_INVALID
    assert c.message() == MSG_HOLD
    c.valid_call_succeeds()


def test_horizon_beyond_lds_refused_before_launch(ctx, callers):
    """S 1, K 1, H 4096, no grid, no circles: 8 * (2H + nb + 4H) = 196,616 B of dynamic LDS with nb = 1, above the
    146 KiB a block may have; the shape is computed and refused before anything is launched."""
    h = 4096
    a = _host_args(1, 1, h, 1)
    p = configs.mppi_params(K=1, H=h, T=h * 0.15, n_obs=0, feasibility_count=1, noise_mode=MP_NOISE_PHILOX)
    plan = [None if k in ("obstacles", "grid", "noise") else ptr(a[k]) for k in PLAN_ORDER]
    st = ctx.lib.mp_mppi_plan(ctx.handle, ctypes.byref(p), 1, *plan, None, None, None, None)
    assert st == MP_ERR_INVALID
    assert ctx.lib.mp_last_error(ctx.handle).decode() == MSG_LDS
    callers["plan"].valid_call_succeeds()
