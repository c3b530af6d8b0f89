"""The cases tests/test_gpu_mppi_ref.py runs on the device, their restatement results (tests/mppi_ref.py), and
MPPICtrl's exact value with its forward error bound.  Shared with tests/test_mppi_ref.py, which holds the
reference's own sequential fold to the same bound without a GPU.

The exact value.  With the rollouts' costs c_i and controls u_i given (they are compared bit for bit first),
MPPIUtils.jl:154-167,186-190 define, in real arithmetic,

    x_i = (c_i - ρ)/λ,  ρ = min c,   E_i = exp(-x_i),   w_i = E_i / Σ_k E_k,   U* = Σ_i w_i u_i.

exact_mppictrl evaluates this with the standard library's decimal at 60 digits: Decimal(float) is exact,
Decimal.exp is correctly rounded, so U* is good to ~1e-57 relative -- exact for the purpose.

The bound.  u = 2^-53 is the unit roundoff (every +, -, *, / below errs by a factor 1 + δ, |δ| <= u); the
reference's loop over m holders computes

    a_i = fl(fl(-1/λ) * fl(c_i - ρ))      three roundings: a_i = -x_i (1 + θ3),  |θ3| <= 3u (first order)
    e_i = exp(a_i) (1 + ε_i)              |ε_i| <= c_exp ulp <= 2 c_exp u
        = E_i (1 + r_i),                  |r_i| <= 3u|x_i| + 2 c_exp u          [exp(-x θ) = 1 - x θ + ...]
    η̂  = e_1 + e_2 + ... + e_m           each term passes at most m - 1 additions
    ŵ_i = fl(fl(1/η̂) * e_i)              two roundings
    Û_t = ŵ_1 u_1 + ... + ŵ_m u_m        one product and at most m - 1 additions per term

so Û_t = N̂/η̂ with N̂ = Σ E_i u_i (1 + r_i)(1 + θ_{m+2}) and η̂ = Σ E_i (1 + r_i)(1 + θ_{m-1}).  Against
N = Σ E_i u_i and D = Σ E_i,  |N̂/η̂ - N/D| <= (|N̂ - N| + |U*| |η̂ - D|)/η̂, which gives per entry t

    |Û_t - U*_t| <= u Σ_i w_i (n_add + 3|x_i| + 2 c_exp) |u_i,t|  +  |U*_t| u Σ_i w_i (n_add + 3|x_i| + 2 c_exp)

with n_add = m + 2 for numerator and denominator alike, times 1.01 for the second-order terms and D/η̂ (the
first-order sum is below 1e-9 on every case here, so 1 % is ample), plus 2^-1000 |u_i| per term for an e_i that
underflowed (exp below 2^-1022 has no relative bound; its absolute error is below 2^-1022).  c_exp = 0.52 ulp
is the figure include/mp_jlmath.h states for its exp.  Nothing in it was fitted to a result.

The device adds the same terms in a tree (32 rollouts per wave, waves in order, blocks in order), whose longest
path is shorter than m - 1, and splits the exponent over two exp calls, exp(nil (c - ρ_b)) exp(nil (ρ_b - ρ)):
both arguments are <= 0, their |x| add up to |x_i|, and the second exp and the product cost 2 c_exp + 1 more u,
which the shorter tree leaves room for at every m used here (m >= 70).  So the device is held to the reference's
bound as it stands.
"""
import functools
import os
from decimal import Decimal, localcontext

import numpy as np

from motionplanning_amd import configs
from motionplanning_amd.abi import MP_NOISE_EXTERNAL, MP_NOISE_PHILOX

import mppi_ref

SIGMA_A = [0.05, 0.021, 0.021, 0.1]
SIGMA_B = [0.05, 0.057, 0.057, 0.1]
C_EXP = 0.52  # ulp, include/mp_jlmath.h on mpj_exp
U_ROUND = 2.0 ** -53

NAMES = ["generic-ref", "generic-A", "generic-B", "lpr1"]
LPR1_ENVS = [{"MPGPU_LPR": "1"}, {"MPGPU_LPR": "1", "MPGPU_PLAN_LEAN": "0"}]  # lean, generic


def build(name):
    """dict(p, S, X0 (S,7), goal, unom (S,H,2), obs (S,n,3) | None, grid (S,ny,nx), z (S,K,H,2) | None, envs)."""
    spec = configs.grid_spec()
    if name.startswith("generic"):
        # S = 2, K = 70, H = 5: at two lanes per rollout one full wave plus six lanes, scene 1 behind scene 0;
        # λ = 400 and small nominal controls spread the weights over many rollouts (the control term's share of
        # the exponent, u_nom' Σ⁻¹ (u - u_nom), does not depend on λ)
        sigma = {"ref": configs.SIGMA_REF, "A": SIGMA_A, "B": SIGMA_B}[name.split("-")[1]]
        S, K, H = 2, 70, 5
        r = np.random.default_rng(900)
        p = configs.mppi_params(K=K, H=H, T=0.15 * H, lam=400.0, sigma=sigma, n_obs=3, feasibility_count=K, grid=spec,
                                noise_mode=MP_NOISE_EXTERNAL)
        X0 = np.array([[3.0, 0.5, 0.1, 0.02, 0.05, 6.0, 0.01], [40.0, -0.7, -0.1, 0.01, -0.03, 7.0, -0.01]])
        # the fans are narrow after five steps (about 0.5 m wide at x0 + 4.4 m): circles at their edges, and one
        # occupied 1.4 m x 0.4 m cell beside each fan's middle, so that some rollouts are hit and some pass
        obs = np.array([[[7.5, 1.45, 0.75], [6.6, 0.05, 0.5], [5.7, 1.0, 0.35]],
                        [[44.15, -1.75, 0.7], [44.15, -0.4, 0.45], [43.1, -0.5, 0.3]]])
        grid = np.zeros((S, spec["ny"], spec["nx"]), np.uint8)
        for s, (gx, gy) in enumerate([(7.5, 0.9), (45.2, -1.4)]):
            grid[s, int((gy - spec["y0"]) / spec["dy"]), int((gx - spec["x0"]) / spec["dx"])] = 1
        un = np.stack([np.c_[r.uniform(-0.03, 0.03, H), r.uniform(-0.15, 0.15, H)] for _ in range(S)])
        z = r.standard_normal((S, K, H, 2))
        envs = [{}]
    else:
        # one rollout per lane, lean and generic instance: 256-lane block 0 and a partial block 1 with 212
        # inactive lanes, where the FeasibilityCount prefix ends
        S, K, H = 2, 300, 7
        r = np.random.default_rng(901)
        p = configs.mppi_params(K=K, H=H, T=0.15 * H, sigma=SIGMA_A, n_obs=0, feasibility_count=255, grid=spec,
                                noise_mode=MP_NOISE_PHILOX, seed=77, offset=2)
        X0 = np.array([[21.5, -0.6, 0.1, 0.02, 0.05, 6.0, 0.01], [60.0, -0.2, -0.1, 0.01, -0.03, 6.5, -0.01]])
        obs = None
        grid = np.stack([configs.rasterize_circles(configs.OBSTACLES_CFG1, spec)] * S)
        un = np.stack([np.c_[r.uniform(-0.1, 0.1, H), r.uniform(-0.5, 0.5, H)] for _ in range(S)])
        z = None
        envs = LPR1_ENVS
    return dict(name=name, p=p, S=S, X0=X0, goal=np.tile(configs.GOAL_REF, (S, 1)), unom=un, obs=obs, grid=grid, z=z,
                envs=envs)


def setting(c, s):
    return mppi_ref.setting_from_params(c["p"], c["X0"][s], c["goal"][s], c["unom"][s],
                                        None if c["obs"] is None else c["obs"][s], c["grid"][s])


def noise_of(c, s):
    p = c["p"]
    if c["z"] is not None:
        return mppi_ref.external_noise(c["z"][s])
    return mppi_ref.philox_noise(p.seed, p.offset, s + p.scene_base, p.H)


@functools.lru_cache(maxsize=None)
def _restatement(name, s):
    c = build(name)
    st, noise = setting(c, s), noise_of(c, s)
    ref = mppi_ref.MPPIPlan(st, noise)
    holders = ref["coll"] + mppi_ref.rollouts_beyond(st, noise, len(ref["coll"]))
    ref["arrays"] = mppi_ref.collection_arrays(holders, c["p"].H)
    return ref


def restatement(c, s):
    """MPPIPlan of scene s by tests/mppi_ref.py, with arrays = all K holders (computed once per process)."""
    return _restatement(c["name"], s)


class env:
    """with env({...}): the launch hooks tests/test_gpu_mppi_lean.py sets, restored afterwards."""

    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def exact_mppictrl(cost, ctrl, lam):
    """(U*, bound): U* (H, 2) of Decimals, bound (H, 2) of Decimals (module docstring).  cost (m,) finite,
    ctrl (m, H, 2)."""
    cost = [float(v) for v in cost]
    ctrl = np.asarray(ctrl, np.float64)
    m, H = len(cost), ctrl.shape[1]
    with localcontext() as cx:
        cx.prec = 60
        c = [Decimal(v) for v in cost]
        rho = min(c)
        lam = Decimal(float(lam))
        x = [(ci - rho) / lam for ci in c]
        E = [(-xi).exp() for xi in x]
        D = sum(E)
        w = [Ei / D for Ei in E]
        u = Decimal(U_ROUND)
        n_add = m + 2
        k = [u * wi * (n_add + 3 * xi + Decimal(2 * C_EXP)) for wi, xi in zip(w, x)]
        ksum = sum(k)
        tiny = Decimal(2) ** -1000
        slack = Decimal("1.01")
        Ustar = np.empty((H, 2), object)
        bound = np.empty((H, 2), object)
        for t in range(H):
            for j in range(2):
                ut = [Decimal(float(ctrl[i, t, j])) for i in range(m)]
                us = sum(wi * v for wi, v in zip(w, ut))
                num = sum((ki + tiny) * abs(v) for ki, v in zip(k, ut))
                Ustar[t, j] = us
                bound[t, j] = slack * (num + abs(us) * ksum)
    return Ustar, bound


def error_ratio(U, Ustar, bound):
    """max over entries of |U - U*| / bound (0 where both are 0; inf where only the bound is)."""
    U = np.asarray(U, np.float64)
    worst = 0.0
    with localcontext() as cx:
        cx.prec = 60
        for idx in np.ndindex(U.shape):
            err = abs(Decimal(float(U[idx])) - Ustar[idx])
            if bound[idx] == 0:
                worst = max(worst, 0.0 if err == 0 else float("inf"))
            else:
                worst = max(worst, float(err / bound[idx]))
    return worst
