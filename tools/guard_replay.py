"""Replay of the MPJ_ANY slow-path guards of the lean MPPI rollout step on the CPU oracle.

The trajectories are bit-exact, so the oracle's collected states and controls of the bench's scenes 0-2
(configs.cfg5_shard(0, 8, Philox, seed 20260415), offset 7, zero nominal control) are the device's.  Each guard's
condition is evaluated on them with the rollouts grouped in 64s (one rollout per lane) and the share of wave-steps
on which some lane fires is printed.  The intermediate operands (slip quotients, tyre forces, the second RK2 stage)
are recomputed here in numpy float64, not with the device's libm: enough for the window conditions, whose only
reachable case is an exact zero, and for the sin_34 range test; its 2^-20 high-word pattern is then only indicative.
Not replayed: the Box-Muller draw's mpj_log_bl and mpj_sincos_bl guards (the Philox stream is not regenerated here);
by their conditions they take 3 and 1 high words in 2^20 per lane.

  python tools/guard_replay.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import oracle
from motionplanning_amd import configs
from motionplanning_amd.abi import MP_NOISE_PHILOX
c = configs.cfg5_shard(0, 8, MP_NOISE_PHILOX, seed=20260415)
p = c["params"]; p.offset = 7
K, H, dt = p.K, p.H, p.dt
la, lb, M, Izz, g, mu = 1.56, 1.64, 2020.0, 4095.0, 9.81, 0.8
KFZF, KFZR, KFZX = 1018.28/2, 963.34/2, 186.22
B, C, E = -10.4/mu, 1.3, 0.1556
def hi(x): return (np.ascontiguousarray(x).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
def div_out(x):
    k = hi(x) & np.uint32(0x7fffffff)
    return (k - np.uint32(0x28000000)) >= np.uint32(0x30000000)
def sc_guard(x):
    xhp = hi(x) & np.uint32(0x7fffffff)
    ext = ((xhp <= 0x400f6a7a) & ((xhp & 0xfffff) == 0x921fb)) | (xhp == 0x4012d97c) | (xhp == 0x401921fb)
    return (xhp > 0x401c463b) | (~(np.abs(x) < np.pi/4) & ext)
def s34_guard(x):
    xhp = hi(x) & np.uint32(0x7fffffff)
    return (xhp > 0x4002d97c) | (~(np.abs(x) < np.pi/4) & ((xhp & 0xfffff) == 0x921fb))
def dyn(x, sr, ax, G, tag):
    v, r, psi, ux, sa = x[...,2], x[...,3], x[...,4], x[...,5], x[...,6]
    t = (ax - r*v)*KFZX
    FZf, FZr = 2*(KFZF*g - t), 2*(KFZR*g + t)
    n1, n2, d = v + la*r, v - lb*r, ux + 0.01
    G[tag+' div2_g(slip quotients)'] = div_out(n1) | div_out(n2) | div_out(d)
    with np.errstate(all='ignore'):
        af, ar = np.arctan(n1/d) - sa, np.arctan(n2/d)
    Xf, Xr = B*af, B*ar
    a1, a2 = C*np.arctan(Xf - E*(Xf - np.arctan(Xf))), C*np.arctan(Xr - E*(Xr - np.arctan(Xr)))
    G[tag+' sin_34 front'] = s34_guard(a1); G[tag+' sin_34 rear'] = s34_guard(a2)
    FY1, FY2 = mu*FZf*np.sin(a1), mu*FZr*np.sin(a2)
    G[tag+' div_gn (FY1+FY2)/M'] = div_out(FY1+FY2)
    G[tag+' div_gn (FY1 la-FY2 lb)/Izz'] = div_out(FY1*la - FY2*lb)
    G[tag+' sincos_bl(psi)'] = sc_guard(psi)
    uxc = np.where(ux <= 0, 0.0, ux)
    return np.stack([uxc*np.cos(psi)-v*np.sin(psi), uxc*np.sin(psi)+v*np.cos(psi), (FY1+FY2)/M - r*uxc,
                     (FY1*la-FY2*lb)/Izz, r, ax+0*r, sr+0*r], axis=-1)
tot = {}; nws = 0
for s in range(3):
    ref = oracle.mppi_plan(p, c["X0"][s], c["goal"][s], np.zeros((H,2)), None, c["grid"][s], None, scene=s, collect=True)
    tr, u = ref["coll"]["traj"], ref["coll"]["ctrl"]       # [K][H+1][7], [K][H][2]
    x = tr[:, :H, :]; sr, ax = u[..., 0], u[..., 1]
    G = {}
    k1 = dyn(x, sr, ax, G, 'stage 1')
    x2 = x + k1*dt
    dyn(x2, sr, ax, G, 'stage 2')
    xs = tr[:, 1:, :]                                     # obstacle_cost: steps 1..H (and the terminal)
    gx, gy = xs[..., 0] - p.grid_x0, xs[..., 1] - p.grid_y0
    G['obstacle div_gn fx (steps 1..H)'] = div_out(gx); G['obstacle div_gn fy (steps 1..H)'] = div_out(gy)
    for k_, m in G.items():
        w = m.reshape(K//64, 64, -1).any(axis=1)
        a = tot.setdefault(k_, [0, 0, np.zeros(w.shape[1], int)]); a[0] += int(w.sum()); a[1] += w.size; a[2] += w.sum(axis=0)
for k_, (n, N, per) in tot.items():
    steps = [int(i) for i in np.nonzero(per)[0]]
    print("%-44s %7d / %d wave-steps = %.4f   steps firing: %s" % (k_, n, N, n/N, steps[:6]))
