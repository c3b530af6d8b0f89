"""The 2x2 corpus shared by tests/test_pinv_cases.py (CPU) and tests/test_gpu_pinv.py (GPU): the matrices on
which the device build of mpj_svd2 / mpj_pinv2 / mpj_pinv2_fast / mpj_pinv2_bl (include/mp_jlmath.h, through
mp_pinv2_eval) is compared with the CPU build bit for bit -- test infrastructure only.

Built once from fixed seeds and cached read-only with its CPU results.  The CPU test asserts that every
disjunct of mpj_pinv2_fast's rare expression is set by some matrix of it, so the GPU comparison cannot pass
without having run the rare paths.
"""
import functools
import itertools

import numpy as np

import oracle
from test_jlmath import _families

# +-0, +-Inf, NaN, the smallest subnormal, a mid subnormal, near-overflow, and two ordinary values
SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, -1e-310, 1e307, -1e307, 1.0, -1.5, 3.0e-3]


def diag_block(r):
    """The diagonal, zero and singular-diagonal block of test_jlmath.test_pinv2_is_julia_pinv."""
    d = np.zeros((40, 2, 2))
    d[:, 0, 0], d[:, 1, 1] = r.standard_normal(40), r.standard_normal(40)
    d[:10, 1, 1] = 0.0
    d[10:20, 0, 0] = 1e-17 * d[10:20, 1, 1]
    d[20, :, :] = 0.0
    d[21, 0, 1] = -0.0
    return d


def quu_like(r, n):
    q = r.standard_normal((n, 2, 2)) * 10.0 ** r.integers(-3, 5, (n, 1, 1))
    return q + np.swapaxes(q, 1, 2)


def special_block(r):
    """Every 2x2 over SPECIALS, and ordinary matrices with one or two entries replaced by a special value."""
    full = np.array(list(itertools.product(SPECIALS, repeat=4))).reshape(-1, 2, 2)
    m = r.standard_normal((4000, 2, 2)) * 10.0 ** r.integers(-3, 4, (4000, 1, 1))
    sp = np.array(SPECIALS)
    i = np.arange(4000)
    m.reshape(4000, 4)[i, r.integers(0, 4, 4000)] = sp[r.integers(0, len(sp), 4000)]
    m.reshape(4000, 4)[i[:2000], r.integers(0, 4, 2000)] = sp[r.integers(0, len(sp), 2000)]
    return np.concatenate([full, m])


def edge_block():
    """Finite matrices aimed at the branches no random family reaches: v2 underflowing to 0 with a21 != 0,
    dlasv2's gbig && fa/ga < eps (|e1| more than 1/eps times both diagonals), mm == 0 (m = g/f underflowing in
    the square), the dbdsqr split on a non-triangular matrix, the 2 eps rank cut-off on either side, and
    ub1 == ub3 == 0: |m| = |e1/d1| in (0.67e154, 1.34e154), where m*m is finite but t*t (t ~ 2|m|) overflows, so
    l = Inf and crt = 2/l = srt = t/l = 0 -- both rotations come out zero (the exact routine takes dlasv2's
    gasmal = 0 branch there)."""
    e = [[[1e-77, 1e77], [1e-232, 0.0]], [[1e-77, 1e77], [1e-232, 1e-78]], [[-1e-77, 1e77], [1e-240, 1e-80]],
         [[1e-70, 1.1e84], [-1e-230, 3e-71]], [[1e-77, 1e77], [1e-77, 1e77]], [[1e-78, 1e77], [1e-232, 1e-77]],
         [[1e-3, 1e15], [1e-30, 1e-2]], [[2.0, 1e17], [1e-9, 0.5]],
         [[1.0, 1.0], [5e-324, 1.0]], [[1e10, 2.0], [1e-310, 3.0]], [[-1.0, 0.5], [-5e-324, 2.0]],
         [[1e-17, 1.0], [1e-18, 1e-17]], [[1e-20, 3.0], [2e-20, -1e-19]], [[1e-3, 1e15], [1e-3, 1e-2]],
         [[1.0, 1e-170], [1e-170, 1.0]], [[1e100, 1e-80], [1e-90, 1e100]], [[2.0, 1e-200], [1e-10, -3.0]],
         [[1.0, 1e-15], [1e-15, 1.0]], [[1.0, 2e-14], [2e-14, 1.0]], [[5.0, 1e-16], [1e-3, 7.0]],
         [[1.0, 1.0], [1.0, 1.0 + 2.0 ** -51]], [[1.0, 1.0], [1.0, 1.0 + 2.0 ** -50]],
         [[1.0, 1.0], [1.0, 1.0 + 2.0 ** -52]], [[3.0, 6.0], [1.0, 2.0 + 2.0 ** -50]]]
    e = np.array(e)
    return np.concatenate([e, -e, np.swapaxes(e, 1, 2), e[:, ::-1, :].copy(), e[:, :, ::-1].copy()])


@functools.lru_cache(maxsize=None)
def corpus():
    """dict(M (n, 2, 2), P pinv2, Pf / rare / mask pinv2_fast, U / S / VT svd2, blocks {name: slice}), read-only."""
    r = np.random.default_rng(31)
    parts = [("families", _families(r, 2000)), ("diag", diag_block(r)), ("quu", quu_like(r, 20000)),
             ("special", special_block(r)), ("edge", edge_block())]
    M = np.ascontiguousarray(np.concatenate([p for _, p in parts]))
    blocks, at = {}, 0
    for name, p in parts:
        blocks[name] = slice(at, at + len(p))
        at += len(p)
    with np.errstate(all="ignore"):
        Pf, rare, mask = oracle.pinv2_fast_batch(M, want_mask=True)
        U, S, VT = oracle.svd2_batch(M)
        out = dict(M=M, P=oracle.pinv2_batch(M), Pf=Pf, rare=rare, mask=mask, U=U, S=S, VT=VT)
    for v in out.values():
        v.setflags(write=False)
    out["blocks"] = blocks
    return out


def rare_classes():
    """(G, {class: R}): one generic matrix and one finite rare matrix per class -- per disjunct of the rare
    expression the first corpus matrix that sets that disjunct alone (else the first that sets it at all), and
    the branches of mpj_pinv2 that several disjuncts share: diagonal, singular diagonal, zero."""
    c = corpus()
    fin = np.isfinite(c["M"]).all(axis=(1, 2))
    out = {}
    for bit, name in enumerate(oracle.RARE_DISJUNCTS):
        alone = np.flatnonzero(fin & (c["mask"] == 1 << bit))
        idx = alone if len(alone) else np.flatnonzero(fin & ((c["mask"] >> bit) & 1 == 1))
        out[name] = c["M"][idx[0]].copy()
    d = c["M"][c["blocks"]["diag"]]
    out.update({"diagonal": d[30].copy(), "singular diagonal": d[0].copy(), "zero": d[20].copy()})
    g = c["M"][c["blocks"]["quu"]][0].copy()
    assert c["rare"][c["blocks"]["quu"]][0] == 0
    return g, out


def assert_bits(got, ref, what=""):
    """Bit-for-bit equality of two float64 arrays; where the reference is NaN only the NaN mask is compared."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(np.int64) != ref.view(np.int64)))
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError("%s: %d entries differ, first at %s: got %r, CPU %r" %
                             (what, int(bad.sum()), tuple(i), got[tuple(i)], ref[tuple(i)]))
