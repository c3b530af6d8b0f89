"""Device build of the 2x2 pinv and SVD of include/mp_jlmath.h vs the CPU build, bit for bit (mp_pinv2_eval).

The device code object is another compile of that header (gfx950's expanded f64 sqrt and division, explicit
fma only, MPJ_SEL as forced selects, MPJ_ANY as a wave vote), and the iLQR Riccati sweep and cubic_fit rest on
it.  The corpus (tests/pinv_cases.py) reaches every branch, as tests/test_pinv_cases.py asserts on the CPU:
every disjunct of mpj_pinv2_fast's rare expression, the isdiag branch, the rank cut-off, and +-0, +-Inf, NaN,
subnormal and near-overflow entries.  Where the CPU result is NaN the NaN mask is compared, every other entry
by its bits.
"""
import numpy as np
import pytest

import pinv_cases as pc
from motionplanning_amd.abi import ptr

pytestmark = pytest.mark.gpu

EXACT, BL, FAST, SVD = 0, 1, 2, 3


def _eval(ctx, mode, M, want_rare=False):
    M = np.ascontiguousarray(M, np.float64).reshape(-1, 4)
    out = np.full((len(M), 10 if mode == SVD else 4), 7.0)
    rare = np.full(len(M), -1, np.int32) if want_rare else None
    ctx.check(ctx.lib.mp_pinv2_eval(ctx.handle, mode, len(M), ptr(M), ptr(out), ptr(rare)))
    if mode == SVD:
        return out[:, :4].reshape(-1, 2, 2), out[:, 4:6].copy(), out[:, 6:].reshape(-1, 2, 2)
    out = out.reshape(-1, 2, 2)
    return (out, rare) if want_rare else out


def test_exact_pinv_bitexact(ctx):
    c = pc.corpus()
    pc.assert_bits(_eval(ctx, EXACT, c["M"]), c["P"], "mpj_pinv2")


def test_svd_bitexact(ctx):
    c = pc.corpus()
    U, S, VT = _eval(ctx, SVD, c["M"])
    pc.assert_bits(U, c["U"], "mpj_svd2 U")
    pc.assert_bits(S, c["S"], "mpj_svd2 S")
    pc.assert_bits(VT, c["VT"], "mpj_svd2 VT")


def test_fast_pinv_and_rare_flags(ctx):
    c = pc.corpus()
    P, rare = _eval(ctx, FAST, c["M"], want_rare=True)
    assert np.array_equal(rare != 0, c["rare"] != 0), np.flatnonzero((rare != 0) != (c["rare"] != 0))[:8]
    ok = c["rare"] == 0
    pc.assert_bits(P[ok], c["Pf"][ok], "mpj_pinv2_fast where not rare")
    pc.assert_bits(P[ok], c["P"][ok], "mpj_pinv2_fast vs mpj_pinv2 where not rare")


def test_bl_pinv_bitexact_on_corpus(ctx):
    """mpj_pinv2_bl == mpj_pinv2 everywhere: the corpus in its own order (waves that mix generic and rare
    lanes, all-generic waves in the Quu block) and reversed (other wave mates)."""
    c = pc.corpus()
    pc.assert_bits(_eval(ctx, BL, c["M"]), c["P"], "mpj_pinv2_bl")
    pc.assert_bits(_eval(ctx, BL, c["M"][::-1]), c["P"][::-1], "mpj_pinv2_bl, reversed")


def _layouts():
    """(name, M, expected P): per rare class R and the generic G -- n in {1, 63, 64, 65, 257} of R, and of G
    with R in the middle; one wave of G with a single R at lane 0, 31, 32 or 63; an all-R wave next to an
    all-G wave, in both orders."""
    import oracle

    g, classes = pc.rare_classes()
    out = []
    for cname, r in classes.items():
        for n in (1, 63, 64, 65, 257):
            out.append(("%s: n=%d all R" % (cname, n), np.repeat(r[None], n, 0)))
            m = np.repeat(g[None], n, 0)
            m[n // 2] = r
            out.append(("%s: n=%d G with one R" % (cname, n), m))
        for lane in (0, 31, 32, 63):
            m = np.repeat(g[None], 64, 0)
            m[lane] = r
            out.append(("%s: R at lane %d" % (cname, lane), m))
        rw, gw = np.repeat(r[None], 64, 0), np.repeat(g[None], 64, 0)
        out.append(("%s: R wave, G wave" % cname, np.concatenate([rw, gw])))
        out.append(("%s: G wave, R wave" % cname, np.concatenate([gw, rw])))
    for n in (1, 63, 64, 65, 257):
        out.append(("n=%d all G" % n, np.repeat(g[None], n, 0)))
    return [(name, m, oracle.pinv2_batch(m), oracle.pinv2_fast_batch(m)) for name, m in out]


def test_wave_layouts(ctx):
    """The header's promise for the wave-uniform fallback -- "the result never depends on which lanes are
    active": in every layout each matrix gets its CPU result, whether its wave takes the fallback for it, for a
    neighbour, or not at all, with partial waves and a second block (n = 257) included."""
    for name, m, P, (Pf, rare) in _layouts():
        pc.assert_bits(_eval(ctx, BL, m), P, "bl, " + name)
        got, grare = _eval(ctx, FAST, m, want_rare=True)
        assert np.array_equal(grare != 0, rare != 0), name
        pc.assert_bits(got[rare == 0], P[rare == 0], "fast, " + name)
        pc.assert_bits(_eval(ctx, EXACT, m), P, "exact, " + name)


def test_bad_arguments(ctx):
    from motionplanning_amd.abi import MP_ERR_INVALID

    m, o = np.zeros((1, 4)), np.zeros((1, 10))
    assert ctx.lib.mp_pinv2_eval(ctx.handle, 4, 1, ptr(m), ptr(o), None) == MP_ERR_INVALID
    assert ctx.lib.mp_pinv2_eval(ctx.handle, -1, 1, ptr(m), ptr(o), None) == MP_ERR_INVALID
    assert ctx.lib.mp_pinv2_eval(ctx.handle, 0, 1, None, ptr(o), None) == MP_ERR_INVALID
    assert ctx.lib.mp_pinv2_eval(ctx.handle, 0, 0, ptr(m), ptr(o), None) == 0
