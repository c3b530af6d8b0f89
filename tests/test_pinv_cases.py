"""CPU conditions on the corpus of tests/pinv_cases.py: what tests/test_gpu_pinv.py compares on the device is
only worth something if the corpus runs every branch of the 2x2 pinv, so that is asserted here, without a GPU."""
import numpy as np

import oracle
import pinv_cases as pc


def test_corpus_sets_every_rare_disjunct():
    """Each disjunct of mpj_pinv2_fast's rare expression (oracle.RARE_DISJUNCTS, the bit mask that
    or_pinv2_fast_mask_batch returns) is set by at least one finite corpus matrix, and by one that sets no other
    disjunct, so each has a witness of its own -- except two that cannot be set alone: a21 == 0 makes
    v2 = a21 * (1 / (a11 - beta)) zero, or NaN when a11 is zero too (d1 = 0 then sets the split and S0 > 0
    terms), and ub1 == ub3 == 0 needs |m| > 6.7e153 (t*t overflows while m*m does not, so both rotations come
    out zero: pinv_cases.edge_block), which implies gbig && fa/ga < eps.  None is unreachable."""
    c = pc.corpus()
    fin = np.isfinite(c["M"]).all(axis=(1, 2))
    for bit, name in enumerate(oracle.RARE_DISJUNCTS):
        hit = (c["mask"] >> bit) & 1 == 1
        assert (hit & fin).any(), name
        if name not in ("a21 == 0", "ub1 == ub3 == 0"):
            assert (fin & (c["mask"] == 1 << bit)).any(), name
    assert (c["mask"] >= 0).all() and (c["mask"] < 256).all()
    assert np.array_equal(c["rare"], (c["mask"] != 0).astype(np.int32))
    # the symmetric Quu-like block is generic throughout, the diagonal block rare throughout
    assert c["rare"][c["blocks"]["quu"]].sum() == 0 and c["rare"][c["blocks"]["diag"]].all()


def test_corpus_holds_the_special_values():
    """+-0, +-Inf, NaN, subnormals (5e-324, 1e-310) and near-overflow (1e307) entries are all present, and the
    CPU results over them include NaN, Inf and subnormal outputs (the comparison's NaN mask is exercised)."""
    c = pc.corpus()
    M = c["M"]
    assert np.isnan(M).any() and np.isposinf(M).any() and np.isneginf(M).any()
    assert ((M == 0) & np.signbit(M)).any() and ((M == 0) & ~np.signbit(M)).any()
    for v in (5e-324, -5e-324, 1e-310, -1e-310, 1e307, -1e307):
        assert (M == v).any(), v
    P = c["P"]  # (never Inf: Julia's pinv(x::Number) zeroes an infinite inverse)
    assert np.isnan(P).any() and (~np.isnan(P)).any() and np.isinf(c["S"]).any() and np.isnan(c["U"]).any()
    tiny = np.abs(P[np.isfinite(P)])
    assert ((tiny > 0) & (tiny < 2.2250738585072014e-308)).any()


def test_fast_path_equals_exact_where_not_rare():
    """On the CPU build: mpj_pinv2_fast == mpj_pinv2 wherever it does not flag rare, over the whole corpus
    (special values included), and the layouts' class matrices are rare while G is not."""
    c = pc.corpus()
    ok = c["rare"] == 0
    assert ok.sum() > 20000
    pc.assert_bits(c["Pf"][ok], c["P"][ok], "pinv2_fast vs pinv2")
    g, classes = pc.rare_classes()
    assert set(oracle.RARE_DISJUNCTS) <= set(classes)
    _, rare = oracle.pinv2_fast_batch(np.stack([g] + list(classes.values())))
    assert rare[0] == 0 and rare[1:].all()
