"""include/mp_jlmath.h, host build: mpj_atan_rows (the 81-row range table indexed by the clamped
ix >> 15) equals mpj_atan bit for bit, and the exact cheap division helpers equal `/` (on the host
they are `/` by definition: this pins their signatures and the guard's window)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "%s/include/mp_jlmath.h"
/* in: n doubles x, n doubles y.  out: atan(x), atan_rows(x), x / y, and the five helper forms */
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  long n;
  if (!f || fread(&n, sizeof n, 1, f) != 1) return 2;
  double* x = malloc(sizeof(double) * n), *y = malloc(sizeof(double) * n), *o = malloc(sizeof(double) * n * 9);
  if (fread(x, sizeof(double), n, f) != (size_t)n || fread(y, sizeof(double), n, f) != (size_t)n) return 2;
  fclose(f);
  double rows[4 * MPJ_ATAN_ROWS], rows2[4 * MPJ_ATAN_ROWS];
  mpj_atan_rows_init(rows);
  for (unsigned t = 0; t < 64; t++) mpj_atan_rows_fill(rows2, t, 64); /* as a 64-thread block fills it */
  if (memcmp(rows, rows2, sizeof rows) != 0) return 3;
  for (long i = 0; i < n; i++) {
    double q1, q2, q3, q4;
    o[9 * i + 0] = mpj_atan(x[i]);
    o[9 * i + 1] = mpj_atan_rows(x[i], rows);
    o[9 * i + 2] = x[i] / y[i];
    o[9 * i + 3] = mpj_div_g(x[i], y[i]);
    o[9 * i + 4] = mpj_div_gn(x[i], y[i], mpj_rcp_nr(y[i]), !mpj_div_out(y[i]));
    o[9 * i + 5] = mpj_div_gf(x[i], y[i], mpj_rcp_nr(y[i]), !mpj_div_out(y[i]));
    mpj_div2_g(x[i], 1.0, y[i], &q1, &q2);
    mpj_div2_g(-1.5, x[i], y[i], &q3, &q4);
    o[9 * i + 6] = q1;
    o[9 * i + 7] = q4;
    o[9 * i + 8] = (double)(mpj_div_out(x[i]) | mpj_div_out(y[i]));
    if (memcmp(&q2, &(double){1.0 / y[i]}, 8) != 0 && q2 == q2) return 4;
    if (mpj_div_r(x[i], y[i], mpj_rcp_nr(y[i])) != x[i] / y[i] && x[i] / y[i] == x[i] / y[i]) return 5;
    if (mpj_div_rf(x[i], y[i], mpj_rcp_nr(y[i])) != x[i] / y[i] && x[i] / y[i] == x[i] / y[i]) return 5;
  }
  f = fopen(argv[2], "wb");
  fwrite(o, sizeof(double), n * 9, f);
  fclose(f);
  return 0;
}
'''


def bucket_boundaries():
    """Every boundary of the 81 rows (high word (0x7fb7 + i) << 15, low word 0), one ulp on each side."""
    hi = (np.arange(0x7fb7, 0x8009, dtype=np.uint64) << np.uint64(15)) << np.uint64(32)
    b = hi.view(np.float64)
    return np.concatenate([b, np.nextafter(b, 0.0), np.nextafter(b, np.inf)])


def atan_inputs():
    r = np.random.default_rng(41)
    b = bucket_boundaries()
    sp = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 2.0 ** -27, np.nextafter(2.0 ** -27, 0),
                   np.nextafter(2.0 ** -27, 1), 0.5, 1.0, 1.5, 2.0 ** 66, np.nextafter(2.0 ** 66, 0),
                   np.nextafter(2.0 ** 66, np.inf), 2.0 ** 67, 1e300, 1.7976931348623157e308, np.inf])
    rnd = np.exp(r.uniform(np.log(1e-310), np.log(1e300), 200000))
    pos = np.concatenate([b, sp, rnd])
    return np.concatenate([pos, -pos, [np.nan]])


def div_inputs(n_rand=50000, seed=43):
    """(numerator, divisor) pairs: log-uniform magnitudes over the whole exponent range, both signs; the tyre
    ranges; zero / Inf / NaN operands; operands and quotients at each edge of the scaling window; subnormal
    numerators."""
    r = np.random.default_rng(seed)

    def logu(n, lo=-1074.0, hi=1023.99):
        return np.ldexp(r.uniform(1.0, 2.0, n), np.floor(r.uniform(lo, hi, n)).astype(int)) * r.choice([-1.0, 1.0], n)

    xs, ys = [logu(n_rand)], [logu(n_rand)]
    # tyre ranges: |n| <= 1e3, d in ±[1e-320, 1e2] and ±0
    m = 6000
    xs.append(r.uniform(-1e3, 1e3, m))
    d = np.exp(r.uniform(np.log(1e-320), np.log(1e2), m)) * r.choice([-1.0, 1.0], m)
    d[:40] = np.tile([0.0, -0.0], 20)
    ys.append(d)
    sp_n = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    sp_d = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 2020.0, -4095.0, 1e-300, 5e-324])
    g = np.array(np.meshgrid(np.r_[sp_n, 1.0, -3.5, 5e-324, 1e300], sp_d)).reshape(2, -1)
    xs.append(g[0])
    ys.append(g[1])
    # the edges: biased exponents 0 / 1 (subnormal | normal), 53 / 54 (tiny numerator), 0x27f / 0x280 and
    # 0x57f / 0x580 (the guard's window), 2044 / 2045 (1/d subnormal), 2046; differences ±767 / ±768, -1022 / -1023
    e_edges = [-1074, -1060, -1023, -1022, -1021, -971, -970, -969, -968, -385, -384, -383, -382, -1, 0, 1, 383, 384,
               385, 386, 1020, 1021, 1022, 1023]
    for man in (1.0, 1.5, 2.0 - 2.0 ** -52):
        g = np.array(np.meshgrid(e_edges, e_edges)).reshape(2, -1)
        xs.append(np.ldexp(man, g[0]))
        ys.append(np.ldexp(1.25, g[1]) * -1.0)
        for diff in (766, 767, 768, 769, -766, -767, -768, -1021, -1022, -1023, -1024, -1074):
            for ed in range(-1022, 1024, 31):
                if -1074 <= ed + diff <= 1023:
                    xs.append(np.array([np.ldexp(man, ed + diff)]))
                    ys.append(np.array([np.ldexp(1.75, ed)]))
    # subnormal numerators over ordinary divisors
    xs.append(np.ldexp(r.uniform(0.0, 1.0, 2000), -1022) * r.choice([-1.0, 1.0], 2000))
    ys.append(logu(2000, -40.0, 40.0))
    return np.concatenate(xs).astype(np.float64), np.concatenate(ys).astype(np.float64)


def guard_out(x):
    """mpj_div_out: the biased exponent is outside the window [0x280, 0x57f]."""
    key = (np.ascontiguousarray(x).view(np.uint64) >> np.uint64(32)) & np.uint64(0x7fffffff)
    return (key < 0x28000000) | (key >= 0x58000000)


def same_bits(a, b):
    """Bit for bit, NaN matching NaN (the sign and payload of a generated NaN differ between x86 and the GPU)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("rows")
    src, exe = d / "rows.c", d / "rows"
    src.write_text(SRC % ROOT)
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-include", "string.h", str(src), "-o", str(exe),
                    "-lm"], check=True)

    def run(x, y):
        with open(d / "in.bin", "wb") as f:
            f.write(np.int64(len(x)).tobytes())
            f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(y, dtype=np.float64).tobytes())
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        return np.fromfile(d / "out.bin", dtype=np.float64).reshape(len(x), 9)

    return run


def test_atan_rows_equals_atan(host):
    x = atan_inputs()
    o = host(x, np.ones_like(x))
    ok = same_bits(o[:, 0], o[:, 1])
    assert ok.all(), x[~ok][:8]
    assert len(bucket_boundaries()) == 3 * 82


def test_division_helpers_equal_division(host):
    x, y = div_inputs()
    o = host(x, y)
    with np.errstate(all="ignore"):
        ref = x / y
    assert same_bits(o[:, 2], ref).all()
    for col, name in ((3, "div_g"), (4, "div_gn"), (5, "div_gf"), (6, "div2_g first"), (7, "div2_g second")):
        ok = same_bits(o[:, col], ref)
        assert ok.all(), (name, x[~ok][:4], y[~ok][:4])
    assert np.array_equal(o[:, 8] != 0, guard_out(x) | guard_out(y))
