"""field29.h (the radix-2^29 Fq of the MSM accumulation, the MSM tail and
the wave engine's products) checked on the host against Python integers:
Montgomery product / square / add / sub, the one-reduction sum of two
products (mul_sum / mul_sub), the conversions from and to
field.h's layout (R = 2^384 <-> 2^377), the packed bucket format (pack377 /
unpack377: the R = 2^377 value's bits in 12 words), the binary-GCD inverse, and the wave
engine's stage product on unreduced operands (a form of weight w is < w p;
the engine feeds products with w_x w_y <= 64, squares with w <= 8)."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001
R = 1 << 384
RI = pow(R, -1, P)


def _w(v):
    return " ".join("%x" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(12))


def _parse(line):
    return sum(int(t, 16) << (32 * i) for i, t in enumerate(line.split()))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("f29") / "test_field29")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_field29.cpp"), "-o", out], check=True)
    return out


def _run(exe, rows):
    inp = "%d\n" % len(rows) + "\n".join("%d %s %s" % (w, _w(a), _w(b)) for w, a, b in rows)
    return subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")


def test_field29_ops_and_inverse(exe):
    rng = random.Random(29)
    vals = [(0, 0), (1, P - 1), (P - 1, P - 1), (P - 1, 1), (1 << 376, 3)]
    vals += [(rng.randrange(P), rng.randrange(P)) for _ in range(2000)]
    out = _run(exe, [(0, a * R % P, b * R % P) for a, b in vals])
    for k, (a, b) in enumerate(vals):
        got = [_parse(out[12 * k + j]) for j in range(12)]
        exp = [a * b % P * R % P, a * a % P * R % P, (a + b) % P * R % P, (a - b) % P * R % P, a * R % P,
               (pow(a, -1, P) * R % P) if a else 0, (a * b + a * a) % P * R % P, (a * b - b * b) % P * R % P,
               a * (1 << 377) % P, a * R % P, (-a) % P * R % P, a * R % P]
        assert got == exp, (a, b)


def test_field29_constructed_edge_operands(exe):
    """Radix-2^29 operands X, Y chosen in the R = 2^377 domain itself
    (arith_vectors.py asserts each class's property from integers): products,
    squares and product sums whose reduction word m_k is zero for every
    column k and for pairs of columns -- where the carry ceil(acc / 2^29)
    differs from floor(acc / 2^29) + 1 --, the bound cases of mul_sum /
    mul_sub, and values Y with 128 Y within 128 of a multiple of p, the
    q - 1 arm of to_std's quotient estimate.  The exe applies from_std to
    its input, so it is fed V = X 2^7 mod p."""
    import arith_vectors as V
    F = V.F29
    rng = random.Random(31)
    prs = [(P - 1, P - 1), (P - 1, 0), (0, P - 1), (F.R % P, F.R % P)]
    for cols in V.mk0_columns(F):
        prs += V.mul_mk0(F, rng, cols)
        a = rng.randrange(1, P) | 1
        prs += [(a, b) for b in V.solve_mk0(F, rng, cols, a * a, a, "mul_sum")]
        b = rng.randrange(1, P) | 1
        prs += [(a2, b) for a2 in V.solve_mk0(F, rng, cols, b * (P - b), b, "mul_sub")]
    sq = V.sqr_m0(F, rng)
    for k in range(1, F.n):
        sq += V.sqr_mk0(F, rng, k)
    prs += [(x, rng.randrange(P)) for x in sq]
    for q in range(1, 128):
        y = -(-q * P // 128)
        assert min(128 * y % P, P - 128 * y % P) <= 128 and min(128 * (y - 1) % P, P - 128 * (y - 1) % P) <= 128
        prs += [(y, y - 1), (y - 1, y)]
    assert len(prs) > 13 * 6 + 12 + 254
    out = _run(exe, [(0, x * 128 % P, y * 128 % P) for x, y in prs])
    Ri = F.Ri
    for k, (x, y) in enumerate(prs):
        got = [_parse(out[12 * k + j]) for j in range(12)]
        v = x * 128 % P
        exp = [x * y * Ri * 128 % P, x * x * Ri * 128 % P, (x + y) * 128 % P, (x - y) * 128 % P, v,
               (pow(v, -1, P) * R * R % P) if v else 0, (x * y + x * x) * Ri * 128 % P,
               (x * y - y * y) * Ri * 128 % P, x, v, (-x) * 128 % P, v]
        assert got == exp, (hex(x), hex(y), [i for i in range(12) if got[i] != exp[i]])


def test_field29_wave_stage_products_on_wide_operands(exe):
    rng = random.Random(30)
    rows = []
    for wx in (1, 2, 4, 8, 16, 32, 64):
        wy = max(1, 64 // wx)
        rows += [(1, rng.randrange(wx * P), rng.randrange(wy * P)) for _ in range(300)]
        rows.append((1, wx * P - 1, wy * P - 1))
    out = _run(exe, rows)
    for k, (_, a, b) in enumerate(rows):
        assert _parse(out[2 * k]) == a * b * RI % P
        if a < 8 * P:
            assert _parse(out[2 * k + 1]) == a * a * RI % P
