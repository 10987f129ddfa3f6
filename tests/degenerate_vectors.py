"""Degenerate polynomials and points for the sqrt-PST commit / open / verify
flow, built from integers, with the class properties each case must keep.

Layout (sqrt_pst.rs:32-75): C = 2^(n // 2) row polynomials of 2^(n - n // 2)
entries, Z[(j << m_col) | i] = entry j of row i, so row i is the index set
idx % C == i.  The point splits into a = point[:m_row] (the PST side) and
b = point[m_row:] (the chi weights of the rows, MSB first).

Zr / ptr are the random polynomial and point of test_sqrt_pst_vs_cpu_oracle
(fr_stream(0x7E57D0, ...)); every case degenerates one of the two:

  zero        Z = 0                                   every element infinity / 1
  const       Z = 7 everywhere                        every PST quotient zero
  const_max   Z = r - 1 everywhere
  two_rows    Zr, rows i >= 2 zeroed                  C - 2 infinity commitments
  upper_rows  Zr, rows i < C / 2 zeroed               the shape of a padded witness
  one_row     Zr, rows i != 1 zeroed                  one live row
  one_col     Zr, entries j >= 1 of each row zeroed
  boolean_Z   Z in {0, 1} from default_rng(1)
  b_boolean   Zr; b = 0, 1, 0, 1, ...                 chi(b) a unit vector
  a_boolean   Zr; a = 1, 0, 1, 0, ...
  point_0 / point_1 / point_max   Zr; every coordinate 0, 1 or r - 1

`check_class` asserts the properties on a commitment and a proof -- on the
reference's first, so that a case cannot quietly stop being degenerate, then
on the device's.  Where a property is a count it is structural (which rows are
zero); for comms_u / comms_t only the presence of an infinity / a one is
stated ("all", "some", "none"), the values themselves are compared with the
oracle.

TEST INFRASTRUCTURE ONLY.
"""
import functools

import numpy as np

import bls377 as O
import orc

SEED_Z = 0x7E57D0
SEED_SRS = 0x7E57D1

TABLE_CASES = ["zero", "const", "const_max", "two_rows", "upper_rows", "one_col", "boolean_Z", "b_boolean",
               "a_boolean", "point_0", "point_1", "point_max"]
CASES = TABLE_CASES + ["one_row"]
# the cases whose openings run the look-ahead rounds (n = 10, 11) and the a-side rebase (n = 16, 17)
MID_CASES = ["zero", "const", "two_rows", "upper_rows", "b_boolean"]
# (case, n) of the CPU class-property test and of the GPU commit / open / verify test
GRID = ([(c, n) for n in (6, 7) for c in CASES] + [(c, n) for n in (10, 11, 16, 17) for c in MID_CASES]
        + [("point_max", 16), ("one_col", 16)])

GT_ONE = np.zeros(72, dtype=np.uint64)
GT_ONE[0] = 1


def fr(v):
    """one canonical Fr (4 little-endian u64 limbs) of the integer v"""
    v = int(v) % O.R
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)


def fr_int(a):
    return sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(a).reshape(4)))


def dims(n):
    m_col = n // 2
    return m_col, n - m_col, 1 << m_col


@functools.lru_cache(maxsize=None)
def _random(n):
    Z, k = orc.fr_stream(SEED_Z, 1 << n)
    pt, _ = orc.fr_stream(SEED_Z, n, k)
    Z.setflags(write=False)
    pt.setflags(write=False)
    return Z, pt


def live_rows(case, n):
    """the rows of the sqrt matrix that are not identically zero, from the case's definition"""
    C = dims(n)[2]
    return {"zero": [], "two_rows": [0, 1], "upper_rows": list(range(C // 2, C)), "one_row": [1]}.get(case, list(range(C)))


def inputs(case, n):
    """(Z (2^n, 4), point (n, 4)) of the case, canonical Fr limbs"""
    m_col, m_row, C = dims(n)
    Zr, ptr = _random(n)
    Z, pt = Zr.copy(), ptr.copy()
    row = np.arange(1 << n) % C     # i of Z[(j << m_col) | i]
    ent = np.arange(1 << n) >> m_col  # j
    if case == "zero":
        Z[:] = 0
    elif case == "const":
        Z[:] = fr(7)
    elif case == "const_max":
        Z[:] = fr(O.R - 1)
    elif case in ("two_rows", "upper_rows", "one_row"):
        Z[~np.isin(row, live_rows(case, n))] = 0
    elif case == "one_col":
        Z[ent >= 1] = 0
    elif case == "boolean_Z":
        Z[:] = 0
        Z[:, 0] = np.random.default_rng(1).integers(0, 2, 1 << n, dtype=np.uint64)
    elif case == "b_boolean":
        for t in range(m_col):
            pt[m_row + t] = fr(t % 2)
    elif case == "a_boolean":
        for t in range(m_row):
            pt[t] = fr(1 - t % 2)
    elif case in ("point_0", "point_1", "point_max"):
        pt[:] = fr({"point_0": 0, "point_1": 1, "point_max": O.R - 1}[case])
    else:
        raise KeyError(case)
    return Z, pt


def unit_row(case, n):
    """the row chi(b) selects when b is boolean (chi MSB first, sqrt_pst.rs:152-166), or None"""
    m_col = dims(n)[0]
    if case == "b_boolean":
        return sum((t % 2) << (m_col - 1 - t) for t in range(m_col))
    return {"point_0": 0, "point_1": (1 << m_col) - 1}.get(case)


def expected_eval(case, n, Z):
    """the evaluation where the case fixes it without field arithmetic, or None"""
    if case in ("zero", "const", "const_max"):
        return fr_int(Z[0])  # sum of chi = 1
    if case == "point_0":
        return fr_int(Z[0])
    if case == "point_1":
        return fr_int(Z[-1])
    return None


# presence of infinity in comms_u / of one in comms_t: "all", "some", "none" or None (not stated)
U_INF = {"zero": "all", "const": "none", "const_max": "none", "two_rows": "some", "upper_rows": "some",
         "one_row": "some", "b_boolean": "some", "point_0": "some", "point_1": "some"}
T_ONE = {"zero": "all", "const": "none", "const_max": "none", "two_rows": "some", "upper_rows": "some",
         "one_row": "some", "b_boolean": "none"}


def is_inf(a, width):
    """per point: True where the canonical affine encoding is all zero (infinity)"""
    return ~np.asarray(a, dtype=np.uint64).reshape(-1, width).any(axis=1)


def is_one(t):
    return (np.asarray(t, dtype=np.uint64).reshape(-1, 72) == GT_ONE).all(axis=1)


def _presence(flags, kind, what):
    if kind == "all":
        assert flags.all(), what
    elif kind == "some":
        assert flags.any(), what
    elif kind == "none":
        assert not flags.any(), what
    else:
        assert kind is None, kind


def check_class(case, n, Z, v, comms, T, pr):
    """the class properties of `case` on a commitment (comms, T), an evaluation
    v and an opening pr (dict: U, pst_proof, comms_t, comms_u, final_a,
    final_h, pst_proof_h)"""
    m_col, m_row, C = dims(n)
    tag = (case, n)
    # the input is what the case says: exactly the live rows are non-zero
    rows_nz = np.zeros(C, dtype=bool)
    rows_nz[np.nonzero(Z.any(axis=1))[0] % C] = True
    live = live_rows(case, n)
    assert sorted(np.nonzero(rows_nz)[0]) == live, tag
    # comm_list: infinity exactly at the zero rows
    assert list(np.nonzero(~is_inf(comms, 12))[0]) == live, tag
    assert int(is_inf(comms, 12).sum()) == {"zero": C, "two_rows": C - 2, "upper_rows": C // 2,
                                            "one_row": C - 1}.get(case, 0), tag
    # T = 1 and U, final_a at infinity for the zero polynomial only
    assert bool(is_one(T)[0]) == (case == "zero"), tag
    assert bool(is_inf(pr["U"], 12)[0]) == (case == "zero"), tag
    assert bool(is_inf(pr["final_a"], 12)[0]) == (case == "zero"), tag
    # a boolean b: chi(b) is a unit vector, U is that row's commitment
    k = unit_row(case, n)
    if k is not None:
        assert np.array_equal(pr["U"], comms[k]), tag
    # pst_proof: every quotient of a constant q is zero; a non-constant q has a non-zero one
    pst_inf = is_inf(pr["pst_proof"], 24)
    assert len(pst_inf) == m_row
    if case in ("zero", "const", "const_max"):
        assert pst_inf.all(), tag
    else:
        assert not pst_inf.all(), tag
    _presence(is_inf(pr["comms_u"], 12), U_INF.get(case), tag + ("comms_u",))
    _presence(is_one(pr["comms_t"]), T_ONE.get(case), tag + ("comms_t",))
    # the SRS side never degenerates
    assert not is_inf(pr["final_h"], 24).any() and not is_inf(pr["pst_proof_h"], 12).any(), tag
    want = expected_eval(case, n, Z)
    if want is not None:
        assert fr_int(v) == want, tag


@functools.lru_cache(maxsize=None)
def oracle_srs(nv):
    return orc.SRS(nv, SEED_SRS)


@functools.lru_cache(maxsize=None)
def reference(case, n):
    """The C++ oracle's commitment, evaluation and opening of the case (computed
    once per process; the arrays are read-only): dict Z, pt, v, comms, T, pr."""
    srs = oracle_srs((n + 1) // 2)
    Z, pt = inputs(case, n)
    v = orc.pst_eval(Z, n, pt)
    comms, T = orc.pst_commit(srs, Z, n)
    pr = orc.pst_open(srs, Z, n, pt, comms)
    out = dict(Z=Z, pt=pt, v=v, comms=comms, T=T, pr=pr)
    for a in (Z, pt, v, comms, T) + tuple(pr.values()):
        a.setflags(write=False)
    return out


def proof_fields(U, pst_proof, mipp):
    """a device opening as the oracle's dict"""
    return dict(U=U, pst_proof=pst_proof, comms_t=mipp.comms_t, comms_u=mipp.comms_u, final_a=mipp.final_a,
                final_h=mipp.final_h, pst_proof_h=mipp.pst_proof_h)
