"""Operands and expected values of the tower self-test (tpst_selftest_tower:
the pairing's RNS chain engine, csrc/rns_engine.h, and its radix wave engine,
csrc/wave_tower.h), shared by the host checks (test_tower_vectors.py) and the
device run (test_tower_arith.py).  Everything is Python integers:

  field values      oracle/py/bls377.py (f12_mul, f12_inv, f12_frob, f12_conj,
                    final_exp_ark, g2_prepare); CYC_SQR on arbitrary inputs is
                    the Granger-Scott formula as tools/gen_wave_ops.py states
                    it (a polynomial identity, not a group fact);
  residue words     tools/gen_rns_ops.py's exact model of rns_engine.h
                    (run_op / mont / crt / store_model), bit for bit.

An Fq12 is its 12 Fq coefficients in tower order (c0.c0.c0 .. c1.c2.c1).
Under the FQ codec a coefficient a travels as the field.h Montgomery word
value a R mod p (R = 2^384); under the RES codec a slot holds an integer
X < 16 p standing for the field value X M^-1 mod p (M = prod of base B), and
travels as its 32 channel residues.

Constructed classes assert their defining property here, from integers alone,
before anything is handed to a device; COUNTS records what each produced.
"""
import functools
import os
import random
import sys

import numpy as np

import bls377 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_rns_ops as G  # noqa: E402
from arith_vectors import ints, words  # noqa: E402
from testudo_amd import engine as E  # noqa: E402

W = G.W
P = O.P
RQ = 1 << 384
RQI = pow(RQ, -1, P)
MB = G.MB
MBI = pow(MB, -1, P)
N1 = G.N1  # 16 p
COUNTS = {}
ONE = [1] + [0] * 11
MINUS_ONE = [P - 1] + [0] * 11
ZERO = [0] * 12

# engine op names -> generator op names
GEN = {"f12_mul": "F12_MUL", "f12_sqr": "F12_SQR", "cyc_sqr": "CYC_SQR", "frob1": "FROB1", "frob2": "FROB2",
       "frob3": "FROB3", "conj": "CONJ", "copy": "COPY"}
RNS_STAGES = ("f12_mul", "f12_sqr", "cyc_sqr", "frob1", "frob2", "frob3", "conj", "copy")
WAVE_STAGES = ("f12_mul", "cyc_sqr", "frob1", "frob2", "conj")


def _count(key, n=1):
    COUNTS[key] = COUNTS.get(key, 0) + n


# ---------------------------------------------------------------- codecs ---
def fq_words(vecs):
    """field-value vectors (k Fq each) -> (n, 12 k) u32 field.h Montgomery words"""
    k = len(vecs[0])
    return words([v * RQ % P for vec in vecs for v in vec], 12).reshape(len(vecs), 12 * k)


def fq_values(arr):
    """(n, 12 k) u32 Montgomery words -> n lists of k word values (v = a R, as held)"""
    return ints(arr, 12)


def res_words(slotvecs):
    """vectors of 12 slot integers -> (n, 384) u32 residue words"""
    return np.array([[G.residues(x) for x in vec] for vec in slotvecs], dtype=np.uint32).reshape(len(slotvecs), 384)


def res_live(arr):
    """(n, 384) residue words without every coefficient's word 31: that lane is
    idle (rns_engine.h: 'a copy of channel 0'), nothing reads what it holds,
    and the engine leaves it unspecified where the model keeps the copy"""
    arr = np.asarray(arr)
    return arr.reshape(len(arr), 12, 32)[:, :, :31].reshape(len(arr), 12 * 31)


def res_lists(arr):
    """(n, 384) u32 -> n lists of 12 residue vectors (32 ints)"""
    return [[[int(w) for w in row[32 * k:32 * k + 32]] for k in range(12)] for row in np.asarray(arr)]


# ---------------------------------------------------- the field reference ---
@functools.lru_cache(maxsize=None)
def tables():
    """gen_rns_ops.check_all(): the built programs (shared with gen_wave_ops's
    evaluate), the RNS programs and the constant slots' residues"""
    built, rp, progs, kin, kout, _, _ = G.check_all()
    kres = [G.residues(k * MB % P) for k in rp.consts]
    return built, rp, progs, kres, kin, kout


def granger_scott(a):
    """gen_wave_ops.cyclotomic_sqr evaluated on the integers a"""
    pg = W.Prog([])
    outs = {"C": W.flat12(W.cyclotomic_sqr(pg, W.reg12("A")))}
    return W.evaluate(pg, outs, {"A": list(a), "B": []})["C"]


def ref(name, a, b=None):
    """oracle value of one op on tower-order field values; 0^-1 := 0"""
    if name in ("copy", "pass"):
        return [v % P for v in a]
    if name == "cyc_sqr":
        return granger_scott(a)
    if name in ("inv", "final_exp") and not any(v % P for v in a):
        return list(ZERO)
    fa = W.t2p(a)
    if name == "f12_mul":
        r = O.f12_mul(fa, W.t2p(b))
    elif name == "f12_sqr":
        r = O.f12_mul(fa, fa)
    elif name.startswith("frob"):
        r = O.f12_frob(fa, int(name[-1]))
    elif name == "conj":
        r = O.f12_conj(fa)
    elif name == "inv":
        r = O.f12_inv(fa)
    elif name == "final_exp":
        r = O.final_exp_ark(fa)
    else:
        raise KeyError(name)
    return W.p2t(r)


def wave_eval(name, a, b=None):
    """the same op through gen_wave_ops's linear forms (what both engines' tables encode)"""
    built = tables()[0]
    env = lambda x, y=None: {"A": list(x), "B": list(y) if y is not None else [0] * 16}  # noqa: E731
    if name == "inv":
        t = W.evaluate(*built["INV1"], env(a))["C"]
        c = W.evaluate(*built["INV2"], env(t))["C"]
        tp = W.evaluate(*built["INV3"], env(c, t))["C"]
        n = W.evaluate(*built["INV4"], env(tp))["C"]
        ni = [pow(n[0], -1, P) if n[0] else 0]
        t2 = W.evaluate(*built["INV5"], env(tp, ni))["C"]
        t6 = W.evaluate(*built["INV6"], env(c, t2))["C"]
        return W.evaluate(*built["INV7"], env(a, t6))["C"]
    return W.evaluate(*built[GEN[name]], env(a, b))["C"]


def tower_norm(a):
    """N_{Fq12/Fq}(a) as the inversion computes it (INV1 .. INV4)"""
    built = tables()[0]
    env = lambda x, y=None: {"A": list(x), "B": list(y) if y is not None else [0] * 16}  # noqa: E731
    t = W.evaluate(*built["INV1"], env(a))["C"]
    c = W.evaluate(*built["INV2"], env(t))["C"]
    tp = W.evaluate(*built["INV3"], env(c, t))["C"]
    return W.evaluate(*built["INV4"], env(tp))["C"][0]


# ------------------------------------------------ the RNS engine's model ---
def model_load(v):
    """rns::load (k = 1) of the field.h word value v (< p): the slot's residues"""
    _, _, _, kres, kin, _ = tables()
    limbs = [(v >> (32 * k)) & G.M32 for k in range(12)]
    t = []
    for ch in range(G.LANES):
        acc = sum(limbs[k] * G.LANE_TABLE[ch][G.POW32_OFF + k] for k in range(12))
        assert acc < 1 << 64
        t.append(G.red64(G.red64(acc, ch) * kres[kin][ch], ch))
    return G.mont(t)


def model_store(res):
    """rns::store of a slot's residues: the canonical field.h word value"""
    _, _, _, kres, _, kout = tables()
    return G.store_model(G.mont([G.red64(res[ch] * kres[kout][ch], ch) for ch in range(G.LANES)]))


def model_stage(gen_name, ra, rb=None):
    """one stage on 12-slot residue registers -> {output index: residues}"""
    _, rp, progs, kres, _, _ = tables()
    return G.run_op(rp, progs[gen_name], {"A": ra, "B": rb if rb is not None else ra, "K": kres}, None)


def model_op(name, ra, rb=None):
    """rns_engine.h's arithmetic for one self-test op on residue registers
    (every internal assert of the model holds, or this raises)"""
    if name == "pass":
        return [list(r) for r in ra]
    if name != "inv":
        out = model_stage(GEN[name], ra, rb)
        return [out[k] for k in range(12)]
    zero = [0] * G.LANES
    t = model_stage("INV1", ra)
    t = [t[k] for k in range(6)]
    c = model_stage("INV2", t + [zero] * 6)
    c = [c[k] for k in range(6)]
    tp = model_stage("INV3", c + [zero] * 6, t + [zero] * 6)
    tp = [tp[0], tp[1]]
    n = model_stage("INV4", tp + [zero] * 10)[0]
    nv = model_store(n)  # n R mod p
    ni = model_load(RQ * RQ * pow(nv, -1, P) % P if nv else 0)
    t2 = model_stage("INV5", tp + [zero] * 10, [ni] + [zero] * 11)
    t2 = [t2[0], t2[1]]
    t6 = model_stage("INV6", c + [zero] * 6, t2 + [zero] * 10)
    t6 = [t6[k] for k in range(6)]
    out = model_stage("INV7", ra, t6 + [zero] * 6)
    return [out[k] for k in range(12)]


# -------------------------------------------------------- operand classes ---
S_EDGE = [0, 1, 2, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2]


@functools.lru_cache(maxsize=None)
def coeff_edges():
    """class a: unit vectors s e_i, constant vectors, the alternating 0 / p-1 vectors"""
    out = []
    for s in S_EDGE:
        if s:
            for i in range(12):
                v = [0] * 12
                v[i] = s
                assert sum(1 for x in v if x) == 1 and v[i] in S_EDGE
                out.append(("a.unit s=%s i=%d" % (_sname(s), i), v))
        out.append(("a.const s=%s" % _sname(s), [s] * 12))
    out.append(("a.alt 0/p-1", [0, P - 1] * 6))
    out.append(("a.alt p-1/0", [P - 1, 0] * 6))
    _count("a coefficient edges", len(out))
    return out


def _sname(s):
    return {0: "0", 1: "1", 2: "2", P - 2: "p-2", P - 1: "p-1", (P - 1) // 2: "(p-1)/2", (P + 1) // 2: "(p+1)/2"}[s]


@functools.lru_cache(maxsize=None)
def mont_word_values():
    """class b: word values v whose field.h words are extreme"""
    top = P >> 352
    vmax = (top << 352) | ((1 << 352) - 1)
    if vmax >= P:
        vmax -= 1 << 352
    assert vmax < P and vmax & ((1 << 352) - 1) == (1 << 352) - 1 and vmax + (1 << 352) >= P
    return [("v=1", 1), ("v=2^32-1", (1 << 32) - 1), ("v=2^352", 1 << 352), ("v=p-1", P - 1), ("v=max low ones", vmax)]


@functools.lru_cache(maxsize=None)
def mont_word_edges():
    out = []
    vals = []
    for nm, v in mont_word_values():
        a = v * RQI % P
        assert a * RQ % P == v  # the device holds exactly the words of v
        vals.append(a)
        out.append(("b.const " + nm, [a] * 12))
        for i in (0, 5, 11):
            vec = [0] * 12
            vec[i] = a
            out.append(("b.unit %s i=%d" % (nm, i), vec))
    for rot in range(5):
        out.append(("b.mix rot=%d" % rot, [vals[(k + rot) % 5] for k in range(12)]))
    _count("b Montgomery-word edges", len(out))
    return out


@functools.lru_cache(maxsize=None)
def gt_generator():
    """an order-r element: the oracle's pairing of the generators"""
    g = W.p2t(O.pairing(O.G1_GEN, O.G2_GEN))
    assert g != ONE and W.p2t(O.f12_pow(W.t2p(g), O.R)) == ONE
    return g


@functools.lru_cache(maxsize=None)
def fq_root_of_minus_one_12():
    """c in Fq with c^12 = -1 (24 | p - 1)"""
    assert (P - 1) % 24 == 0
    for h in range(2, 200):
        c = pow(h, (P - 1) // 24, P)
        if pow(c, 12, P) == P - 1:
            return c
    raise AssertionError


def _mul(a, b):
    return W.p2t(O.f12_mul(W.t2p(a), W.t2p(b)))


def _rand12(rng):
    return [rng.randrange(P) for _ in range(12)]


@functools.lru_cache(maxsize=None)
def structured():
    """class f: elements of Fq and Fq2, c1 = 0, c0 = 0, norm 1 and p-1, 1, -1,
    an order-r element and its conjugate"""
    rng = random.Random(0xF12)
    g = gt_generator()
    gc = W.p2t(O.f12_conj(W.t2p(g)))
    assert _mul(g, gc) == ONE
    c = fq_root_of_minus_one_12()
    nm1 = _mul([c] + [0] * 11, g)
    out = [("f.one", list(ONE)), ("f.minus one", list(MINUS_ONE)),
           ("f.Fq 2", [2] + [0] * 11), ("f.Fq (p-1)/2", [(P - 1) // 2] + [0] * 11), ("f.Fq rnd", [rng.randrange(P)] + [0] * 11),
           ("f.Fq2 (1,1)", [1, 1] + [0] * 10), ("f.Fq2 (0,p-1)", [0, P - 1] + [0] * 10),
           ("f.Fq2 rnd", [rng.randrange(P), rng.randrange(P)] + [0] * 10),
           ("f.c1=0", _rand12(rng)[:6] + [0] * 6), ("f.c0=0", [0] * 6 + _rand12(rng)[:6]),
           ("f.pure w", [0] * 6 + [1] + [0] * 5),
           ("f.order r", g), ("f.order r conj", gc), ("f.norm p-1", nm1), ("f.norm p-1 in Fq", [c] + [0] * 11),
           ("f.rnd", _rand12(rng))]
    by = dict(out)
    assert all(v == 0 for v in by["f.c1=0"][6:]) and all(v == 0 for v in by["f.c0=0"][:6])
    assert tower_norm(g) == 1 and tower_norm(gc) == 1 and tower_norm(ONE) == 1 and tower_norm(MINUS_ONE) == 1
    assert tower_norm(nm1) == P - 1 and tower_norm(by["f.norm p-1 in Fq"]) == P - 1
    _count("f structured", len(out))
    return out


@functools.lru_cache(maxsize=None)
def unary_vectors():
    return coeff_edges() + mont_word_edges() + structured()


@functools.lru_cache(maxsize=None)
def binary_pairs():
    """operand pairs of F12_MUL: the full cross of a subset of the classes
    with itself (class a / b / f), then class c: results of exactly 1, -1, 0"""
    ce = dict(coeff_edges())
    sub = [("a.unit s=1 i=0", None), ("a.unit s=p-1 i=0", None), ("a.unit s=p-1 i=11", None), ("a.unit s=2 i=6", None),
           ("a.unit s=(p-1)/2 i=3", None), ("a.unit s=(p+1)/2 i=7", None), ("a.unit s=p-2 i=5", None),
           ("a.const s=0", None), ("a.const s=1", None), ("a.const s=p-1", None), ("a.const s=(p+1)/2", None),
           ("a.const s=p-2", None), ("a.alt 0/p-1", None), ("a.alt p-1/0", None)]
    sub = [(n, ce[n]) for n, _ in sub]
    mw = dict(mont_word_edges())
    sub += [(n, mw[n]) for n in ("b.const v=1", "b.const v=p-1", "b.const v=max low ones", "b.const v=2^352",
                                 "b.mix rot=0")]
    stv = dict(structured())
    sub += [(n, stv[n]) for n in ("f.order r", "f.norm p-1", "f.rnd")]
    out = [("%s x %s" % (na, nb), a, b) for na, a in sub for nb, b in sub]
    _count("a/b/f cross pairs", len(out))
    # class c
    rng = random.Random(0xC0DE)
    cls_c = []
    srcs = [("rnd%d" % i, _rand12(rng)) for i in range(6)]
    srcs += [(n, v) for n, v in coeff_edges() if n.startswith("a.unit") and n.endswith(("i=1", "i=6", "i=11"))]
    srcs += [(n, v) for n, v in mont_word_edges() if n.startswith("b.const") or n.startswith("b.mix")]
    srcs += [(n, v) for n, v in structured() if n not in ("f.one",)]
    for n, a in srcs:
        ai = ref("inv", a)
        nai = [(P - v) % P for v in ai]
        assert _mul(a, ai) == ONE and _mul(a, nai) == MINUS_ONE  # eleven outputs exactly 0, one 1 or p-1
        cls_c.append(("c.a*a^-1 " + n, a, ai))
        cls_c.append(("c.a^-1*a " + n, ai, a))
        cls_c.append(("c.a*-a^-1 " + n, a, nai))
        assert _mul(a, ZERO) == ZERO
        cls_c.append(("c.a*0 " + n, a, list(ZERO)))
        cls_c.append(("c.0*a " + n, list(ZERO), a))
    _count("c exact-multiple products", len(cls_c))
    return out + cls_c


@functools.lru_cache(maxsize=None)
def unary_for(name):
    """operands of a unary op: classes a, b, f, the inverses that class c
    multiplies with, and for conj / frob the class c inputs 1 and -1"""
    v = list(unary_vectors())
    if name in ("conj", "frob1", "frob2", "frob3"):
        for nm, x in (("c.op(1)", ONE), ("c.op(-1)", MINUS_ONE)):
            assert ref(name, x) == x  # results of exactly 1 and -1
            v.append((nm, list(x)))
    if name == "inv":
        v.append(("f.zero", list(ZERO)))
    if name == "cyc_sqr":  # on the cyclotomic subgroup the formula is the square
        for nm, x in structured():
            if nm.startswith("f.order r"):
                assert granger_scott(x) == _mul(x, x)
    return v


# class d: RES slot integers
@functools.lru_cache(maxsize=None)
def res_slot_edges():
    out = [("d.%s" % n, v) for n, v in (("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("8p", 8 * P),
                                        ("15p", 15 * P), ("16p-2", N1 - 2), ("16p-1", N1 - 1))]
    for k in range(1, 16):
        out += [("d.%dp-1" % k, k * P - 1), ("d.%dp" % k, k * P), ("d.%dp+1" % k, k * P + 1)]
    for ch in range(G.LANES - 1):
        m = G.lane_mod(ch) or (1 << 32)
        top0 = (N1 - 1) - (N1 - 1) % m          # largest X < 16 p with X = 0 mod m
        top1 = top0 - 1 if top0 + m - 1 >= N1 else top0 + m - 1  # ... with X = m - 1 mod m
        assert top0 < N1 <= top0 + m and top0 % m == 0
        assert top1 < N1 <= top1 + m and top1 % m == m - 1
        out += [("d.ch%d m-1" % ch, m - 1), ("d.ch%d m" % ch, m), ("d.ch%d top=0" % ch, top0),
                ("d.ch%d top=m-1" % ch, top1)]
        for nm, x in out[-4:]:
            r = G.residues(x)[ch]
            assert r == (m - 1 if nm.endswith("m-1") else 0), (nm, r)
    for fv, nm in ((0, "0"), (1, "1"), (P - 1, "-1")):
        x = fv * MB % P
        for k in range(16):
            assert (x + k * P) * MBI % P == fv and x + k * P < N1
            out.append(("d.rep %s +%dp" % (nm, k), x + k * P))
    assert all(0 <= x < N1 for _, x in out)
    _count("d RES slot integers", len(out))
    return out


@functools.lru_cache(maxsize=None)
def res_vectors():
    """class d as 12-slot registers: the slot integers in order, twelve at a
    time, rotated so that consecutive registers start at different slots, and
    the constant registers of the extremes"""
    se = res_slot_edges()
    out = []
    for i in range(0, len(se), 12):
        chunk = se[i:i + 12]
        chunk = chunk + se[:12 - len(chunk)]
        rot = (i // 12) % 12
        chunk = chunk[rot:] + chunk[:rot]
        out.append(("d[%d..] %s.." % (i, chunk[0][0]), [x for _, x in chunk]))
    for nm, x in (("0", 0), ("p", P), ("15p", 15 * P), ("16p-1", N1 - 1)):
        out.append(("d.const " + nm, [x] * 12))
    assert {x for _, v in out for x in v} == {x for _, x in se}
    _count("d RES registers", len(out))
    return out


@functools.lru_cache(maxsize=None)
def res_pairs():
    rv = res_vectors()
    top = rv[-1]
    out = []
    for i, (n, v) in enumerate(rv):
        nn, w = rv[(i + 1) % len(rv)]
        out += [("%s x same" % n, v, v), ("%s x %s" % (n, nn), v, w), ("%s x 16p-1" % n, v, top[1]),
                ("16p-1 x %s" % n, top[1], v)]
    return out


def res_field(vec):
    """field values a register of slot integers stands for"""
    return [x * MBI % P for x in vec]


# class e: form maximisers of the wave engine
@functools.lru_cache(maxsize=None)
def wave_form_maximisers(name):
    """(class name, A, B) per linear form of op `name` whose atoms are input
    slots: product forms x_i, y_i and the output forms over inputs.  A term
    with a positive coefficient reads the slot's value, one with a negative
    coefficient the slot's stored negation p - x (0 for x = 0): the first kind
    of slot is set to p - 1 and the second to 1, so every term adds c (p - 1).
    (A 0 in the second kind of slot would add nothing: neg(0) = 0.)
    Output forms over products cannot be set directly and are left to the
    other classes."""
    pg, outs = tables()[0][GEN[name]]
    forms = []
    for i, (x, y) in enumerate(pg.products):
        forms.append(("x%d" % i, x))
        if x is not y:
            forms.append(("y%d" % i, y))
    for k, lin in enumerate(outs["C"]):
        forms.append(("out%d" % k, lin))
    out = []
    for fn, lin in forms:
        if not lin or any(kind not in ("A", "B") for kind, _ in lin):
            continue
        regs = {"A": [0] * 12, "B": [0] * 12}
        for (kind, i), c in lin.items():
            regs[kind][i] = P - 1 if c > 0 else 1
        value = sum(abs(c) * (regs[kind][i] if c > 0 else (P - regs[kind][i]) % P) for (kind, i), c in lin.items())
        assert 2 * value >= lin.weight() * P and value == lin.weight() * (P - 1), (name, fn)
        out.append(("e.%s %s w=%d" % (name, fn, lin.weight()), regs["A"], regs["B"]))
    _count("e form maximisers " + name, len(out))
    return out


# ----------------------------------------------------------------- cases ---
class Case:
    """one device call: operands a (and b), class name per element, expected words"""

    def __init__(self, name, op, names, a, b, exp, inputs):
        self.name, self.op, self.names, self.a, self.b, self.exp, self.inputs = name, op, names, a, b, exp, inputs


@functools.lru_cache(maxsize=None)
def fq_operands(engine, name):
    """(class names, A vectors, B vectors or None) of an FQ-codec op"""
    if name == "f12_mul":
        ps = list(binary_pairs())
        if engine == "wave":
            ps += wave_form_maximisers(name)
        return [n for n, _, _ in ps], [a for _, a, _ in ps], [b for _, _, b in ps]
    vs = list(unary_for(name))
    if engine == "wave" and name in WAVE_STAGES:
        vs += [(n, a) for n, a, _ in wave_form_maximisers(name)]
    if name == "final_exp":
        vs = final_exp_vectors()
    return [n for n, _ in vs], [a for _, a in vs], None


@functools.lru_cache(maxsize=None)
def final_exp_vectors():
    """class a (units of 1 and p-1, constants, alternating), b (constants), f, and zero"""
    vs = [(n, v) for n, v in coeff_edges() if n.startswith(("a.const", "a.alt")) or "s=1 " in n or
          (("s=p-1 " in n or "s=(p+1)/2 " in n) and n.endswith(("i=0", "i=7", "i=11")))]
    vs += [(n, v) for n, v in mont_word_edges() if n.startswith("b.const")]
    vs += structured()
    assert len(vs) <= 64
    return vs


@functools.lru_cache(maxsize=None)
def fq_case(engine, name):
    names, A, B = fq_operands(engine, name)
    exp = [ref(name, a, B[i] if B else None) for i, a in enumerate(A)]
    return Case("%s.fq.%s" % (engine, name), E.selftest_tower_op(engine, name), names, fq_words(A),
                fq_words(B) if B else None, fq_words(exp), [a + (B[i] if B else []) for i, a in enumerate(A)])


@functools.lru_cache(maxsize=None)
def res_case(name):
    """RES -> RES on class d: bit-exact residues from the model"""
    if name == "f12_mul":
        ps = res_pairs()
        names, A, B = [n for n, _, _ in ps], [a for _, a, _ in ps], [b for _, _, b in ps]
    else:
        names, A, B = [n for n, _ in res_vectors()], [v for _, v in res_vectors()], None
    exp = []
    for i, a in enumerate(A):
        ra = [G.residues(x) for x in a]
        rb = [G.residues(x) for x in B[i]] if B else None
        out = model_op(name, ra, rb)
        want = ref(name, res_field(a), res_field(B[i]) if B else None)
        for k in range(12):
            y = G.crt(out[k])
            assert y < N1 and y * MBI % P == want[k], (name, names[i], k)
        exp.append(out)
    return Case("rns.res.%s" % name, E.selftest_tower_op("rns", name, "res", "res"), names, res_words(A),
                res_words(B) if B else None, np.array(exp, dtype=np.uint32).reshape(len(A), 384),
                [a + (B[i] if B else []) for i, a in enumerate(A)])


@functools.lru_cache(maxsize=None)
def pass_cases():
    """the codecs alone: FQ -> RES is rns::load bit for bit, RES -> FQ rns::store
    of every class d slot integer (all 16 representatives of 0, 1 and -1 among them)"""
    names = [n for n, _ in unary_vectors()]
    A = [v for _, v in unary_vectors()]
    exp = [[model_load(v * RQ % P) for v in a] for a in A]
    for a, e in zip(A, exp):
        assert all(G.crt(r) < N1 and G.crt(r) * MBI % P == v for v, r in zip(a, e))
    load = Case("rns.fq->res.pass", E.selftest_tower_op("rns", "pass", "fq", "res"), names, fq_words(A), None,
                np.array(exp, dtype=np.uint32).reshape(len(A), 384), A)
    rn = [n for n, _ in res_vectors()]
    RA = [v for _, v in res_vectors()]
    want = [[x * MBI % P for x in v] for v in RA]
    for v, w in zip(RA, want):
        assert [model_store(G.residues(x)) for x in v] == [f * RQ % P for f in w]
    store = Case("rns.res->fq.pass", E.selftest_tower_op("rns", "pass", "res", "fq"), rn, res_words(RA), None,
                 fq_words(want), RA)
    return [load, store]


# class g
@functools.lru_cache(maxsize=None)
def g2_points():
    gen = O.G2_GEN
    pts = [("g.generator", gen), ("g.-generator", O.g2_neg(gen)), ("g.[2]generator", O.g2_add(gen, gen))]
    assert O.g2_on_curve(pts[1][1]) and O.g2_on_curve(pts[2][1]) and pts[1][1][1] == O.f2_neg(gen[1])
    S = S_EDGE
    coords = [((1, 0), (1, 0)), ((0, 1), (P - 1, 0)), ((P - 1, P - 1), (P - 1, P - 1)), ((0, 0), (1, 0)),
              ((1, 0), (0, 0)), ((2, P - 2), ((P - 1) // 2, (P + 1) // 2)), (((P + 1) // 2, 0), (0, P - 2)),
              ((P - 1, 0), (0, P - 1)), ((0, 0), (0, 0)), (((P - 1) // 2, (P - 1) // 2), (2, 2))]
    for x, y in coords:
        assert all(c in S for c in x + y)
    pts += [("g.a (%s,%s),(%s,%s)" % tuple(_sname(c) for c in x + y), (x, y)) for x, y in coords]
    _count("g G2 points", len(pts))
    return pts


def g2_words(pts):
    return fq_words([[p[0][0], p[0][1], p[1][0], p[1][1]] for p in pts])


def g2_expected(pts):
    """(n, 69, 72) u32 words of O.g2_prepare, point-major"""
    rows = [[c for co in O.g2_prepare(p) for f2 in co for c in f2] for p in pts]
    assert all(len(r) == 69 * 6 for r in rows)
    return fq_words(rows).reshape(len(pts), 69, 72)


# GT_POW
DIGIT_MAX = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def gt_pow_vectors():
    """(class name, base, digits, member, expected): members are raised to
    e = sum d_j x^j, reduced mod r by their order; non-members give ok = 0"""
    rng = random.Random(0x6790)
    g = gt_generator()
    gc = W.p2t(O.f12_conj(W.t2p(g)))
    g7 = W.p2t(O.f12_pow(W.t2p(g), 7))
    digs = [("0", (0, 0, 0, 0)), ("1", (1, 0, 0, 0)), ("x", (0, 1, 0, 0)), ("x^3", (0, 0, 0, 1)),
            ("max", (DIGIT_MAX,) * 4), ("max,0,0,0", (DIGIT_MAX, 0, 0, 0)), ("0,0,0,max", (0, 0, 0, DIGIT_MAX)),
            ("rnd", tuple(rng.randrange(1 << 64) for _ in range(4)))]
    out = []
    for bn, base in (("one", ONE), ("g", g), ("conj g", gc), ("g^7", g7)):
        assert W.p2t(O.f12_pow(W.t2p(base), O.R)) == ONE
        for dn, d in digs:
            e = sum(dj * O.X ** j for j, dj in enumerate(d))
            out.append(("f.gt_pow %s ^ %s" % (bn, dn), base, d, 1, W.p2t(O.f12_pow(W.t2p(base), e % O.R))))
    # non-members: zero, -1 (order 2), an Fq element, a random element, and an
    # element of the cyclotomic subgroup outside GT (the easy part of a random one)
    rnd = _rand12(rng)
    fr = W.t2p(rnd)
    cyc = O.f12_mul(O.f12_conj(fr), O.f12_inv(fr))
    cyc = O.f12_mul(O.f12_frob(cyc, 2), cyc)
    assert O.f12_mul(O.f12_frob(cyc, 4), cyc) == O.f12_frob(cyc, 2)  # in the cyclotomic subgroup
    non = [("zero", ZERO), ("minus one", MINUS_ONE), ("Fq 2", [2] + [0] * 11), ("rnd", rnd), ("cyclotomic", W.p2t(cyc))]
    for bn, base in non:
        if any(base):
            assert W.p2t(O.f12_pow(W.t2p(base), O.R)) != ONE
        out.append(("f.gt_pow non-member " + bn, list(base), digs[-1][1], 0, list(ZERO)))
    _count("f gt_pow", len(out))
    return out
