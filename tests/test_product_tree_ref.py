"""CPU tests of the grand-product argument's restatement
(tests/product_tree_ref.py) and its fixture tests/golden/product_tree.json: no
GPU, no library."""
import copy
import functools

import pytest

import hyrax_ref as H
import product_tree_ref as T

R = T.R
SHAPES = [(1, 1, 0), (2, 1, 0), (2, 2, 2), (3, 3, 2), (5, 2, 4)]


@functools.lru_cache(maxsize=None)
def _run(ell, P, D, special=False):
    polys, dotps, whole = T.random_inputs(ell, P, D, 7000 + 100 * ell + 10 * P + D, special)
    return polys, dotps, whole, T.run(polys, dotps)


def _verify(v, proof=None, claims_prod=None, claims_dotp=None, ell=None):
    n = 1 << (ell if ell is not None else len(v["rand"]))
    return T.verify(proof or v["proof"], claims_prod or v["claims_prod"],
                    v["claims_dotp"] if claims_dotp is None else claims_dotp, n, H.Transcript())


def test_restatement_reproduces_fixture():
    import golden_io as G
    cases = [T.load_case(d) for d in G.load("product_tree.json")["cases"]]
    assert [(c["ell"], c["P"], c["D"]) for c in cases] == [(3, 2, 2)]
    for c in cases:
        v = T.run(c["polys"], c["dotp"])
        for k in ("claims_prod", "claims_dotp", "proof", "rand", "claims_out", "claims_dotp_out", "transcript_end"):
            assert v[k] == c[k], k
        assert [len(L["polys"]) for L in c["proof"]["layers"]] == [0, 1, 2]
        flat = T.flatten(c["proof"], c["ell"], c["P"], c["D"])
        assert T.unflatten(flat, c["ell"], c["P"], c["D"]) == c["proof"]


@pytest.mark.parametrize("ell,P,D", SHAPES)
def test_prove_verify_accepts(ell, P, D):
    polys, dotps, whole, v = _run(ell, P, D)
    assert len(v["rand"]) == ell
    assert [len(L["polys"]) for L in v["proof"]["layers"]] == list(range(ell))
    res = _verify(v)
    assert res is not False
    claims, claims_dotp, rand = res
    assert rand == v["rand"]
    # every product instance's final claim is its input evaluated at rand
    assert claims == [H.evaluate(p, rand) for p in polys]
    # each dot-product triple is the unsplit left / right / weight at rand
    assert claims_dotp == [H.evaluate(vec, rand) for w in whole for vec in w]
    # the claimed products are the products
    for p, c in zip(polys, v["claims_prod"]):
        acc = 1
        for x in p:
            acc = acc * x % R
        assert c == acc
    for (left, right, weight), c in zip(dotps, v["claims_dotp"]):
        assert c == sum(a * b * w for a, b, w in zip(left, right, weight)) % R


def test_special_values_in_the_inputs():
    """0, 1 and r - 1 among the entries"""
    polys, dotps, whole, v = _run(3, 2, 2, True)
    assert 1 in polys[0] and R - 1 in polys[0] and 0 in whole[0][0] and R - 1 in whole[0][2]
    claims, claims_dotp, rand = _verify(v)
    assert claims == [H.evaluate(p, rand) for p in polys]
    assert claims_dotp == [H.evaluate(vec, rand) for w in whole for vec in w]


def test_zero_entry_gives_a_zero_product():
    polys, dotps, _whole = T.random_inputs(3, 2, 2, 7777)
    polys[1][5] = 0
    v = T.run(polys, dotps)
    assert v["claims_prod"][1] == 0 and v["claims_prod"][0] != 0
    res = _verify(v)
    assert res is not False and res[0] == [H.evaluate(p, res[2]) for p in polys]


@pytest.mark.parametrize("ell,P,D", [(3, 3, 2), (5, 2, 4)])
def test_tampering_is_rejected(ell, P, D):
    _polys, _dotps, _whole, v = _run(ell, P, D)
    assert _verify(v) is not False
    bump = lambda x: (x + 1) % R  # noqa: E731
    for layer in range(1, ell):  # a round coefficient of every layer that has rounds
        for c in range(4):
            p = copy.deepcopy(v["proof"])
            p["layers"][layer]["polys"][layer - 1][c] = bump(p["layers"][layer]["polys"][layer - 1][c])
            assert _verify(v, proof=p) is False
    for layer in range(ell):
        for side in ("left", "right"):
            p = copy.deepcopy(v["proof"])
            p["layers"][layer][side][P - 1] = bump(p["layers"][layer][side][P - 1])
            assert _verify(v, proof=p) is False  # the layer equation
    for k in range(3):
        p = copy.deepcopy(v["proof"])
        p["dotp"][k][D - 1] = bump(p["dotp"][k][D - 1])
        assert _verify(v, proof=p) is False
    for k in range(P):
        cp = list(v["claims_prod"])
        cp[k] = bump(cp[k])
        assert _verify(v, claims_prod=cp) is False
    cd = list(v["claims_dotp"])
    cd[0] = bump(cd[0])
    assert _verify(v, claims_dotp=cd) is False
    # a layer proof short of a round, or a missing layer
    p = copy.deepcopy(v["proof"])
    p["layers"][ell - 1]["polys"].pop()
    assert _verify(v, proof=p) is False
    p = copy.deepcopy(v["proof"])
    p["layers"].pop()
    assert _verify(v, proof=p) is False
