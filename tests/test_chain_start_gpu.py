"""G1 MSMs whose bucket chains start in every way the accumulation kernels'
step 1 can meet (msm_acc.h: the chain-start form of the mixed add runs there,
where every live accumulator is infinity or has ZZ = ZZZ = 1), bit-exact
against the CPU oracle orc.g1_msm:

  sizes   n = 64 (one window group, k_bucket_acc_short*), n = 2^17 (the
          smallest size on the window-grouped path, 16-entry chunks) and a
          batched commit of 8 rows x 256 (k_bucket_acc_chunk_lds);
  inputs  'equal': all bases equal and all scalars equal -- step 1 is a
          doubling in every lane;
          'cancel': bases alternating P, -P with equal scalars -- step 1
          cancels to infinity;
          'tiny': scalars in {0, 1, 2} -- one- and two-entry buckets,
          sentinels, bucket boundaries at steps 0 and 1;
          'uniform': random scalars.
"""
import numpy as np
import pytest

import bls377 as O
import orc
from testudo_amd.encoding import fr_array, g1_array, g1_from_array

pytestmark = pytest.mark.gpu

N_BIG = 1 << 17
KINDS = ("equal", "cancel", "tiny", "uniform")


@pytest.fixture(scope="module")
def points(ctx):
    k, _ = orc.fr_stream(0xC5A1, N_BIG)
    return ctx.g1_mul_generator(k)


def _inputs(points, kind, n, seed):
    """(bases, scalars) of n entries"""
    bases = points[:n].copy()
    if kind == "equal":
        bases[:] = points[3]
        s = np.repeat(orc.fr_stream(seed, 1)[0], n, axis=0)
    elif kind == "cancel":
        (x, y), = g1_from_array(points[5:6])
        bases[0::2] = points[5]
        bases[1::2] = g1_array([(x, (O.P - y) % O.P)])[0]
        s = np.repeat(orc.fr_stream(seed, 1)[0], n, axis=0)
    elif kind == "tiny":
        rng = np.random.default_rng(seed)
        s = np.zeros((n, 4), dtype=np.uint64)
        s[:, 0] = rng.integers(0, 3, n, dtype=np.uint64)
        assert set(np.unique(s[:, 0])) == {0, 1, 2}
    else:
        s, _ = orc.fr_stream(seed, n)
    return bases, np.ascontiguousarray(s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [64, N_BIG])
def test_g1_msm_chain_starts_vs_oracle(ctx, points, kind, n):
    bases, s = _inputs(points, kind, n, 0xC5A2 + n)
    ref = orc.g1_msm(bases, s, parallel=n > 4096)
    if kind == "cancel":
        assert not ref.any()  # n is even: the pairs cancel
    assert np.array_equal(ctx.g1_msm(bases, s), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_batched_commit_chain_starts_vs_oracle(ctx, points, kind):
    from testudo_amd.engine import Gens
    rows, cols = 8, 256
    bases, _ = _inputs(points, kind, cols, 1)
    Z = np.concatenate([_inputs(points, kind, cols, 0xC5B0 + r)[1] for r in range(rows)])
    gens = Gens(ctx, bases)
    got = gens.msm_batch(Z, rows, cols, 1)
    gens.close()
    for r in range(rows):
        assert np.array_equal(got[r], orc.g1_msm(bases, np.ascontiguousarray(Z[r * cols:(r + 1) * cols]))), (kind, r)
