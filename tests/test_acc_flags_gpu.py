"""The first / last-of-bucket flags that k_sort_bin sets in the sorted values
(msm_pieces.h entry_flags) and the flag-driven walk of the G1 short-chunk
accumulation kernels (msm_acc.h), bit-exact against the CPU oracle.

  sizes   n = 64 and 65 (one window group, 32-entry chunks, the GLV threshold);
          n = 2^17 and 2^17 + 3 (the smallest window-grouped size, 16-entry
          chunks, chunks split between two groups' launches);
  inputs  'uniform'; 'equal': all bases and scalars equal -- one bucket per
          window across every chunk, the long list; 'cancel': P, -P
          alternating; 'sparse': 7 of 8 scalars zero -- buckets of a few
          entries, i.e. the whole-bucket branch and its key load, sentinels
          beside the live entries; 'rminus1': scalars r - 1 (top digits and
          carries); 'inf': some bases at infinity.

Pipelined calls on different inputs must equal their synchronised results
(stale flags when an arena is reused), and the G2 pair kernel, which reads the
same flagged values, is checked at n = 64 and at the smallest grouped size.
"""
import numpy as np
import pytest

import bls377 as O
import orc
from testudo_amd.encoding import fr_array, g1_array, g1_from_array, limbs_to_int

pytestmark = pytest.mark.gpu

N_BIG = 1 << 17
SIZES = (64, 65, N_BIG, N_BIG + 3)
KINDS = ("uniform", "equal", "cancel", "sparse", "rminus1", "inf")


@pytest.fixture(scope="module")
def points(ctx):
    k, _ = orc.fr_stream(0xF1A6, N_BIG + 3)
    p = ctx.g1_mul_generator(k)
    p.setflags(write=False)
    return p


def _inputs(points, kind, n, seed):
    """(bases, scalars) of n entries"""
    bases = points[:n].copy()
    s, _ = orc.fr_stream(seed, n)
    if kind == "equal":
        bases[:] = points[3]
        s = np.repeat(s[:1], n, axis=0)
    elif kind == "cancel":
        (x, y), = g1_from_array(points[5:6])
        bases[0::2] = points[5]
        bases[1::2] = g1_array([(x, (O.P - y) % O.P)])[0]
        s = np.repeat(s[:1], n, axis=0)
    elif kind == "sparse":
        keep = np.arange(n) % 8 == 3
        s[~keep] = 0
    elif kind == "rminus1":
        s = np.repeat(fr_array([O.R - 1]), n, axis=0)
    elif kind == "inf":
        bases[1::5] = 0
        bases[n - 1] = 0
    else:
        assert kind == "uniform"
    return bases, np.ascontiguousarray(s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_g1_msm_flag_walk_vs_oracle(ctx, points, kind, n):
    bases, s = _inputs(points, kind, n, 0xF1A7 + n)
    ref = orc.g1_msm(bases, s, parallel=n > 4096)
    if kind == "cancel" and n % 2 == 0:
        assert not ref.any()  # the pairs cancel
    assert np.array_equal(ctx.g1_msm(bases, s), ref)


def test_g1_msm_pipelined_calls_on_different_inputs(ctx, points):
    """Three inputs with different bucket shapes, pipelined twice over (six
    calls: every arena is used again by an input of another shape), against the
    same calls made one at a time."""
    import torch
    n = N_BIG + 3
    dev = torch.device("cuda", 0)
    # bases k_i G in the device entry points' format (made on the device)
    k, _ = orc.fr_stream(0xF1B8, n)
    sets = []
    for i, kind in enumerate(("uniform", "sparse", "equal")):
        _, s = _inputs(points, kind, n, 0xF1B0 + i)
        sets.append((np.repeat(k[7:8], n, axis=0) if kind == "equal" else k, s))
    d_k = [torch.from_numpy(np.ascontiguousarray(kk).view(np.int64)).to(dev) for kk, _ in sets]
    d_s = [torch.from_numpy(s.view(np.int64)).to(dev) for _, s in sets]
    d_b = [torch.empty(n * 12, dtype=torch.int64, device=dev) for _ in sets]
    order = [0, 1, 2, 1, 0, 2]
    ref = torch.zeros((3, 12), dtype=torch.int64, device=dev)
    out = torch.zeros((len(order), 12), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for j in range(3):
        ctx.g1_mul_generator_dev(d_k[j].data_ptr(), n, d_b[j].data_ptr())
    for j in range(3):
        ctx.g1_msm_dev(d_b[j].data_ptr(), d_s[j].data_ptr(), n, ref[j].data_ptr())
        ctx.synchronize()
    for o, j in enumerate(order):
        ctx.g1_msm_dev_async(d_b[j].data_ptr(), d_s[j].data_ptr(), n, out[o].data_ptr())
    ctx.synchronize()
    ref = ref.cpu().numpy().view(np.uint64)
    out = out.cpu().numpy().view(np.uint64)
    assert len({r.tobytes() for r in ref}) == 3
    for o, j in enumerate(order):
        assert np.array_equal(out[o], ref[j]), (o, j)
    for j, (kk, s) in enumerate(sets):  # each sum is (sum s_i k_i) G
        tot = sum(limbs_to_int(a) * limbs_to_int(b) for a, b in zip(s, kk)) % O.R
        assert np.array_equal(ref[j], orc.g1_mul_gen(fr_array([tot]))[0]), j


@pytest.mark.parametrize("n", [64, N_BIG])
def test_g2_msm_flagged_values_vs_oracle(ctx, n):
    k, _ = orc.fr_stream(0xF1C0, min(n, 1024))
    bases = np.concatenate([orc.g2_mul_gen(k)] * (n // len(k)))
    s, _ = orc.fr_stream(0xF1C1 + n, n)
    s[2::8] = 0  # sentinels beside the live entries
    assert np.array_equal(ctx.g2_msm(bases, s), orc.g2_msm(bases, s, parallel=True))
