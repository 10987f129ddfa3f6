"""Time the grand-product argument (tpst_prodcircuit_prove_dev /
tpst_prodcircuit_verify) on one GPU.

    python tools/prodcircuit_time.py [--shapes 20:12:6,20:4:0] [--runs 7]
                                     [--out profiles/product_tree/prodcircuit_time.json]

The default shapes (ell:P:D) are the two calls of ProductLayerProof::prove for a
2^20-entry (A, B, C) batch.  Per shape, after one warm-up of every call,
medians over --runs of:
  prove_wall_ms       host clock around prove_dev from device-resident inputs
                      (the call ends synchronised)
  build_dev_ms        HIP events of tpst_profile_*: the Montgomery copies, one
                      pass per layer, the dot products' evaluations
  rounds_ms           every layer proof, first squeeze to last claims (device
                      work and the host transcript between launches)
  round0_dev_ms       layer 0's round 0 (round kernel + reduce): reads
                      (2P + 3D + 1) 2^(ell-1) Fr, binds nothing
  round1_dev_ms       layer 0's round 1: reads the same tables and writes half
                      of them back (the fused bind of round 0's challenge)
  host_transcript_ms  the prover's absorbs and squeezes replayed alone on the
                      host: per layer the coefficient squeezes, per round 4
                      absorbs and 1 squeeze, the claim appends, 1 squeeze (one
                      C-ABI call each) -- the floor the prover is reported against
  verify_wall_ms      the host verifier on a fresh transcript
and the two rounds' rates against the bytes the algorithm needs (32 B per Fr
read; round 1 also writes half as many) and the 8 TB/s HBM peak.
Prints one JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def replay_transcript(ell, P, D, FrTranscript, one):
    """the prover's transcript traffic alone (values do not matter)"""
    tr = FrTranscript()
    t0 = time.perf_counter()
    for i in range(ell):
        ni = P + (D if i == ell - 1 else 0)
        for _ in range(ni):
            tr.challenge_scalar()
        for _j in range(i):
            for _c in range(4):
                tr.append_scalar(one)
            tr.challenge_scalar()
        for _ in range(2 * P + (3 * D if i == ell - 1 else 0)):
            tr.append_scalar(one)
        tr.challenge_scalar()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20:12:6,20:4:0")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from testudo_amd import Context
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.sqrt_pst import fr_stream

    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    med = statistics.median
    lines = []
    for shape in args.shapes.split(","):
        ell, P, D = (int(x) for x in shape.split(":"))
        n = 1 << ell
        polys, k = fr_stream(0x5054 + ell, P * n)
        d_p = torch.from_numpy(np.ascontiguousarray(polys).view(np.int64)).to(dev)
        d_d = []
        for _ in range(3):
            if D:
                v, k = fr_stream(0x5054 + ell, D * (n // 2), k)
                d_d.append(torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).to(dev))
        ctx.torch_to_lib()
        ptrs = [t.data_ptr() for t in d_d] if D else [0, 0, 0]

        def prove():
            return PT.prove_dev(ctx, ell, P, d_p.data_ptr(), D, *ptrs, FrTranscript())

        proof, cp, cd, _rand = prove()  # warm-up
        assert PT.verify(cp, cd, proof, FrTranscript()) is not False  # warm-up, and the proof is sound
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        replay_transcript(ell, P, D, FrTranscript, one)
        wall, build, rounds, r0, r1, vwall, thost = [], [], [], [], [], [], []
        ctx.profile(True)
        for _ in range(args.runs):
            ctx.profile_reset()
            t0 = time.perf_counter()
            prove()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.profile_read()
            build.append(st["prodtree_build"][0])
            rounds.append(st["prodtree_rounds"][0])
            r0.append(st["prodtree_round0"][0])
            r1.append(st["prodtree_round1"][0])
        ctx.profile(False)
        for _ in range(args.runs):
            t0 = time.perf_counter()
            ok = PT.verify(cp, cd, proof, FrTranscript())
            vwall.append((time.perf_counter() - t0) * 1e3)
            assert ok is not False
            thost.append(replay_transcript(ell, P, D, FrTranscript, one))
        read_bytes = (2 * P + 3 * D + 1) * (n // 2) * 32
        gbs0 = read_bytes / (med(r0) * 1e-3) / 1e9 if ell > 1 else 0.0
        gbs1 = 1.5 * read_bytes / (med(r1) * 1e-3) / 1e9 if ell > 2 else 0.0
        res = {"ell": ell, "P": P, "D": D, "runs": args.runs, "rounds": ell * (ell - 1) // 2,
               "prove_wall_ms": round(med(wall), 3), "build_dev_ms": round(med(build), 4),
               "rounds_ms": round(med(rounds), 3), "round0_dev_ms": round(med(r0), 4),
               "round1_dev_ms": round(med(r1), 4), "round_read_bytes": read_bytes,
               "round0_gbs": round(gbs0, 1), "round0_fraction_of_hbm_peak": round(gbs0 / HBM_PEAK_GBS, 4),
               "round1_gbs_read_plus_write": round(gbs1, 1),
               "round1_fraction_of_hbm_peak": round(gbs1 / HBM_PEAK_GBS, 4),
               "host_transcript_ms": round(med(thost), 3),
               "host_transcript_share_of_prove": round(med(thost) / med(wall), 4),
               "verify_wall_ms": round(med(vwall), 3)}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del d_p, d_d
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
