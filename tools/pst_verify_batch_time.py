"""Time tpst_pst_verify_batch against B sequential tpst_pst_verify calls, on one GPU.

    python tools/pst_verify_batch_time.py [--n 20] [--batches 1,8,64] [--runs 7]
                                          [--out profiles/verify_batch/verify_batch_time.json]

One polynomial of n variables is committed and opened once; a batch is B copies
of that proof, each with its own transcript.  Per B, after one warm-up of both
paths, medians over --runs of the host clock around (both paths end
synchronised; the item arrays are packed before the clock starts):
  batch_ms        one tpst_pst_verify_batch call (multipliers drawn before the clock starts)
  single_ms       B tpst_pst_verify calls, one after the other, in the same run
  speedup         single_ms / batch_ms
and, from the library's profile counters in further runs of the batch call
(device spans between HIP events, so a span holds whatever else ran beside it):
  lincomb_dev_ms  the three k_lincomb2 launches
  pairing_dev_ms  the multi-pairing call (G2 preparation to the final exponentiation)
  gt_pow_dev_ms   the GT-power launch (side stream, beside the two above)
  other_ms        batch_ms - max(lincomb + pairing, gt_pow): validation and the transcript replay on host
                  threads, staging, the G1 MSM of the U check, conversions, the host's GT product
Prints one JSON line per B.
"""
import argparse
import ctypes as C
import json
import os
import secrets
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np

    from testudo_amd import Context
    from testudo_amd import sqrt_pst as S
    from testudo_amd.encoding import ptr

    ctx = Context(0)
    n = args.n
    med = statistics.median
    S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
    Z, k = S.fr_stream(0x7E57D0, 1 << n)
    pt, _ = S.fr_stream(0x7E57D0, n, k)
    pl = S.Polynomial.from_evaluations(ctx, Z)
    v = pl.eval(pt)
    comms, T = pl.commit()
    U, pst_proof, mipp = pl.open(S.PoseidonTranscript(), comms, pt, T)
    body = (U, pt, v, pst_proof, mipp, T)
    assert S.verify(ctx, S.PoseidonTranscript(), *body)

    def draw(B):
        rho = np.zeros((B, 4, 2), dtype=np.uint64)
        for j in range(B):
            for q in range(4):
                x = secrets.randbits(128) | 1
                rho[j, q] = (x & (2**64 - 1), x >> 64)
        return rho

    lines = []
    for B in [int(x) for x in args.batches.split(",")]:
        ok = np.zeros(B, dtype=np.uint8)

        def batch():
            items = [(S.PoseidonTranscript(),) + body for _ in range(B)]
            nn, arr, keep = S.pack_items(items)
            rho = draw(B)
            t0 = time.perf_counter()
            rc = ctx.lib.tpst_pst_verify_batch(ctx.h, nn, C.cast(arr, C.c_void_p), B, ptr(rho),
                                               ok.ctypes.data_as(C.POINTER(C.c_uint8)))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and ok.all(), rc
            del keep
            return dt

        def singles():
            items = [(S.PoseidonTranscript(),) + body for _ in range(B)]
            nn, arr, keep = S.pack_items(items)
            t0 = time.perf_counter()
            for j in range(B):
                rc = ctx.lib.tpst_pst_verify(ctx.h, arr[j].tr, nn, arr[j].point, arr[j].v, arr[j].T, arr[j].proof)
                assert rc == 0, rc
            dt = (time.perf_counter() - t0) * 1e3
            del keep
            return dt

        batch()
        singles()
        tb = med([batch() for _ in range(args.runs)])
        ts = med([singles() for _ in range(args.runs)])
        ctx.profile(True)
        prof = {"lincomb": [], "verify_batch_pairing": [], "verify_batch_gt_pow": []}
        for _ in range(args.runs):
            ctx.profile_reset()
            batch()
            rd = ctx.profile_read()
            for name in prof:
                prof[name].append(rd[name][0])
        ctx.profile(False)
        lc, pr, gp = (med(prof[x]) for x in ("lincomb", "verify_batch_pairing", "verify_batch_gt_pow"))
        res = {"n": n, "B": B, "runs": args.runs, "batch_ms": round(tb, 3), "single_ms": round(ts, 3),
               "speedup": round(ts / tb, 3), "batch_ms_per_item": round(tb / B, 3),
               "single_ms_per_item": round(ts / B, 3), "lincomb_dev_ms": round(lc, 3),
               "pairing_dev_ms": round(pr, 3), "gt_pow_dev_ms": round(gp, 3),
               "other_ms": round(tb - max(lc + pr, gp), 3)}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
