"""Time the multi-point opening (tpst_poly_open_multi) against the parent's way
to the same claims, K separate openings, on one GPU.

    python tools/open_multi_time.py [--n 20,24] [--shapes 1x2,2x2,8x8,8x32] [--runs 5]
                                    [--out profiles/open_multi/open_multi_time.json]

Per (n, B, K) -- B resident polynomials of n variables (random tables made on
the device), committed; claim k on polynomial k mod B at its own random point,
with the true value -- after one warm-up of every call, medians of --runs with
min and max, everything in one run.  Host clock around calls that end
synchronised:
  open_multi_ms        tpst_poly_open_multi (reduction + combined opening at rho)
  separate_opens_ms    the parent's way: K Polynomial.open calls, one per claim, fresh transcripts
  open_combined_ms     tpst_poly_open_combined of the same B polynomials at one point: what open_multi
                       spends after its reduction
  reduction_ms         tpst_poly_multi_sumcheck_stages: the device reduction alone (uploads, the n
                       round trips of the sums and challenges included)
From the library's profile counters in further runs of the reduction (device spans between HIP events,
round kernel + reduce launch):
  round0_dev_ms        round 0: reads B 2^n 32 B
  round1_dev_ms        round 1: reads the same, writes 2B 2^(n-1) 32 B
  rounds_dev_ms        every later round and the closing bind: reads and writes halve each round
and for rounds 0 and 1 that traffic over the span as GB/s and as a share of 8 TB/s.
Prints one JSON line per case.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E


def timed(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="20,24")
    ap.add_argument("--shapes", default="1x2,2x2,8x8,8x32")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from testudo_amd import Context
    from testudo_amd import sqrt_pst as S
    from testudo_amd.encoding import fr_array

    R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    shapes = [tuple(int(v) for v in x.split("x")) for x in args.shapes.split(",")]
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x3A17 + n)
        polys, commitments, tens = [], [], []

        def handle(j):
            """a fresh handle on table j: a handle keeps the q of the first point it is evaluated or opened at
            (sqrt_pst.rs:105-115), so every claim of the parent's way needs its own"""
            return S.Polynomial.from_device(ctx, tens[j].data_ptr(), n, keep=tens[j])

        for j in range(max(B for B, _ in shapes)):
            # uniform 252-bit values: canonical Fr (r > 2^252)
            t = torch.randint(-2**63, 2**63 - 1, (1 << n, 4), dtype=torch.int64, device=dev, generator=gen)
            t[:, 3] &= (1 << 60) - 1
            torch.cuda.synchronize()
            tens.append(t)
            p = handle(j)
            commitments.append(p.commit())
            polys.append(p)
        print("# n = %d: %d polynomials committed" % (n, len(polys)), file=sys.stderr, flush=True)
        for B, K in shapes:
            ps, cs = polys[:B], commitments[:B]
            rng = random.Random(0x3A17 + 64 * n + 8 * B + K)
            claims = []
            for k in range(K):
                pt = fr_array([rng.randrange(R) for _ in range(n)])
                claims.append((k % B, pt, handle(k % B).eval(pt)))
            a = fr_array([rng.randrange(R) for _ in range(K)])
            rho = fr_array([rng.randrange(R) for _ in range(n)])
            one_point = claims[0][1]

            def multi():
                return S.open_multi(ps, cs, S.PoseidonTranscript(), claims)

            def separate():
                for j, pt, _ in claims:
                    handle(j).open(S.PoseidonTranscript(), cs[j][0], pt, cs[j][1])

            def combined():
                return S.open_combined(ps, cs, S.PoseidonTranscript(), one_point)

            def reduction():
                return S.multi_sumcheck_stages(ps, claims, a, rho)

            calls = {"open_multi_ms": multi, "separate_opens_ms": separate, "open_combined_ms": combined,
                     "reduction_ms": reduction}
            # warm-up, and the proof verifies
            proof = multi()[0]
            assert S.verify_multi(ctx, S.PoseidonTranscript(), claims, [T for _, T in cs], proof)
            for fn in calls.values():
                fn()
            res = {"n": n, "B": B, "K": K, "runs": args.runs}
            for name, fn in calls.items():
                res[name] = stat(timed(fn, args.runs))
            ctx.profile(True)
            r0, r1, rr = [], [], []
            for _ in range(args.runs):
                ctx.profile_reset()
                reduction()
                rd = ctx.profile_read()
                r0.append(rd["multi_round0"][0])
                r1.append(rd["multi_round1"][0])
                rr.append(rd["multi_rounds"][0])
            ctx.profile(False)
            res["round0_dev_ms"], res["round1_dev_ms"], res["rounds_dev_ms"] = stat(r0), stat(r1), stat(rr)
            res["reduction_dev_ms"] = round(statistics.median(r0) + statistics.median(r1) + statistics.median(rr), 3)
            table = B * (1 << n) * 32
            for name, ms, traffic in (("round0", r0, table), ("round1", r1, 2 * table)):
                rate = traffic / (statistics.median(ms) * 1e-3)
                res[name + "_gbs"] = round(rate / 1e9, 1)
                res[name + "_share_of_peak"] = round(rate / PEAK_BYTES_PER_S, 4)
            res["multi_vs_separate"] = round(res["separate_opens_ms"]["median"] / res["open_multi_ms"]["median"], 3)
            res["multi_minus_combined_ms"] = round(res["open_multi_ms"]["median"] - res["open_combined_ms"]["median"], 3)
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
        del polys, commitments
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
