"""Time the product sum-check (tpst_poly_sumcheck_open) against the combined
opening it ends in, on one GPU.

    python tools/sumcheck_time.py [--n 20,24] [--shapes b,c,d,e8] [--runs 5]
                                  [--out profiles/poly_sumcheck/sumcheck_time.json]

Shapes, over resident polynomials of n variables (random tables made on the
device), committed:
  b    B = 2, g = f_0 f_1                               D = 2
  c    B = 3 with tau, g = f_0 f_1 - f_2                D = 3
  d    B = 3, g = f_0 f_1 f_2                           D = 3
  e8   B = 8 with tau, g = sum over the two halves of
       3 f_0 f_1 + (r - 1) f_2 f_2 + f_3                D = 3
(the tables are random: c's claim is the sum as it comes out, not 0).  After one
warm-up of every call, medians of --runs with min and max, everything in one
run.  Host clock around calls that end synchronised:
  sumcheck_open_ms     tpst_poly_sumcheck_open (rounds + combined opening at rho)
  open_combined_ms     tpst_poly_open_combined of the same B polynomials at one point: what sumcheck_open
                       spends after its rounds; the difference of the two is the sum-check's cost
  reduction_ms         tpst_poly_sumcheck_stages: the device rounds alone (uploads, the half tables, the n
                       round trips of the sums and challenges included)
From the library's profile counters in further runs of the rounds (device spans between HIP events, round
kernel + reduce launch):
  round0_dev_ms        round 0: reads B 2^n 32 B
  round1_dev_ms        round 1: reads the same, writes (B + has_tau) 2^(n-1) 32 B
  rounds_dev_ms        every later round and the closing bind: reads and writes halve each round
and for rounds 0 and 1 that traffic over the span as GB/s and as a share of 8 TB/s, and the Montgomery products
of round 0 over its span: per index pair (D + 1) (sum_t deg_t + has_tau) for the summand at t = 0..D and
2 has_tau for eq from the half tables.
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
R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001


def shape(name):
    """(B, [(coeff, [indices])], has_tau)"""
    if name == "b":
        return 2, [(1, [0, 1])], False
    if name == "c":
        return 3, [(1, [0, 1]), (R - 1, [2])], True
    if name == "d":
        return 3, [(1, [0, 1, 2])], False
    if name == "e8":
        return 8, [t for b in (0, 4) for t in ((3, [b, b + 1]), (R - 1, [b + 2, b + 2]), (1, [b + 3]))], True
    raise SystemExit("unknown shape " + name)


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
    ap.add_argument("--shapes", default="b,c,d,e8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from testudo_amd import Context
    from testudo_amd import sqrt_pst as S
    from testudo_amd.encoding import fr_array

    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    shapes = [(name,) + shape(name) for name in args.shapes.split(",")]
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x5C17 + n)
        polys, commitments, tens = [], [], []
        for j in range(max(B for _, B, _, _ in shapes)):
            # uniform 252-bit values: canonical Fr (r > 2^252)
            t = torch.randint(-2**63, 2**63 - 1, (1 << n, 4), dtype=torch.int64, device=dev, generator=gen)
            t[:, 3] &= (1 << 60) - 1
            torch.cuda.synchronize()
            tens.append(t)
            p = S.Polynomial.from_device(ctx, t.data_ptr(), n, keep=t)
            commitments.append(p.commit())
            polys.append(p)
        print("# n = %d: %d polynomials committed" % (n, len(polys)), file=sys.stderr, flush=True)
        for name, B, terms, has_tau in shapes:
            ps, cs = polys[:B], commitments[:B]
            rng = random.Random(0x5C17 + 64 * n + B)
            lt = [(fr_array([c])[0], idx) for c, idx in terms]
            tau = fr_array([rng.randrange(R) for _ in range(n)]) if has_tau else None
            rho = fr_array([rng.randrange(R) for _ in range(n)])
            one_point = fr_array([rng.randrange(R) for _ in range(n)])
            D = max(max(len(idx) for _, idx in terms) + has_tau, 2)

            def opened():
                return S.sumcheck_open(ps, cs, S.PoseidonTranscript(), lt, tau)

            def combined():
                # (the weights from given values: Polynomial.eval would cache a q per handle)
                w = fr_array([rng.randrange(1, R) for _ in range(B)])
                return S.open_combined(ps, cs, S.PoseidonTranscript(), one_point, w)

            def reduction():
                return S.sumcheck_stages(ps, lt, tau, rho)

            calls = {"sumcheck_open_ms": opened, "open_combined_ms": combined, "reduction_ms": reduction}
            # warm-up, and the proof verifies
            e0, proof = opened()[:2]
            assert S.verify_sumcheck(ctx, S.PoseidonTranscript(), lt, tau, [T for _, T in cs], e0, proof)
            for fn in calls.values():
                fn()
            res = {"n": n, "shape": name, "B": B, "M": len(terms), "D": D, "tau": has_tau, "runs": args.runs}
            for key, fn in calls.items():
                res[key] = stat(timed(fn, args.runs))
            ctx.profile(True)
            r0, r1, rr = [], [], []
            for _ in range(args.runs):
                ctx.profile_reset()
                reduction()
                rd = ctx.profile_read()
                r0.append(rd["sumcheck_round0"][0])
                r1.append(rd["sumcheck_round1"][0])
                rr.append(rd["sumcheck_rounds"][0])
            ctx.profile(False)
            res["round0_dev_ms"], res["round1_dev_ms"], res["rounds_dev_ms"] = stat(r0), stat(r1), stat(rr)
            res["reduction_dev_ms"] = round(statistics.median(r0) + statistics.median(r1) + statistics.median(rr), 3)
            table = B * (1 << n) * 32
            for key, ms, traffic in (("round0", r0, table), ("round1", r1, table + (B + has_tau) * (1 << n) * 16)):
                rate = traffic / (statistics.median(ms) * 1e-3)
                res[key + "_gbs"] = round(rate / 1e9, 1)
                res[key + "_share_of_peak"] = round(rate / PEAK_BYTES_PER_S, 4)
            per_pair = (D + 1) * (sum(len(idx) for _, idx in terms) + has_tau) + 2 * has_tau
            res["round0_products_per_pair"] = per_pair
            for key, ms in (("median", statistics.median(r0)), ("min", max(r0)), ("max", min(r0))):
                res["round0_gproducts_per_s_" + key] = round(per_pair * (1 << (n - 1)) / (ms * 1e-3) / 1e9, 1)
            res["open_minus_combined_ms"] = round(res["sumcheck_open_ms"]["median"] - res["open_combined_ms"]["median"], 3)
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
