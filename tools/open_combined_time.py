"""Time the combined opening (tpst_poly_open_combined and its parts) against the
parent's ways to the same values, on one GPU.

    python tools/open_combined_time.py [--n 20,24] [--batches 2,8,32] [--runs 7]
                                       [--out profiles/open_combined/open_combined_time.json]

Per (n, B, weight size) -- B resident polynomials of n variables (random tables
made on the device), committed and evaluated at one point; weights of 128 bits
or of full size -- after one warm-up of every call, medians of --runs with min
and max, everything in one run.  Host clock around calls that end synchronised:
  lincomb_ms           tpst_poly_lincomb (allocation of Z* included)
  commit_lincomb_ms    tpst_commit_lincomb: row lists and T_j from the host, both outputs
  recommit_ms          the parent's way to the same (comm_list*, T*), Z* GIVEN on the host:
                       Polynomial.from_evaluations(Z*) + commit()
  open_combined_ms     tpst_poly_open_combined (lincomb + commit_lincomb + eval + open)
  separate_opens_ms    B Polynomial.open calls of the parent, one per polynomial (q cached by the
                       evaluation before the clock starts), fresh transcripts
  host_route_ms        "combine on the host, re-commit, open once" WITHOUT the host combination
                       (Z* given): from_evaluations(Z*) + commit + eval + open -- a lower bound of that route
From the library's profile counters in further runs (device spans between HIP events):
  fr_lincomb_dev_ms    k_fr_lincomb alone; fr_lincomb_gbs = (B + 1) 2^n 32 B over it, and
                       fr_lincomb_share_of_peak against 8 TB/s
  lincomb_rows_dev_ms  k_g1_lincomb_rows and the sum of its chains (chains = how many per row)
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
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from testudo_amd import Context
    from testudo_amd import sqrt_pst as S
    from testudo_amd.encoding import fr_array

    R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    batches = [int(x) for x in args.batches.split(",")]
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
        pt, _ = S.fr_stream(0x0C0B + n, n)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x0C0B + n)
        polys, commitments = [], []
        for j in range(max(batches)):
            # uniform 252-bit values: canonical Fr (r > 2^252)
            t = torch.randint(-2**63, 2**63 - 1, (1 << n, 4), dtype=torch.int64, device=dev, generator=gen)
            t[:, 3] &= (1 << 60) - 1
            torch.cuda.synchronize()
            p = S.Polynomial.from_device(ctx, t.data_ptr(), n, keep=t)
            commitments.append(p.commit())
            p.eval(pt)
            polys.append(p)
        print("# n = %d: %d polynomials committed" % (n, len(polys)), file=sys.stderr, flush=True)
        for B in batches:
            ps, cs = polys[:B], commitments[:B]
            cl, tl = [c for c, _ in cs], [T for _, T in cs]
            for bits in (128, 253):
                rng = random.Random(0x0C0B + 64 * n + B + bits)
                w = fr_array([(rng.getrandbits(128) | 1) if bits == 128 else rng.randrange(1, R) for _ in range(B)])
                zstar = S.Polynomial.lincomb(ps, w).evaluations()  # "Z* given" of the parent's routes

                def recommit():
                    return S.Polynomial.from_evaluations(ctx, zstar).commit()

                def host_route():
                    pl = S.Polynomial.from_evaluations(ctx, zstar)
                    comms, T = pl.commit()
                    pl.eval(pt)
                    return comms, T, pl.open(S.PoseidonTranscript(), comms, pt, T)

                def separate():
                    for p, (c, T) in zip(ps, cs):
                        p.open(S.PoseidonTranscript(), c, pt, T)

                def combined():
                    return S.open_combined(ps, cs, S.PoseidonTranscript(), pt, w)

                calls = {
                    "lincomb_ms": lambda: S.Polynomial.lincomb(ps, w),
                    "commit_lincomb_ms": lambda: S.commit_lincomb(ctx, n, cl, tl, w),
                    "recommit_ms": recommit,
                    "open_combined_ms": combined,
                    "separate_opens_ms": separate,
                    "host_route_ms": host_route,
                }
                # warm-up, and the routes agree
                a, b = combined(), host_route()
                assert np.array_equal(a[1], b[0]) and np.array_equal(a[2], b[1]) and np.array_equal(a[4][0], b[2][0])
                for fn in calls.values():
                    fn()
                res = {"n": n, "B": B, "weight_bits": bits, "runs": args.runs}
                for name, fn in calls.items():
                    res[name] = stat(timed(fn, args.runs))
                ctx.profile(True)
                fl, lr = [], []
                for _ in range(args.runs):
                    ctx.profile_reset()
                    S.Polynomial.lincomb(ps, w)
                    S.commit_lincomb(ctx, n, cl, None, w)
                    rd = ctx.profile_read()
                    fl.append(rd["fr_lincomb"][0])
                    lr.append(rd["lincomb_rows"][0])
                ctx.profile(False)
                res["fr_lincomb_dev_ms"], res["lincomb_rows_dev_ms"] = stat(fl), stat(lr)
                rate = (B + 1) * (1 << n) * 32 / (statistics.median(fl) * 1e-3)
                res["fr_lincomb_gbs"] = round(rate / 1e9, 1)
                res["fr_lincomb_share_of_peak"] = round(rate / PEAK_BYTES_PER_S, 4)
                res["chains"] = int(os.environ.get("TPST_ROW_CHAINS") or min(B, 16, max(1, 32768 >> (n // 2))))
                res["commit_lincomb_vs_recommit"] = round(res["recommit_ms"]["median"] /
                                                          res["commit_lincomb_ms"]["median"], 3)
                res["combined_vs_separate"] = round(res["separate_opens_ms"]["median"] /
                                                    res["open_combined_ms"]["median"], 3)
                res["combined_vs_host_route"] = round(res["host_route_ms"]["median"] /
                                                      res["open_combined_ms"]["median"], 3)
                line = json.dumps(res)
                print(line, flush=True)
                lines.append(line)
                del zstar
        del polys, commitments
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
