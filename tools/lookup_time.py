"""Time the lookup argument (tpst_poly_lookup_open) stage by stage on one GPU
(DESIGN.md §4), against the yardstick of one Polynomial.commit() at the same n.

    python tools/lookup_time.py [--n 20,24] [--L 1,4] [--witness uniform,all_equal] [--runs 5]
                                [--out profiles/lookup/lookup_time.json]

The table is the range table t(y) = y; the witnesses are resident polynomials
of n variables made on the device, uniform in range or all equal to one value,
committed before the clock starts.  After one warm-up (the proof is verified),
medians of --runs with min and max, everything in one run:
  lookup_open_ms   host clock around tpst_poly_lookup_open (it ends synchronised)
  commit_ms        host clock around Polynomial.commit() of a witness: the yardstick
and, from the library's profile counters of the same lookup_open runs (device
spans between HIP events):
  index            the table's index: the memset of the slots and k_lk_index
  count            the probes and counts: two memsets, k_lk_count, k_lk_counts_fr
  inversion        k_lk_inverse over the L witnesses and the table
  half_evals       k_lk_sum over the L + 1 tables h: their values at the 1/2 point
  commits          the L + 2 commits of m and every h (sqrt_commit spans)
  sumcheck         the product sum-check's rounds (B = 2L + 3, 2L + 3 terms under tau)
  multi_reduction  the multi-point reduction's rounds (3L + 4 claims)
  combine          the combined opening's table and row combinations
  opening          the opening of the combination (sqrt_open span)
helpers_over_commit is (index + count + inversion) / the commit's device span
(commit_dev_ms) of the same run: the issue expects it below 1.
Prints one JSON line per case.
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

STAGES = {
    "index": ["lookup_index"], "count": ["lookup_count"], "inversion": ["lookup_inverse"],
    "half_evals": ["lookup_sums"], "commits": ["sqrt_commit"],
    "sumcheck": ["sumcheck_round0", "sumcheck_round1", "sumcheck_rounds"],
    "multi_reduction": ["multi_round0", "multi_round1", "multi_rounds"],
    "combine": ["fr_lincomb", "lincomb_rows"], "opening": ["sqrt_open"],
}


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="20,24")
    ap.add_argument("--L", default="1,4")
    ap.add_argument("--witness", default="uniform,all_equal")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from testudo_amd import Context
    from testudo_amd import sqrt_pst as S

    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    Ls = [int(x) for x in args.L.split(",")]
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        N = 1 << n
        S.srs_setup(ctx, (n + 1) // 2, 0x7E57D1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x10E0 + n)
        tt = torch.zeros((N, 4), dtype=torch.int64, device=dev)
        tt[:, 0] = torch.arange(N, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        table = S.Polynomial.from_device(ctx, tt.data_ptr(), n, keep=tt)
        table_c = table.commit()
        for kind in args.witness.split(","):
            wits, wcs = [], []
            for l in range(max(Ls)):
                w = torch.zeros((N, 4), dtype=torch.int64, device=dev)
                if kind == "uniform":
                    w[:, 0] = torch.randint(0, N, (N,), dtype=torch.int64, device=dev, generator=gen)
                else:
                    w[:, 0] = (N // 3) + l
                torch.cuda.synchronize()
                p = S.Polynomial.from_device(ctx, w.data_ptr(), n, keep=w)
                wcs.append(p.commit())
                wits.append(p)
            print("# n = %d, %s: %d witnesses committed" % (n, kind, len(wits)), file=sys.stderr, flush=True)
            for L in Ls:
                ps, cs = wits[:L], wcs[:L] + [table_c]

                def opened():
                    return S.lookup_open(ps, table, cs, S.PoseidonTranscript())

                proof = opened()[0]                                   # warm-up, and the proof verifies
                assert S.verify_lookup(ctx, S.PoseidonTranscript(), [T for _, T in cs], proof)
                wall, spans = [], {k: [] for k in STAGES}
                ctx.profile(True)
                for _ in range(args.runs):
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    opened()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    rd = ctx.profile_read()
                    for k, names in STAGES.items():
                        spans[k].append(sum(rd[x][0] for x in names))
                # the yardstick: one commit of a witness, wall and device span
                cw, cd = [], []
                ps[0].commit()
                for _ in range(args.runs):
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    ps[0].commit()
                    cw.append((time.perf_counter() - t0) * 1e3)
                    cd.append(ctx.profile_read()["sqrt_commit"][0])
                ctx.profile(False)
                res = {"n": n, "L": L, "witness": kind, "B": 2 * L + 3, "runs": args.runs, "lookup_open_ms": stat(wall),
                       "commit_ms": stat(cw), "commit_dev_ms": stat(cd)}
                for k in STAGES:
                    res[k + "_dev_ms"] = stat(spans[k])
                helpers = sum(statistics.median(spans[k]) for k in ("index", "count", "inversion"))
                res["helpers_dev_ms"] = round(helpers, 3)
                res["helpers_over_commit"] = round(helpers / statistics.median(cd), 3)
                line = json.dumps(res)
                print(line, flush=True)
                lines.append(line)
            del wits, wcs
            torch.cuda.empty_cache()
        del table, table_c
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
