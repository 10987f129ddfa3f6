"""Time the Hyrax evaluation proof (tpst_hyrax_eval_prove_dev / _verify) on one
GPU.

    python tools/hyrax_time.py [--ells 20,24] [--runs 7] [--out profiles/hyrax_eval/hyrax_time.json]

Per ell, after one warm-up of every call, medians over --runs of:
  prove_wall_ms       host clock around eval_prove from a device-resident Z (the
                      call ends synchronised), zero blinds
  eq_tables_dev_ms    HIP events of tpst_profile_*: the L / R eq tables
  bound_dev_ms        the bound kernel and its partial-sum pass
  rounds_ms           the dot-product proof from its first launch to the last
                      round's results (device work and the host work between)
  host_transcript_ms  the same absorbs and squeezes replayed alone on the host:
                      append_scalar_vector of the R-entry vector (R / 2
                      Poseidon<Fr> permutations, the protocol's floor), two
                      points and a challenge per round, two points and a challenge
  verify_wall_ms      eval_verify with a fresh transcript (the subgroup checks of
                      the 2^(ell/2) row commitments, MSM(comm, L), the s vector,
                      G_hat, a_hat and the host's final equation)
and the bound kernel's rate: the bytes the algorithm needs (32 B per evaluation,
L and the LZ output) over bound_dev_ms, against the 8 TB/s HBM peak.
Prints one JSON line per ell.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ells", default="20,24")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from testudo_amd import Context
    from testudo_amd.engine import dense_commit
    from testudo_amd.hyrax import FrTranscript, HyraxGens, dense_evaluate, eval_prove, eval_verify
    from testudo_amd.sqrt_pst import fr_stream

    ctx = Context(0)
    med = statistics.median
    lines = []
    for ell in [int(x) for x in args.ells.split(",")]:
        lv = ell // 2
        rv = ell - lv
        Ls, Rs = 1 << lv, 1 << rv
        hg = HyraxGens.setup(ctx, ell, b"hyrax_time")
        Z, k = fr_stream(0x4879 + ell, 1 << ell)
        r, k = fr_stream(0x4879 + ell, ell, k)
        rnd, _ = fr_stream(0x4879 + ell, 3 + 4 * rv, k)
        comm = dense_commit(hg.gens, Z)
        Zr = dense_evaluate(ctx, Z, r)
        d_Z = torch.from_numpy(np.ascontiguousarray(Z).view(np.int64)).to(torch.device("cuda", ctx.device))
        ctx.torch_to_lib()

        def prove():
            return eval_prove(hg, d_Z.data_ptr(), r, Zr, rnd, FrTranscript(), ell=ell)

        proof, C_Zr = prove()  # warm-up
        assert eval_verify(hg, r, C_Zr, comm, FrTranscript(), proof)  # warm-up
        wall, eq, bound, rounds, vwall = [], [], [], [], []
        ctx.profile(True)
        for _ in range(args.runs):
            ctx.profile_reset()
            t0 = time.perf_counter()
            prove()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.profile_read()
            eq.append(st["hyrax_eq"][0])
            bound.append(st["hyrax_bound"][0])
            rounds.append(st["hyrax_rounds"][0])
        ctx.profile(False)
        for _ in range(args.runs):
            t0 = time.perf_counter()
            ok = eval_verify(hg, r, C_Zr, comm, FrTranscript(), proof)
            vwall.append((time.perf_counter() - t0) * 1e3)
            assert ok
        # the host transcript alone: the prover's absorbs and squeezes
        a_vec, _ = fr_stream(1, Rs)
        tvec, tall = [], []
        for _ in range(args.runs):
            tr = FrTranscript()
            t0 = time.perf_counter()
            tr.append_point(C_Zr)
            tr.append_point(C_Zr)
            t1 = time.perf_counter()
            tr.append_scalars(a_vec)
            t2 = time.perf_counter()
            for _k in range(rv + 1):
                tr.append_point(C_Zr)
                tr.append_point(C_Zr)
                tr.challenge_scalar()
            t3 = time.perf_counter()
            tvec.append((t2 - t1) * 1e3)
            tall.append((t3 - t0) * 1e3)
        bound_bytes = 32 * ((1 << ell) + Ls + Rs)
        gbs = bound_bytes / (med(bound) * 1e-3) / 1e9
        res = {"ell": ell, "L": Ls, "R": Rs, "runs": args.runs,
               "prove_wall_ms": round(med(wall), 3), "eq_tables_dev_ms": round(med(eq), 4),
               "bound_dev_ms": round(med(bound), 4), "rounds_ms": round(med(rounds), 3),
               "host_transcript_ms": round(med(tall), 3), "host_scalar_vector_ms": round(med(tvec), 3),
               "host_transcript_share_of_prove": round(med(tall) / med(wall), 4),
               "bound_bytes": bound_bytes, "bound_gbs": round(gbs, 1),
               "bound_fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
               "verify_wall_ms": round(med(vwall), 3)}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del d_Z
        hg.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
