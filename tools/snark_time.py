"""Time TestudoSnark end to end (tpst_snark_prove / tpst_snark_verify) against
the sum of its parts, on one GPU.

    python tools/snark_time.py [--logs 16,20] [--runs 7] [--out profiles/snark/snark_time.json]

Per size (a synthetic instance of 2^log constraints and variables, 10 inputs),
from a resident instance, commitment and decommitment, after one warm-up of
every call, over --runs repetitions of each, in the same run:
  prove_wall_ms / verify_wall_ms   host clock around TestudoSnark.prove / .verify
  the parts alone, at the proof's own (rx, ry):
    sat_prove_ms     R1CSProof.prove (tpst_r1cs_prove)
    evaluate_ms      R1CSInstance.evaluate (tpst_r1cs_evaluate)
    eval_prove_ms    R1CSEvalProof.prove (tpst_r1cs_eval_prove)
    sat_verify_ms    tpst_r1cs_verify_evals
    eval_verify_ms   tpst_r1cs_eval_verify
  absorb_ms          the host replay alone of step 1 (the commitment's absorb:
                     6 append_u64 and one append_point per row) plus step 8
                     (1 + |rx| + |ry| + 3 append_scalar), what the composition
                     adds to the transcript; it runs once in prove and once in verify
  prove_parts_ms / verify_parts_ms   the medians of the parts summed
  prove_assembly_ms / verify_assembly_ms   whole call - parts, beside the parts'
                     own min-max spread (prove_parts_spread_ms, verify_parts_spread_ms:
                     the sum of each part's max - min over the repetitions)
  absorb_share_of_assembly   absorb_ms / the assembly of prove
  proof_bytes        the wire format of the SNARK proof
Every figure is a median with its min and max.  Prints one JSON line per size.
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
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from testudo_amd import Context, sqrt_pst
    from testudo_amd.hyrax import FrTranscript
    from testudo_amd.r1cs import R1CSInstance, R1CSProof
    from testudo_amd.r1cs_eval import R1CSEvalProof
    from testudo_amd.snark import TestudoSnark, TestudoSnarkGens, encode
    from testudo_amd.sqrt_pst import PoseidonTranscript, fr_stream

    ctx = Context(0)
    lines = []
    for lg in (int(x) for x in args.logs.split(",")):
        n = 1 << lg
        inst, vars_, inputs = R1CSInstance.produce_synthetic_r1cs(ctx, n, n, 10, 0x534E + lg)
        gens = TestudoSnarkGens.setup(ctx, n, n, 10, n)
        sqrt_pst.srs_setup(ctx, gens.srs_nv, 0x7E57D1)
        sz, eg = gens.sizes, gens.gens_r1cs_eval
        comm, decomm = encode(inst, gens)
        rnd, k = [], 0
        for j in range(3):
            r, k = fr_stream(0x534F + lg, sz.rnd_len[j], k)
            rnd.append(r)

        def prove():
            return TestudoSnark.prove(comm, decomm, vars_, inputs, gens, FrTranscript(), rnd)

        proof = prove()  # warm-up
        assert proof.verify(gens, comm, inputs, FrTranscript())  # warm-up, and the proof is sound
        sat, rx, ry, evals = proof.r1cs_sat_proof, proof.r1cs_sat_proof.rx, proof.r1cs_sat_proof.ry, proof.inst_evals

        def absorb():
            tr = FrTranscript()
            comm.write_to_transcript(tr)
            tr.append_scalar(sat.transcript_sat_state)
            tr.append_scalars(rx)
            tr.append_scalars(ry)
            tr.append_scalars(evals)

        parts = {
            "sat_prove_ms": lambda: R1CSProof.prove(inst, vars_, inputs, PoseidonTranscript()),
            "evaluate_ms": lambda: inst.evaluate(rx, ry),
            "eval_prove_ms": lambda: R1CSEvalProof.prove(decomm.decomm, rx, ry, evals, eg, FrTranscript(), rnd),
        }
        # the verifiers' parts on proofs that verify: made on fresh transcripts, as the parts take them
        sat_alone, _rx, _ry = R1CSProof.prove(inst, vars_, inputs, PoseidonTranscript())
        ev_alone_evals = inst.evaluate(sat_alone.rx, sat_alone.ry)
        ev_alone = R1CSEvalProof.prove(decomm.decomm, rx, ry, evals, eg, FrTranscript(), rnd)

        def sat_verify():
            assert sat_alone.verify(inst, inputs, PoseidonTranscript(), evals=ev_alone_evals)

        def eval_verify():
            assert ev_alone.verify(comm.comm, rx, ry, evals, eg, FrTranscript())

        vparts = {"sat_verify_ms": sat_verify, "eval_verify_ms": eval_verify}
        for fn in list(parts.values()) + list(vparts.values()) + [absorb]:
            fn()  # warm-up
        res = {"log_cons": lg, "runs": args.runs, "ops_rows": sz.ops_rows, "mem_rows": sz.mem_rows}
        res["prove_wall_ms"] = stat(timed(prove, args.runs))
        res["verify_wall_ms"] = stat(timed(lambda: proof.verify(gens, comm, inputs, FrTranscript()), args.runs))
        for name, fn in list(parts.items()) + list(vparts.items()) + [("absorb_ms", absorb)]:
            res[name] = stat(timed(fn, args.runs))
        for side, group in (("prove", parts), ("verify", vparts)):
            total = sum(res[k]["median"] for k in group)
            spread = sum(res[k]["max"] - res[k]["min"] for k in group)
            res[side + "_parts_ms"] = round(total, 3)
            res[side + "_parts_spread_ms"] = round(spread, 3)
            res[side + "_assembly_ms"] = round(res[side + "_wall_ms"]["median"] - total, 3)
        asm = res["prove_assembly_ms"]
        res["absorb_share_of_assembly"] = round(res["absorb_ms"]["median"] / asm, 3) if asm > 0 else None
        res["absorb_share_of_prove"] = round(res["absorb_ms"]["median"] / res["prove_wall_ms"]["median"], 4)
        res["absorb_share_of_verify"] = round(res["absorb_ms"]["median"] / res["verify_wall_ms"]["median"], 4)
        res["proof_bytes"] = len(proof.to_bytes(gens))
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        decomm.decomm.close()
        gens.close()
        del inst, decomm, proof, sat_alone, ev_alone
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
