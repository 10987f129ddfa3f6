"""Time the SPARK evaluation proof (tpst_r1cs_eval_prove / tpst_r1cs_eval_verify)
on one GPU.

    python tools/r1cs_eval_time.py [--logs 16,20] [--runs 7] [--out profiles/r1cs_eval/r1cs_eval_time.json]

Per size (a synthetic instance of 2^log constraints and variables, 10 inputs),
from a resident decommitment and after one warm-up of every call, medians over
--runs of:
  prove_wall_ms / verify_wall_ms   host clock around the two calls (both end
                      synchronised)
  deref / hash_ops / hash_mem / seg_eval   HIP events of tpst_profile_* around
                      the four new stages, with the bytes the algorithm needs
                      and that rate's share of the 8 TB/s HBM peak:
                        k_deref     6 N (4 B address + 32 B gathered + 32 B written)
                        k_hash_ops  6 N (4 + 4 + 32 B read) + 12 N 32 B written
                        k_hash_mem  2 cells (32 + 4 B read) + 4 cells 32 B written
                        k_seg_eval  (21 + 1) N 32 B + (2 + 1) cells 32 B read
                      (seg_eval covers both groups and their partial sums)
  verify_rows_host16_once_ms   the verifier's row-commitment validation alone, the way the host
                      does it (tpst_microbench kind 20: host::parallel_for over point_valid, up to
                      16 threads) over as many points as comm_derefs, comm_ops and comm_mem hold,
                      one pass (the verifier makes two)
  verify_point_codec_dev_ms / _launches   the device row checks of one verify (point_codec stage)
  proof_bytes / commitment_bytes   the arkworks wire format (Compress::Yes) of the proof and of the
                      commitment it opens, as the library's writers give them
  host_transcript_ms  the prover's absorbs and squeezes replayed alone on the host
  parts_wall_ms       what could be timed before this call existed, on
                      same-shaped inputs: three tpst_hyrax_eval_prove_dev (ell =
                      derefs, ops, mem) and two tpst_prodcircuit_prove_dev at
                      (log N, 12, 6) and (log cells, 4, 0), summed
  assembly_ms         prove_wall_ms - parts_wall_ms: the eq tables, the
                      dereference and its commitment, the hash layer, the 23
                      evaluations and the host work between the parts
Prints one JSON line per size.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def replay_prodcircuit(tr, ell, P, D, one):
    for i in range(ell):
        for _ in range(P + (D if i == ell - 1 else 0)):
            tr.challenge_scalar()
        for _j in range(i):
            for _c in range(4):
                tr.append_scalar(one)
            tr.challenge_scalar()
        for _ in range(2 * P + (3 * D if i == ell - 1 else 0)):
            tr.append_scalar(one)
        tr.challenge_scalar()


def replay_transcript(sz, FrTranscript, one, pt):
    """the prover's transcript traffic alone (values do not matter)"""
    tr = FrTranscript()
    t0 = time.perf_counter()
    for _ in range(sz.derefs_rows):
        tr.append_point(pt)
    for _ in range(2):
        tr.challenge_scalar()
    for _ in range(16 + 6):
        tr.append_scalar(one)
    replay_prodcircuit(tr, sz.log_ops, 12, 6, one)
    replay_prodcircuit(tr, sz.log_cells, 4, 0, one)
    for n_evals, ell in ((8, sz.ell_derefs), (16, sz.ell_ops), (2, sz.ell_mem)):
        for _ in range(n_evals):
            tr.append_scalar(one)
        for _ in range(n_evals.bit_length() - 1):
            tr.challenge_scalar()
        tr.append_scalar(one)
        lg = ell - ell // 2
        tr.append_point(pt)  # Cx, Cy, the vector a, per round L, R and a challenge, delta, beta, c
        tr.append_point(pt)
        for _ in range(1 << lg):
            tr.append_scalar(one)
        for _ in range(lg):
            tr.append_point(pt)
            tr.append_point(pt)
            tr.challenge_scalar()
        tr.append_point(pt)
        tr.append_point(pt)
        tr.challenge_scalar()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from testudo_amd import Context
    from testudo_amd import product_tree as PT
    from testudo_amd import serialize as W
    from testudo_amd.hyrax import FrTranscript, HyraxGens, eval_prove
    from testudo_amd.r1cs import R1CSInstance
    from testudo_amd.r1cs_eval import R1CSCommitmentGens, R1CSEvalProof, commit_decomm
    from testudo_amd.sqrt_pst import fr_stream

    ctx = Context(0)
    dev = torch.device("cuda", ctx.device)
    med = statistics.median
    label = b"r1cs_eval_time"
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    lines = []
    for lg in (int(x) for x in args.logs.split(",")):
        n = 1 << lg
        inst, _v, _x = R1CSInstance.produce_synthetic_r1cs(ctx, n, n, 10, 0x5345 + lg)
        gens = R1CSCommitmentGens.setup(ctx, label, n, n, 10, n)
        sz = gens.sizes
        comm, decomm = commit_decomm(inst, gens)
        N, cells = sz.num_ops, sz.num_mem_cells
        pts, k = fr_stream(0x5346 + lg, lg + lg + 1)
        rx, ry = pts[:lg], pts[lg:]
        rnd = []
        for j in range(3):
            r, k = fr_stream(0x5346 + lg, sz.rnd_len[j], k)
            rnd.append(r)
        evals = inst.evaluate(rx, ry)

        def prove():
            return R1CSEvalProof.prove(decomm, rx, ry, evals, gens, FrTranscript(), rnd)

        proof = prove()  # warm-up
        assert proof.verify(comm, rx, ry, evals, gens, FrTranscript())  # warm-up, and the proof is sound
        replay_transcript(sz, FrTranscript, one, comm.comm_mem[0])
        wall, vwall, thost = [], [], []
        dev_ms = {s: [] for s in ("sparse_deref", "sparse_hash_ops", "sparse_hash_mem", "sparse_seg_eval")}
        ctx.profile(True)
        for _ in range(args.runs):
            ctx.profile_reset()
            t0 = time.perf_counter()
            prove()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.profile_read()
            for s in dev_ms:
                dev_ms[s].append(st[s][0])
        ctx.profile(False)
        for _ in range(args.runs):
            t0 = time.perf_counter()
            ok = proof.verify(comm, rx, ry, evals, gens, FrTranscript())
            vwall.append((time.perf_counter() - t0) * 1e3)
            assert ok
            thost.append(replay_transcript(sz, FrTranscript, one, comm.comm_mem[0]))
        vcodec = []  # the device row checks, in runs of their own (stage events stay out of the wall time)
        ctx.profile(True)
        for _ in range(args.runs):
            ctx.profile_reset()
            assert proof.verify(comm, rx, ry, evals, gens, FrTranscript())
            vcodec.append(ctx.profile_read()["point_codec"])
        ctx.profile(False)
        # the verifier's row-commitment validation alone, as the host does it below the device
        # threshold, over as many points as comm_derefs, comm_ops and comm_mem hold, once
        # (the verifier checks every row twice: in its own element checks and in each opening's)
        n_rows = len(proof.comm_derefs) + len(comm.comm_ops) + len(comm.comm_mem)
        rows_host = []
        for _ in range(args.runs + 1):
            ms = C.c_double(0)
            assert ctx.lib.tpst_microbench(ctx.h, 20, n_rows, 1, C.byref(ms)) == 0
            rows_host.append(ms.value)
        rows_host = rows_host[1:]

        # ---- the parts the parent could already time, on same-shaped inputs
        def dev_fr(count, seed):
            v, _ = fr_stream(seed, count)
            return torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).to(dev)

        parts = []
        hy = []
        for j, ell in enumerate((sz.ell_derefs, sz.ell_ops, sz.ell_mem)):
            hg = HyraxGens.setup(ctx, ell, label)
            hy.append((hg, ell, dev_fr(1 << ell, 0x60 + j), fr_stream(0x70 + j, ell)[0], rnd[j]))
        pc = [(sz.log_ops, 12, 6, dev_fr(12 * N, 0x80), [dev_fr(6 * (N // 2), 0x81 + j) for j in range(3)]),
              (sz.log_cells, 4, 0, dev_fr(4 * cells, 0x90), [])]
        ctx.torch_to_lib()

        def run_parts():
            for hg, ell, d_Z, r, rn in hy:
                eval_prove(hg, d_Z.data_ptr(), r, one, rn, FrTranscript(), ell=ell)
            for ell, P, D, d_p, d_d in pc:
                PT.prove_dev(ctx, ell, P, d_p.data_ptr(), D, *([t.data_ptr() for t in d_d] if D else [0, 0, 0]),
                             FrTranscript())

        run_parts()  # warm-up
        for _ in range(args.runs):
            t0 = time.perf_counter()
            run_parts()
            parts.append((time.perf_counter() - t0) * 1e3)
        for hg, *_rest in hy:
            hg.close()

        nbytes = {"sparse_deref": 6 * N * (4 + 32 + 32), "sparse_hash_ops": 6 * N * (4 + 4 + 32) + 12 * N * 32,
                  "sparse_hash_mem": 2 * cells * (32 + 4) + 4 * cells * 32,
                  "sparse_seg_eval": (21 + 1) * N * 32 + (2 + 1) * cells * 32}
        res = {"log_cons": lg, "num_ops": N, "num_mem_cells": cells, "runs": args.runs,
               "prove_wall_ms": round(med(wall), 3), "verify_wall_ms": round(med(vwall), 3),
               "host_transcript_ms": round(med(thost), 3), "parts_wall_ms": round(med(parts), 3),
               "assembly_ms": round(med(wall) - med(parts), 3),
               "proof_bytes": len(W.ser_r1cs_eval_proof(proof, sz)),
               "commitment_bytes": len(W.ser_r1cs_commitment(comm, n, n, 10)),
               "verify_rows": n_rows, "verify_rows_host16_once_ms": round(med(rows_host), 3),
               "verify_point_codec_dev_ms": round(med([v[0] for v in vcodec]), 3),
               "verify_point_codec_launches": int(med([v[1] for v in vcodec]))}
        for s, ms in dev_ms.items():
            gbs = nbytes[s] / (med(ms) * 1e-3) / 1e9 if med(ms) > 0 else 0.0
            res[s] = {"dev_ms": round(med(ms), 4), "bytes": nbytes[s], "gbs": round(gbs, 1),
                      "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        decomm.close()
        gens.close()
        del inst, hy, pc
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
