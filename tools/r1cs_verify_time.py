"""Time tpst_r1cs_evaluate and tpst_r1cs_verify on one GPU.

    python tools/r1cs_verify_time.py [--log-cons 18 --log-vars 16 --inputs 17] [--runs 7] [--python-sum]

evaluate: the median wall time of the call and the median device time of its
two stages (HIP events of tpst_profile_*: the eq tables; the reduction kernel
and its partial sum) after one warm-up; verify: the median wall time of
R1CSProof.verify with a fresh transcript.  --python-sum also times the
interpreter's sum of eq(rx)[row] eq(ry)[col] val over every entry (the ABC
check of tests/test_r1cs.py::test_r1cs_prove_2p18_verifier_checks) and checks
the device values against it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle", "py")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-cons", type=int, default=18)
    ap.add_argument("--log-vars", type=int, default=16)
    ap.add_argument("--inputs", type=int, default=17)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--python-sum", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from testudo_amd import Context
    from testudo_amd import r1cs as D
    from testudo_amd import sqrt_pst as S
    from testudo_amd.encoding import limbs_to_int

    ctx = Context(0)
    num_cons, num_vars = 1 << args.log_cons, 1 << args.log_vars
    S.srs_setup(ctx, (args.log_vars + 1) // 2, 0x7E57D1)
    inst, vars_, inputs = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, args.inputs, 99)
    proof, rx, ry = D.R1CSProof.prove(inst, vars_, inputs, S.PoseidonTranscript())

    evals = inst.evaluate(rx, ry)  # warm-up
    wall, dev_eq, dev_red = [], [], []
    ctx.profile(True)
    for _ in range(args.runs):
        ctx.profile_reset()
        t0 = time.perf_counter()
        inst.evaluate(rx, ry)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.profile_read()
        dev_eq.append(st["r1cs_eval_eq"][0])
        dev_red.append(st["r1cs_eval"][0])
    ctx.profile(False)

    assert proof.verify(inst, inputs, S.PoseidonTranscript())  # warm-up
    vwall, vewall = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ok = proof.verify(inst, inputs, S.PoseidonTranscript())
        vwall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ok = proof.verify(inst, inputs, S.PoseidonTranscript(), evals=evals) and ok
        vewall.append((time.perf_counter() - t0) * 1e3)
        assert ok

    nnz = 3 * num_cons  # the synthetic instance: one entry per row and matrix
    # algorithmic bytes of the reduction: value + column index per entry, one
    # eq(ry) gather per entry, the row pointers and one eq(rx) read per row
    red_bytes = nnz * (32 + 4) + nnz * 32 + 3 * num_cons * (4 + 32)
    med = statistics.median
    res = {"num_cons": num_cons, "num_vars": num_vars, "num_inputs": args.inputs, "runs": args.runs,
           "evaluate_wall_ms": round(med(wall), 4), "evaluate_eq_tables_dev_ms": round(med(dev_eq), 4),
           "evaluate_reduce_dev_ms": round(med(dev_red), 4), "reduce_bytes": red_bytes,
           "reduce_gbs": round(red_bytes / (med(dev_red) * 1e-3) / 1e9, 1),
           "reduce_fraction_of_hbm_peak": round(red_bytes / (med(dev_red) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "verify_wall_ms": round(med(vwall), 3), "verify_evals_wall_ms": round(med(vewall), 3)}
    if args.python_sum:
        import bls377 as O
        import r1cs as Q
        mats, _, _ = Q.synthetic_r1cs(num_cons, num_vars, args.inputs, 99)
        irx = [limbs_to_int(x) for x in rx]
        iry = [limbs_to_int(x) for x in ry]
        t0 = time.perf_counter()
        ex, ey = Q.eq_evals(irx), Q.eq_evals(iry)
        want = [sum(ex[r] * ey[c] * val for r, c, val in M) % O.R for M in mats]
        res["python_sum_s"] = round(time.perf_counter() - t0, 3)
        assert want == [limbs_to_int(x) for x in evals], "device evaluate differs from the Python sum"
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    del inst
    ctx.close()


if __name__ == "__main__":
    main()
