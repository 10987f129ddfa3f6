"""Time the batched point codec (csrc/point_codec.hip) against the host paths it
replaces, on one GPU.

    python tools/point_codec_time.py [--max-log 14] [--runs 7] [--out profiles/point_codec/point_codec_time.json]

Per n = 2^0 .. 2^max-log valid points, after one warm-up of every call, medians
over --runs of the host clock around (every call ends synchronised):
  de_g1_batch_ms / check_g1_batch_ms   tpst_de_g1_batch / tpst_g1_check_batch (upload, kernel,
  de_g2_batch_ms / check_g2_batch_ms   download), and the same for G2
  *_kernel_ms          the kernel alone (HIP events of the point_codec stage)
  de_g1_loop_ms        n calls of tpst_de_g1 on one host thread (what a reader did per point);
                       fewer runs at large n (loop_runs), it is seconds long there
  host_check16_ms      the verifiers' own host loop (host::parallel_for over point_valid, up to 16
                       threads) over n points, timed inside the library: tpst_microbench kind 20
Prints one JSON line per n; the last line names the threshold the medians give:
the smallest power of two from which check_g1_batch_ms < host_check16_ms at
every larger n measured (POINT_CHECK_DEVICE_MIN of csrc/point_codec.h).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-log", type=int, default=14)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np

    from testudo_amd import Context
    from testudo_amd.sqrt_pst import fr_stream

    ctx = Context(0)
    lib = ctx.lib
    med = statistics.median
    u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    n_max = 1 << args.max_log
    scalars, _ = fr_stream(0xC0DEC, n_max)
    g1 = np.ascontiguousarray(ctx.g1_mul_generator(scalars))
    g2 = np.ascontiguousarray(ctx.g2_mul_generator(scalars))
    b1, b2 = C.create_string_buffer(48 * n_max), C.create_string_buffer(96 * n_max)
    for i in range(n_max):
        assert lib.tpst_ser_g1(u64p(g1[i]), C.cast(C.byref(b1, 48 * i), C.c_char_p)) == 0
        assert lib.tpst_ser_g2(u64p(g2[i]), C.cast(C.byref(b2, 96 * i), C.c_char_p)) == 0
    b1, b2 = b1.raw, b2.raw
    out1, out2 = np.zeros_like(g1), np.zeros_like(g2)

    def timed(fn, runs):
        fn()  # warm-up
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return med(ts)

    def kernel_ms(fn, runs):
        ctx.profile(True)
        ms = []
        for _ in range(runs):
            ctx.profile_reset()
            fn()
            ms.append(ctx.profile_read()["point_codec"][0])
        ctx.profile(False)
        return med(ms)

    lines, rows = [], []
    for lg in range(args.max_log + 1):
        n = 1 << lg
        bad = C.c_size_t(0)

        def de1():
            assert lib.tpst_de_g1_batch(ctx.h, b1, n, u64p(out1), C.byref(bad)) == 0

        def de2():
            assert lib.tpst_de_g2_batch(ctx.h, b2, n, u64p(out2), C.byref(bad)) == 0

        def ck1():
            assert lib.tpst_g1_check_batch(ctx.h, u64p(g1), n, C.byref(bad)) == 0

        def ck2():
            assert lib.tpst_g2_check_batch(ctx.h, u64p(g2), n, C.byref(bad)) == 0

        one = np.zeros(12, dtype=np.uint64)

        def loop():
            for i in range(n):
                assert lib.tpst_de_g1(b1[48 * i:48 * i + 48], u64p(one)) == 0

        def host16():
            ms = C.c_double(0)
            assert lib.tpst_microbench(ctx.h, 20, n, 1, C.byref(ms)) == 0
            return ms.value

        loop_runs = args.runs if n <= 256 else 3 if n <= 2048 else 1
        res = {"n": n, "runs": args.runs, "loop_runs": loop_runs}
        for name, fn in (("de_g1_batch", de1), ("check_g1_batch", ck1), ("de_g2_batch", de2), ("check_g2_batch", ck2)):
            res[name + "_ms"] = round(timed(fn, args.runs), 4)
            res[name + "_kernel_ms"] = round(kernel_ms(fn, args.runs), 4)
        assert np.array_equal(out1[:n], g1[:n]) and np.array_equal(out2[:n], g2[:n])
        res["de_g1_loop_ms"] = round(timed(loop, loop_runs), 4)
        host16()  # warm-up
        res["host_check16_ms"] = round(med([host16() for _ in range(args.runs)]), 4)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        rows.append(res)
    wins = [r["check_g1_batch_ms"] < r["host_check16_ms"] for r in rows]
    k = len(rows)
    while k > 0 and wins[k - 1]:
        k -= 1
    line = json.dumps({"threshold": rows[k]["n"] if k < len(rows) else None,
                       "rule": "smallest n from which check_g1_batch_ms < host_check16_ms at every larger n measured"})
    print(line, flush=True)
    lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
