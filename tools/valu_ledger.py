"""The VALU ledger of the G1 MSM: SQ_INSTS_VALU per kernel name per MSM, for
every kernel of the plain bench (2^20 points), from ONE rocprofv3 counter pass
(counters only, in a run of its own, the program after `--`):

    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -o run -- \\
        python bench.py --gpus 1 --steps K --warmup W
    python tools/valu_ledger.py OUT.json DIR MSMS        # MSMS = K + W

The plain bench runs exactly K + W MSMs and, before them, the generation of
the bases (k_mul_gen*, listed as setup: launch count not a multiple of MSMS).
SQ_INSTS_VALU counts wave instructions (x 64 for lane instructions; one
field29.h Montgomery product is 474 of them).  The output gives every
kernel's launches and instructions per MSM and its share, the total, and the
split between the accumulation (k_bucket_acc*) and everything else.
"""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict


def short(name):
    """kernel name without its argument list and the tpst:: prefix"""
    name = re.sub(r"^void\s+", "", name.strip().strip('"'))
    depth, out = 0, []
    for ch in name:  # cut at the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    name = "".join(out).replace("tpst::", "")
    return name.replace("Fp<FqCfg>", "Fq").replace(" [clone .kd]", "").replace(".kd", "")


def main():
    out, d, msms = sys.argv[1], sys.argv[2], int(sys.argv[3])
    per_disp = defaultdict(float)
    kname = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != "SQ_INSTS_VALU":
                continue
            did = (f, int(r.get("Dispatch_Id", r.get("Correlation_Id", 0))))
            per_disp[did] += float(r["Counter_Value"])
            kname[did] = short(r["Kernel_Name"])
    if not per_disp:
        print("no SQ_INSTS_VALU rows under", d)
        return 1
    agg = defaultdict(lambda: [0, 0.0])
    for did, v in per_disp.items():
        a = agg[kname[did]]
        a[0] += 1
        a[1] += v
    kernels, setup = {}, {}
    for k, (n, v) in agg.items():
        if n % msms == 0:
            kernels[k] = {"launches_per_msm": n // msms, "valu_per_msm": v / msms}
        else:
            setup[k] = {"launches": n, "valu": v}
    total = sum(x["valu_per_msm"] for x in kernels.values())
    acc = sum(x["valu_per_msm"] for k, x in kernels.items() if "k_bucket_acc" in k)
    for x in kernels.values():
        x["share"] = x["valu_per_msm"] / total
    res = {"counter": "SQ_INSTS_VALU (wave instructions)", "msms": msms, "valu_per_msm": total,
           "accumulation_valu_per_msm": acc, "outside_accumulation_valu_per_msm": total - acc,
           "outside_accumulation_share": (total - acc) / total,
           "kernels": dict(sorted(kernels.items(), key=lambda kv: -kv[1]["valu_per_msm"])), "setup_kernels": setup}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print("VALU per MSM %.4f G, accumulation %.4f G, outside %.4f G (%.1f %%)"
          % (total / 1e9, acc / 1e9, (total - acc) / 1e9, 100 * (total - acc) / total))
    for k, x in res["kernels"].items():
        print("%-64s x%-3d %10.4f M  %5.2f %%" % (k[:64], x["launches_per_msm"], x["valu_per_msm"] / 1e6, 100 * x["share"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
