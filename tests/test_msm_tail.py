"""The G1 MSM's tail forms (INTEGRATION.md "Tunables", TPST_MSM_TAIL) and the
count-ordered fixup, at 2^17 + 37 points -- the smallest size on the
window-grouped path.  The switch is read once per process, so every setting
runs in a child process (the pattern of test_switches.py).

* TPST_MSM_TAIL=throughput and =latency against the CPU oracle on four inputs:
  uniform scalars; the skewed scalars of test_switches.py; scalars in
  {0, 1, 2}, which put almost every entry of a window into two buckets (the
  long list, filled by the order kernel); all-equal bases and scalars.  The
  inputs and the oracle's answers are made once (a child with the default
  setting writes them) and shared.
* auto: six back-to-back pipelined calls (two of them n = 0 and n = 64) with
  differing scalars and outputs equal the stream-ordered call's outputs, and
  TPST_MSM_TAIL_TRACE shows every stream-ordered call and the first pipelined
  call after a synchronize on the latency forms.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_HEAD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/oracle/cpu")
import orc
from testudo_amd import Context
ctx = Context(0)
n = (1 << 17) + 37
'''

_PREP = _HEAD + r'''
k, _ = orc.fr_stream(191, n)
bases = ctx.g1_mul_generator(k)
uni, _ = orc.fr_stream(192, n)
skew = uni.copy()
skew[::3] = 0
skew[1::3, 1:] = 0
small = np.zeros_like(uni)
small[:, 0] = np.arange(n, dtype=np.uint64) %% 3
same_b = np.repeat(bases[:1], n, axis=0)
same_s = np.repeat(uni[:1], n, axis=0)
cases = {"uniform": (bases, uni), "skewed": (bases, skew), "small": (bases, small), "same": (same_b, same_s)}
out = {}
for name, (b, s) in cases.items():
    out[name + "_b"], out[name + "_s"] = b, s
    out[name + "_ref"] = orc.g1_msm(b, s, parallel=True)
np.savez(%(path)r, **out)
# the default setting's host entry point keeps the latency forms
ok = {name: bool(np.array_equal(ctx.g1_msm(b, s), out[name + "_ref"])) for name, (b, s) in cases.items()}
print("RESULT " + json.dumps(ok))
'''

_FORCED = _HEAD + r'''
d = np.load(%(path)r)
ok = {}
for name in ("uniform", "skewed", "small", "same"):
    ok[name] = bool(np.array_equal(ctx.g1_msm(d[name + "_b"], d[name + "_s"]), d[name + "_ref"]))
print("RESULT " + json.dumps(ok))
'''

_AUTO = _HEAD + r'''
import torch
dev = torch.device("cuda", 0)
sizes = [n, n, 0, n, 64, n]
k, _ = orc.fr_stream(193, n)
d_k = torch.from_numpy(k.view(np.int64)).to(dev)
d_bases = torch.empty(n * 12, dtype=torch.int64, device=dev)
sc = [orc.fr_stream(200 + i, n)[0] for i in range(len(sizes))]
d_sc = [torch.from_numpy(s.view(np.int64)).to(dev) for s in sc]
d_ref = [torch.zeros(12, dtype=torch.int64, device=dev) for _ in sizes]
d_out = [torch.zeros(12, dtype=torch.int64, device=dev) for _ in sizes]
torch.cuda.synchronize()
ctx.g1_mul_generator_dev(d_k.data_ptr(), n, d_bases.data_ptr())
ctx.synchronize()
print("MARK sync", file=sys.stderr, flush=True)
for i, m in enumerate(sizes):  # stream-ordered: one after another on the device
    ctx.g1_msm_dev(d_bases.data_ptr(), d_sc[i].data_ptr(), m, d_ref[i].data_ptr())
ctx.synchronize()
print("MARK async", file=sys.stderr, flush=True)
for i, m in enumerate(sizes):  # pipelined, back to back
    ctx.g1_msm_dev_async(d_bases.data_ptr(), d_sc[i].data_ptr(), m, d_out[i].data_ptr())
ctx.synchronize()
print("MARK end", file=sys.stderr, flush=True)
ref = [x.cpu().numpy().view(np.uint64) for x in d_ref]
out = [x.cpu().numpy().view(np.uint64) for x in d_out]
ok = {"call%%d_n%%d" %% (i, m): bool(np.array_equal(ref[i], out[i])) for i, m in enumerate(sizes)}
ok["distinct"] = len({r.tobytes() for r in ref}) == len(sizes)  # differing scalars or sizes: differing sums
bases = ctx.g1_mul_generator(k[:64])
ok["n64_vs_oracle"] = bool(np.array_equal(out[4], orc.g1_msm(bases, sc[4][:64])))
print("RESULT " + json.dumps(ok))
'''


def _run(script, env_extra, timeout=240):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPST_MSM_TAIL")}
    env.update(env_extra)
    r =subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:]), r.stderr


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """inputs and oracle answers of the four cases (npz), made once"""
    path = str(tmp_path_factory.mktemp("msm_tail") / "vectors.npz")
    ok, _ = _run(_PREP % {"root": ROOT, "path": path}, {})
    assert all(ok.values()), ok
    return path


@pytest.mark.parametrize("mode", ["throughput", "latency"])
def test_forced_tail_forms_vs_oracle(vectors, mode):
    ok, err = _run(_FORCED % {"root": ROOT, "path": vectors}, {"TPST_MSM_TAIL": mode, "TPST_MSM_TAIL_TRACE": "1"})
    assert all(ok.values()), ok
    lines = [x for x in err.splitlines() if x.startswith("msm tail ")]
    assert len(lines) == 4 and all(x.startswith("msm tail " + mode + " ") for x in lines), lines


def test_auto_pipelined_calls_equal_stream_ordered_ones():
    ok, err = _run(_AUTO % {"root": ROOT}, {"TPST_MSM_TAIL_TRACE": "1"})
    assert all(ok.values()), ok
    lines = [x for x in err.splitlines() if x.startswith(("msm tail ", "MARK "))]
    a, b, c = lines.index("MARK sync"), lines.index("MARK async"), lines.index("MARK end")
    sync, pipe = lines[a + 1:b], lines[b + 1:c]
    # four of the six calls are window-grouped (n = 0 and n = 64 are not)
    assert len(sync) == 4 and len(pipe) == 4, lines
    assert all(x.startswith("msm tail latency ") for x in sync), sync  # a synchronised call: latency forms
    assert pipe[0].startswith("msm tail latency "), pipe  # nothing pending before it
