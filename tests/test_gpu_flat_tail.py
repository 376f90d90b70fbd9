"""The bookkeeping tail of the flat path on the GPU: tk_flat_firstdoc_kernel, tk_merge_wavefirst_kernel, tk_flat_todo_kernel,
tk_flat_counts_kernel, tk_flat_assemble_kernel and the exclusive scans between them, launched by the product's launch functions on
the made-up layouts of tests/flat_tail_cases.py (the same ones tests/test_flat_tail_emu.py runs on the CPU wave emulator), every
array between guard bands; and the three-kernel scan alone at its tile edges.  Through the test hooks of the development build
(csrc/tk_test_hooks.h), in a worker process (tests/flat_tail_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)


def test_flat_tail_and_scan_on_the_gpu(tmp_path):
    """every layout gives exactly the arrays the restatement expects, optimistic and final pass; nothing is written outside
    [0, total) of out_ids, nothing at all when the pass has to skip the copy; every guard word is intact; the scan is exact
    against numpy.cumsum in uint64 for n around 1, 64, 2048 (a block) and 524 288 (256 block sums), totals beyond 2^32"""
    import flat_tail_cases as ftc
    from flat_tail_worker import SCAN_N
    # (every time: a development library from before the hooks would not have them; a no-op when it is up to date)
    subprocess.check_call(["make", "-s", "-j16", "-C", os.path.join(ROOT, "tekken-rs_amd"), "ablate"])
    lib = os.path.join(ROOT, "tekken-rs_amd", "libtekken_hip_ablate.so")
    out = str(tmp_path / "flat_tail.txt")
    r = subprocess.run([sys.executable, os.path.join(HERE, "flat_tail_worker.py"), out], env=dict(os.environ, TK_HIP_LIB=lib),
                       capture_output=True, text=True, timeout=120)
    verdict = open(out).read() if os.path.exists(out) else "(the worker left no verdict)"
    assert r.returncode == 0 and verdict.startswith("ok "), verdict + "\n" + (r.stdout + r.stderr)[-2000:]
    n_tail, n_scan = (int(v) for v in verdict.split()[1:])
    assert n_scan == 3 * len(SCAN_N)
    assert n_tail == 3 * len(list(ftc.directed_cases())) + 2 * ftc.N_RANDOM
