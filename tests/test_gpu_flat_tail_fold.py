"""The folded bookkeeping tail of the flat path on the GPU: tk_scan_block_sums -> tk_fold_apply_kernel (prefix sums, wave_first,
wave_first_wide, TKC_NARROW_LEFT in one pass) and tk_flat_counts_sums_kernel -> tk_flat_assemble_fold_kernel (output offsets made
by the assembly), launched by the product's launch functions on the made-up layouts of tests/flat_tail_cases.py and the edges of
tests/flat_tail_fold_cases.py (the same ones tests/test_flat_tail_fold_emu.py runs on the CPU wave emulator), every array between
guard bands.  Through the test hook of the development build (csrc/tk_test_hooks.h: tk_test_flat_tail_fold), in a worker process
(tests/flat_tail_fold_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)


def test_folded_flat_tail_on_the_gpu(tmp_path):
    """every layout gives exactly the arrays the restatement expects (what the pinned kernels are held to as well), optimistic and
    final pass, folded wherever it can run and with the bounds forced to 1 (the three-kernel scans above one partial sum): n_docs
    around 64, 4096 and 8192, 5 n_chunks around 2048 and 4096, sub-queues empty / narrow / wide / both / 33..64 bytes only, totals
    beyond 2^32, and two large layouts with more than 64 partial sums on either side (26 300 chunks; 266 300 documents), where the
    folds' strided loads run a second round; after every run the prefix sums of the sub-queue counts are read back and compared with
    numpy.cumsum; nothing is written outside [0, total) of out_ids, nothing at all when the pass has to skip the copy; every guard
    word is intact"""
    import flat_tail_fold_worker as w
    # (every time: a development library from before the hook would not have it; a no-op when it is up to date)
    subprocess.check_call(["make", "-s", "-j16", "-C", os.path.join(ROOT, "tekken-rs_amd"), "ablate"])
    lib = os.path.join(ROOT, "tekken-rs_amd", "libtekken_hip_ablate.so")
    out = str(tmp_path / "flat_tail_fold.txt")
    r = subprocess.run([sys.executable, os.path.join(HERE, "flat_tail_fold_worker.py"), out], env=dict(os.environ, TK_HIP_LIB=lib),
                       capture_output=True, text=True, timeout=120)
    verdict = open(out).read() if os.path.exists(out) else "(the worker left no verdict)"
    assert r.returncode == 0 and verdict.startswith("ok "), verdict + "\n" + (r.stdout + r.stderr)[-2000:]
    assert int(verdict.split()[1]) == w.n_runs()
