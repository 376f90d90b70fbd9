"""The single merge launch of the folded tail (csrc/tk_flat.hip: tk_merge_all_kernel) against the two merge kernels of the
three-kernel form (TK_TAIL_FOLD=0), id for id: on tests/golden/merge_vectors.json and merge_vectors_hf.json (whose expected ids both
forms must give) and on small batches with pieces of every class, with the memo of merged pieces forced on and off.  In a worker
process (tests/merge_one_worker.py): the knobs are read from the environment."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_one_merge_launch_gives_the_ids_of_two(tmp_path):
    out = str(tmp_path / "merge_one.txt")
    env = dict(os.environ, TK_NO_SMALL_PATH="1")
    for k in ("TK_HIP_LIB", "TK_PIPELINE", "TK_TAIL"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "merge_one_worker.py"), out], env=env, capture_output=True, text=True, timeout=120)
    verdict = open(out).read() if os.path.exists(out) else "(the worker left no verdict)"
    assert r.returncode == 0 and verdict.startswith("ok "), verdict + "\n" + (r.stdout + r.stderr)[-2000:]
    assert int(verdict.split()[1]) >= 2 * 4 * 6 + 3 * 2 * 4
