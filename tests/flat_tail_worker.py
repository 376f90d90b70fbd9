"""tests/test_gpu_flat_tail.py: the bookkeeping tail of the flat path (csrc/tk_flat_tail_impl.h through the kernels and launch
functions of csrc/tk_flat.hip) and the three-kernel exclusive scan (csrc/tk_kernels.hip) on the GPU, on the layouts of
tests/flat_tail_cases.py, through the test hooks of the development build (csrc/tk_test_hooks.h; `make ablate`).  The library is
named by TK_HIP_LIB; a process of its own, so that a fault ends here and not in the test session.  It stops at the first case that
fails: nothing more is started on the GPU after that.

  python tests/flat_tail_worker.py <out_path>        -> "ok <tail runs> <scan runs>" or what went wrong"""
import ctypes
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flat_tail_cases as ftc  # noqa: E402

SCAN_N = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 524287, 524288, 524289, 1048577)   # 2048 counts a block, 256 block sums a round of the top scan
SENT64 = 0x5E5E5E5E5E5E5E5E


def scan_cases():
    rng = np.random.RandomState(77)
    for n in SCAN_N:
        yield "zeros", np.zeros(n, np.uint32)
        yield "all 0xFFFFFFFF", np.full(n, 0xFFFFFFFF, np.uint32)
        yield "random", rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def main():
    out_path = sys.argv[1]
    verdict, n_tail, n_scan, where = None, 0, 0, "loading the library"
    try:
        lib = ctypes.CDLL(os.environ["TK_HIP_LIB"])
        lib.tk_test_flat_tail.restype = ctypes.c_int
        lib.tk_test_flat_tail.argtypes = [ctypes.c_int, ctypes.POINTER(ftc.TkTestTailCase)]
        lib.tk_test_scan.restype = ctypes.c_int
        lib.tk_test_scan.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]

        def call(t):
            return lib.tk_test_flat_tail(0, t)
        for n, counts in scan_cases():
            where = "scan of %d counts, %s" % (counts.size, n)
            offs = np.full(counts.size + 2, SENT64, np.uint64)
            rc = lib.tk_test_scan(0, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), counts.size, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
            assert rc == 0, "rc=%d (a failed call, or a guard word changed)" % rc
            want = np.zeros(counts.size + 1, np.uint64)
            want[1:] = np.cumsum(counts, dtype=np.uint64)
            assert np.array_equal(offs[:-1], want), "offs[%d] differs" % int(np.flatnonzero(offs[:-1] != want)[0])
            assert int(offs[-2]) == int(counts.astype(np.uint64).sum()) and int(offs[-1]) == SENT64, "the total / the word behind it"
            n_scan += 1
        layouts = list(ftc.directed_cases()) + [("random_%d" % s, ftc.random_layout(s)) for s in range(ftc.N_RANDOM)]
        for name, layout in layouts:
            a = layout.arrays()
            ms = ftc.modes(a) if not name.startswith("random_") else [(0, 0 if a["flags"].any() or int(name[7:]) % 4 else 2), (1, 0)]
            for final_pass, long_recs in ms:
                where = "%s, final_pass=%d, long-piece records=%d" % (name, final_pass, long_recs)
                ftc.run_and_check(call, a, final_pass, long_recs)
                n_tail += 1
        verdict = "ok %d %d" % (n_tail, n_scan)
    except BaseException as e:  # noqa: BLE001
        verdict = "FAILED at %s:\n%s" % (where, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-2500:])
    with open(out_path, "w") as f:
        f.write(verdict)
    return 0 if verdict.startswith("ok") else 1


if __name__ == "__main__":
    sys.exit(main())
