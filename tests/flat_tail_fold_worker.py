"""tests/test_gpu_flat_tail_fold.py: the folded bookkeeping tail of the flat path (tk_fold_apply_kernel,
tk_flat_counts_sums_kernel, tk_flat_assemble_fold_kernel of csrc/tk_flat.hip through their launch functions) on the GPU, on the
layouts of tests/flat_tail_cases.py and the edges of tests/flat_tail_fold_cases.py, through the development build's
tk_test_flat_tail_fold (csrc/tk_test_hooks.h; `make ablate`).  The library is named by TK_HIP_LIB; a process of its own, so that a
fault ends here and not in the test session.  It stops at the first case that fails: nothing more is started on the GPU after that.

  python tests/flat_tail_fold_worker.py <out_path>        -> "ok <runs>" or what went wrong"""
import ctypes
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flat_tail_cases as ftc  # noqa: E402
import flat_tail_fold_cases as ffc  # noqa: E402

N_RANDOM = 100                 # of flat_tail_cases.random_layout (the emulator runs all of them)


def plan():
    """(name, layout, modes, configurations)"""
    for name, layout in list(ftc.directed_cases()) + list(ffc.edge_cases()):
        yield name, layout, None, ffc.CONFIGS[:2]
    for s in range(N_RANDOM):
        yield "random_%d" % s, ftc.random_layout(s), "random", ffc.CONFIGS[:1]


N_BIG = 2                      # flat_tail_fold_cases.big_cases(): the final pass, folded


def n_runs():
    return sum(3 * len(cfg) if modes is None else 2 * len(cfg) for _, _, modes, cfg in plan()) + N_BIG


def main():
    out_path = sys.argv[1]
    verdict, n, where = None, 0, "loading the library"
    try:
        lib = ctypes.CDLL(os.environ["TK_HIP_LIB"])
        lib.tk_test_flat_tail_fold.restype = ctypes.c_int
        lib.tk_test_flat_tail_fold.argtypes = [ctypes.c_int, ctypes.POINTER(ftc.TkTestTailCase), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.POINTER(ctypes.c_uint64)]
        cur = {}

        def call3(t, fold, mm, dm):
            """the hook, and the prefix sums of the sub-queue counts read back: what the merge kernels would search"""
            mc = cur["a"]["miss_count"]
            got = np.full(mc.size + 1, 0x5E5E5E5E5E5E5E5E, np.uint64)
            rc = lib.tk_test_flat_tail_fold(0, t, fold, mm, dm, got.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
            if rc == 0 and cur["a"]["n_chunks"]:
                want = np.zeros(mc.size + 1, np.uint64)
                want[1:] = np.cumsum(mc, dtype=np.uint64)
                assert np.array_equal(got, want), "fold=%d: miss_prefix[%d] differs" % (fold, int(np.flatnonzero(got != want)[0]))
            return rc
        for name, layout, modes, configs in plan():
            a = cur["a"] = layout.arrays()
            ms = ftc.modes(a) if modes is None else [(0, 0 if a["flags"].any() or int(name[7:]) % 4 else 2), (1, 0)]
            for final_pass, long_recs in ms:
                where = "%s, final_pass=%d, long-piece records=%d" % (name, final_pass, long_recs)
                ffc.check(call3, a, final_pass, long_recs, configs=configs)
                n += len(configs)
        for name, a, x in ffc.big_cases():
            where, cur["a"] = "%s, final pass, folded" % name, a
            ffc.check(call3, a, 1, 0, configs=ffc.CONFIGS[:1], x=x)
            n += 1
        verdict = "ok %d" % n
    except BaseException as e:  # noqa: BLE001
        verdict = "FAILED at %s:\n%s" % (where, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-2500:])
    with open(out_path, "w") as f:
        f.write(verdict)
    return 0 if verdict.startswith("ok") else 1


if __name__ == "__main__":
    sys.exit(main())
