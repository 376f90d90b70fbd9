"""The 64-ary wave search of the packed-rows and join kernels (tky_wave_count_le, csrc/tk_layout.h) step for step in
Python: the one piece of those kernels whose invariant and termination are not plain to see.  tests/test_seqpack_cpu.py checks it
against bisect; everything else of the kernels is checked on the GPU (tests/test_gpu_seqpack.py)."""

def wave_count_le(a, n, key):
    """tky_wave_count_le: entries of the non-decreasing a[0 .. n) at or before key, 64 probes a step."""
    lo, hi = 0, n
    while hi > lo:
        step = (hi - lo + 63) // 64
        probes = [min(lo + (lane + 1) * step - 1, hi - 1) for lane in range(64)]
        ballot = [a[p] <= key for p in probes]
        c = sum(ballot)
        assert ballot == [i < c for i in range(64)]           # a prefix of the lanes
        if c == 64:
            return hi
        lo, hi = lo + c * step, min(lo + (c + 1) * step - 1, hi - 1)
    return lo
