"""The placement of the whole-document rows (csrc/tk_rowfit.hip) step for step in Python: next-fit looks sequential,
the kernels do it with a prefix sum, one search per document and pointer doubling.  tests/test_rowfit_cpu.py checks this model
against the plain loop of the definition; the kernels themselves are checked on the GPU (tests/test_gpu_rowfit.py)."""
import bisect

UNMARKED = -1


def rounds_for(n_ids, n_docs, L):
    """The rounds the host launches: two neighbouring rows hold more than L ids together, so n_rows <= 2 * (N // (L + 1)) + 1
    (and <= D); after round k the first 2^(k+1) positions of the chain are marked."""
    r_max = min(2 * (n_ids // (L + 1)) + 1, n_docs)
    rounds = 0
    while (1 << rounds) <= r_max:
        rounds += 1
    return rounds


def nxt_table(E, L):
    """tk_rowfit_nxt_kernel: nxt(v) = the largest j with E[j] <= E[v] + L, by a galloping search forward from v + 1 and a
    binary one; the sentinel D jumps to itself in 0 steps.  -> [(target, steps)]."""
    D = len(E) - 1
    jump = []
    for v in range(D):
        key = E[v] + L
        lo, w = v + 1, 1
        assert E[lo] <= key
        while lo + w <= D and E[lo + w] <= key:
            lo, w = lo + w, w << 1
        hi = lo + w if lo + w <= D else D + 1
        jump.append((lo + bisect.bisect_right(E, key, lo, hi) - lo - 1, 1))
    jump.append((D, 0))
    return jump


def place(lengths, L, order=None):
    """doc_start and n_rows of next-fit as the kernels compute them.  order(k, D + 1): the order in which the nodes of round k run
    (any order gives the same marks: a mark is the node's position in the chain)."""
    D = len(lengths)
    e = [min(n, L) for n in lengths]
    E = [0]
    for x in e:
        E.append(E[-1] + x)
    if E[D] == 0:
        return [0] * D, 0, 0
    jump = nxt_table(E, L)
    for v in range(D):
        assert jump[v][0] > v
    row = [UNMARKED] * (D + 1)
    row[0] = 0
    rounds = rounds_for(sum(lengths), D, L)
    for k in range(rounds):                               # tk_rowfit_round_kernel
        out = [None] * (D + 1)
        for v in (order(k, D + 1) if order else range(D + 1)):
            t, steps = jump[v]
            if row[v] != UNMARKED and steps:
                assert row[t] in (UNMARKED, row[v] + steps)
                row[t] = row[v] + steps
            out[v] = (jump[t][0], steps + jump[t][1])
        jump = out
    n_rows = row[D]
    assert n_rows != UNMARKED
    opener = [None] * (n_rows + 1)                        # tk_rowfit_open_kernel
    for v in range(D + 1):
        if row[v] != UNMARKED:
            opener[row[v]] = v
    assert opener[0] == 0 and opener[n_rows] == D and all(a < b for a, b in zip(opener, opener[1:]))
    doc_start = []                                        # tk_rowfit_place_kernel: the last marked v <= d, wave by wave
    for base in range(0, D, 64):
        c = bisect.bisect_right(opener, base, 0, n_rows)
        pm = 0
        for lane in range(min(64, D - base)):
            d = base + lane
            if row[d] != UNMARKED:
                pm = lane + 1
            v, rv = (base + pm - 1, row[base + pm - 1]) if pm else (opener[c - 1], c - 1)
            doc_start.append(rv * L + E[d] - E[v])
    return doc_start, n_rows, rounds
