"""A model of the regroup pass as the kernels run it (tekken-rs_amd/csrc/tk_regroup.hip), in plain Python: the stable
least-significant-digit radix sort block by block (digit-major counts, their exclusive scan, the in-order scatter with the rank
among the equal digits of a wave), the key sequences of the four orders with the passes the host launches, and the search of
nxt(i) through the maximum pyramid.  tests/test_regroup_cpu.py holds it against Python's `sorted` and the plain loop of the
definition; the kernels are held against that restatement on the GPU."""

CHUNK, BLOCK, WAVE, FAN = 2048, 256, 64, 64
KEEP, LENGTH, SHUFFLE, GROUPED = 0, 1, 2, 3
M32 = 0xFFFFFFFF


def h(seed, d):
    """Step 2 of the definition: a bijection of the 32-bit d."""
    x = (d * 0x9E3779B1 + seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def radix_passes(largest):
    """8-bit passes the host launches for keys up to `largest`: none above its highest set bit."""
    n = 0
    while largest:
        n, largest = n + 1, largest >> 8
    return n


def radix_pass(keys, vals, shift, chunk=CHUNK, block=BLOCK):
    """One pass: tk_regroup_hist_kernel, tk_launch_scan, tk_regroup_scatter_kernel."""
    n = len(keys)
    blocks = (n + chunk - 1) // chunk
    hist = [0] * (256 * blocks)
    for b in range(blocks):
        for i in range(b * chunk, min(n, (b + 1) * chunk)):
            hist[((keys[i] >> shift) & 255) * blocks + b] += 1     # digit-major
    hpos, run = [], 0
    for c in hist:
        hpos.append(run)
        run += c
    out_k, out_v = [None] * n, [None] * n
    for b in range(blocks):
        base = [hpos[dg * blocks + b] for dg in range(256)]
        c1 = min(n, (b + 1) * chunk)
        for r0 in range(b * chunk, c1, block):                     # a round: `block` pairs in element order
            per_wave = [[0] * 256 for _ in range(block // WAVE)]
            rank = {}
            for t in range(min(block, c1 - r0)):
                dg, w = (keys[r0 + t] >> shift) & 255, t // WAVE
                rank[t] = per_wave[w][dg]                          # the lanes in front of it in its wave with the same digit
                per_wave[w][dg] += 1
            for t in rank:
                dg, w = (keys[r0 + t] >> shift) & 255, t // WAVE
                pos = base[dg] + sum(per_wave[x][dg] for x in range(w)) + rank[t]
                assert out_k[pos] is None
                out_k[pos], out_v[pos] = keys[r0 + t], vals[r0 + t]
            for dg in range(256):
                base[dg] += sum(pw[dg] for pw in per_wave)
    return out_k, out_v


def radix_sort(keys, vals, passes, chunk=CHUNK, block=BLOCK):
    for p in range(passes):
        keys, vals = radix_pass(keys, vals, 8 * p, chunk, block)
    return keys, vals


def permutation(lengths, kept, order, seed=0, window=0, desc=False, chunk=CHUNK, block=BLOCK):
    """perm of the kept documents (increasing indices into lengths), by the key sequences and passes of run_regroup.
    -> (perm, radix passes run)"""
    K = len(kept)
    if order == KEEP or K <= 1:
        return list(kept), 0
    longest = max(lengths[d] for d in kept)
    lkey = (lambda d: longest - lengths[d]) if desc else (lambda d: lengths[d])
    if order == LENGTH:
        n = radix_passes(longest)
        return radix_sort([lkey(d) for d in kept], list(kept), n, chunk, block)[1], n
    n = 4
    shuf = radix_sort([h(seed, d) for d in kept], list(kept), 4, chunk, block)[1]
    if order == SHUFFLE:
        return shuf, n
    p1 = radix_passes(longest)                                    # (length key, shuffle rank): the less significant part first
    keys, ranks = radix_sort([lkey(d) for d in shuf], list(range(K)), p1, chunk, block)
    p2 = radix_passes((K - 1) // window)
    keys, ranks = radix_sort([r // window for r in ranks], ranks, p2, chunk, block)
    return [shuf[r] for r in ranks], n + p1 + p2


def pyramid(m):
    """levels[l][j] = max of m over [j * 64^l, (j + 1) * 64^l); levels[0] = m; the top level has one entry (none above m for K <= 1)."""
    levels = [list(m)]
    while len(levels) - 1 < 6 and 64 ** (len(levels) - 1) < len(m):
        lo = levels[-1]
        levels.append([max(lo[i:i + FAN]) for i in range(0, len(lo), FAN)])
    return levels


def nxt(levels, v, T, max_docs):
    """tk_regroup_nxt_kernel for document v -> (nxt(v), the longest document of v .. nxt(v) - 1, entries of the pyramid read)"""
    m, K = levels[0], len(levels[0])
    mx, p, lvl, top, steps = m[v], v + 1, 0, len(levels) - 1, 0
    while p < K:
        while lvl < top and p % 64 ** (lvl + 1) == 0:
            lvl += 1
        end = min(K, p + 64 ** lvl)
        m2, cnt = max(mx, levels[lvl][p >> (6 * lvl)]), end - v
        steps += 1
        if not (cnt * m2 > T or (max_docs and cnt > max_docs)):
            mx, p = m2, end
            continue
        if lvl == 0:
            break
        lvl -= 1
        top = lvl
    return p, mx, steps


def batches(m, T, max_docs=0):
    """batch_offsets, batch_rowlen by the chain 0, nxt(0), nxt(nxt(0)), ... -> (bo, rowlen, the most pyramid entries one document read)"""
    if not m:
        return [0], [], 0
    levels = pyramid(m)
    found = [nxt(levels, v, T, max_docs) for v in range(len(m))]
    bo, rl, v = [0], [], 0
    while v < len(m):
        rl.append(found[v][1])
        v = found[v][0]
        bo.append(v)
    return bo, rl, max(f[2] for f in found)
