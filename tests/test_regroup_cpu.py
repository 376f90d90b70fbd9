"""Documents selected, reordered and cut into batches (include/tekken_hip.h tk_regroup_from_ids_device), the parts that need no
GPU: the plain restatement of the definition that tests/test_gpu_regroup.py checks the kernels against, the hand-made cases of
every rule, the hash, the model of the radix passes and of the batch search (tools/regroup_model.py) against `sorted` and the
plain loop, the header's values, the exported symbols and the shim's declarations, and the binding's description of the struct."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_layout_binding_cpu import header_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_regroup_from_ids_device", "tk_encode_batch_device_regroup", "tk_encode_batch_regroup", "tk_free_regroup",
               "tk_last_regroup_ms"]
KEEP, LENGTH, SHUFFLE, GROUPED = 0, 1, 2, 3
DESC, LABELS, PERM, BATCHES, BATCH_OFFSETS, BATCH_ROWLEN = 1, 2, 4, 8, 16, 32
ALL = LABELS | PERM | BATCHES | BATCH_OFFSETS | BATCH_ROWLEN
NB = LABELS | PERM             # ... without max_tokens
VALUES = {"TK_REGROUP_ORDER_KEEP": 0, "TK_REGROUP_ORDER_LENGTH": 1, "TK_REGROUP_ORDER_SHUFFLE": 2, "TK_REGROUP_ORDER_GROUPED": 3,
          "TK_REGROUP_DESC": 1, "TK_REGROUP_LABELS": 2, "TK_REGROUP_PERM": 4, "TK_REGROUP_BATCHES": 8, "TK_REGROUP_BATCH_OFFSETS": 16,
          "TK_REGROUP_BATCH_ROWLEN": 32}
M32 = 0xFFFFFFFF


def h(seed, d):
    """Step 2 of the definition."""
    x = (d * 0x9E3779B1 + seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def opts(order=KEEP, flags=None, min_length=0, max_length=0, seed=0, window=0, max_tokens=0, max_docs=0):
    """flags None: every optional output that the other options allow."""
    if flags is None:
        flags = ALL if max_tokens else NB
    return dict(order=order, flags=flags, min_length=min_length, max_length=max_length, seed=seed, window=window, max_tokens=max_tokens,
                max_docs=max_docs)


def expected_regroup(ids, oo, lab, keep, o):
    """The definition restated with plain loops and `sorted` on explicit key tuples.  o: the dict of opts().  -> dict(ids uint32,
    offsets uint64, labels int32, perm uint32, batch_offsets uint64, batch_rowlen uint32 (an unselected one: None), n_docs, n_ids,
    n_masked, n_short, n_long, n_batches, n_oversize, n_batch_pad).  Invalid options raise ValueError (the entries:
    TK_ERR_INVALID_ARG)."""
    oo = [int(x) for x in oo]
    D, N = len(oo) - 1, int(oo[-1])
    order, flags, lo, hi, w, T, max_docs = o["order"], o["flags"], o["min_length"], o["max_length"], o["window"], o["max_tokens"], o["max_docs"]
    if order not in (KEEP, LENGTH, SHUFFLE, GROUPED) or flags & ~(DESC | ALL):
        raise ValueError("order / flags")
    if D >= 2 ** 32 or (D == 0 and len(ids) > 0) or len(ids) != N:
        raise ValueError("documents / offsets")
    if (order == GROUPED and w == 0) or (flags & BATCHES and T == 0) or (flags & LABELS and lab is None and N > 0) or lo > hi > 0:
        raise ValueError("window / max_tokens / labels / min_length")
    n = [oo[d + 1] - oo[d] for d in range(D)]
    if any(x < 0 or x >= 2 ** 32 for x in n):
        raise ValueError("a document of 2^32 ids or more")
    kept, n_masked, n_short, n_long = [], 0, 0, 0
    for d in range(D):
        if keep is not None and not keep[d]:
            n_masked += 1
        elif n[d] < lo:
            n_short += 1
        elif hi and n[d] > hi:
            n_long += 1
        else:
            kept.append(d)
    sign = -1 if flags & DESC else 1
    if order == KEEP:
        perm = kept
    elif order == LENGTH:
        perm = sorted(kept, key=lambda d: (sign * n[d], d))
    else:
        perm = sorted(kept, key=lambda d: h(o["seed"], d))
        if order == GROUPED:
            rank = {d: r for r, d in enumerate(perm)}
            perm = sorted(perm, key=lambda d: (rank[d] // w, sign * n[d], rank[d]))
    src = np.asarray(ids, np.int64).tolist()
    lsrc = np.asarray(lab, np.int64).tolist() if lab is not None else None
    out_ids, out_lab, offs = [], [], [0]
    for d in perm:
        out_ids += src[oo[d]:oo[d + 1]]
        if lsrc is not None:
            out_lab += lsrc[oo[d]:oo[d + 1]]
        offs.append(len(out_ids))
    K, m = len(perm), [n[d] for d in perm]
    bo, rowlen, n_oversize, padded = [0], [], 0, 0
    if flags & BATCHES:
        start, mx = 0, 0
        for k in range(K):
            mm, cnt = max(mx, m[k]), k - start + 1
            if cnt > 1 and (cnt * mm > T or (max_docs and cnt > max_docs)):
                bo.append(k)
                start, mm = k, m[k]
            mx = mm
        if K > 0:
            bo.append(K)
        for b in range(len(bo) - 1):
            cnt, rl = bo[b + 1] - bo[b], max(m[bo[b]:bo[b + 1]])
            rowlen.append(rl)
            n_oversize += cnt * rl > T
            padded += cnt * rl
    n_batches = len(bo) - 1
    return {"ids": np.array(out_ids, np.uint32), "offsets": np.array(offs, np.uint64),
            "labels": np.array(out_lab, np.int32) if flags & LABELS else None,
            "perm": np.array(perm, np.uint32) if flags & PERM else None,
            "batch_offsets": np.array(bo, np.uint64) if flags & BATCHES and flags & BATCH_OFFSETS else None,
            "batch_rowlen": np.array(rowlen, np.uint32) if flags & BATCHES and flags & BATCH_ROWLEN else None,
            "n_docs": K, "n_ids": len(out_ids), "n_masked": n_masked, "n_short": n_short, "n_long": n_long, "n_batches": n_batches,
            "n_oversize": n_oversize, "n_batch_pad": padded - len(out_ids) if n_batches else 0}


def ragged(rows):
    oo = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        oo[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], np.uint32)
    return ids, oo


def docs_of_lengths(lengths):
    """Document d is [100 * d + 0, 100 * d + 1, ...]: every id says where it came from."""
    return [[100 * d + j for j in range(n)] for d, n in enumerate(lengths)]


def run(lengths, keep=None, **kw):
    ids, oo = ragged(docs_of_lengths(lengths))
    return expected_regroup(ids, oo, -ids.astype(np.int64) - 1, keep, opts(**kw))


# what the GPU tests run on the device too: (name, lengths, keep, the keywords of opts())
HAND_CASES = [
    ("drop-count precedence", [0, 5, 9, 3, 12, 5], [1, 1, 0, 0, 1, 1], dict(min_length=4, max_length=9)),
    ("stable ascending", [3, 1, 3, 2, 1, 3], None, dict(order=LENGTH)),
    ("stable descending", [3, 1, 3, 2, 1, 3], None, dict(order=LENGTH, flags=NB | DESC)),
    ("last group shorter", [5, 1, 4, 2, 3, 9, 7], None, dict(order=GROUPED, window=3, seed=7)),
    ("fits exactly", [2, 4, 3, 1], None, dict(max_tokens=12)),
    ("exceeds by one", [2, 4, 3, 1], None, dict(max_tokens=11)),
    ("oversize alone", [2, 9, 2, 2], None, dict(max_tokens=6)),
    ("max_docs 1", [2, 4, 3, 1], None, dict(max_tokens=100, max_docs=1)),
    ("nothing kept", [2, 4, 3], [0, 0, 0], dict(max_tokens=10, order=LENGTH)),
]


def test_hand_made_selection_and_drop_count_precedence():
    # d0 empty: short; d2 masked (and long: counted once, as masked); d3 masked (and short); d4 long; d1, d5 kept
    e = run([0, 5, 9, 3, 12, 5], keep=[1, 1, 0, 0, 1, 1], min_length=4, max_length=9)
    assert (e["n_masked"], e["n_short"], e["n_long"], e["n_docs"]) == (2, 1, 1, 2)
    assert e["perm"].tolist() == [1, 5] and e["offsets"].tolist() == [0, 5, 10]
    assert e["ids"].tolist() == [100, 101, 102, 103, 104, 500, 501, 502, 503, 504]
    assert e["labels"].tolist() == [-x - 1 for x in e["ids"].tolist()] and e["labels"].dtype == np.int32
    assert run([4, 9], min_length=4, max_length=9)["n_docs"] == 2      # both bounds are inclusive
    assert run([3, 10], min_length=4, max_length=9)["n_docs"] == 0


def test_hand_made_length_order_is_stable_both_ways():
    assert run([3, 1, 3, 2, 1, 3], order=LENGTH)["perm"].tolist() == [1, 4, 3, 0, 2, 5]
    assert run([3, 1, 3, 2, 1, 3], order=LENGTH, flags=NB | DESC)["perm"].tolist() == [0, 2, 5, 3, 1, 4]
    e = run([2, 0, 1], order=LENGTH)
    assert e["offsets"].tolist() == [0, 0, 1, 3] and e["ids"].tolist() == [200, 0, 1]


def test_hand_made_shuffle_and_groups():
    lengths = [5, 1, 4, 2, 3, 9, 7]
    sh = sorted(range(7), key=lambda d: h(7, d))
    assert run(lengths, order=SHUFFLE, seed=7)["perm"].tolist() == sh
    assert run(lengths, order=SHUFFLE, seed=7, flags=NB | DESC)["perm"].tolist() == sh      # DESC means nothing to SHUFFLE
    g = run(lengths, order=GROUPED, window=3, seed=7)["perm"].tolist()                     # groups of 3, 3 and 1
    assert [sorted(g[i:i + 3]) for i in (0, 3, 6)] == [sorted(sh[i:i + 3]) for i in (0, 3, 6)]
    for i in (0, 3, 6):
        assert [lengths[d] for d in g[i:i + 3]] == sorted(lengths[d] for d in sh[i:i + 3])
    gd = run(lengths, order=GROUPED, window=3, seed=7, flags=NB | DESC)["perm"].tolist()
    for i in (0, 3, 6):
        assert [lengths[d] for d in gd[i:i + 3]] == sorted((lengths[d] for d in sh[i:i + 3]), reverse=True)
    assert run(lengths, order=GROUPED, window=1, seed=7)["perm"].tolist() == sh
    assert run(lengths, order=GROUPED, window=7, seed=7)["perm"].tolist() == sorted(sh, key=lambda d: lengths[d])
    # equal lengths inside a group stay in shuffled order
    same = run([2] * 6, order=GROUPED, window=4, seed=3)["perm"].tolist()
    assert same == sorted(range(6), key=lambda d: h(3, d))
    # dropping a document does not reorder the others
    keep = [1, 1, 0, 1, 1, 1, 1]
    assert run(lengths, keep=keep, order=SHUFFLE, seed=7)["perm"].tolist() == [d for d in sh if d != 2]


def test_hand_made_batches():
    e = run([2, 4, 3, 1], max_tokens=12)                  # 3 documents * 4 == 12 fits exactly; the fourth would make 16
    assert e["batch_offsets"].tolist() == [0, 3, 4] and e["batch_rowlen"].tolist() == [4, 1]
    assert (e["n_batches"], e["n_oversize"], e["n_batch_pad"]) == (2, 0, 12 + 1 - 10)
    e = run([2, 4, 3, 1], max_tokens=11)                  # exceeds by one: the third document opens a batch
    assert e["batch_offsets"].tolist() == [0, 2, 4] and e["batch_rowlen"].tolist() == [4, 3] and e["n_batch_pad"] == 8 + 6 - 10
    e = run([2, 9, 2, 2], max_tokens=6)                   # an oversize document alone
    assert e["batch_offsets"].tolist() == [0, 1, 2, 4] and e["batch_rowlen"].tolist() == [2, 9, 2]
    assert (e["n_oversize"], e["n_batch_pad"]) == (1, 2 + 9 + 4 - 15)
    e = run([2, 4, 3, 1], max_tokens=100, max_docs=1)
    assert e["batch_offsets"].tolist() == [0, 1, 2, 3, 4] and e["batch_rowlen"].tolist() == [2, 4, 3, 1] and e["n_batch_pad"] == 0
    e = run([0, 0, 0, 5, 0], max_tokens=4, max_docs=0)    # empty documents cost nothing until a longer one joins them
    assert e["batch_offsets"].tolist() == [0, 3, 4, 5] and e["batch_rowlen"].tolist() == [0, 5, 0] and e["n_oversize"] == 1
    e = run([2, 4], max_tokens=8, flags=PERM | BATCHES)   # the counts without the arrays
    assert e["batch_offsets"] is None and e["batch_rowlen"] is None and (e["n_batches"], e["n_batch_pad"]) == (1, 2)
    e = run([2, 4], flags=PERM | BATCH_OFFSETS)           # the array flags select nothing without BATCHES
    assert e["batch_offsets"] is None and (e["n_batches"], e["n_oversize"], e["n_batch_pad"]) == (0, 0, 0)


def test_hand_made_nothing_kept():
    for lengths, keep in (([], None), ([2, 4, 3], [0, 0, 0]), ([0, 0], None)):
        e = run(lengths, keep=keep, max_tokens=10, order=LENGTH, min_length=1 if keep is None else 0)
        assert e["n_docs"] == e["n_ids"] == e["n_batches"] == e["n_batch_pad"] == 0
        assert e["offsets"].tolist() == [0] and e["batch_offsets"].tolist() == [0] and e["batch_rowlen"].tolist() == []
        assert e["ids"].shape == e["labels"].shape == e["perm"].shape == (0,)


def test_hash_is_a_bijection_and_depends_on_the_seed():
    d = np.arange(1 << 20, dtype=np.uint64) + 123456
    seen = []
    for seed in (0, 1, 0xDEADBEEF):
        x = (d * 0x9E3779B1 + seed) & M32
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M32
        x ^= x >> 16
        assert len(np.unique(x)) == len(d)
        assert [int(v) for v in x[:50]] == [h(seed, int(v)) for v in d[:50]]       # the vectorised form is the scalar one
        seen.append(x)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[1], seen[2])
    assert not np.array_equal(np.argsort(seen[0][:1000]), np.argsort(seen[1][:1000]))


def test_radix_model_against_sorted():
    """tools/regroup_model.py restates the passes as the kernels run them (digit-major block counts, their scan, the in-order
    scatter): each sort equals `sorted` by the key with ties in the order they came in, for chunk sizes that put many blocks,
    partial rounds and partial waves into a pass."""
    import regroup_model as rm
    rng = np.random.default_rng(31)
    for case in range(60):
        n = int(rng.integers(1, 3000))
        top = int(rng.choice([1, 3, 41, 255, 256, 70000, 2 ** 32 - 1]))
        keys = rng.integers(0, top + 1, n).tolist()
        vals = list(range(n))
        chunk, block = [(2048, 256), (512, 256), (320, 128), (64, 64)][case % 4]
        k2, v2 = rm.radix_sort(keys, vals, rm.radix_passes(max(keys)), chunk, block)
        assert v2 == sorted(vals, key=lambda i: (keys[i], i)) and k2 == [keys[i] for i in v2], case
    assert [rm.radix_passes(x) for x in (0, 1, 255, 256, 65535, 65536, 2 ** 24, 2 ** 32 - 1)] == [0, 1, 1, 2, 2, 3, 4, 4]


def test_order_model_against_the_restatement():
    import regroup_model as rm
    assert [rm.h(s, d) for s in (0, 9) for d in (0, 1, 77, 2 ** 32 - 1)] == [h(s, d) for s in (0, 9) for d in (0, 1, 77, 2 ** 32 - 1)]
    rng = np.random.default_rng(32)
    for case in range(32):
        D = int(rng.integers(1, 700))
        lengths = rng.integers(0, int(rng.choice([2, 41, 300, 70000])), D).tolist()
        keep = (rng.random(D) < 0.8).tolist()
        order, desc = case % 4, bool(case & 4)
        w, seed = int(rng.choice([1, 7, 64, 4096])), int(rng.integers(0, 2 ** 32))
        ids, oo = np.zeros(sum(lengths), np.uint32), np.concatenate([[0], np.cumsum(lengths)])
        e = expected_regroup(ids, oo, None, keep, opts(order, PERM | (DESC if desc else 0), seed=seed, window=w))
        kept = [d for d in range(D) if keep[d]]
        perm, _ = rm.permutation(lengths, kept, order, seed, w, desc, chunk=256, block=128)
        assert perm == e["perm"].tolist(), (case, order, desc, w)


def test_batch_search_model_against_the_plain_loop():
    """The walk through the maximum pyramid finds the batch boundaries of the plain loop, and reads at most 2 * 63 entries a
    level however long a batch is (a run of empty documents without max_docs included)."""
    import regroup_model as rm
    rng = np.random.default_rng(33)
    for case in range(45):
        K = int(rng.integers(1, 6000))
        m = rng.integers(0, int(rng.choice([1, 2, 41, 500])), K)
        if case % 3 == 0:
            a = int(rng.integers(0, K))
            m[a:a + int(rng.integers(1, 5000))] = 0
        m = m.tolist()
        T, max_docs = int(rng.choice([1, 64, 512, 4096, 10 ** 9])), int(rng.choice([0, 0, 1, 8, 100]))
        e = expected_regroup(np.zeros(sum(m), np.uint32), np.concatenate([[0], np.cumsum(m)]), None, None,
                             opts(flags=BATCHES | BATCH_OFFSETS | BATCH_ROWLEN, max_tokens=T, max_docs=max_docs))
        bo, rl, steps = rm.batches(m, T, max_docs)
        assert bo == e["batch_offsets"].tolist() and rl == e["batch_rowlen"].tolist(), (case, T, max_docs)
        assert steps <= 2 * 64 * 3                         # K < 64^3: three levels, each way
    bo, rl, steps = rm.batches([0] * 70000, 5, 0)         # one batch of 70 000 empty documents: three levels
    assert bo == [0, 70000] and rl == [0] and steps <= 2 * 64 * 3


def test_every_invalid_option_raises():
    ids, oo = ragged(docs_of_lengths([2, 4, 3]))
    lab = ids.astype(np.int32)
    ok = expected_regroup(ids, oo, lab, None, opts())
    assert ok["n_docs"] == 3
    for bad in (opts(order=4), opts(flags=NB | 64), opts(flags=1 << 31), opts(order=GROUPED, window=0), opts(flags=BATCHES, max_tokens=0),
                opts(min_length=5, max_length=4)):
        with pytest.raises(ValueError):
            expected_regroup(ids, oo, lab, None, bad)
    with pytest.raises(ValueError):                       # labels without a labels stream
        expected_regroup(ids, oo, None, None, opts(flags=LABELS))
    assert expected_regroup([], [0, 0], None, None, opts(flags=LABELS))["n_docs"] == 1     # N == 0: no labels stream is needed
    with pytest.raises(ValueError):                       # ids without a document
        expected_regroup(ids, [0], lab, None, opts())
    with pytest.raises(ValueError):                       # offsets that do not end at n_ids
        expected_regroup(ids, [0, 2, 6, 8], lab, None, opts())
    assert expected_regroup(ids, oo, lab, None, opts(min_length=4, max_length=4))["n_docs"] == 1
    assert expected_regroup(ids, oo, lab, None, opts(min_length=9, max_length=0))["n_docs"] == 0   # max_length 0: no upper bound


def test_header_values_and_shim_declarations():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    for name, value in VALUES.items():
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert re.search(r"\bconst %s\s*:\s*\w+\s*=\s*%d\s*;" % (name, value), ffi), name
    assert re.search(r"typedef struct tk_regroup_opts\b", hdr) and re.search(r"typedef struct tk_regroup\b", hdr)
    assert re.search(r"\bstruct TkRegroupOpts\b", ffi) and re.search(r"\bstruct TkRegroup\b", ffi)
    for text in (hdr, open(os.path.join(ROOT, "INTEGRATION.md")).read()):      # the pass is pointed to where sorting by hand was advised
        assert not re.search(r"sorts? or buckets?", text) and "tk_regroup_from_ids_device" in text


def test_python_constants_and_exported_symbols(tk):
    assert (tk.REGROUP_ORDER_KEEP, tk.REGROUP_ORDER_LENGTH, tk.REGROUP_ORDER_SHUFFLE, tk.REGROUP_ORDER_GROUPED) == (KEEP, LENGTH, SHUFFLE, GROUPED)
    assert (tk.REGROUP_DESC, tk.REGROUP_LABELS, tk.REGROUP_PERM, tk.REGROUP_BATCHES, tk.REGROUP_BATCH_OFFSETS, tk.REGROUP_BATCH_ROWLEN) \
        == (DESC, LABELS, PERM, BATCHES, BATCH_OFFSETS, BATCH_ROWLEN)
    for name in NEW_SYMBOLS:
        assert hasattr(tk.lib(), name), name
    for name in ("regroup_from_ids_device", "encode_batch_device_regroup", "encode_batch_regroup", "dense_from_regroup_batch", "last_regroup_ms"):
        assert hasattr(tk.Engine, name), name
    assert hasattr(tk.RegroupResult, "batches") and hasattr(tk.Tekkenizer, "encode_batch_regrouped")
    assert ctypes.sizeof(tk._RegroupOpts) == 40           # uint64 first: no padding in front of the seven uint32 + 4 at the end


def test_result_class_declares_the_header_struct(tk):
    """tests/test_layout_binding_cpu.py's first check, for "regroup"."""
    R, members = tk.RegroupResult, header_members("regroup")
    assert R.PASS == "regroup"
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr]
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr]
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)


def test_result_attributes_and_views_follow_the_declaration(tk):
    """... and its second: the ids and offsets have fixed types, as a join's (no I64 flag, no typestr)."""
    R = tk.RegroupResult
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in [o[0] for o in R.OUTPUTS] else i + 2)
    first_optional = next(o[0] for o in R.OUTPUTS if o[4])
    setattr(st, first_optional, None)
    r = R(st)
    assert R.I64 is None and not hasattr(r, "typestr") and hasattr(r, "n_docs")
    views = r.views()
    assert len(views) == len(R.OUTPUTS)
    for (out, typestr, shape, _, optional), v in zip(R.OUTPUTS, views):
        if out == first_optional:
            assert getattr(r, out + "_ptr") is None and v is None
            continue
        assert getattr(r, out + "_ptr") == getattr(st, out)
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r)) and cai["typestr"] == typestr
    for k in R.COUNTS:
        assert getattr(r, k) == getattr(st, k)
    assert set(r._counts()) == set(R.DICT_COUNTS) <= set(R.COUNTS)
