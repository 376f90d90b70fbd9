"""What the decode tests share: a plain-Python restatement of the emit kernel's bookkeeping (csrc/tk_decode.hip) that says which
path every 64-id step takes and how every id is stored and sized, and the case tables of tests/test_gpu_decode.py over
helpers.table_edge_vocab.  tests/test_decode_cases_cpu.py holds the tables to the paths they are meant to reach, so a table cannot
drift off its target while the GPU tests stay green."""
import itertools

import numpy as np

import tk_oracle

IGNORE, KEEP, RAISE = 0, 1, 2
IMG_BYTES = 4096          # TKD_IMG_BYTES: the LDS image of one step's text
L8_LDS = 32768            # TKD_L8_LDS: one-byte lengths of the ranks below this live in LDS
GROUP_DOCS = 16           # TK_DECODE_GROUP_DOCS: consecutive documents a wave takes as one stream of ids
STEP = 64                 # ids per step
EMPTY = 3                 # the empty special string of helpers.EDGE_SPECIALS: no bytes under any policy


# ---- the model ----
def piece_len(v, i, policy):
    ns = v["num_special"]
    if i < ns:
        return len(v["specials"][i].encode()) if policy == KEEP else 0
    return len(v["tokens"][i - ns]) if i - ns < len(v["tokens"]) else 0


def id_class(v, i, policy, direct):
    """(store class, length source) of one id in a step of the image path / the direct path."""
    ns = v["num_special"]
    if i < ns:
        if policy != KEEP:
            return "special:dropped", "none"
        n = len(v["specials"][i].encode())
        return "special:" + ("0" if n == 0 else "1-15" if n < 16 else "16" if n == 16 else "17+"), "sp_offs"
    r = i - ns
    if r >= len(v["tokens"]):
        return "oov", "none"
    n = len(v["tokens"][r])
    where = "lds" if r < L8_LDS else "global"
    src = where if n < 255 else "fallback_" + where        # (a length byte of 0xFF: the length comes from the offsets)
    if direct:
        return ("direct_regs" if n <= 15 else "direct_blob"), src
    return ("inline" if n <= 15 else "blob16" if n == 16 else "image_loop"), src


def step_paths(tokens, specials, num_special, id_lists, policy):
    """The steps of tk_decode_emit_kernel over a batch: groups of 16 documents are one id stream, taken 64 ids at a time, the
    cursor runs across the whole batch.  Per step: its group, the ids, cursor & 3, span, whether (cursor & 3) + span > 4096 (the
    direct-store path), per id (store class, length source), and how many documents (empty ones too) begin in it."""
    v = {"tokens": tokens, "specials": specials, "num_special": num_special}
    steps, cursor = [], 0
    for g in range(0, len(id_lists), GROUP_DOCS):
        docs = id_lists[g:g + GROUP_DOCS]
        stream = [i for d in docs for i in d]
        starts = list(itertools.accumulate([0] + [len(d) for d in docs[:-1]]))
        for c0 in range(0, len(stream), STEP):
            ids = stream[c0:c0 + STEP]
            span = sum(piece_len(v, i, policy) for i in ids)
            direct = (cursor & 3) + span > IMG_BYTES
            begun = [k for k, s in enumerate(starts) if c0 <= s < c0 + STEP and s < len(stream)]
            steps.append({"group": g // GROUP_DOCS, "ids": ids, "residue": cursor & 3, "span": span, "direct": direct,
                          "classes": [id_class(v, i, policy, direct) for i in ids], "doc_starts": len(begun),
                          "empty_starts": sum(1 for k in begun if not docs[k]),
                          "empty_at_end": sum(1 for s in starts if s >= len(stream))})
            cursor += span
    return steps


def paths_of(v, id_lists, policy):
    return step_paths(v["tokens"], v["specials"], v["num_special"], id_lists, policy)


def reached(steps):
    return {("direct" if s["direct"] else "image",) + c for s in steps for c in s["classes"]}


def reference(v, id_lists, policy):
    """tk_oracle.decode_ref document by document: ("ok", texts), or ("err", first document that raises, what it raises)."""
    out = []
    for d, ids in enumerate(id_lists):
        try:
            out.append(tk_oracle.decode_ref(v["tokens"], v["specials"], v["num_special"], ids, policy))
        except ValueError as e:
            return ("err", d, str(e))
    return ("ok", out)


KIND = {"special": "SpecialTokenPolicy", "key": "Tokenizers", "utf8": "Tokenizers"}      # decode_ref's classes as TokenizerError.kind


# ---- building blocks ----
def tok(v, n, k=0, flavour=None):
    """The id of a token of n bytes that is valid UTF-8 on its own; k rotates through the flavours that are."""
    ns = v["num_special"]
    if n == 1:
        return ns + 0x61 + k % 26
    if flavour is None:
        ok = ["ascii", "mb"] + ["e"] * (n % 2 == 0) + ["rocket"] * (n % 4 == 0) + ["zh_cut"] * (n % 3 == 0)
        flavour = ok[k % len(ok)]
    return ns + v["edge"][(n, flavour)]


def compose(v, n_ids, total, k=0):
    """n_ids token ids (no specials) of `total` bytes of text, each valid alone: the longest length that still fits, each time."""
    import helpers
    lengths = sorted(set(helpers.EDGE_LENGTHS) | {1}, reverse=True)
    assert n_ids <= total <= n_ids * lengths[0], (n_ids, total)
    out = []
    for j in range(n_ids):
        n = next(x for x in lengths if x <= total - (n_ids - j - 1))
        out.append(tok(v, n, k + j))
        total -= n
    assert total == 0
    return out


def front(v, k, specials=True):
    """A full step of 64 ids in front of a step under test.  With specials: k one-byte tokens and 64 - k empty specials (k bytes);
    without: 64 tokens of one or two bytes (k bytes, k >= 64)."""
    if specials:
        ids = [tok(v, 1, j) for j in range(k)]
        for j in range(STEP - k):
            ids.insert(3 + 7 * j, EMPTY)
        return ids
    return [tok(v, 2 if j < k - STEP else 1, j) for j in range(STEP)]


def as_group(stream, layout):
    """A stream of ids as exactly 16 documents: the cuts and the empty documents of one of four layouts."""
    n = len(stream)
    if layout == 0:                                   # one document, empty ones at the group's end
        docs = [stream]
    elif layout == 1:                                 # empty ones at the group's start, cuts in both steps
        docs = [[], []] + [stream[a:b] for a, b in zip([0, 30, 74, 104], [30, 74, 104, n])]
    elif layout == 2:                                 # a cut every nine ids
        docs = [[]] + [stream[a:a + 9] for a in range(0, n, 9)]
        docs = docs[:15] + [sum(docs[15:], [])]
    else:                                             # empty documents between the pieces, a one-id document
        docs = [stream[:64], [], [], stream[64:65], [], stream[65:100], stream[100:]]
    assert len(docs) <= GROUP_DOCS and sum(docs, []) == list(stream)
    return docs + [[] for _ in range(GROUP_DOCS - len(docs))]


def text_len(v, ids, policy):
    return sum(piece_len(v, i, policy) for i in ids)


class _Batch:
    """Groups of 16 documents one behind the other; the running cursor says which step in front gives a wanted cursor & 3."""
    def __init__(self, v, policy):
        self.v, self.policy, self.docs, self.cursor = v, policy, [], 0

    def add(self, residue, main, layout):
        v, sp = self.v, self.policy != RAISE
        lo = 61 if sp else 64
        k = lo + (residue - self.cursor - lo) % 4
        stream = front(v, k, sp) + list(main)
        self.docs += as_group(stream, layout)
        self.cursor += text_len(v, stream, self.policy)


# ---- table a: the image boundary ----
TOTALS = range(4092, 4101)


def boundary_step(v, total, variant):
    """64 ids of `total` bytes from tokens of 63, 64 and 65 bytes; variant 1 has two more 65 / 63 pairs, and the cut pair
    (a 64-byte token that ends inside 中, the 65-byte token that completes it)."""
    d = total - STEP * 64
    lens = [65] * max(d, 0) + [63] * max(-d, 0)
    if variant:
        lens += [65, 63, 65, 63]
    ids = [tok(v, n, j) for j, n in enumerate(lens + [64] * (STEP - len(lens)))]
    if variant:
        pair = [v["num_special"] + v["edge"][(64, "zh_cut")], v["num_special"] + v["edge"][(65, "zh_tail")]]
        at64 = [j for j, n in enumerate(lens + [64] * (STEP - len(lens))) if n == 64][:1]
        at65 = [j for j, n in enumerate(lens) if n == 65][:1]
        if at64 and at65:                            # the pair stands together: one 64 and one 65 leave, the pair goes to the end
            ids = [x for j, x in enumerate(ids) if j not in (at64[0], at65[0])] + pair
    return ids


def mixed_step(v, total, policy, k):
    """One id of every store class in one step of `total` bytes: an inline token, 16 bytes from the blob, 17 bytes, 300 bytes, and
    (not under Raise) the specials of 16, 18, 36 and 300 bytes and the empty one."""
    ns = v["num_special"]
    picks = [tok(v, 9, k), tok(v, 15, k + 1), tok(v, 16, k + 2), tok(v, 17, k + 3), tok(v, 300, k)]
    picks += [ns + v["edge"][(14, "ascii")], ns + v["edge"][(16, "rocket")]]
    if policy != RAISE:
        picks += [5, 4, 7, EMPTY, 6, 1]
    rest = compose(v, STEP - len(picks), total - text_len(v, picks, policy), k)
    for j, x in enumerate(picks):
        rest.insert(4 * j + 1, x)
    return rest


def table_a(v, policy):
    """One batch: every total 4092..4100 at every cursor & 3, plain and mixed steps, the 5000-byte token, x * 300 specials."""
    b = _Batch(v, policy)
    n = 0
    for total in TOTALS:
        for residue in range(4):
            for variant in (0, 1):
                b.add(residue, boundary_step(v, total, variant), n % 4)
                n += 1
    for residue in range(4):
        for side in (0, 1):                          # both sides of (cursor & 3) + span > 4096
            b.add(residue, mixed_step(v, IMG_BYTES - residue + side, policy, n), n % 4)
            n += 1
            if policy != RAISE:                      # x * 300 specials beside 64 / 65-byte tokens (13 of them: 3900 bytes under Keep)
                want = IMG_BYTES - residue + side
                sp = [7] * 13
                rest = compose(v, STEP - 13, want - text_len(v, sp, policy), n)
                b.add(residue, rest[:20] + sp + rest[20:], n % 4)
                n += 1
    longs = [v["num_special"] + v["long"]] + [v["num_special"] + r for r, m in v["high"].items() if m == 5000]
    for j, big in enumerate(longs):
        short = compose(v, STEP - 1, 500 + j, j)
        for layout in (0, 2):
            b.add(j, short[:20] + [big] + short[20:], layout)
    return b.docs


# ---- table b: long tokens and the length passes ----
def table_b(v, policy):
    ns, toks = v["num_special"], v["tokens"]
    longs = [ns + v["edge"][(n, f)] for n in (254, 255, 256, 300) for f in ("ascii", "mb")]
    longs += [ns + v["edge"][k] for k in ((255, "zh_cut"), (300, "zh_cut"), (254, "e"), (256, "e"), (300, "e"), (256, "rocket"), (300, "rocket"))]
    longs.append(ns + v["long"])
    hand = [ns + r for r in sorted(v["hand"])]
    high = [ns + r for r in sorted(v["high"])]
    around = [ns + r for r in range(L8_LDS - 8, L8_LDS + 8) if r < len(toks)]       # filler and hand-placed ranks, both sides
    a, z = tok(v, 1, 0), tok(v, 1, 25)
    docs = []
    for t in longs + hand + high:                    # (at most six long tokens in a group: steps of the image path)
        docs += [[t], [], [a, z]]
    docs += [[] for _ in range(-len(docs) % GROUP_DOCS)]
    docs += [[a, z, t, a] for t in longs + hand + high]
    docs += [longs, hand, hand[::-1], high, high[::-1], around, around[::-1], []]
    docs += [[x, y] for x, y in zip(hand, hand[1:])] + [[y, x] for x, y in zip(hand, hand[1:])]
    # more than 256 ids in one group (the unrolled loop of the group length pass), long tokens on every lane residue
    cycle = longs + hand + high + [a, z, tok(v, 7, 1), tok(v, 16, 1), tok(v, 17, 1)]
    docs.append([cycle[j % len(cycle)] for j in range(300)])
    docs.append([cycle[(5 * j) % len(cycle)] for j in range(131)])
    if policy != RAISE:
        docs += [[7, longs[0], 4], [1] + hand + [2], [EMPTY] + high[::-1] + [6]]
    return docs


# ---- table c: UTF-8 validation around long tokens ----
def cut_tokens(v):
    """(id of a token that ends inside a character, the byte-token ids that complete the character)."""
    ns = v["num_special"]
    out = []
    for n, f in ((7, "zh_cut"), (16, "zh_cut"), (17, "zh_cut"), (64, "zh_cut"), (254, "zh_cut"), (256, "zh_cut"), (15, "e"), (255, "e"),
                 (7, "rocket"), (65, "rocket"), (254, "rocket")):
        t = v["tokens"][v["edge"][(n, f)]]
        ch = {"zh_cut": "中", "e": "é", "rocket": "\U0001f680"}[f].encode()
        done = n % len(ch)
        assert done, (n, f)
        out.append((ns + v["edge"][(n, f)], [ns + x for x in ch[done:]]))
        assert (t + ch[done:]).decode("utf-8")
    return out


def table_c(v, policy):
    """[(name, documents, bad document or None)]: 40 documents, the one under test at index 21 (the middle of the second group).
    Every cut token with the bytes that complete it (valid), with a special id in between (two runs, each invalid), and with the
    document's end in between (invalid; the completion begins the next document); each once in a step of the image path and
    once -- fourteen 300-byte tokens in front -- in a step of the direct path.  Raise has no special id: those cases are left out."""
    ns = v["num_special"]
    fill = [[tok(v, 1, j), tok(v, 3, j, "zh_cut"), tok(v, 4, j, "rocket"), tok(v, 2, j, "e"), tok(v, 7, j), tok(v, 1, j + 1), tok(v, 9, j), tok(v, 2, j)]
            for j in range(40)]
    lead = ns + 0xE4
    tails = [ns + v["edge"][(n, "zh_tail")] for n in (8, 17, 65, 254)]        # begin with the last two bytes of 中, end on a character
    cases = []
    for path in ("image", "direct"):
        pre = [tok(v, 300, j) for j in range(14)] if path == "direct" else [tok(v, 1, 7)]
        post = [tok(v, 2, 3), tok(v, 1, 1)]

        def batch(doc, nxt=None):
            docs = [list(d) for d in fill]
            docs[21] = doc
            if nxt is not None:
                docs[22] = nxt
            return docs

        for j, (cut, comp) in enumerate(cut_tokens(v)):
            name = "%s/cut%d" % (path, cut)
            cases.append((name + "/valid", batch(pre + [cut] + comp + post), None))
            if policy != RAISE:
                cases.append((name + "/special", batch(pre + [cut, (EMPTY, 1)[j % 2]] + comp + post), 21))
            cases.append((name + "/end", batch(pre + [cut], comp + post), 21))
        for j, t in enumerate(tails):
            name = "%s/tail%d" % (path, t)
            cases.append((name + "/valid", batch(pre + [lead, t] + post), None))
            if policy != RAISE:
                cases.append((name + "/special", batch(pre + [lead, (1, EMPTY)[j % 2], t] + post), 21))
            cases.append((name + "/start", batch([t] + pre + post), 21))
    return cases


# ---- table d: which document, which class ----
def table_d(v):
    """Batches of about 50 documents with three offenders of different kinds in different documents -- an id outside the
    vocabulary, an invalid run, a special id (an offender under Raise only) -- in every order, each the first id of a document
    behind one, two or 17 empty documents; and one batch whose very last id is outside the vocabulary."""
    ns = v["num_special"]
    ok = [[tok(v, 1, j), tok(v, 4, j), tok(v, 17, j), tok(v, 2, j)] for j in range(8)]
    body = [tok(v, 1, 2), tok(v, 3, 0, "zh_cut")]
    offender = {"key": [ns + len(v["tokens"]) + 5] + body, "utf8": [ns + v["edge"][(17, "zh_tail")]] + body, "special": [1] + body}
    batches = []
    for order in itertools.permutations(("key", "utf8", "special")):
        for gaps in ((1, 2, 17), (17, 1, 2), (2, 17, 1)):
            docs = ok[:3]
            for kind, gap in zip(order, gaps):
                docs = docs + [[] for _ in range(gap)] + [offender[kind]] + ok[3:7]
            docs = docs + [[] for _ in range(max(0, 50 - len(docs)))]
            batches.append(docs)
    last = ok[:5] + [[] for _ in range(17)] + ok[5:] + [[], body + [ns + len(v["tokens"])]]
    batches.append(last)
    batches.append(last + [[], []])
    return batches


# ---- e: the sweeps ----
def sweep_docs(v, n_docs=20000, seed=11):
    """n_docs documents of 0..40 ids, each id valid UTF-8 on its own; a third of the documents hold a multi-byte character.  The
    documents at and around 8192 and 16384 (the second sweep of the length pass and of the validate kernel) are not empty."""
    ns, toks = v["num_special"], v["tokens"]
    rng = np.random.default_rng(seed)
    plain = np.array([ns + r for r in range(0x20, 0x7F)] + [ns + r for r in range(400, 3000) if toks[r][0] < 0x80]
                     + [ns + r for r in range(32772, min(len(toks), 33000)) if toks[r][0] < 0x80 and len(toks[r]) < 8])
    multi = np.array([ns + v["edge"][(n, f)] for n, f in ((2, "e"), (3, "zh_cut"), (4, "rocket"), (7, "mb"), (9, "zh_cut"), (16, "rocket"), (17, "mb"))]
                     + [ns + r for r in range(400, 3000) if toks[r][0] >= 0x80]
                     + [ns + r for r in range(32772, min(len(toks), 33000)) if toks[r][0] >= 0x80])
    docs = []
    for d in range(n_docs):
        n = int(rng.integers(0, 41))
        if d % 8192 < 12 or d % 8192 > 8180:
            n = 5 + d % 30
        ids = plain[rng.integers(0, len(plain), n)].tolist()
        if d % 3 == 0 and n:
            for at in rng.integers(0, n, 1 + n // 8).tolist():
                ids[at] = int(multi[rng.integers(0, len(multi))])
        if d % 7 == 0 and n:
            ids[int(rng.integers(0, n))] = (1, 2, EMPTY, 6)[d % 4]
        docs.append(ids)
    return docs
