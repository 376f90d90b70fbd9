#!/usr/bin/env python3
"""Golden vectors of the LAYOUT passes from a THIRD-PARTY engine: HuggingFace `tokenizers` (Rust; 0.22.2 in this image)
-> tests/golden/layout_vectors_hf.json.

Label: "independent engine, different authors, NOT the reference".  tools/gen_golden_hf.py pins split and merge loop against
`tokenizers`; this script does the same for every output the README names after HuggingFace: `offset_mapping` (characters and
UTF-16 units), `word_ids()`, padding / truncation side / `pad_to_multiple_of`, `stride` / `return_overflowing_tokens` /
`overflow_to_sample_mapping`, `text_pair` with its three truncation strategies, `token_type_ids`, `sequence_ids`, and special
strings parsed out of text.  The kernels, the header definitions and the restatements in tests/test_*_cpu.py have one author; the
values written here have another.

  * vocabulary: trained exactly as tools/gen_golden_hf.py trains it and ASSERTED equal to `tokens_hex` of the committed
    tests/golden/merge_vectors_hf.json, so this fixture carries no vocabulary of its own;
  * specials: `<s>`, `</s>`, `[SEP]`, `<pad>` added to the HF tokenizer (two made-up strings more for the `specials` section) and
    mapped to the ids the engine uses for them; every other HF id -> rank + num_special, as the existing generator does;
  * class condition: a text is kept only if every pre-token is inside the class `in_class` of gen_golden_hf.py checks (tiktoken's
    bytes-keyed ranks and the merge list provably pick the same merges); more than 5 % outside it fails the run;
  * every recorded value is HF's, untouched.  The only conversions: the id mapping, None -> TK_WORD_NONE / TK_PAIR_SEQ_NONE, and
    UTF-16 / byte offsets computed from HF's CHARACTER offsets with Python `str` (len(text[:c].encode(...)));
  * a case HF refuses (it raises where this project cuts with `max_fixed`) is skipped and counted; more than 10 % of a section
    fails the run.

Run: python tools/gen_golden_hf_layout.py   (needs `tokenizers`; the committed JSON is what tests/test_layout_golden_hf.py reads).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden_hf import NUM_SPECIAL, PATTERN, bytes_to_unicode, in_class      # noqa: E402

WORD_NONE, SEQ_NONE = 0xFFFFFFFF, 255
ENGINE_IDS = {"<s>": 1, "</s>": 2, "<pad>": 3, "[SEP]": 4, "<<mk": 5, "<<mk>>": 6}      # the engine's special ids (0 is <unk>)
TEMPLATE_SINGLE, TEMPLATE_PAIR = "<s> $A </s>", "<s> $A [SEP] $B:1 </s>:1"
MAX_TEXT_BYTES, MAX_KEPT_IDS = 600, 8
DENSE_LENGTHS, DENSE_MULTIPLES = (8, 13, 16), (None, 4, 7)
WINDOWS = ((7, 2), (16, 0), (16, 5), (33, 8))
PAIR_WINDOWS = ((20, 0), (20, 4), (41, 7))
MAX_FIXTURE_BYTES = 460 * 1000


def trained_tokenizer():
    """The tokenizer of tools/gen_golden_hf.py, trained the same way -> (tokenizer, token byte strings by rank, {HF id: rank})."""
    from tokenizers import Tokenizer, Regex, models, pre_tokenizers, trainers
    import corpus
    tok = Tokenizer(models.BPE(ignore_merges=True))
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(PATTERN), behavior="isolated"),
                                                 pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    trainer = trainers.BpeTrainer(vocab_size=256 + 2500, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), special_tokens=[],
                                  show_progress=False)
    train = []
    for kind, n, dl, sd in (("ascii", 500, 512, 11), ("mixed", 120, 2048, 12)):
        d, o = corpus.generate(kind, n, dl, seed=corpus.BASE_SEED + sd)
        train += [x.decode("utf-8") for x in corpus.docs_of(d, o)]
    tok.train_from_iterator(train, trainer)
    model = json.loads(tok.to_str())["model"]
    u2b = bytes_to_unicode()

    def tb(s):
        return bytes(u2b[c] for c in s)

    merges = [(tb(a), tb(b)) for a, b in model["merges"]]
    tokens = [bytes([i]) for i in range(256)] + [a + b for a, b in merges]
    rank = {t: i for i, t in enumerate(tokens)}
    id2rank = {i: rank[tb(s)] for s, i in model["vocab"].items()}
    return tok, tokens, merges, id2rank, tb


def the_texts():
    """About 40 texts, none near the 600 bytes allowed (every row of every text is recorded, so the fixture grows with them): fresh seeds of the ascii and mixed shapes (cut at a character boundary to a spread of
    lengths), the reference's edge inputs of gen_golden_hf.py, the empty text, one-character texts, emoji / CJK the vocabulary leaves
    as byte-fallback tokens (tokens begin and end inside a character), astral characters (UTF-16 units differ from code points)."""
    import corpus
    texts = []
    # (short: every window and dense row of every text is in the fixture, and mixed text is a token a byte where it is not ASCII)
    for kind, dl, sd, cuts in (("ascii", 512, 31, (200, 37, 90, 23, 120, 12, 64)), ("mixed", 2048, 32, (100, 30, 60, 16, 44))):
        d, o = corpus.generate(kind, len(cuts), dl, seed=corpus.BASE_SEED + sd)
        for x, cut in zip(corpus.docs_of(d, o), cuts):
            t = x.decode("utf-8")
            while len(t.encode("utf-8")) > cut:
                t = t[:-1]
            texts.append(t)
    texts += ["Hello, world!", "it's IT'S x's 'abc 'sabc", "1234 56 7", "   whitespace   handling   ", "Line1\nLine2\rLine3\r\nLine4",
              "hi !!\n\nyo", "  \n  \n  x", "a  1", "x\t\ty", "end   ", "Hello\x00World", "日本語 のテキスト", "naïve café — “quotes”"]
    texts += ["", "a", " ", "é", "中", "\U0001f680"]
    texts += ["go \U0001f680\U0001f680 now \U0001f9d1‍\U0001f680!", "漢字かな、テスト。𠮷野家で𩸽",
              "\U0001d54f = \U0001d7d8 + \U00010348; a\U0001f600b\U0001f601c", "x\U0001f680", "\U0001f680x é中\U0001f680"]
    assert all(len(t.encode("utf-8")) <= MAX_TEXT_BYTES for t in texts)
    return texts


def flat(pairs):
    return [x for p in pairs for x in p]


def in_unit(text, offsets, encoding):
    """HF's character offsets in the code units of `encoding`, by Python str."""
    w = 2 if encoding == "utf-16-le" else 1
    return [(len(text[:s].encode(encoding)) // w, len(text[:e].encode(encoding)) // w) for s, e in offsets]


def main():
    import tokenizers
    from tokenizers import AddedToken, Tokenizer, processors
    tok, tokens, merges, id2rank, tb = trained_tokenizer()
    with open(os.path.join(ROOT, "tests", "golden", "merge_vectors_hf.json")) as f:
        committed = json.load(f)
    own_vocab = [t.hex() for t in tokens] != committed["tokens_hex"] or committed["num_special"] != NUM_SPECIAL
    assert not own_vocab, "training did not reproduce tokens_hex of merge_vectors_hf.json: store the vocabulary here and say so in the label"
    rank = {t: i for i, t in enumerate(tokens)}
    pair_of = {a + b: (a, b) for a, b in merges}
    tokens_set = set(tokens[256:])

    def inside(text):
        pieces = [tb(s) for s, _ in tok.pre_tokenizer.pre_tokenize_str(text)]
        assert b"".join(pieces) == text.encode("utf-8"), text[:40]
        return all(p in rank or in_class(p, tokens_set, pair_of, rank) for p in pieces)

    def add_specials(t, names):
        t.add_special_tokens([AddedToken(s, special=True, normalized=False) for s in names])
        return {t.token_to_id(s): ENGINE_IDS[s] for s in names}

    base = ("<s>", "</s>", "[SEP]", "<pad>")
    sp_of = add_specials(tok, base)
    hf_id = {s: tok.token_to_id(s) for s in base}
    tok.post_processor = processors.TemplateProcessing(single=TEMPLATE_SINGLE, pair=TEMPLATE_PAIR,
                                                       special_tokens=[(s, hf_id[s]) for s in ("<s>", "</s>", "[SEP]")])

    def ids_of(hf_ids, m=None):
        m = sp_of if m is None else m
        return [m[i] if i in m else id2rank[i] + NUM_SPECIAL for i in hf_ids]

    def fresh():
        return Tokenizer.from_str(tok.to_str())

    candidates = the_texts()
    texts = [t for t in candidates if inside(t)]
    excluded = len(candidates) - len(texts)
    if excluded * 20 > len(candidates):
        sys.exit("%d of %d texts outside the class: more than 5 %%" % (excluded, len(candidates)))
    plain = [tok.encode(t, add_special_tokens=False) for t in texts]
    out = {"label": "independent engine (HuggingFace tokenizers %s: offsets, word ids, truncation, padding, overflow, pair templates, type "
                    "and sequence ids, added special tokens), different authors, NOT the reference; vocabulary: tokens_hex of "
                    "merge_vectors_hf.json, reproduced by training and asserted equal" % tokenizers.__version__,
           "tokenizers": tokenizers.__version__, "pattern": PATTERN, "num_special": NUM_SPECIAL, "special_ids": ENGINE_IDS,
           "word_none": WORD_NONE, "seq_none": SEQ_NONE, "template_single": TEMPLATE_SINGLE, "template_pair": TEMPLATE_PAIR,
           "n_texts": len(candidates), "n_excluded_outside_class": excluded,
           "texts": [{"text_hex": t.encode("utf-8").hex(), "ids": ids_of(e.ids)} for t, e in zip(texts, plain)]}
    counts = {}

    def section(name, cases, skipped, **params):
        total = len(cases) + skipped
        if skipped * 10 > total:
            sys.exit("section %s: HF refused %d of %d cases: more than 10 %%" % (name, skipped, total))
        out[name] = dict(params, n_cases=len(cases), n_skipped=skipped, cases=cases)
        counts[name] = (len(cases), skipped)

    # ---- offsets and words: per text, without and with BOS / EOS through the template
    off_cases, word_cases = [], []
    for t, e0 in zip(texts, plain):
        e1 = tok.encode(t)
        assert e1.ids[1:-1] == e0.ids
        c = {}
        for key, e in (("", e0), ("_sp", e1)):
            c["char" + key] = flat(e.offsets)
            c["utf16" + key] = flat(in_unit(t, e.offsets, "utf-16-le"))
            c["byte" + key] = flat(in_unit(t, e.offsets, "utf-8"))
        c["char_to_token"] = [e0.char_to_token(k) for k in range(len(t))]         # (every character lies under a token)
        off_cases.append(c)
        w = {}
        for key, e in (("", e0), ("_sp", e1)):
            w["word_ids" + key] = [WORD_NONE if x is None else x for x in e.word_ids]
            n_words = 1 + max((x for x in e.word_ids if x is not None), default=-1)
            w["word_first" + key] = [e.word_to_tokens(k)[0] for k in range(n_words)]
        word_cases.append(w)
    section("offsets", off_cases, 0)
    section("words", word_cases, 0)

    # ---- dense: encode_batch over the whole list; every length x truncation side, the padding options rotated through them
    dense = []
    k = 0
    for T in DENSE_LENGTHS:
        for trunc in ("right", "left"):
            for _ in range(2):
                # (k = 0 .. 11: each of the 12 of multiple x side x fixed once, two to every length x truncation side)
                mult, pad_dir, fixed = DENSE_MULTIPLES[k % 3], ("right", "left")[k % 2], bool(k // 2 % 2)
                k += 1
                t2 = fresh()
                t2.enable_truncation(max_length=T, direction=trunc)
                lengths = [len(e.ids) for e in t2.encode_batch(texts)]
                t2.enable_padding(direction=pad_dir, pad_id=hf_id["<pad>"], pad_token="<pad>", pad_to_multiple_of=mult,
                                  length=T if fixed else None)
                encs = t2.encode_batch(texts)
                dense.append({"max_length": T, "truncation_side": trunc, "padding_side": pad_dir, "multiple_of": mult, "fixed": fixed,
                              "ids": [ids_of(e.ids) for e in encs], "attention_mask": [e.attention_mask for e in encs],
                              "lengths": lengths})
    section("dense", dense, 0)

    # ---- windows: every text's encoding followed by its overflowing list
    windows = []
    for T, s in WINDOWS:
        t2 = fresh()
        t2.enable_truncation(max_length=T, stride=s)
        rows = [(d, w) for d, e in enumerate(t2.encode_batch(texts)) for w in [e] + e.overflowing]
        c = {"max_length": T, "stride": s, "sample": [d for d, _ in rows], "ids": [ids_of(w.ids) for _, w in rows],
             "offsets": [flat(w.offsets) for _, w in rows]}
        for key, length in (("mask_longest", None), ("mask_fixed", T)):
            t2.enable_padding(direction="right", pad_id=hf_id["<pad>"], pad_token="<pad>", length=length)
            padded = [w for e in t2.encode_batch(texts) for w in [e] + e.overflowing]
            assert [ids_of(w.ids)[:len(r)] for w, r in zip(padded, c["ids"])] == c["ids"]
            c[key] = [w.attention_mask for w in padded]
        windows.append(c)
    section("windows", windows, 0)

    # ---- pairs: about 20, the kept side of the only_* strategies at most MAX_KEPT_IDS ids
    n_ids = [len(e.ids) for e in plain]
    short = [i for i, n in enumerate(n_ids) if n <= MAX_KEPT_IDS]
    longer = sorted((i for i, n in enumerate(n_ids) if 12 <= n <= 52), key=lambda i: n_ids[i])
    empty = texts.index("")
    spread = [longer[k] for k in (1, len(longer) // 2, -2, -1)]      # (the last two are split at both lengths)
    kept_long = [(short[k % len(short)], i) for k, i in enumerate(spread)] + [(empty, spread[1]), (short[1], empty), (empty, empty)]
    by_strategy = {
        "only_second": kept_long,
        "only_first": [(b, a) for a, b in kept_long],
        # both sides long, the two sides equal and over the budget, one side empty, one side short
        "longest_first": [(spread[k], spread[-1 - k]) for k in range(len(spread))] + [(i, i) for i in spread[1:3]]
                         + [(empty, spread[-1]), (spread[-1], empty), (short[2], spread[-2]), (spread[-2], short[3]), (empty, empty)],
    }
    pair_cases, refused = [], 0
    for strategy, plist in by_strategy.items():
        # (longest_first: the same lengths at stride 0 -- this project has no overflow under that strategy)
        for T, s in sorted({(T, 0) for T, _ in PAIR_WINDOWS}) if strategy == "longest_first" else PAIR_WINDOWS:
            t2 = fresh()
            t2.enable_truncation(max_length=T, stride=s, strategy=strategy)
            c = {"strategy": strategy, "max_length": T, "stride": s, "overflow": strategy != "longest_first", "pairs": [], "sample": [],
                 "ids": [], "type_ids": [], "sequence_ids": [], "offsets": []}
            for a, b in plist:
                try:
                    e = t2.encode(texts[a], texts[b])
                except Exception:                   # HF raises where the kept side leaves no room; this project cuts with max_fixed
                    refused += 1
                    continue
                p = len(c["pairs"])
                c["pairs"].append([a, b])
                for w in [e] + (e.overflowing if c["overflow"] else []):
                    c["sample"].append(p)
                    c["ids"].append(ids_of(w.ids))
                    c["type_ids"].append(w.type_ids)
                    c["sequence_ids"].append([SEQ_NONE if q is None else q for q in w.sequence_ids])
                    c["offsets"].append(flat(w.offsets))
            t2.enable_padding(direction="right", pad_id=hf_id["<pad>"], pad_token="<pad>", length=T)
            c["attention_mask"] = [w.attention_mask for a, b in c["pairs"] for e in [t2.encode(texts[a], texts[b])]
                                   for w in [e] + (e.overflowing if c["overflow"] else [])]
            pair_cases.append(c)
    n_pairs = sum(len(c["pairs"]) for c in pair_cases)
    if refused * 10 > n_pairs + refused:
        sys.exit("section pairs: HF refused %d of %d pairs: more than 10 %%" % (refused, n_pairs + refused))
    section("pairs", pair_cases, 0, n_pairs=n_pairs, n_pairs_skipped=refused)

    # ---- specials: the four and two made-up strings, one a proper prefix of the other, parsed out of text; no template
    t3 = fresh()
    t3.post_processor = processors.TemplateProcessing(single="$A", pair="$A $B:1", special_tokens=[])
    names = ("<s>", "</s>", "[SEP]", "<pad>", "<<mk", "<<mk>>")
    sp3 = add_specials(t3, names)
    # (a text as its segments: a str is text, a 1-tuple a special string)
    S, E, SEP, PAD, MK, MK2 = (("<s>",), ("</s>",), ("[SEP]",), ("<pad>",), ("<<mk",), ("<<mk>>",))
    seg_texts = [[S, "Hello, world!", E], [S], [E, E], ["no specials here"], [S, E, SEP, PAD], ["in", SEP, "side a word"],
                 ["a ", MK2, " b"], ["a ", MK, " b"], [MK, MK2], [MK2, ">"], [MK, ">"], ["only a prefix <<m of one"], ["<<m"], ["<s"],
                 ["x[SEP"], [PAD, PAD, "naïve café", PAD], ["日本語", SEP, "のテキスト", E], ["tail ", MK], [MK, "head"], ["it's ", S, "1234 56 7", E, "\n"],
                 ["<", S, ">"], ["[", SEP, "]"], ["go \U0001f680", MK2, "\U0001f680 now"], [""]]
    sp_cases, sp_out = [], 0
    for segs in seg_texts:
        text = "".join(x if isinstance(x, str) else x[0] for x in segs)
        runs, cur = [], ""
        for x in segs:                              # the text between the specials, as HF pre-tokenizes it: run by run
            if isinstance(x, str):
                cur += x
            else:
                runs.append(cur)
                cur = ""
        runs.append(cur)
        if not all(inside(r) for r in runs):
            sp_out += 1
            continue
        e = t3.encode(text)
        got = ids_of(e.ids, sp3)
        want = [ENGINE_IDS[x[0]] for x in segs if not isinstance(x, str)]
        # the construction says which specials HF must have found (">" behind "<<mk" makes the longer string: leftmost-longest)
        if text in ("<<mk>", "<<mk>>>"):
            want = [ENGINE_IDS["<<mk"]] if text == "<<mk>" else [ENGINE_IDS["<<mk>>"]]
        assert [i for i in got if i < NUM_SPECIAL] == want, (text, got)
        sp_cases.append({"text_hex": text.encode("utf-8").hex(), "ids": got})
    if sp_out * 20 > len(seg_texts):
        sys.exit("section specials: %d of %d texts outside the class" % (sp_out, len(seg_texts)))
    section("specials", sp_cases, 0, strings=list(names), n_excluded_outside_class=sp_out)

    path = os.path.join(ROOT, "tests", "golden", "layout_vectors_hf.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %s: %d texts (%d outside the class excluded), %.1f KB" % (path, len(texts), excluded, size / 1e3))
    for name, (n, skipped) in counts.items():
        print("  %-8s %3d cases, %d skipped%s" % (name, n, skipped, ", %d pairs, %d refused by HF" % (n_pairs, refused) if name == "pairs" else ""))
    if size > MAX_FIXTURE_BYTES:
        sys.exit("fixture larger than %d bytes: trim texts or parameter combinations" % MAX_FIXTURE_BYTES)


if __name__ == "__main__":
    main()
