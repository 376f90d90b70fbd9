"""Time the specials pass (csrc/tk_specials.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/specials_time.json.

On C2 (1 M x 512 B ASCII) and the 500 k Zipf share, with a Tekken-like set of special strings on the context (control tokens and
<SPECIAL_n> fillers: every string begins with "<" or "["), three texts each:
  none     no "<" and no "[" in the text: what a caller who turns the pass on "just in case" pays;
  markers  "[INST]" / "[/INST]" every ~200 bytes and one "</s>" at the end of every document;
  html     "<" at 2 % of the bytes and no ">" anywhere: every one of them is walked into the trie, none is a match.
Per text: the GPU time of tk_specials_split_device (HIP events around the call, warm, median and min of --steps) and inside it the
candidate, chain, part-table and compaction stages as the library's own events see them (tk_last_specials_ms); split + encode + join
(tk_encode_batch_device_parsed) against plain tk_encode_batch_device on the same text in the same run; the compaction kernel
against a device-to-device copy of the bytes it writes, in the same run, as its fraction of that copy's bandwidth.
The baseline of the whole feature is what a user writes without it, timed here on the first --baseline-docs documents of the
markers text: `re` over the documents on the host, the parts rebuilt, tk_encode_parts_join -- beside tk_encode_batch_parsed on the
same documents, checked equal first.

    python tools/specials_time.py [--steps 10] [--warmup 2] [--shapes C2,zipf] [--baseline-docs 100000] [--out profiles/specials_time.json]
"""
import argparse
import importlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}
NAMED = [b"<unk>", b"<s>", b"</s>", b"[INST]", b"[/INST]", b"[PREFIX]", b"[SUFFIX]", b"[MIDDLE]"]
EVERY = 200


def strings(n):
    return (NAMED + [b"<SPECIAL_%d>" % i for i in range(len(NAMED), n)])[:n]


def scrub(data, also=b""):
    out = data.copy()
    for ch in b"<[" + also:
        out[out == ch] = ord("(")
    return out


def with_markers(data, offs):
    """[INST] / [/INST] in turn every EVERY bytes of a document, </s> at its end."""
    lens = np.diff(offs).astype(np.int64)
    per = np.maximum((lens - 1) // EVERY, 0)
    doc = np.repeat(np.arange(len(lens)), per)
    k = np.arange(len(doc)) - np.repeat(np.cumsum(per) - per, per)
    at = offs[:-1].astype(np.int64)[doc] + (k + 1) * EVERY
    pos, val = [], []
    for sel, s in ((k % 2 == 0, b"[INST]"), (k % 2 == 1, b"[/INST]"), (None, b"</s>")):
        p = offs[1:].astype(np.int64) if sel is None else at[sel]
        pos.append(np.repeat(p, len(s)))
        val.append(np.tile(np.frombuffer(s, np.uint8), len(p)))
    pos, val = np.concatenate(pos), np.concatenate(val)
    order = np.argsort(pos, kind="stable")
    pos, val = pos[order], val[order]
    out = np.insert(data, pos, val)
    added = np.searchsorted(pos, offs.astype(np.int64), side="right")      # (a document's </s> is in front of its end)
    added[0] = 0
    return out, (offs.astype(np.int64) + added).astype(np.uint64)


def with_html(data, seed=7):
    out = scrub(data, b">")
    rng = np.random.default_rng(seed)
    out[rng.random(len(out)) < 0.02] = ord("<")
    return out


def by_hand(tk, eng, pattern, ids_of, docs, bos, eos):
    """What a user writes without the pass: re over every document, the parts rebuilt, encode_parts_join."""
    texts, ctrl, conv = [], [], [0]
    for d in docs:
        ctrl.append(bos)
        last = 0
        for m in pattern.finditer(d):
            texts.append(d[last:m.start()])
            ctrl.append(ids_of[m.group()])
            last = m.end()
        texts.append(d[last:])
        texts.append(b"")
        ctrl.append(eos)
        conv.append(len(ctrl))
    data, offs = tk.pack_docs(texts)
    return eng.encode_parts_join(data, offs, np.array(ctrl, np.uint32), None, np.array(conv, np.uint64), flags=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--baseline-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specials_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    sset = strings(ns)
    eng.set_special_tokens(sset)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/specials_time.py", "steps": args.steps, "warmup": args.warmup, "n_strings": ns, "marker_every": EVERY}
    try:
        with open(os.path.join(ROOT, "tekken-rs_amd", "BUILD_INFO.json")) as f:
            out["build"] = json.load(f).get("git")
    except OSError:
        pass

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    med = lambda x: round(float(np.median(x)), 4)
    for name in args.shapes.split(","):
        kind, n_docs, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        res = {"n_docs": n_docs}
        for case in ("none", "markers", "html"):
            if case == "markers":
                text, toffs = with_markers(scrub(data), offs)
            else:
                text, toffs = (scrub(data) if case == "none" else with_html(data)), offs
            n_bytes = len(text)
            d_bytes = torch.from_numpy(text).cuda()
            d_offs = torch.from_numpy(toffs.astype(np.int64)).cuda()
            a = (d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes)
            t_split, t_st, t_parsed, t_plain, t_copy = [], [], [], [], []
            for k in range(args.warmup + args.steps):
                ms_s, r = timed(lambda: eng.split_specials_device(*a, None, tk.SPECIALS_BOS | tk.SPECIALS_EOS, 0, sp))
                st = eng.last_specials_ms()
                ms_p, (parts, j) = timed(lambda: eng.encode_batch_device_parsed(*a, True, True, None, stream=sp))
                ms_e, enc = timed(lambda: eng.encode_batch_device(*a, True, True, sp))
                dst = torch.empty(max(parts.n_bytes, 1), dtype=torch.uint8, device="cuda")
                ms_c, _ = timed(lambda: dst.copy_(d_bytes[:dst.numel()]))
                if k >= args.warmup:
                    t_split.append(ms_s); t_st.append(st); t_parsed.append(ms_p); t_plain.append(ms_e); t_copy.append(ms_c)
                del dst
            st = np.median(np.array(t_st), axis=0)
            rec = {"n_bytes": n_bytes, "n_matches": r.n_matches, "n_removed": r.n_removed, "n_parts": r.n_parts,
                   "split_ms": med(t_split), "split_min_ms": round(float(np.min(t_split)), 4),
                   "candidates_ms": round(float(st[0]), 4), "chain_ms": round(float(st[1]), 4), "tables_ms": round(float(st[2]), 4),
                   "compact_ms": round(float(st[3]), 4), "candidates_gbs": round(n_bytes / (float(st[0]) * 1e-3) / 1e9, 1) if st[0] > 0 else None,
                   "parsed_ms": med(t_parsed), "plain_encode_ms": med(t_plain),
                   "parsed_over_plain": round(float(np.median(t_parsed)) / float(np.median(t_plain)), 3), "n_ids_parsed": j.n_ids, "n_ids_plain": enc[2]}
            if r.n_removed:
                rec.update({"d2d_copy_ms": med(t_copy), "compact_frac_of_copy": round(float(np.median(t_copy)) / float(st[3]), 3)})
            if case == "markers":
                nb = min(args.baseline_docs, n_docs)
                docs = [text[int(toffs[d]):int(toffs[d + 1])].tobytes() for d in range(nb)]
                pattern = re.compile(b"|".join(re.escape(s) for s in sorted(sset, key=len, reverse=True)))
                ids_of = {s: i for i, s in reversed(list(enumerate(sset)))}
                sub, soffs = tk.pack_docs(docs)
                want = by_hand(tk, eng, pattern, ids_of, docs, bos, eos)
                got = eng.encode_batch_parsed(sub, soffs, True, True)
                assert np.array_equal(want["ids"], got["ids"]) and np.array_equal(want["offsets"], got["offsets"])
                t_hand, t_host = [], []
                for _ in range(3):
                    t0 = time.perf_counter(); by_hand(tk, eng, pattern, ids_of, docs, bos, eos); t_hand.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter(); eng.encode_batch_parsed(sub, soffs, True, True); t_host.append((time.perf_counter() - t0) * 1e3)
                rec["baseline"] = {"n_docs": nb, "n_bytes": len(sub), "by_hand_ms": med(t_hand), "encode_batch_parsed_ms": med(t_host),
                                   "by_hand_over_parsed": round(float(np.median(t_hand)) / float(np.median(t_host)), 1)}
                del docs
            res[case] = rec
            print("%s %s: %s" % (name, case, json.dumps(rec)), file=sys.stderr, flush=True)
            del d_bytes, d_offs
            torch.cuda.empty_cache()
        out[name] = res
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
