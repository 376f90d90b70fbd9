"""tests/test_gpu_merge_one.py: the single merge launch of the folded tail (tk_merge_all_kernel: the narrow loop, then the wide loops
on the same LDS) against the two merge kernels of the three-kernel form (TK_TAIL_FOLD=0), id for id, with the memo of merged pieces
forced on (two calls: the second one probes the table and logs into it) and off.  A process of its own: the knobs are read from the
environment when a context is created, the one-launch small path is switched off for the whole process (TK_NO_SMALL_PATH), and a
fault ends here.  It stops at the first difference.

  python tests/merge_one_worker.py <out_path>        -> "ok <comparisons>" or what went wrong"""
import importlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

MEMO = {"on": {"TK_MEMO_LOG2": "16", "TK_MEMO_POLICY": "always"}, "off": {"TK_MEMO_LOG2": "0"}}
FORMS = {"two kernels": {"TK_TAIL_FOLD": "0"}, "one kernel": {"TK_TAIL_FOLD": "1"}, "folded, two kernels": {"TK_TAIL_FOLD": "1", "TK_TAIL_FOLD_MERGE": "0"},
         "one kernel behind the three-kernel scan": {"TK_TAIL_FOLD_MISS_MAX": "0", "TK_TAIL_FOLD_DOC_MAX": "0"}}


def engine(tk, vocab, env):
    for k in ("TK_MEMO_LOG2", "TK_MEMO_POLICY", "TK_TAIL_FOLD", "TK_TAIL_FOLD_MERGE", "TK_TAIL_FOLD_MISS_MAX", "TK_TAIL_FOLD_DOC_MAX"):
        os.environ.pop(k, None)
    os.environ.update(env)
    return tk.Engine(*vocab, device=0)


def main():
    out_path = sys.argv[1]
    verdict, n, where = None, 0, "loading"
    try:
        tk = importlib.import_module("tekken-rs_amd")
        import corpus
        import synth_vocab
        golden = []
        with open(os.path.join(ROOT, "tests", "golden", "merge_vectors_hf.json")) as f:
            g = json.load(f)
        golden.append(("merge_vectors_hf.json", ([bytes.fromhex(t) for t in g["tokens_hex"]], g["num_special"], 1, 2),
                       [bytes.fromhex(v["text_hex"]) for v in g["vectors"]], [v["ids"] for v in g["vectors"]]))
        for name in ("merge_vectors.json",):
            with open(os.path.join(ROOT, "tests", "golden", name)) as f:
                g = json.load(f)
            for v in g["vocabs"]:
                docs = [bytes.fromhex(p) for p, _ in v["pieces"]] + [t.encode("utf-8") for t, _ in v["texts"]]
                exp = [ids for _, ids in v["pieces"]] + [ids for _, ids in v["texts"]]
                golden.append(("%s:%s" % (name, v["name"]), ([bytes.fromhex(t) for t in v["tokens_hex"]], v["num_special"], 1, 2), docs, exp))
        for memo, menv in MEMO.items():
            for name, vocab, docs, exp in golden:
                for form, fenv in FORMS.items():
                    where = "%s, memo %s, %s" % (name, memo, form)
                    e = engine(tk, vocab, dict(menv, **fenv))
                    for call in (1, 2):
                        got = e.encode_docs(docs, False, False)
                        for d, x, y in zip(docs, exp, got):
                            assert x == y, "call %d: %r: expected %r, got %r" % (call, d[:60], x[:12], y[:12])
                    e.close()
                    n += 1
        # a small batch with pieces of every class (mixed UTF-8: the wide classes are busy; Zipf lengths: long pieces, handed-back
        # documents) on the bench vocabulary: the forms against each other
        toks, ns, bos, eos = synth_vocab.load_tokens(synth_vocab.ensure_default())
        for kind, nd, dl, sd in (("mixed", 300, 2048, 2), ("zipf", 1500, 0, 4), ("ascii", 2000, 512, 1)):
            data, offs = corpus.generate(kind, nd, dl, seed=corpus.BASE_SEED + sd)
            for memo, menv in MEMO.items():
                ref = None
                for form, fenv in FORMS.items():
                    where = "%s batch, memo %s, %s" % (kind, memo, form)
                    e = engine(tk, (toks, ns, bos, eos), dict(menv, **fenv))
                    for call in (1, 2):
                        ids, oo = e.encode_batch(data, offs, True, True)
                        if ref is None:
                            ref = (ids.copy(), oo.copy())
                        assert np.array_equal(oo, ref[1]), "call %d: the output offsets differ" % call
                        assert np.array_equal(ids, ref[0]), "call %d: id %d differs" % (call, int(np.flatnonzero(ids != ref[0])[0]))
                    e.close()
                    n += 1
        verdict = "ok %d" % n
    except BaseException as e:  # noqa: BLE001
        verdict = "FAILED at %s:\n%s" % (where, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-2500:])
    with open(out_path, "w") as f:
        f.write(verdict)
    return 0 if verdict.startswith("ok") else 1


if __name__ == "__main__":
    sys.exit(main())
