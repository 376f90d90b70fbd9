"""Time the words pass (csrc/tk_words.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/words_time.json.

On encode's own ids for C2 (1 M x 512 B ASCII) and for the 500 k Zipf share: the GPU time of tk_words_from_ids_device with and
without TK_WORDS_FIRST and with TK_WORDS_CHECK_ALIGNED, HIP events around the call, warm, median and min of --steps, and inside it
the four stages as the library's own events see them (tk_last_words_ms: the split launch, the words kernel, the scan, the
word_first kernel).  The words kernel as a fraction of 6.3 TB/s counts 9 bytes an id (4 read, 4 written, 1 gathered).  Beside it,
in the same process:
  (a) the byte-spans call on the same ids (tk_token_spans_device without checks: its kernel, 12 algorithmic bytes an id, plus the
      memset, the 32-byte read and the wait that end the call -- the library has no event around that kernel alone), and the
      words kernel over it;
  (b) the same definition composed from torch on the same device (the flags of tk_split_batch uploaded once,
      flags[doc_start + span_start], two cumsums made per document by subtracting their value at the document's first id),
      checked equal to the pass before anything is timed.

    python tools/words_time.py [--steps 20] [--warmup 3] [--torch-steps 3] [--shapes C2,zipf] [--out profiles/words_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

HBM_TBS = 6.3
SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}


def torch_today(torch, ids, oo, offs, flags, tok_len, ns):
    """The definition from torch: -> (word_ids int32 [-1: None], doc_words int64, word_first int32)."""
    dev = ids.device
    D = oo.numel() - 1
    idl = ids.to(torch.int64)
    lens = torch.where(idl >= ns, tok_len[(idl - ns).clamp(min=0)], torch.zeros_like(idl))
    cs = torch.zeros(idl.numel() + 1, dtype=torch.int64, device=dev)
    cs[1:] = torch.cumsum(lens, 0)
    doc = torch.repeat_interleave(torch.arange(D, device=dev), oo[1:] - oo[:-1])
    st = cs[:-1] - cs[oo[:-1]][doc]
    body = (lens > 0) & (st < (offs[1:] - offs[:-1])[doc])
    pos = (offs[:-1][doc] + st).clamp(max=max(flags.numel() - 1, 0))
    b = body & (flags[pos] != 0)
    cb = torch.zeros(idl.numel() + 1, dtype=torch.int64, device=dev)
    cb[1:] = torch.cumsum(b.to(torch.int64), 0)
    word = cb[1:] - cb[oo[:-1]][doc] - 1
    at = torch.nonzero(b).squeeze(1)
    return torch.where(lens > 0, word, torch.full_like(word, -1)).to(torch.int32), cb[oo], (at - oo[:-1][doc[at]]).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "words_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    tok_len = torch.tensor([len(t) for t in toks], dtype=torch.int64).cuda()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/words_time.py", "steps": args.steps, "warmup": args.warmup, "torch_steps": args.torch_steps, "hbm_tbs": HBM_TBS}
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
    frac = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / (HBM_TBS * 1e12), 3) if ms > 0 else None
    for name in args.shapes.split(","):
        kind, n_docs, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        # the flags of the composition from torch: the host entry of the same split, once
        h_flags = np.zeros(max(n_bytes, 1), np.uint8)
        rc = tk.lib().tk_split_batch(eng._h, data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                     n_docs, h_flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc == 0
        flags = torch.from_numpy(h_flags).cuda()
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        call = lambda fl=tk.WORDS_FIRST, ck=0: eng.words_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, d_bytes.data_ptr(),
                                                                           d_offs.data_ptr(), n_bytes, fl, ck, sp)
        # the pass and the composition from torch compute the same thing
        r, ref = call(ck=tk.WORDS_CHECK_ALIGNED), torch_today(torch, ids, oo, d_offs, flags, tok_len, ns)
        v = r.views()
        for got, want in zip(v, ref):
            assert torch.equal(torch.as_tensor(got, device="cuda"), want)
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids, "n_words": r.n_words, "ids_per_word": round(n_ids / max(r.n_words, 1), 3)}
        del ref, v
        for label, fl, ck in (("first", tk.WORDS_FIRST, 0), ("plain", 0, 0), ("first_checked", tk.WORDS_FIRST, tk.WORDS_CHECK_ALIGNED)):
            t_k, t_st = [], []
            for k in range(args.warmup + args.steps):
                ms_k, r = timed(lambda: call(fl, ck))
                if k >= args.warmup:
                    t_k.append(ms_k)
                    t_st.append(eng.last_words_ms())
            st = np.median(np.array(t_st), axis=0)
            res[label] = {"call_ms": med(t_k), "call_min_ms": round(float(np.min(t_k)), 4), "split_ms": round(float(st[0]), 4),
                          "words_kernel_ms": round(float(st[1]), 4), "scan_ms": round(float(st[2]), 4), "word_first_ms": round(float(st[3]), 4),
                          "words_kernel_frac_hbm": frac(9 * n_ids, float(st[1])), "split_over_call": round(float(st[0]) / float(np.median(t_k)), 3)}
        t_sp = []
        for k in range(args.warmup + args.steps):
            ms_s, _ = timed(lambda: eng.token_spans_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, 0, 0, 0, sp))
            if k >= args.warmup:
                t_sp.append(ms_s)
        res["spans_call_ms"] = med(t_sp)
        res["spans_call_min_ms"] = round(float(np.min(t_sp)), 4)
        res["spans_call_frac_hbm"] = frac(12 * n_ids, float(np.median(t_sp)))
        res["words_kernel_over_spans_call"] = round(res["plain"]["words_kernel_ms"] / float(np.median(t_sp)), 3)
        t_torch = []
        for k in range(1 + args.torch_steps):
            ms_t, ref = timed(lambda: torch_today(torch, ids, oo, d_offs, flags, tok_len, ns))
            del ref
            if k:
                t_torch.append(ms_t)
        res["torch_ms"] = med(t_torch)
        res["torch_over_call"] = round(float(np.median(t_torch)) / res["first"]["call_ms"], 1)
        out[name] = res
        del ids, oo, flags, d_bytes, d_offs
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
