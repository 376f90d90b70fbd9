"""Time the fill-in-the-middle pass (csrc/tk_fim.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/fim_time.json.

On C2 (1 M x 512 B ASCII) and the 500 k Zipf share, Mistral's format (suffix first, no middle token) at rate 0.5, HIP events, warm,
the median of --steps:
  text     tk_fim_split_device: the call, and inside it the cut and permute kernels as the library's own events see them
           (tk_last_fim_ms); the permute kernel against a device-to-device copy of the same bytes in the same run, as its fraction
           of that copy's bandwidth; split + encode + join (tk_encode_batch_device_fim) against plain tk_encode_batch_device of the
           same batch.
  ids      tk_fim_split_ids_device over the ids of the same batch (BOS / EOS stored: head = tail = 1) against the same definition
           composed from torch indexing on the same device, the cuts given to it for nothing, checked equal first.
The baseline of the whole feature is what a user writes without it, timed on the first --baseline-docs documents: slice the
documents on the host at the same cuts, rebuild the parts, tk_encode_parts_join -- beside tk_encode_batch_fim on the same
documents, checked equal first.

    python tools/fim_time.py [--steps 20] [--warmup 2] [--shapes C2,zipf] [--baseline-docs 100000] [--out profiles/fim_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}
PREFIX, SUFFIX = 5, 6           # ids below num_special: what they are called does not matter to the timing


def torch_fim_ids(torch, ids, offs, cuts, mode, head, tail):
    """The definition's units output composed from torch indexing: one gather index over all ids."""
    lens = offs[1:] - offs[:-1]
    doc = torch.repeat_interleave(torch.arange(len(lens), device=ids.device), lens)
    pos = torch.arange(len(ids), device=ids.device)
    b = pos - offs[:-1][doc] - head                     # the position in the body
    m = mode.to(torch.int64)[doc]
    lo, hi = cuts[:, 0][doc], cuts[:, 1][doc]
    n = lens[doc] - head - tail
    inside = (m != 0) & (b >= 0) & (b < n)
    spm = m == 2
    e1 = torch.where(spm, n - hi, lo)
    e2 = e1 + torch.where(spm, lo, n - hi)
    shift = torch.where(b < e1, torch.where(spm, hi, torch.zeros_like(hi)),
                        torch.where(b < e2, torch.where(spm, hi - n, hi - lo), hi - n))
    return ids[pos + torch.where(inside, shift, torch.zeros_like(shift))]


def by_hand(tk, eng, docs, cuts, mode, bos, eos):
    """What a user writes without the pass: slice every document, rebuild the parts, encode_parts_join."""
    none = tk.JOIN_NONE
    texts, ctrl, conv = [], [], [0]
    for d, (lo, hi), m in zip(docs, cuts, mode):
        if m:
            texts += [b"", d[hi:], d[:lo], d[lo:hi], b""]
            ctrl += [bos, SUFFIX, PREFIX, none, eos]
        else:
            texts += [b"", d, b"", b"", b""]
            ctrl += [bos, none, none, none, eos]
        conv.append(len(ctrl))
    data, offs = tk.pack_docs(texts)
    return eng.encode_parts_join(data, offs, np.array(ctrl, np.uint32), None, np.array(conv, np.uint64), flags=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--baseline-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fim_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    one = 1 << 32
    text_opts = dict(rate_q32=one // 2, spm_q32=one, seed=1, prefix_id=PREFIX, suffix_id=SUFFIX, flags=tk.FIM_SNAP | tk.FIM_BOS | tk.FIM_EOS)
    ids_opts = dict(rate_q32=one // 2, spm_q32=one, seed=1, prefix_id=PREFIX, suffix_id=SUFFIX, head=1, tail=1)
    out = {"tool": "tools/fim_time.py", "steps": args.steps, "warmup": args.warmup, "rate": 0.5, "format": "mistral",
           "tile_bytes": int(tk.lib().tk_fim_tile(1)), "tile_ids": int(tk.lib().tk_fim_tile(4))}
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
        n_bytes = len(data)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        a = (d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes)
        # ---- text
        t_split, t_st, t_fim, t_plain, t_copy = [], [], [], [], []
        dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
        for k in range(args.warmup + args.steps):
            ms_s, r = timed(lambda: eng.fim_split_device(*a, stream=sp, **text_opts))
            st = eng.last_fim_ms()
            ms_f, (parts, j) = timed(lambda: eng.encode_batch_device_fim(*a, stream=sp, **text_opts))
            ms_e, enc = timed(lambda: eng.encode_batch_device(*a, True, True, sp))
            ms_c, _ = timed(lambda: dst.copy_(d_bytes))
            if k >= args.warmup:
                t_split.append(ms_s); t_st.append(st); t_fim.append(ms_f); t_plain.append(ms_e); t_copy.append(ms_c)
        del dst
        st = np.median(np.array(t_st), axis=0)
        rec = {"n_docs": n_docs, "n_bytes": n_bytes, "n_transformed": r.n_transformed, "n_skipped": r.n_skipped,
               "text": {"split_ms": med(t_split), "split_min_ms": round(float(np.min(t_split)), 4), "cut_ms": round(float(st[0]), 4),
                        "permute_ms": round(float(st[1]), 4), "permute_gbs": round(2 * n_bytes / (float(st[1]) * 1e-3) / 1e9, 1),
                        "d2d_copy_ms": med(t_copy), "permute_frac_of_copy": round(float(np.median(t_copy)) / float(st[1]), 3),
                        "fim_encode_ms": med(t_fim), "plain_encode_ms": med(t_plain),
                        "fim_over_plain": round(float(np.median(t_fim)) / float(np.median(t_plain)), 3), "n_ids_fim": j.n_ids, "n_ids_plain": enc[2]}}
        # ---- ids: the batch's own ids, BOS and EOS stored
        p_ids, p_oo, n_ids = eng.encode_batch_device(*a, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        b = (ids.data_ptr(), oo.data_ptr(), n_docs, n_ids)
        f = eng.fim_split_ids_device(*b, stream=sp, **ids_opts)
        v = f.views()
        got = torch.as_tensor(v[0], device="cuda").clone()
        cuts = torch.as_tensor(v[6], device="cuda").clone()
        mode = torch.as_tensor(v[7], device="cuda").clone()
        assert torch.equal(torch_fim_ids(torch, ids, oo, cuts, mode, 1, 1), got)
        t_ids, t_ist, t_torch, t_icopy = [], [], [], []
        dst = torch.empty_like(ids)
        for k in range(args.warmup + args.steps):
            ms_i, f = timed(lambda: eng.fim_split_ids_device(*b, stream=sp, **ids_opts))
            ist = eng.last_fim_ms()
            ms_t, _ = timed(lambda: torch_fim_ids(torch, ids, oo, cuts, mode, 1, 1))
            ms_c, _ = timed(lambda: dst.copy_(ids))
            if k >= args.warmup:
                t_ids.append(ms_i); t_ist.append(ist); t_torch.append(ms_t); t_icopy.append(ms_c)
        ist = np.median(np.array(t_ist), axis=0)
        rec["ids"] = {"n_ids": n_ids, "n_transformed": f.n_transformed, "split_ms": med(t_ids), "cut_ms": round(float(ist[0]), 4),
                      "permute_ms": round(float(ist[1]), 4), "d2d_copy_ms": med(t_icopy),
                      "permute_frac_of_copy": round(float(np.median(t_icopy)) / float(ist[1]), 3), "torch_ms": med(t_torch),
                      "torch_over_split": round(float(np.median(t_torch)) / float(np.median(t_ids)), 1)}
        del ids, oo, got, cuts, mode, dst
        # ---- host to host against the loop a user writes today
        nb = min(args.baseline_docs, n_docs)
        docs = [data[int(offs[d]):int(offs[d + 1])].tobytes() for d in range(nb)]
        sub, soffs = tk.pack_docs(docs)
        got, parts = eng.encode_batch_fim(sub, soffs, return_parts=True, **text_opts)
        want = by_hand(tk, eng, docs, parts["cuts"].tolist(), parts["mode"].tolist(), bos, eos)
        assert np.array_equal(want["ids"], got["ids"]) and np.array_equal(want["offsets"], got["offsets"])
        c, m = parts["cuts"].tolist(), parts["mode"].tolist()
        t_hand, t_host = [], []
        for _ in range(3):
            t0 = time.perf_counter(); by_hand(tk, eng, docs, c, m, bos, eos); t_hand.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); eng.encode_batch_fim(sub, soffs, **text_opts); t_host.append((time.perf_counter() - t0) * 1e3)
        rec["baseline"] = {"n_docs": nb, "n_bytes": len(sub), "by_hand_ms": med(t_hand), "encode_batch_fim_ms": med(t_host),
                           "by_hand_over_fim": round(float(np.median(t_hand)) / float(np.median(t_host)), 1)}
        del docs
        out[name] = rec
        print("%s: %s" % (name, json.dumps(rec)), file=sys.stderr, flush=True)
        del d_bytes, d_offs
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
