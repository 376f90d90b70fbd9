"""Time the window pass (csrc/tk_window.hip) on one MI355X; prints ONE JSON line.

For the 500 k Zipf share (max_length 512, stride 128) and C2 (1 M x 512 B ASCII; max_length 64, stride 16, so that most documents
split), fixed rows, int32 and int64, with and without mask: the GPU time of tk_window_from_ids_device over encode's own ids
against what a user can do without it -- a torch composition of the same definition over the ragged device views (a per-document
window count, a cumulative sum, a [W, L] int64 index, a gather and a where; BOS / EOS repeated, h = t = 1) --, alternating the two
in one process, HIP events around each, warm, median and min; the algorithmic HBM bytes of the pass and their fraction of
6.3 TB/s; the dense kernel's time in the same run on a tensor of the same W * L (the windows as ragged rows: the sibling to read
the pass against); and the same-box wall time of one step of tk_encode_batch_device_ex against tk_encode_batch_device_window
(interleaved).

    python tools/window_time.py [--steps 20] [--warmup 3] [--shapes zipf,C2]
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

HBM_TBS = 6.3
SHAPES = {"zipf": ("zipf", 500_000, 0, dict(max_length=512, stride=128)),
          "C2": ("ascii", 1_000_000, 512, dict(max_length=64, stride=16))}
PAD = 11


def torch_windows(torch, ids, oo, T, s, pad_id, dtype, want_mask):
    """The definition over the ragged views, as well as torch allows (h = t = 1, fixed rows of T): the window count of every
    document, their cumulative sum (one read: W sizes everything), the document and number of every window, one int64 [W, T]
    index, one gather, one where."""
    h = t = 1
    c = T - h - t
    step = c - s
    D = oo.numel() - 1
    start = oo[:-1]
    n = oo[1:] - start
    w = torch.where(n > T, 1 + (n - T + step - 1) // step, torch.ones_like(n))
    dw = torch.zeros(D + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(w, 0, out=dw[1:])
    W = int(dw[-1])
    doc = torch.repeat_interleave(torch.arange(D, device=ids.device), w, output_size=W)
    k = torch.arange(W, device=ids.device) - dw[doc]
    nn = n[doc]
    split = nn > T
    lo = k * step                                      # the body index of the window's first body id
    blen = torch.where(split, torch.clamp(nn - (h + t) - lo, max=c), nn)
    hh = torch.where(split, h, 0)
    hb = hh + blen
    length = hb + torch.where(split, t, 0)
    col = torch.arange(T, device=ids.device, dtype=torch.int64)[None, :]
    src = torch.where(col < hh[:, None], col, torch.where(col < hb[:, None], col + lo[:, None], col + (nn - length)[:, None]))
    kept = col < length[:, None]
    idx = (start[doc][:, None] + src).clamp_(max=ids.numel() - 1)
    out = torch.where(kept, ids[idx].to(dtype), torch.full((), pad_id, dtype=dtype, device=ids.device))
    mask = kept.to(torch.uint8) if want_mask else None
    return out, mask, length.to(torch.int32), doc.to(torch.int32), torch.minimum(h + lo, nn).to(torch.int32), dw, (n > T).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="zipf,C2")
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/window_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS}
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

    for name in args.shapes.split(","):
        kind, n_docs, doc_len, o = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        print("%s: %d documents, %d bytes" % (name, n_docs, n_bytes), file=sys.stderr, flush=True)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        T, s = o["max_length"], o["stride"]
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids, "max_length": T, "stride": s, "fixed": True}
        rows = None
        for label, fl in (("i32_mask", tk.WINDOW_MASK), ("i32", 0), ("i64_mask", tk.WINDOW_I64 | tk.WINDOW_MASK), ("i64", tk.WINDOW_I64)):
            t_k, t_t = [], []
            tdt = torch.int64 if fl & tk.WINDOW_I64 else torch.int32
            for k in range(args.warmup + args.steps):
                ms_k, r = timed(lambda: eng.window_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, T, s, 0, PAD, 1, 1,
                                                                   tk.WINDOW_FIXED | fl, 0, sp))
                ms_t, ref = timed(lambda: torch_windows(torch, ids, oo, T, s, PAD, tdt, bool(fl & tk.WINDOW_MASK)))
                if k == 0:    # the two sides compute the same thing
                    v = [None if x is None else torch.as_tensor(x, device="cuda") for x in r.views()]
                    assert r.n_windows == ref[0].shape[0] and r.row_len == T and int(ref[6]) == r.n_split
                    assert torch.equal(v[0], ref[0]) and (ref[1] is None or torch.equal(v[1], ref[1]))
                    assert torch.equal(v[2], ref[2]) and torch.equal(v[3], ref[3]) and torch.equal(v[4], ref[4]) and torch.equal(v[5], ref[5])
                    if rows is None:      # the windows as ragged rows: what the dense kernel makes the same tensor from
                        lens = ref[2].to(torch.int64)
                        roo = torch.zeros(r.n_windows + 1, dtype=torch.int64, device="cuda")
                        torch.cumsum(lens, 0, out=roo[1:])
                        rows = (ref[0][torch.arange(T, device="cuda")[None, :] < lens[:, None]].to(torch.int32).contiguous(),
                                roo, ref[0].to(torch.int32) if tdt == torch.int64 else ref[0].clone())
                del ref
                if k >= args.warmup:
                    t_k.append(ms_k)
                    t_t.append(ms_t)
            W, L = r.n_windows, r.row_len
            esz = 8 if fl & tk.WINDOW_I64 else 4
            # every id read once, the offsets, every element (and mask byte) written once, the three per-window words, doc_windows
            alg = 4 * n_ids + 8 * (n_docs + 1) + W * L * esz + (W * L if fl & tk.WINDOW_MASK else 0) + 12 * W + 8 * (n_docs + 1)
            # the dense kernel on the same tensor, in the same run
            rid, roo, want = rows
            t_d = []
            dfl = tk.DENSE_FIXED | (tk.DENSE_I64 if fl & tk.WINDOW_I64 else 0) | (tk.DENSE_MASK if fl & tk.WINDOW_MASK else 0)
            for k in range(args.warmup + args.steps):
                ms_d, rd = timed(lambda: eng.dense_from_ids_device(rid.data_ptr(), roo.data_ptr(), W, rid.numel(), T, 0, PAD, 1, 1, dfl, sp))
                if k == 0:
                    assert rd.row_len == L and torch.equal(torch.as_tensor(rd.views()[0], device="cuda").to(torch.int32), want)
                if k >= args.warmup:
                    t_d.append(ms_d)
            ms, ms_d = float(np.median(t_k)), float(np.median(t_d))
            print("%s %s: %.3f ms, torch %.3f ms, dense %.3f ms" % (name, label, ms, float(np.median(t_t)), ms_d), file=sys.stderr, flush=True)
            res[label] = {"n_windows": W, "row_len": L, "n_split": r.n_split, "kernel_ms": round(ms, 4), "kernel_min_ms": round(float(np.min(t_k)), 4),
                          "torch_ms": round(float(np.median(t_t)), 4), "torch_min_ms": round(float(np.min(t_t)), 4),
                          "torch_over_kernel": round(float(np.median(t_t)) / ms, 2), "kernel_not_slower": bool(ms <= float(np.median(t_t))),
                          "dense_same_size_ms": round(ms_d, 4), "window_over_dense": round(ms / ms_d, 2), "alg_bytes": alg,
                          "tb_s": round(alg / (ms * 1e-3) / 1e12, 3), "frac_hbm": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}
        del rows, rid, roo, want
        # one step of each entry, interleaved (the call drains the stream: wall time is the step)
        t_enc, t_wn = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp, checks=0)
            t1 = time.perf_counter()
            eng.encode_batch_device_window(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, T, s, True, True, 0, PAD,
                                           tk.WINDOW_FIXED | tk.WINDOW_MASK, 0, sp)
            t2 = time.perf_counter()
            if k >= args.warmup:
                t_enc.append((t1 - t0) * 1e3)
                t_wn.append((t2 - t1) * 1e3)
        res["step_encode_ms"] = round(float(np.median(t_enc)), 3)
        res["step_encode_window_ms"] = round(float(np.median(t_wn)), 3)
        res["step_delta_ms"] = round(res["step_encode_window_ms"] - res["step_encode_ms"], 3)
        out[name] = res
        del d_bytes, d_offs, ids, oo
        torch.cuda.empty_cache()
    eng.close()
    # the requirement: the kernel is not slower than the torch composition on any measured shape
    out["kernel_not_slower_everywhere"] = all(v["kernel_not_slower"] for r in out.values() if isinstance(r, dict)
                                              for v in r.values() if isinstance(v, dict) and "kernel_not_slower" in v)
    print(json.dumps(out))
    if not out["kernel_not_slower_everywhere"]:
        sys.exit("tools/window_time.py: the kernel is slower than the torch composition on a measured shape")


if __name__ == "__main__":
    main()
