"""Time the chunk pass (csrc/tk_chunk.hip) on one MI355X; prints ONE JSON line and writes it to profiles/chunk_time.json.

For C2 (1 M x 512 B ASCII; max_length 64, min_length 32, overlap 8) and the 500 k Zipf share (max_length 512, min_length 256,
overlap 64), fixed int32 rows with mask, BOS / EOS repeated (h = t = 1), over encode's own ids, spans and tk_chunk_levels_device's
levels, warm, median and min of `--steps` calls:
  * the three stage times of tk_last_chunk_ms (levels | the two walks and the scan | fill) and the whole tk_chunk_from_ids_device
    call (HIP events around it);
  * in the same run, alternating, tk_window_from_ids_device on the same ids at stride = overlap (the whole call: it keeps no stage
    times), and both per byte of rows written (ids and mask): the fill kernel is the window kernel with one more load a row;
  * what a user writes without the pass: ids' offsets and levels copied to the host and the definition's greedy loop in numpy over
    the documents that need splitting (the first `--host-docs` documents; the cuts are checked against the pass's).

    python tools/chunk_time.py [--steps 20] [--warmup 3] [--shapes C2,zipf] [--host-docs 100000] [--out profiles/chunk_time.json]
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

SHAPES = {"C2": ("ascii", 1_000_000, 512, dict(max_length=64, min_length=32, overlap=8)),
          "zipf": ("zipf", 500_000, 0, dict(max_length=512, min_length=256, overlap=64))}
PAD = 11


def host_walk(oo, lev, T, m, o, h, t, n_docs):
    """The definition's greedy chain in numpy over the split documents among the first n_docs -> (window_start of their chunks, cuts)."""
    c = T - h - t
    starts, n_cuts = [], 0
    for d in np.nonzero(np.diff(oo[:n_docs + 1]) > T)[0].tolist():
        p, n = int(oo[d]), int(oo[d + 1] - oo[d])
        b = n - h - t
        L = lev[p + h:p + h + b]
        a = 0
        while True:
            starts.append(h + a)
            if b - a <= c:
                break
            cand = L[a + m:a + c + 1]
            e = a + m + len(cand) - 1 - int(np.argmax(cand[::-1] == cand.max()))
            n_cuts += 1
            lo = max(a + 1, e - o)
            front = L[lo:e]
            words = np.nonzero(front >= 2)[0]
            if len(words):
                a = lo + int(words[0])
            else:
                tokens = np.nonzero(front >= 1)[0]
                a = lo + int(tokens[0]) if len(tokens) else e
    return np.array(starts, np.int64), n_cuts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--host-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/chunk_time.py", "steps": args.steps, "warmup": args.warmup}
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

    def med(x):
        return round(float(np.median(x)), 4)

    for name in args.shapes.split(","):
        kind, n_docs, doc_len, o = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        print("%s: %d documents, %d bytes" % (name, n_docs, n_bytes), file=sys.stderr, flush=True)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, p_sp, n_ids = eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, stream=sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        spans = torch.as_tensor(tk.DeviceView(p_sp, 2 * n_ids, "<i4"), device="cuda").clone()
        torch.cuda.synchronize()
        T, m, ov = o["max_length"], o["min_length"], o["overlap"]
        cfl, wfl = tk.CHUNK_FIXED | tk.CHUNK_MASK, tk.WINDOW_FIXED | tk.WINDOW_MASK
        t_lev, t_walk, t_fill, t_call, t_win = [], [], [], [], []
        for k in range(args.warmup + args.steps):
            p_lev = eng.chunk_levels_device(spans.data_ptr(), oo.data_ptr(), n_docs, n_ids, d_bytes.data_ptr(), d_offs.data_ptr(), n_bytes,
                                            tk.CHUNK_LEVELS_ALL, sp)
            ms_c, r = timed(lambda: eng.chunk_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, p_lev, T, m, ov, 0, PAD, 1, 1, cfl, 0, sp))
            stages = eng.last_chunk_ms()
            ms_w, w = timed(lambda: eng.window_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, T, ov, 0, PAD, 1, 1, wfl, 0, sp))
            if k >= args.warmup:
                t_lev.append(stages[0]); t_walk.append(stages[1]); t_fill.append(stages[2]); t_call.append(ms_c); t_win.append(ms_w)
        counts = torch.as_tensor(r.views()[9], device="cuda").cpu().numpy().tolist()
        cb, wb = r.n_windows * r.row_len * 5, w.n_windows * w.row_len * 5        # bytes of rows written: int32 ids and the mask
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids, "max_length": T, "min_length": m, "overlap": ov, "n_windows": r.n_windows,
               "n_split": r.n_split, "level_counts": counts, "levels_ms": med(t_lev), "walks_scan_ms": med(t_walk), "fill_ms": med(t_fill),
               "fill_min_ms": round(float(np.min(t_fill)), 4), "call_ms": med(t_call), "call_min_ms": round(float(np.min(t_call)), 4),
               "window_n_windows": w.n_windows, "window_call_ms": med(t_win), "window_call_min_ms": round(float(np.min(t_win)), 4),
               "fill_ns_per_row_kib": round(float(np.median(t_fill)) * 1e6 / (cb / 1024), 4),
               "window_call_ns_per_row_kib": round(float(np.median(t_win)) * 1e6 / (wb / 1024), 4)}
        res["fill_over_window_call_per_byte"] = round(res["fill_ns_per_row_kib"] / res["window_call_ns_per_row_kib"], 3)
        # the host: what comes down, then the greedy loop
        nd = min(args.host_docs, n_docs)
        wstart = torch.as_tensor(r.views()[4], device="cuda").cpu().numpy().astype(np.int64)
        dwin = torch.as_tensor(r.views()[5], device="cuda").cpu().numpy()
        t0 = time.perf_counter()
        h_oo = oo.cpu().numpy()
        h_lev = torch.as_tensor(tk.DeviceView(p_lev, n_ids, "|u1"), device="cuda").cpu().numpy()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        starts, n_cuts = host_walk(h_oo, h_lev, T, m, ov, 1, 1, nd)
        t2 = time.perf_counter()
        split = np.diff(h_oo[:nd + 1]) > T
        rows = np.concatenate([np.arange(int(dwin[d]), int(dwin[d + 1])) for d in np.nonzero(split)[0].tolist()] or [np.zeros(0, np.int64)])
        assert np.array_equal(starts, wstart[rows.astype(np.int64)]), "the host loop and the pass disagree"
        res.update({"host_docs": nd, "host_split_docs": int(split.sum()), "host_cuts": n_cuts, "host_copy_ms": round((t1 - t0) * 1e3, 3),
                    "host_loop_ms": round((t2 - t1) * 1e3, 3)})
        print("%s: %s" % (name, json.dumps(res)), file=sys.stderr, flush=True)
        out[name] = res
        del d_bytes, d_offs, ids, oo, spans
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
