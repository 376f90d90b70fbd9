"""Time the noise pass (csrc/tk_noise.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/noise_time.json.

On the ids of C2 (1 M x 512 B ASCII) and of the 500 k Zipf share (BOS / EOS stored), HIP events, warm, the median of --steps:
  replace  tk_noise_replace_device as masked LM draws it (15 % of the tokens, 80 / 10 / 10): the call and, inside it, the one kernel
           as the library's own events see it (tk_last_noise_ms);
  spans    tk_noise_spans_device as T5 draws it (15 % covered by spans of 1..5 tokens, 100 sentinels, a final id, the split
           form): the call, and the selection, the counts and scans, and the fill kernel;
each against the same definition composed from torch ops on the same device (checked equal first) and, in the same run, against a
device-to-device copy of the same bytes and the regroup pass's gather kernel over the same ids (tk_last_regroup_ms).

    python tools/noise_time.py [--steps 20] [--warmup 2] [--shapes C2,zipf] [--out profiles/noise_time.json]
"""
import argparse
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

SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}
M32 = 0xFFFFFFFF
MASK_ID, SENTINEL_FIRST, N_SENTINELS, FINAL = 3, 100, 100, 2   # ids below num_special: what they are called does not matter to the timing


def h_int(seed, d):
    x = (d * 0x9E3779B1 + seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def h_t(seed, d):
    """The hash over int64 tensors (seed: a tensor or an int); every product is cut to 32 bits before it is shifted."""
    x = (d * 0x9E3779B1 + seed) & M32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def torch_select(torch, ids, offs, o, num_special):
    """Steps 1 and 2 (token unit) from torch ops: (selected, doc, pos, t[4]).  covered: where a span starts it reaches to q + len,
    clamped to its document's end; the running maximum of that lies behind a covered position."""
    lens = offs[1:] - offs[:-1]
    D = len(lens)
    doc = torch.repeat_interleave(torch.arange(D, device=ids.device), lens)
    g = torch.arange(len(ids), device=ids.device)
    p = g - offs[:-1][doc]
    s = [h_int(o["seed"], (0x4E4F4900 + k) & M32) for k in range(4)]
    t = [h_t(s[k], doc) for k in range(4)]
    start = h_t(t[0], p) < o["start_q32"]
    ln = o["span_min"] + ((h_t(t[1], p) * (o["span_max"] - o["span_min"] + 1)) >> 32)
    reach = torch.where(start, torch.minimum(g + ln, offs[1:][doc]), torch.zeros_like(g))
    covered = torch.cummax(reach, 0).values > g
    return covered & (ids >= num_special), doc, p, t


def torch_replace(torch, ids, offs, o, num_special, n_ordinary):
    sel, doc, p, t = torch_select(torch, ids, offs, o, num_special)
    r = h_t(t[2], p)
    rnd = num_special + ((h_t(t[3], p) * n_ordinary) >> 32)
    out = torch.where(sel & (r < o["mask_q32"]), torch.full_like(ids, o["mask_id"]),
                      torch.where(sel & (r < o["mask_q32"] + o["random_q32"]), rnd, ids))
    return out, torch.where(sel, ids, torch.full_like(ids, o["ignore_index"]))


def torch_spans(torch, ids, offs, o, num_special):
    """Step 4, the split form: (inputs, input_offsets, targets, target_offsets)."""
    sel, doc, p, _ = torch_select(torch, ids, offs, o, num_special)
    D = len(offs) - 1
    prev = torch.cat([sel.new_zeros(1), sel[:-1]])
    rs = sel & ((p == 0) | ~prev)
    zero = torch.zeros(1, dtype=torch.int64, device=ids.device)
    R = torch.cat([zero, torch.cumsum(rs.to(torch.int64), 0)])
    run = R[1:] - R[offs[:-1]][doc] - 1                 # the run of a selected id, inside its document
    kept = sel & (run < o["n_sentinels"])
    krs = rs & kept
    sentinel = o["sentinel_first"] + run
    in_mask = ~kept | krs
    inputs = torch.where(krs, sentinel, ids)[in_mask]
    I = torch.cat([zero, torch.cumsum(in_mask.to(torch.int64), 0)])
    in_offs = I[offs]
    cnt = kept.to(torch.int64) + krs.to(torch.int64)
    C = torch.cat([zero, torch.cumsum(cnt, 0)])
    tg_offs = C[offs] + torch.arange(D + 1, device=ids.device)          # (one final id a document)
    targets = torch.full((int(tg_offs[-1]),), o["final_id"], dtype=torch.int64, device=ids.device)
    at = C[:-1] + doc
    targets[at[krs]] = sentinel[krs]
    targets[(at + krs.to(torch.int64))[kept]] = ids[kept]
    return inputs, in_offs, targets, tg_offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    one = 1 << 32
    mlm = dict(start_q32=tk.noise_start_q32(0.15, 1, 1), mask_q32=tk.fim_q32(0.8), random_q32=tk.fim_q32(0.1), seed=1, span_min=1, span_max=1,
               mask_id=MASK_ID, ignore_index=-100)
    t5 = dict(start_q32=tk.noise_start_q32(0.15, 1, 5), seed=1, span_min=1, span_max=5, n_sentinels=N_SENTINELS, sentinel_first=SENTINEL_FIRST,
              final_id=FINAL, flags=tk.NOISE_SPLIT, ignore_index=-100)
    assert mlm["mask_q32"] + mlm["random_q32"] <= one
    out = {"tool": "tools/noise_time.py", "steps": args.steps, "warmup": args.warmup, "tile_ids": int(tk.lib().tk_noise_tile()),
           "replace_opts": "15 % tokens, 80 / 10 / 10", "spans_opts": "15 % covered, spans 1..5, 100 sentinels, final id, split form"}
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
    view = lambda v: torch.as_tensor(v, device="cuda")
    for name in args.shapes.split(","):
        kind, n_docs, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(data), True, True, sp)
        ids32 = view(tk.DeviceView(p_ids, n_ids, "<i4")).clone()
        oo = view(tk.DeviceView(p_oo, n_docs + 1, "<i8")).clone()
        del d_bytes, d_offs
        ids64 = ids32.to(torch.int64)
        b = (ids32.data_ptr(), oo.data_ptr(), n_docs, n_ids)
        # ---- the torch compositions give what the pass gives
        r = eng.noise_replace_device(*b, stream=sp, **mlm)
        want_ids, want_lab = torch_replace(torch, ids64, oo, mlm, ns, len(toks))
        assert torch.equal(view(r.views()[0]).to(torch.int64), want_ids) and torch.equal(view(r.views()[1]).to(torch.int64), want_lab)
        s = eng.noise_spans_device(*b, stream=sp, **t5)
        w = torch_spans(torch, ids64, oo, t5, ns)
        for got, want in zip(s.views()[:4], w):
            assert torch.equal(view(got).to(torch.int64), want)
        del want_ids, want_lab, w
        rec = {"n_docs": n_docs, "n_ids": n_ids, "replace": {"n_selected": r.n_selected, "n_masked": r.n_masked, "n_random": r.n_random},
               "spans": {"n_selected": s.n_selected, "n_runs": s.n_runs, "n_runs_dropped": s.n_runs_dropped, "n_inputs": s.n_inputs,
                         "n_targets": s.n_targets}}
        t = {k: [] for k in ("replace", "replace_kernel", "replace_torch", "spans", "spans_stages", "spans_torch", "copy", "gather")}
        dst = torch.empty_like(ids32)
        for k in range(args.warmup + args.steps):
            ms_r, _ = timed(lambda: eng.noise_replace_device(*b, stream=sp, **mlm))
            k_r = eng.last_noise_ms()[0]
            ms_rt, _ = timed(lambda: torch_replace(torch, ids64, oo, mlm, ns, len(toks)))
            ms_s, _ = timed(lambda: eng.noise_spans_device(*b, stream=sp, **t5))
            st = eng.last_noise_ms()
            ms_st, _ = timed(lambda: torch_spans(torch, ids64, oo, t5, ns))
            ms_c, _ = timed(lambda: dst.copy_(ids32))
            eng.regroup_from_ids_device(*b, stream=sp)
            ms_g = eng.last_regroup_ms()[2]
            if k >= args.warmup:
                for key, v in zip(t, (ms_r, k_r, ms_rt, ms_s, st, ms_st, ms_c, ms_g)):
                    t[key].append(v)
        st = np.median(np.array(t["spans_stages"]), axis=0)
        copy, gather = float(np.median(t["copy"])), float(np.median(t["gather"]))
        rec["d2d_copy_ms"], rec["regroup_gather_ms"] = round(copy, 4), round(gather, 4)
        rec["replace"].update({"call_ms": med(t["replace"]), "kernel_ms": med(t["replace_kernel"]), "torch_ms": med(t["replace_torch"]),
                               "torch_over_call": round(float(np.median(t["replace_torch"])) / float(np.median(t["replace"])), 1),
                               # the kernel reads the ids and writes ids and labels: 3 streams against the copy's 2
                               "kernel_gbs": round(12 * n_ids / (float(np.median(t["replace_kernel"])) * 1e-3) / 1e9, 1),
                               "copy_gbs": round(8 * n_ids / (copy * 1e-3) / 1e9, 1),
                               "kernel_over_copy": round(float(np.median(t["replace_kernel"])) / copy, 2)})
        rec["spans"].update({"call_ms": med(t["spans"]), "select_ms": round(float(st[0]), 4), "counts_scans_ms": round(float(st[1]), 4),
                             "fill_ms": round(float(st[2]), 4), "torch_ms": med(t["spans_torch"]),
                             "torch_over_call": round(float(np.median(t["spans_torch"])) / float(np.median(t["spans"])), 1),
                             "fill_over_copy": round(float(st[2]) / copy, 2), "fill_over_gather": round(float(st[2]) / gather, 2)})
        out[name] = rec
        print("%s: %s" % (name, json.dumps(rec)), file=sys.stderr, flush=True)
        del ids32, ids64, oo, dst
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
