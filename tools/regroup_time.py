"""Time the regroup pass (csrc/tk_regroup.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/regroup_time.json.

On encode's own ids for C2 (1 M x 512 B ASCII) and for the 500 k Zipf share, per order (KEEP with a length filter, LENGTH, SHUFFLE,
GROUPED with a window of 4096), batches on (--max-tokens), with and without labels (the ids again as a second int32 stream): the
GPU time of tk_regroup_from_ids_device, HIP events around the call, warm, median and min of --steps, and inside it the select,
sort, gather and batch stages as the library's own events see them (tk_last_regroup_ms).  The gather kernel as a fraction of
6.3 TB/s counts 8 bytes an id (4 read, 4 written), 16 with labels.  Beside it, in the same process:
  (a) the same definition composed from torch on the same device (torch.sort(stable=True), repeat_interleave, index; the batch
      boundaries, a sequential loop, are left out of it), checked equal to the pass first;
  (b) the two existing kernels of the gather's shape on the same ids: the rowfit fill kernel (tk_last_rowfit_ms, ids only, int32,
      seq_len 8192) and the join call with no control id (every document a part of its own: has, scan, parts and the fill kernel
      -- the call is what events can see of it), each as a fraction of 6.3 TB/s over the bytes it moves.
n_batch_pad / n_ids of the batches of every order: the padding of dense batches cut from the regrouped documents.

    python tools/regroup_time.py [--steps 20] [--warmup 3] [--torch-steps 3] [--shapes C2,zipf] [--max-tokens 65536] [--out profiles/regroup_time.json]
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

HBM_TBS = 6.3
SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}
WINDOW, SEED = 4096, 12345
M32 = 0xFFFFFFFF


def torch_today(torch, ids, lab, oo, order, lo, hi, seed, w, desc=False):
    """Steps 1 to 3 of the definition from torch: -> (ids, offsets, labels, perm)."""
    dev = ids.device
    n = oo[1:] - oo[:-1]
    keep = n >= lo
    if hi:
        keep &= n <= hi
    kept = torch.nonzero(keep).squeeze(1)
    key = -n[kept] if desc else n[kept]
    if order == 0:
        perm = kept
    elif order == 1:
        perm = kept[torch.sort(key, stable=True)[1]]
    else:
        x = (kept * 0x9E3779B1 + seed) & M32
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M32
        x ^= x >> 16
        idx = torch.sort(x, stable=True)[1]
        perm = kept[idx]
        if order == 3:
            group = torch.arange(perm.numel(), device=dev) // w
            k2 = group * (int(n.max()) + 1) + (key[idx] - key.min())
            perm = perm[torch.sort(k2, stable=True)[1]]
    m = n[perm]
    offs = torch.zeros(perm.numel() + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(m, 0)
    doc = torch.repeat_interleave(torch.arange(perm.numel(), device=dev), m)
    src = oo[:-1][perm][doc] + (torch.arange(doc.numel(), device=dev) - offs[doc])
    return ids[src], offs, (lab[src] if lab is not None else None), perm.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--max-tokens", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regroup_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/regroup_time.py", "steps": args.steps, "warmup": args.warmup, "torch_steps": args.torch_steps, "hbm_tbs": HBM_TBS,
           "max_tokens": args.max_tokens, "window": WINDOW}
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
    BATCH = tk.REGROUP_BATCHES | tk.REGROUP_BATCH_OFFSETS | tk.REGROUP_BATCH_ROWLEN
    for name in args.shapes.split(","):
        kind, n_docs, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        lab = ids.clone()
        torch.cuda.synchronize()
        del d_bytes, d_offs
        lens = (oo[1:] - oo[:-1])
        lo, hi = int(torch.quantile(lens[::7].float(), 0.05)), int(torch.quantile(lens[::7].float(), 0.95))   # KEEP: the middle 90 % by length
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids, "longest": int(lens.max()), "filter": [lo, hi]}
        # (b) the existing kernels of the same shape, on the same ids
        ctrl = torch.full((n_docs,), -1, dtype=torch.int32, device="cuda")             # TK_JOIN_NONE
        conv = torch.arange(n_docs + 1, dtype=torch.int64, device="cuda")
        t_join, t_fill = [], []
        for k in range(args.warmup + args.steps):
            ms_j, j = timed(lambda: eng.join_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, ctrl.data_ptr(), 0, conv.data_ptr(), n_docs,
                                                             -100, 0, 0, sp))
            fit = eng.rowfit_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, 8192, 11, 1, 0, 0, -100, sp)
            if k >= args.warmup:
                t_join.append(ms_j)
                t_fill.append(eng.last_rowfit_ms()["fill_ms"])
        assert j.n_ids == n_ids
        fit_bytes = 4 * (fit.n_rows * 8192 - fit.n_pad) + 4 * fit.n_rows * 8192
        res["same_shape"] = {"join_call_ms": med(t_join), "join_call_frac_hbm": frac(8 * n_ids + 24 * n_docs, float(np.median(t_join))),
                             "rowfit_fill_ms": med(t_fill), "rowfit_fill_frac_hbm": frac(fit_bytes, float(np.median(t_fill))),
                             "rowfit_pad_frac": round(fit.n_pad / (fit.n_rows * 8192), 4)}
        del ctrl, conv
        for label, order, flt in (("keep_filtered", tk.REGROUP_ORDER_KEEP, (lo, hi)), ("length", tk.REGROUP_ORDER_LENGTH, (0, 0)),
                                  ("shuffle", tk.REGROUP_ORDER_SHUFFLE, (0, 0)), ("grouped", tk.REGROUP_ORDER_GROUPED, (0, 0))):
            for with_lab in (False, True):
                fl = BATCH | tk.REGROUP_PERM | (tk.REGROUP_LABELS if with_lab else 0)
                call = lambda: eng.regroup_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, order, flt[0], flt[1], SEED, WINDOW,
                                                           args.max_tokens, 0, fl, lab.data_ptr() if with_lab else 0, 0, sp)
                if with_lab:  # the pass and the composition from torch compute the same thing
                    r, ref = call(), torch_today(torch, ids, lab, oo, order, flt[0], flt[1], SEED, WINDOW)
                    v = r.views()
                    for got, want in ((v[0], ref[0]), (v[1], ref[1]), (v[2], ref[2]), (v[3], ref[3])):
                        assert torch.equal(torch.as_tensor(got, device="cuda"), want)
                    del ref, v
                t_k, t_st, t_torch = [], [], []
                for k in range(args.warmup + args.steps):
                    ms_k, r = timed(call)
                    if k >= args.warmup:
                        t_k.append(ms_k)
                        t_st.append(eng.last_regroup_ms())
                if with_lab:
                    for k in range(1 + args.torch_steps):
                        ms_t, ref = timed(lambda: torch_today(torch, ids, lab, oo, order, flt[0], flt[1], SEED, WINDOW))
                        del ref
                        if k:
                            t_torch.append(ms_t)
                st = np.median(np.array(t_st), axis=0)
                per_id = 16 if with_lab else 8
                rec = {"n_kept": r.n_docs, "n_ids": r.n_ids, "call_ms": med(t_k), "call_min_ms": round(float(np.min(t_k)), 4),
                       "select_ms": round(float(st[0]), 4), "sort_ms": round(float(st[1]), 4), "gather_ms": round(float(st[2]), 4),
                       "batch_ms": round(float(st[3]), 4), "gather_frac_hbm": frac(per_id * r.n_ids, float(st[2])),
                       "n_batches": r.n_batches, "n_oversize": r.n_oversize, "batch_pad_over_ids": round(r.n_batch_pad / max(r.n_ids, 1), 4)}
                if with_lab:
                    rec.update({"torch_ms": med(t_torch), "torch_over_call": round(float(np.median(t_torch)) / float(np.median(t_k)), 1)})
                res[label + ("_labels" if with_lab else "")] = rec
        out[name] = res
        del ids, oo, lab
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
