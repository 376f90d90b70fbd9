"""Time the dense layout pass (csrc/tk_dense.hip) on one MI355X; prints ONE JSON line.

For C2 (1 M x 512 B ASCII; max_length 128, fixed rows, int32 and int64, with and without mask) and the 500 k Zipf share
(max_length 512, longest mode, multiple_of 64): the GPU time of tk_dense_from_ids_device over encode's own ids against what a
user can do without it -- a torch composition of the same definition over the ragged device views (right truncation, right
padding, BOS / EOS kept) --, alternating the two in one process, HIP events around each, warm, median and min; the algorithmic
HBM bytes of the pass and their fraction of 6.3 TB/s; the same-box wall time of one step of tk_encode_batch_device_ex against
tk_encode_batch_device_dense (interleaved); and tk_ragged_from_dense_device on the C2 tensor.

    python tools/dense_time.py [--steps 20] [--warmup 3] [--shapes C2,zipf]
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
SHAPES = {"C2": ("ascii", 1_000_000, 512, dict(max_length=128, multiple_of=0, fixed=True)),
          "zipf": ("zipf", 500_000, 0, dict(max_length=512, multiple_of=64, fixed=False))}
PAD = 11


def torch_dense(torch, ids, oo, T, L, pad_id, dtype, want_mask):
    """The definition over the ragged views, as well as torch allows: right truncation with BOS / EOS kept (h = t = 1), right
    padding.  One int64 [D, L] index, one gather, one where; the lengths and the truncated count come from the offsets."""
    start = oo[:-1]
    n = oo[1:] - start
    k = torch.clamp(n, max=T)
    col = torch.arange(L, device=ids.device, dtype=torch.int64)[None, :]
    kept = col < k[:, None]
    # position j reads j, the last kept position of a truncated row reads the row's last id
    src = torch.where(col == (T - 1), (n - 1)[:, None], col)
    idx = start[:, None] + src
    # only the batch's last rows can point past the ids under their pads (every document has BOS / EOS, so at most L / 2 rows):
    # clamp those, not the whole index
    idx[max(idx.shape[0] - L, 0):].clamp_(max=ids.numel() - 1)
    dense = torch.where(kept, ids[idx].to(dtype), torch.full((), pad_id, dtype=dtype, device=ids.device))
    mask = kept.to(torch.uint8) if want_mask else None
    return dense, mask, k.to(torch.int32), (n > T).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/dense_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS}
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
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        T = o["max_length"]
        base = (tk.DENSE_FIXED if o["fixed"] else 0)
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids, "max_length": T, "fixed": o["fixed"], "multiple_of": o["multiple_of"]}
        kept_ids = int(torch.clamp(oo[1:] - oo[:-1], max=T).sum())
        variants = [("i32_mask", tk.DENSE_MASK), ("i32", 0), ("i64_mask", tk.DENSE_I64 | tk.DENSE_MASK), ("i64", tk.DENSE_I64)]
        if name != "C2":
            variants = variants[:1] + variants[2:3]
        dense_c2 = None
        for label, fl in variants:
            t_k, t_t = [], []
            tdt = torch.int64 if fl & tk.DENSE_I64 else torch.int32
            for k in range(args.warmup + args.steps):
                ms_k, r = timed(lambda: eng.dense_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, T, o["multiple_of"], PAD, 1, 1,
                                                                  base | fl, sp))
                L = r.row_len
                ms_t, ref = timed(lambda: torch_dense(torch, ids, oo, T, L, PAD, tdt, bool(fl & tk.DENSE_MASK)))
                if k == 0:    # the two sides compute the same thing
                    v_ids, v_mask, v_len = r.views()
                    assert torch.equal(torch.as_tensor(v_ids, device="cuda"), ref[0]) and torch.equal(torch.as_tensor(v_len, device="cuda"), ref[2])
                    assert ref[1] is None or torch.equal(torch.as_tensor(v_mask, device="cuda"), ref[1])
                    assert int(ref[3]) == r.n_truncated
                del ref
                if k >= args.warmup:
                    t_k.append(ms_k)
                    t_t.append(ms_t)
            esz = 8 if fl & tk.DENSE_I64 else 4
            alg = 4 * kept_ids + 8 * (n_docs + 1) + n_docs * L * esz + (n_docs * L if fl & tk.DENSE_MASK else 0) + 4 * n_docs
            ms = float(np.median(t_k))
            res[label] = {"row_len": L, "n_truncated": r.n_truncated, "kernel_ms": round(ms, 4), "kernel_min_ms": round(float(np.min(t_k)), 4),
                          "torch_ms": round(float(np.median(t_t)), 4), "torch_min_ms": round(float(np.min(t_t)), 4),
                          "torch_over_kernel": round(float(np.median(t_t)) / ms, 2), "kernel_not_slower": bool(ms <= float(np.median(t_t))),
                          "alg_bytes": alg,
                          "tb_s": round(alg / (ms * 1e-3) / 1e12, 3), "frac_hbm": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}
            if name == "C2" and label == "i32_mask":
                v_ids, _, v_len = r.views()
                dense_c2 = (torch.as_tensor(v_ids, device="cuda").clone(), torch.as_tensor(v_len, device="cuda").clone(), L)
        # one step of each entry, interleaved (the call drains the stream: wall time is the step)
        t_enc, t_dn = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp, checks=0)
            t1 = time.perf_counter()
            eng.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, T, o["multiple_of"], PAD,
                                          base | tk.DENSE_MASK, 0, sp)
            t2 = time.perf_counter()
            if k >= args.warmup:
                t_enc.append((t1 - t0) * 1e3)
                t_dn.append((t2 - t1) * 1e3)
        res["step_encode_ms"] = round(float(np.median(t_enc)), 3)
        res["step_encode_dense_ms"] = round(float(np.median(t_dn)), 3)
        res["step_delta_ms"] = round(res["step_encode_dense_ms"] - res["step_encode_ms"], 3)
        if dense_c2 is not None:
            dn, ln, L = dense_c2
            for label, lp in (("ragged_given_lengths", ln.data_ptr()), ("ragged_pad_trim", 0)):
                ts = []
                for k in range(args.warmup + args.steps):
                    ms_r, rr = timed(lambda: eng.ragged_from_dense_device(dn.data_ptr(), n_docs, L, 0, lp, PAD, sp))
                    if k >= args.warmup:
                        ts.append(ms_r)
                assert rr[2] == int(ln.sum())
                alg = n_docs * L * 4 + rr[2] * 4 + n_docs * 12 + (n_docs + 1) * 8   # the tensor read, the ids written, lengths in / out, offsets
                ms = float(np.median(ts))
                res[label] = {"ms": round(ms, 4), "min_ms": round(float(np.min(ts)), 4), "alg_bytes": alg,
                              "frac_hbm": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}
            del dn, ln
        out[name] = res
        del d_bytes, d_offs, ids, oo
        torch.cuda.empty_cache()
    eng.close()
    # the requirement: the kernel is not slower than the torch composition on any measured shape
    out["kernel_not_slower_everywhere"] = all(v["kernel_not_slower"] for r in out.values() if isinstance(r, dict)
                                              for v in r.values() if isinstance(v, dict) and "kernel_not_slower" in v)
    print(json.dumps(out))
    if not out["kernel_not_slower_everywhere"]:
        sys.exit("tools/dense_time.py: the kernel is slower than the torch composition on a measured shape")


if __name__ == "__main__":
    main()
