"""Time the whole-document rows (csrc/tk_rowfit.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/rowfit_time.json.

On encode's own ids for C2 (1 M x 512 B ASCII) at seq_len 2048 and 8192 and for the 500 k Zipf share at 8192 (over-long documents
truncated), all outputs (labels: the ids again as a second int32 stream), int32 and int64, and an `ids_only` leg: the GPU time
of tk_rowfit_from_ids_device, HIP events around the call, warm, median and min of --steps, and inside it the placement stage
(lengths, scans, nxt, doubling rounds, doc_start) and the fill kernel as the library's own events see them (tk_last_rowfit_ms).
Two yardsticks, alternated with it in the same process:
  (a) tk_seqpack_from_ids_device on the same ids and seq_len: the same tensors (no labels, no doc_start) with one search fewer
      and no placement -- the whole cut call (its main kernel is not timed apart here: DESIGN 4.5d has it at 0.85-0.89 of
      6.3 TB/s from a kernel trace, which is what frac_hbm_fill stands beside);
  (b) what a user does without the pass: offsets to the host, the plain next-fit loop there, the assignment uploaded, the tensors
      built with torch indexing (--user-steps of it: a million-document Python loop is slow); checked equal to the pass first.
The algorithmic HBM bytes of the pass (ids and labels read once, 8 * (D + 1) of offsets; every selected tensor, cu_seqlens and
doc_start written once) and their fraction of 6.3 TB/s; n_pad / (n_rows * L).

    python tools/rowfit_time.py [--steps 20] [--warmup 3] [--user-steps 3] [--shapes C2,zipf] [--out profiles/rowfit_time.json]
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
SHAPES = {"C2": ("ascii", 1_000_000, 512, (2048, 8192)), "zipf": ("zipf", 500_000, 0, (8192,))}
PAD, IGN = 11, -100


def user_today(torch, ids, lab, oo, L, keep_tail, dtype):
    """Without the pass: the offsets go to the host, the plain next-fit loop runs there (with the segment numbers and cu_seqlens
    it sees on the way), the assignment goes up, and torch indexing scatters ids, labels, positions and segments."""
    dev = ids.device
    oo_h = oo.cpu().tolist()
    D = len(oo_h) - 1
    r, fill, in_row = -1, L, 0
    ds, segno, cu = [0] * D, [0] * D, []
    for d in range(D):
        e = min(oo_h[d + 1] - oo_h[d], L)
        if e > 0 and fill + e > L:
            if 0 <= r and fill < L:
                cu.append(r * L + fill)
            r, fill, in_row = r + 1, 0, 0
        ds[d] = r * L + fill
        if e:
            in_row += 1
            segno[d] = in_row
            cu.append(ds[d])
        fill += e
    if r >= 0 and fill < L:
        cu.append(r * L + fill)
    n_rows = r + 1
    cu.append(n_rows * L)
    ds_d = torch.tensor(ds, dtype=torch.int64, device=dev)
    sg_d = torch.tensor(segno, dtype=dtype, device=dev)
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
    n = oo[1:] - oo[:-1]
    e = n.clamp(max=L)
    E = torch.cumsum(e, 0) - e
    doc = torch.repeat_interleave(torch.arange(D, device=dev), e)
    k = torch.arange(doc.numel(), device=dev) - E[doc]
    src = torch.where((n[doc] > L) & (k >= L - keep_tail), oo[1:][doc] - (L - k), oo[:-1][doc] + k)
    dest = ds_d[doc] + k
    total = n_rows * L
    inp = torch.full((total,), PAD, dtype=dtype, device=dev)
    labels = torch.full((total,), IGN, dtype=torch.int32, device=dev)
    pos = torch.zeros(total, dtype=dtype, device=dev)
    seg = torch.zeros(total, dtype=dtype, device=dev)
    inp[dest] = ids[src].to(dtype)
    labels[dest] = lab[src]
    pos[dest] = k.to(dtype)
    seg[dest] = sg_d[doc]
    shape = (n_rows, L)
    return inp.view(shape), labels.view(shape), pos.view(shape), seg.view(shape), cu_d, ds_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--user-steps", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowfit_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/rowfit_time.py", "steps": args.steps, "warmup": args.warmup, "user_steps": args.user_steps, "hbm_tbs": HBM_TBS}
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

    ALL = tk.ROWFIT_POSITIONS | tk.ROWFIT_SEGMENTS | tk.ROWFIT_CU_SEQLENS | tk.ROWFIT_LABELS | tk.ROWFIT_DOC_START
    SP_ALL = tk.SEQPACK_POSITIONS | tk.SEQPACK_SEGMENTS | tk.SEQPACK_CU_SEQLENS
    med = lambda x: round(float(np.median(x)), 4)
    for name in args.shapes.split(","):
        kind, n_docs, doc_len, row_lens = SHAPES[name]
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
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids}
        for L in row_lens:
            for label, fl in (("i32", ALL), ("i64", ALL | tk.ROWFIT_I64), ("i32_ids_only", 0)):
                full = bool(fl & ALL)
                tdt = torch.int64 if fl & tk.ROWFIT_I64 else torch.int32
                call = lambda: eng.rowfit_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, L, PAD, 1, fl,
                                                          lab.data_ptr() if full else 0, IGN, sp)
                cut = lambda: eng.seqpack_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, L, PAD,
                                                          (SP_ALL if full else 0) | (tk.SEQPACK_I64 if fl & tk.ROWFIT_I64 else 0), sp)
                if full:      # the pass and the user's composition compute the same thing
                    r, ref = call(), user_today(torch, ids, lab, oo, L, 1, tdt)
                    for v, e in zip(r.views(), ref):
                        assert torch.equal(torch.as_tensor(v, device="cuda"), e)
                    del ref
                t_k, t_cut, t_user, t_place, t_fill = [], [], [], [], []
                for k in range(args.warmup + args.steps):
                    ms_k, r = timed(call)
                    stages = eng.last_rowfit_ms()
                    ms_c, c = timed(cut)
                    if k >= args.warmup:
                        t_k.append(ms_k)
                        t_cut.append(ms_c)
                        t_place.append(stages["placement_ms"])
                        t_fill.append(stages["fill_ms"])
                if full:
                    for k in range(1 + args.user_steps):
                        ms_u, ref = timed(lambda: user_today(torch, ids, lab, oo, L, 1, tdt))
                        del ref
                        if k:
                            t_user.append(ms_u)
                esz = 8 if fl & tk.ROWFIT_I64 else 4
                elems, used = r.n_rows * L, r.n_rows * L - r.n_pad
                alg = 4 * used + 8 * (n_docs + 1) + elems * esz
                if full:
                    alg += 4 * used + elems * (2 * esz + 4) + 4 * (r.n_segments + 1) + 8 * n_docs
                ms = float(np.median(t_k))
                rec = {"seq_len": L, "n_rows": r.n_rows, "n_segments": r.n_segments, "max_seqlen": r.max_seqlen, "n_truncated": r.n_truncated,
                       "pad_frac": round(r.n_pad / elems, 4), "call_ms": med(t_k), "call_min_ms": round(float(np.min(t_k)), 4),
                       "placement_ms": med(t_place), "fill_ms": med(t_fill), "alg_bytes": alg,
                       "frac_hbm_call": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3),
                       "frac_hbm_fill": round(alg / (float(np.median(t_fill)) * 1e-3) / (HBM_TBS * 1e12), 3),
                       "seqpack_ms": med(t_cut), "seqpack_rows": c.n_rows, "call_over_seqpack": round(ms / float(np.median(t_cut)), 3),
                       "fill_over_seqpack_call": round(float(np.median(t_fill)) / float(np.median(t_cut)), 3)}
                if full:
                    rec.update({"user_ms": med(t_user), "user_over_call": round(float(np.median(t_user)) / ms, 1)})
                res["L%d_%s" % (L, label)] = rec
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
