"""Time the packed-rows pass (csrc/tk_seqpack.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/seqpack_time.json.

On encode's own ids for C2 (1 M x 512 B ASCII) at seq_len 2048 and 8192 and for the 500 k Zipf share at 8192, all four tensors,
int32 and int64: the GPU time of tk_seqpack_from_ids_device against what a user can do without it -- a torch composition of
the same definition over the ragged device views (searchsorted over the document starts, index arithmetic, where) --, alternating the
two in one process, HIP events around each, warm, median and min of --steps; the two are checked equal at the first step.  The
algorithmic HBM bytes of the pass (4 * n_used + 8 * (D + 1) read; n_rows * L * elt * outputs + 4 * (n_segments + 1) written) and
their fraction of 6.3 TB/s.  `ids_only` is the same call with no optional output selected: the document search is not made, so
the difference to the full call at equal bytes per output shows what the search costs.

    python tools/seqpack_time.py [--steps 20] [--warmup 3] [--shapes C2,zipf] [--out profiles/seqpack_time.json]
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
PAD = 11


def torch_packed(torch, ids, starts, L, pad_id, dtype):
    """The definition over the ragged views, as well as torch allows: one searchsorted over the starts of the non-empty documents
    (compacted by the caller, outside the timed region: a boolean mask is a host wait) for every position, one for every row,
    index arithmetic and where; cu_seqlens from a sorted unique of both kinds of start (its one host wait stays in the time)."""
    N = ids.numel()
    n_rows = (N + L - 1) // L
    dev = ids.device
    g = torch.arange(n_rows * L, device=dev, dtype=torch.int64)
    valid = g < N
    k = torch.searchsorted(starts, g, right=True)                    # starts at or before g (>= 1 under an id)
    row_start = torch.arange(n_rows, device=dev, dtype=torch.int64) * L
    k_row = torch.searchsorted(starts, row_start, right=True)
    seg_start = torch.maximum(starts[(k - 1).clamp_(min=0)].view(n_rows, L), row_start[:, None])
    zero = torch.zeros((), dtype=dtype, device=dev)
    valid2 = valid.view(n_rows, L)
    pos = torch.where(valid2, (g.view(n_rows, L) - seg_start).to(dtype), zero)
    seg = torch.where(valid2, (k.view(n_rows, L) - k_row[:, None] + 1).to(dtype), zero)
    inp = torch.where(valid, ids[g.clamp(max=N - 1)].to(dtype), torch.full((), pad_id, dtype=dtype, device=dev)).view(n_rows, L)
    cu = torch.cat([torch.unique(torch.cat([starts, row_start])), torch.full((1,), N, dtype=torch.int64, device=dev)]).to(torch.int32)
    return inp, pos, seg, cu, (cu[1:] - cu[:-1]).max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqpack_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/seqpack_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS}
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

    ALL = tk.SEQPACK_POSITIONS | tk.SEQPACK_SEGMENTS | tk.SEQPACK_CU_SEQLENS
    for name in args.shapes.split(","):
        kind, n_docs, doc_len, row_lens = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        starts = oo[:-1][oo[1:] > oo[:-1]].clone()
        torch.cuda.synchronize()
        del d_bytes, d_offs
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids}
        for L in row_lens:
            for label, fl in (("i32", ALL), ("i64", ALL | tk.SEQPACK_I64), ("i32_ids_only", 0)):
                t_k, t_t = [], []
                tdt = torch.int64 if fl & tk.SEQPACK_I64 else torch.int32
                for k in range(args.warmup + args.steps):
                    ms_k, r = timed(lambda: eng.seqpack_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, L, PAD, fl, sp))
                    if fl & ALL:
                        ms_t, ref = timed(lambda: torch_packed(torch, ids, starts, L, PAD, tdt))
                        if k == 0:    # the two sides compute the same thing
                            for v, e in zip(r.views(), ref[:4]):
                                assert torch.equal(torch.as_tensor(v, device="cuda"), e)
                            assert int(ref[4]) == r.max_seqlen and r.n_segments == ref[3].numel() - 1 and r.n_left == 0
                        del ref
                    else:
                        ms_t = float("nan")
                    if k >= args.warmup:
                        t_k.append(ms_k)
                        t_t.append(ms_t)
                esz = 8 if fl & tk.SEQPACK_I64 else 4
                outputs = 3 if fl & ALL else 1
                alg = 4 * r.n_used + 8 * (n_docs + 1) + r.n_rows * L * esz * outputs + (4 * (r.n_segments + 1) if fl & ALL else 0)
                ms = float(np.median(t_k))
                rec = {"seq_len": L, "n_rows": r.n_rows, "n_segments": r.n_segments, "max_seqlen": r.max_seqlen,
                       "kernel_ms": round(ms, 4), "kernel_min_ms": round(float(np.min(t_k)), 4), "alg_bytes": alg,
                       "tb_s": round(alg / (ms * 1e-3) / 1e12, 3), "frac_hbm": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}
                if fl & ALL:
                    rec.update({"torch_ms": round(float(np.median(t_t)), 4), "torch_min_ms": round(float(np.min(t_t)), 4),
                                "torch_over_kernel": round(float(np.median(t_t)) / ms, 2)})
                res["L%d_%s" % (L, label)] = rec
        out[name] = res
        del ids, oo
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
