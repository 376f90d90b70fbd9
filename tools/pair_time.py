"""Time the pair pass (csrc/tk_pair.hip) on one MI355X; prints ONE JSON line (--out: also writes it to a file).

C2 reshaped as pairs (1 M x 512 B ASCII texts = 500 k pairs of two 512-byte texts) and the 500 k Zipf share paired the same way
(250 k pairs), each text encoded on its own without BOS / EOS; max_length 256, ONLY_SECOND + OVERFLOW, stride 32, max_fixed 64,
head [BOS], sep [EOS], tail [EOS], fixed rows, int32 + mask + type_ids.  Three things alternate in one process, HIP events around
each, warm, median and min:
  - tk_pair_from_ids_device over encode's own ids;
  - tk_window_from_ids_device on the same ids (every text a document; max_length 256, stride 32, mask): the same launch shape,
    and the pair kernel does strictly more per row -- the yardstick, compared per output byte (ids + mask + type_ids against
    ids + mask);
  - a torch composition of the same definition over the ragged device views (per-pair window counts, a cumulative sum, an int64
    [W, T] index, a gather and the wheres), checked equal to the pass on every output (--no-torch leaves it out).
Then one step of tk_encode_batch_device_ex against tk_encode_pairs_device (interleaved wall time).  The fill kernels alone are not
visible to events around a call: --trace SHAPE=DIR names the output directory of a `rocprofv3 --kernel-trace --stats
--output-format csv` run of this tool (--no-torch --shapes SHAPE) on the same box, from whose kernel trace the median durations of
tk_pair_kernel and tk_window_kernel are taken.

    python tools/pair_time.py [--steps 20] [--warmup 3] [--shapes C2,zipf] [--no-torch] [--trace C2=DIR] [--out profiles/pair_time.json]
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
from join_time import trace_ms  # noqa: E402

HBM_TBS = 6.3
SHAPES = {"C2": ("ascii", 1_000_000, 512), "zipf": ("zipf", 500_000, 0)}
T, STRIDE, MAX_FIXED, PAD = 256, 32, 64, 11


def torch_pairs(torch, ids, oo, T, s, F, head, sep, tail, pad_id, dtype):
    """ONLY_SECOND + OVERFLOW over the ragged views, as well as torch allows (fixed rows of T, one id in each fixed list): the
    window count of every pair, their cumulative sum (one read: W sizes everything), the pair and number of every row, one int64
    [W, T] index, one gather, the wheres."""
    dev = ids.device
    c = T - 3
    oa, ob = oo[0:-1:2], oo[1::2]
    a, b = ob - oa, oo[2::2] - ob
    f = torch.clamp(a, max=F)
    cw = c - f
    step = cw - s
    w = torch.where(b > cw, 1 + (b - cw + step - 1) // step, torch.ones_like(b))
    P = a.numel()
    pw = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    torch.cumsum(w, 0, out=pw[1:])
    W = int(pw[-1])
    pair = torch.repeat_interleave(torch.arange(P, device=dev), w, output_size=W)
    k = torch.arange(W, device=dev) - pw[pair]
    vs = k * step[pair]
    blen = torch.minimum(b[pair] - vs, cw[pair])
    e1 = (1 + f[pair])[:, None]
    e2 = e1 + 1
    e3 = e2 + blen[:, None]
    e4 = e3 + 1
    col = torch.arange(T, device=dev, dtype=torch.int64)[None, :]
    is_a, is_b = (col >= 1) & (col < e1), (col >= e2) & (col < e3)
    src = torch.where(is_a, oa[pair][:, None] + (col - 1), ob[pair][:, None] + vs[:, None] + (col - e2)).clamp_(0, max(ids.numel() - 1, 0))
    val = ids[src].to(dtype)

    def const(x):
        return torch.full((), x, dtype=dtype, device=dev)
    out = torch.where(is_a | is_b, val, torch.where(col < 1, const(head), torch.where(col < e2, const(sep), torch.where(col < e4, const(tail), const(pad_id)))))
    kept = col < e4
    return (out, kept.to(torch.uint8), ((col >= e2) & kept).to(torch.uint8), e4[:, 0].to(torch.int32), pair.to(torch.int32), vs.to(torch.int32),
            e2[:, 0].to(torch.int32), pw, (w > 1).sum(), (a > F).sum(), ((a > F) | (b > cw)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,zipf")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace", action="append", default=[], help="SHAPE=DIR: the rocprofv3 output directory of a traced run of that shape")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    traces = dict(x.split("=", 1) for x in args.trace)
    out = {"tool": "tools/pair_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS, "max_length": T, "stride": STRIDE,
           "max_fixed": MAX_FIXED, "strategy": "only_second", "overflow": True, "outputs": "int32 + mask + type_ids, fixed rows"}
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

    pflags = tk.PAIR_FIXED | tk.PAIR_MASK | tk.PAIR_TYPE_IDS | tk.PAIR_OVERFLOW
    wflags = tk.WINDOW_FIXED | tk.WINDOW_MASK
    for name in args.shapes.split(","):
        kind, n_parts, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_parts, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        print("%s: %d texts, %d bytes" % (name, n_parts, n_bytes), file=sys.stderr, flush=True)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, n_bytes, False, False, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_parts + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        t_p, t_w, t_t = [], [], []
        for k in range(args.warmup + args.steps):
            ms_p, r = timed(lambda: eng.pair_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_parts, n_ids, T, tk.PAIR_ONLY_SECOND, STRIDE, MAX_FIXED,
                                                             0, PAD, (bos,), (eos,), (eos,), pflags, 0, sp))
            ms_w, rw = timed(lambda: eng.window_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_parts, n_ids, T, STRIDE, 0, PAD, 0, 0, wflags, 0, sp))
            if not args.no_torch:
                ms_t, ref = timed(lambda: torch_pairs(torch, ids, oo, T, STRIDE, MAX_FIXED, bos, eos, eos, PAD, torch.int32))
                if k == 0:    # the two sides compute the same thing
                    v = [None if x is None else torch.as_tensor(x, device="cuda") for x in r.views()]
                    assert r.n_windows == ref[0].shape[0] and r.row_len == T
                    assert (r.n_split, r.n_fixed_cut, r.n_truncated) == (int(ref[8]), int(ref[9]), int(ref[10]))
                    for got, want in ((v[0], ref[0]), (v[1], ref[1]), (v[2], ref[2]), (v[4], ref[3]), (v[5], ref[4]), (v[6], ref[5]), (v[7], ref[6]),
                                      (v[9], ref[7])):
                        assert torch.equal(got, want)
                del ref
            if k >= args.warmup:
                t_p.append(ms_p)
                t_w.append(ms_w)
                if not args.no_torch:
                    t_t.append(ms_t)
        W, L, Ww = r.n_windows, r.row_len, rw.n_windows
        # the bytes the rows hold: ids + mask + type_ids against ids + mask
        pair_out, window_out = W * L * 6, Ww * rw.row_len * 5
        # every id read at most once a row it lies in (the kept ones), the offsets, the outputs, the four per-row words, pair_windows
        alg = pair_out + 8 * (n_parts + 1) + 16 * W + 8 * (n_parts // 2 + 1)
        ms, ms_w = float(np.median(t_p)), float(np.median(t_w))
        res = {"n_pairs": n_parts // 2, "n_bytes": n_bytes, "n_ids": n_ids, "n_windows": W, "row_len": L, "n_split": r.n_split,
               "n_truncated": r.n_truncated, "n_fixed_cut": r.n_fixed_cut, "pair_call_ms": round(ms, 4), "pair_call_min_ms": round(float(np.min(t_p)), 4),
               "window_call_ms": round(ms_w, 4), "window_call_min_ms": round(float(np.min(t_w)), 4), "window_n_windows": Ww,
               "pair_out_bytes": pair_out, "window_out_bytes": window_out,
               "call_per_out_byte_pair_over_window": round((ms / pair_out) / (ms_w / window_out), 3),
               "written_bytes": alg, "written_tb_s_of_call": round(alg / (ms * 1e-3) / 1e12, 3)}
        if t_t:
            res.update({"torch_ms": round(float(np.median(t_t)), 4), "torch_min_ms": round(float(np.min(t_t)), 4),
                        "torch_over_pair_call": round(float(np.median(t_t)) / ms, 2)})
        if name in traces:
            kp, n_p = trace_ms(traces[name], "tk_pair_kernel")
            kw, n_w = trace_ms(traces[name], "tk_window_kernel")
            res.update({"fill_kernel_ms": round(kp, 4), "fill_kernel_launches": n_p, "window_kernel_ms": round(kw, 4), "window_kernel_launches": n_w,
                        "kernel_per_out_byte_pair_over_window": round((kp / pair_out) / (kw / window_out), 3),
                        "fill_kernel_written_tb_s": round(alg / (kp * 1e-3) / 1e12, 3),
                        "fill_kernel_written_frac_hbm": round(alg / (kp * 1e-3) / (HBM_TBS * 1e12), 3)})
        print("%s: pair %.3f ms, window %.3f ms%s" % (name, ms, ms_w, ", torch %.3f ms" % res["torch_ms"] if t_t else ""), file=sys.stderr, flush=True)
        # one step of each entry, interleaved (the call drains the stream: wall time is the step)
        t_enc, t_pr = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, n_bytes, False, False, sp, checks=0)
            t1 = time.perf_counter()
            eng.encode_pairs_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, n_bytes, T, tk.PAIR_ONLY_SECOND, STRIDE, MAX_FIXED, 0, PAD,
                                    (bos,), (eos,), (eos,), pflags, 0, sp)
            t2 = time.perf_counter()
            if k >= args.warmup:
                t_enc.append((t1 - t0) * 1e3)
                t_pr.append((t2 - t1) * 1e3)
        res["step_encode_ms"] = round(float(np.median(t_enc)), 3)
        res["step_encode_pairs_ms"] = round(float(np.median(t_pr)), 3)
        res["step_delta_ms"] = round(res["step_encode_pairs_ms"] - res["step_encode_ms"], 3)
        out[name] = res
        del d_bytes, d_offs, ids, oo
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
