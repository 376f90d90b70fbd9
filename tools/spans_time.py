"""Time the per-token span pass (csrc/tk_spans.hip) on one MI355X; prints ONE JSON line.

For C2 (1 M x 512 B ASCII), C3 (1 M x 2 KiB mixed UTF-8) and the 500 k Zipf share: the median GPU time of tk_token_spans_device
over encode's own ids (HIP events around the call on its stream: the kernel, a 32-byte memset and the 32-byte copy of the error
words), without a check and with each check; the algorithmic HBM bytes of the pass and their fraction of 6.3 TB/s; and the
same-box wall time of one step of tk_encode_batch_device_ex against tk_encode_batch_device_spans (interleaved).

    python tools/spans_time.py [--steps 20] [--warmup 3] [--shapes C2,C3,zipf]
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
SHAPES = {"C2": ("ascii", 1_000_000, 512), "C3": ("mixed", 1_000_000, 2048), "zipf": ("zipf", 500_000, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,C3,zipf")
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/spans_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS}
    try:
        with open(os.path.join(ROOT, "tekken-rs_amd", "BUILD_INFO.json")) as f:
            out["build"] = json.load(f).get("git")
    except OSError:
        pass
    for name in args.shapes.split(","):
        kind, n_docs, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        n_bytes = len(data)
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp)
        # encode's outputs copied out of the context (the spans calls below leave them alone anyway; the copy keeps this tool honest)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        res = {"n_docs": n_docs, "n_bytes": n_bytes, "n_ids": n_ids}
        base_bytes = n_ids * (4 + 8) + (n_docs + 1) * 8          # ids read, (start, end) written, id offsets read
        for label, checks, extra in (("none", 0, 0), ("cover", tk.SPANS_CHECK_COVER, (n_docs + 1) * 8),
                                     ("bytes", tk.SPANS_CHECK_BYTES, (n_docs + 1) * 8 + n_bytes)):
            times = []
            for k in range(args.warmup + args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.token_spans_device(ids.data_ptr(), oo.data_ptr(), n_docs, n_ids, d_offs.data_ptr(), d_bytes.data_ptr(), checks, sp)
                e1.record(stream)
                e1.synchronize()
                if k >= args.warmup:
                    times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            alg = base_bytes + extra
            res["spans_" + label] = {"ms": round(ms, 4), "min_ms": round(float(np.min(times)), 4), "alg_bytes": alg,
                                     "tb_s": round(alg / (ms * 1e-3) / 1e12, 3), "frac_hbm": round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}
        # one step of each entry, interleaved (the call drains the stream: wall time is the step)
        t_enc, t_spn = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, sp, checks=0)
            t1 = time.perf_counter()
            eng.encode_batch_device_spans(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, True, True, checks=0, stream=sp)
            t2 = time.perf_counter()
            if k >= args.warmup:
                t_enc.append((t1 - t0) * 1e3)
                t_spn.append((t2 - t1) * 1e3)
        res["step_encode_ms"] = round(float(np.median(t_enc)), 3)
        res["step_encode_spans_ms"] = round(float(np.median(t_spn)), 3)
        res["step_delta_ms"] = round(res["step_encode_spans_ms"] - res["step_encode_ms"], 3)
        out[name] = res
        del d_bytes, d_offs, ids, oo
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
