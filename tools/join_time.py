"""Time the join pass of the chat batches (csrc/tk_join.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/join_time.json.

Shape: the bench's C2 corpus (1 M x 512-byte ASCII documents) as parts, 4 parts a conversation, a control id on every part,
labels and part_index selected.  Legs, alternated in one process, HIP events around each, warm, median and min of --steps:
  join        tk_join_from_ids_device on encode's own ids (add_bos = add_eos = 0): the pass alone, with its one host wait
  torch       a torch composition of the same definition over the same device arrays (cumsum, repeat_interleave, searchsorted,
              gathers and where), checked equal to the join at the first step
  encode      tk_encode_batch_device alone;  fused: tk_encode_parts_device_join (encode + the pass)
The algorithmic HBM bytes of the pass are 4 * n_text_ids read and 12 * N written (ids, labels, part_index), reported as a
fraction of 6.3 TB/s.  The main kernel alone is not visible to events around a call: --trace-join / --trace-seqpack name output
directories of `rocprofv3 --kernel-trace --stats --output-format csv` runs of this tool and of tools/seqpack_time.py (--shapes
C2) on the same box, from whose kernel traces the median durations of tk_join_kernel and of tk_seqpack_kernel<0, 1> (all
outputs: the first leg of that tool) are taken.

    python tools/join_time.py [--steps 20] [--warmup 3] [--no-torch] [--trace-join DIR] [--trace-seqpack DIR] [--out profiles/join_time.json]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

HBM_TBS = 6.3
N_PARTS, PART_LEN, PARTS_PER_CONV = 1_000_000, 512, 4
IGN = -100


def torch_joined(torch, ids, oo, ctrl, pf, conv, none):
    """The definition over the device arrays, as well as torch allows (N is read back once, as the join's own wait does)."""
    P = ctrl.numel()
    dev = ids.device
    has = (ctrl != none).to(torch.int64)
    cb = torch.cumsum(has, 0) - has                                   # control ids before each part
    n = oo[1:] - oo[:-1] + has                                        # |T_p|
    start = oo[:-1] + cb
    N = int(oo[-1] + cb[-1] + has[-1])
    part = torch.repeat_interleave(torch.arange(P, device=dev), n, output_size=N)
    g = torch.arange(N, device=dev)
    is_ctrl = (g == start[part]) & (has[part] != 0)
    val = torch.where(is_ctrl, ctrl[part], ids[(g - cb[part] - has[part]).clamp_(0, ids.numel() - 1)])
    fl = pf[part]
    ign = torch.full((), IGN, dtype=torch.int32, device=dev)
    labels = torch.where(torch.where(is_ctrl, fl & 1, fl & 2) != 0, val, ign)
    pidx = torch.arange(P, device=dev)
    plocal = pidx - conv[torch.searchsorted(conv[:-1].contiguous(), pidx, right=True) - 1]
    offsets = torch.cat([start, torch.full((1,), N, dtype=torch.int64, device=dev)])[conv]
    return val, offsets, labels, plocal[part].to(torch.int32), (labels != ign).sum()


def trace_ms(trace_dir, kernel, take=None):
    """Median duration (ms) of the launches of `kernel` in the kernel trace under trace_dir (take: the first so many launches)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *_kernel_trace.csv under %s" % trace_dir)
    rows = [r for r in csv.DictReader(open(files[0])) if kernel in r["Kernel_Name"].replace(" ", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows][:take]
    if not d:
        raise SystemExit("no launch of %s in %s" % (kernel, files[0]))
    return float(np.median(d)), len(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace-join")
    ap.add_argument("--trace-seqpack")
    ap.add_argument("--seqpack-json", help="the line tools/seqpack_time.py wrote in the traced run (its n_rows, seq_len and n_used give the kernel's bytes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/join_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS,
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.node()}}
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

    data, offs = corpus.generate("ascii", N_PARTS, PART_LEN, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
    P, C, n_bytes = N_PARTS, N_PARTS // PARTS_PER_CONV, len(data)
    rng = np.random.default_rng(5)
    d_bytes = torch.from_numpy(data).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    ctrl = torch.from_numpy(rng.integers(0, ns, P).astype(np.int32)).cuda()
    pf = torch.from_numpy(rng.integers(0, 4, P).astype(np.int32)).cuda()
    conv = torch.arange(0, P + 1, PARTS_PER_CONV, dtype=torch.int64, device="cuda")
    p_ids, p_oo, n_text = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), P, n_bytes, False, False, sp)
    ids = torch.as_tensor(tk.DeviceView(p_ids, n_text, "<i4"), device="cuda").clone()
    oo = torch.as_tensor(tk.DeviceView(p_oo, P + 1, "<i8"), device="cuda").clone()
    torch.cuda.synchronize()
    flags = tk.JOIN_LABELS | tk.JOIN_PART_INDEX
    legs = {"join": lambda: eng.join_from_ids_device(ids.data_ptr(), oo.data_ptr(), P, n_text, ctrl.data_ptr(), pf.data_ptr(), conv.data_ptr(),
                                                      C, IGN, flags, 0, sp),
            "encode": lambda: eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), P, n_bytes, False, False, sp),
            "fused": lambda: eng.encode_parts_device_join(d_bytes.data_ptr(), d_offs.data_ptr(), P, n_bytes, ctrl.data_ptr(), pf.data_ptr(),
                                                          conv.data_ptr(), C, IGN, flags, 0, sp)}
    if not args.no_torch:
        legs["torch"] = lambda: torch_joined(torch, ids, oo, ctrl, pf, conv, -1)
    t = {k: [] for k in legs}
    for k in range(args.warmup + args.steps):
        got = {}
        for name, fn in legs.items():
            ms, got[name] = timed(fn)
            if k >= args.warmup:
                t[name].append(ms)
        if k == 0:
            r = got["join"]
            assert r.n_ids == n_text + P == got["fused"].n_ids and r.n_ctrl == P
            if "torch" in got:          # the two sides compute the same thing
                for v, e in zip(r.views(), got["torch"][:4]):
                    assert torch.equal(torch.as_tensor(v, device="cuda"), e.to(torch.as_tensor(v, device="cuda").dtype))
                assert int(got["torch"][4]) == r.n_labelled
        del got
    N = n_text + P
    alg = 4 * n_text + 12 * N
    frac = lambda ms: round(alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"n_parts": P, "n_convs": C, "n_bytes": n_bytes, "n_text_ids": n_text, "n_ids": N, "alg_bytes": alg,
           "join_ms": round(med["join"], 4), "join_min_ms": round(float(np.min(t["join"])), 4), "join_frac_hbm": frac(med["join"]),
           "encode_ms": round(med["encode"], 4), "fused_ms": round(med["fused"], 4), "fused_over_encode": round(med["fused"] / med["encode"], 3)}
    if "torch" in med:
        res.update({"torch_ms": round(med["torch"], 4), "torch_min_ms": round(float(np.min(t["torch"])), 4),
                    "torch_over_join": round(med["torch"] / med["join"], 2)})
    if args.trace_join:
        ms, n = trace_ms(args.trace_join, "tk_join_kernel")
        res.update({"main_kernel_ms": round(ms, 4), "main_kernel_launches": n, "main_kernel_frac_hbm": frac(ms)})
    if args.trace_seqpack:
        sq = json.loads(open(args.seqpack_json).read().strip().splitlines()[-1])
        leg = sq["C2"]["L2048_i32"]
        ms, n = trace_ms(args.trace_seqpack, "tk_seqpack_kernel<0,1>", take=sq["warmup"] + sq["steps"])
        sq_alg = 4 * sq["C2"]["n_ids"] + 12 * leg["n_rows"] * leg["seq_len"]        # the main kernel's own bytes: the ids in, three int32 tensors out
        res.update({"seqpack_main_kernel_ms": round(ms, 4), "seqpack_main_kernel_launches": n,
                    "seqpack_main_kernel_frac_hbm": round(sq_alg / (ms * 1e-3) / (HBM_TBS * 1e12), 3)})
    out["C2_parts"] = res
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
