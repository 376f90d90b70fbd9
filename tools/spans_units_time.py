"""Time the units pass and the annotation look-up (csrc/tk_spans_units.hip) on one MI355X; prints ONE JSON line and
writes it to profiles/spans_units_time.json.

Shapes: the bench's C2 corpus (1 M x 512-byte ASCII documents) and C3 (1 M x 2 KiB mixed UTF-8), encoded once with BOS / EOS.
Legs, alternated in one process, HIP events around each, warm, median and min of --steps; every leg ends in its one host wait:
  bytes       tk_token_spans_device without checks: existing code with the same global traffic (4 B in, 8 B out per id)
  char, utf16 tk_token_spans_units_device in the two units
  locate      tk_spans_locate_device, 8 random annotations a document over the char spans
  torch       a torch composition of the same definition over the same device arrays (a per-rank table gather, a cumulative sum
              and a cumulative maximum with per-document bases), checked equal to the char leg at the first step (and, with the UTF-16 columns of
              its table, to the utf16 leg)
The bytes leg is run TWICE per step (bytes, bytes_again), which shows the spread inside one process.  The spread the units legs
are read against is the byte pass's own from run to run: --bytes-only times the bytes leg alone (a library built from the parent
commit, selected with TK_HIP_LIB, has no units entries), and --parent-runs takes the JSON lines of two such runs and records
their medians, their difference (parent_spread_ms) and how far the units legs lie from the byte leg of this run.

    python tools/spans_units_time.py [--steps 20] [--warmup 3] [--shapes C2,C3] [--no-torch] [--bytes-only]
                                     [--parent-runs A.json B.json] [--out profiles/spans_units_time.json]
"""
import argparse
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
SHAPES = {"C2": ("ascii", 1_000_000, 512), "C3": ("mixed", 1_000_000, 2048)}
ANN_PER_DOC = 8


def rank_tables(toks, ns):
    """By id, for code points and for UTF-16 units: the units, the units in front of the last character start + 1 (0: no start);
    and whether the first byte starts a character."""
    n = ns + len(toks)
    un, last1, un16, last16, first = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, bool)
    for r, t in enumerate(toks):
        a = np.frombuffer(t, np.uint8)
        st = (a & 0xC0) != 0x80
        k, four = int(st.sum()), int((a >= 0xF0).sum())
        last4 = int(a[np.nonzero(st)[0][-1]] >= 0xF0) if k else 0
        un[ns + r], last1[ns + r], first[ns + r] = k, k, len(a) == 0 or bool(st[0])
        un16[ns + r], last16[ns + r] = k + four, (k + four - last4) if k else 0
    return un, last1, un16, last16, first


def torch_char_spans(torch, ids, oo, t_un, t_last1, t_first):
    i = ids.to(torch.int64)
    un = t_un[i]
    excl = torch.cumsum(un, 0) - un
    doc = torch.repeat_interleave(torch.arange(oo.numel() - 1, device=ids.device), oo[1:] - oo[:-1], output_size=ids.numel())
    starts = oo[:-1].clamp(max=ids.numel() - 1)
    base = excl[starts][doc]
    l1 = t_last1[i]
    cand = torch.where(l1 > 0, excl + l1, torch.zeros_like(excl))
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=ids.device), torch.cummax(cand, 0).values[:-1]])
    lead = torch.maximum(before - 1, base)
    st = torch.where(t_first[i], excl, lead) - base
    return torch.stack([st, excl + un - base], 1).to(torch.int32)


def same(torch, got, exp, oo, what):
    """Both [n, 2] tensors equal, or stop and say where they differ."""
    if torch.equal(got, exp):
        return
    bad = (got != exp).any(1).nonzero().flatten()
    i = int(bad[0])
    d = int(torch.searchsorted(oo, torch.tensor([i], device=oo.device), right=True)[0]) - 1
    raise SystemExit("%s: %d of %d ids differ, first id %d (document %d, ids %d..%d): got %s, expected %s; last differing id %d" %
                     (what, bad.numel(), got.shape[0], i, d, int(oo[d]), int(oo[d + 1]), got[i].tolist(), exp[i].tolist(), int(bad[-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--bytes-only", action="store_true")
    ap.add_argument("--parent-runs", nargs=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans_units_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/spans_units_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS, "ann_per_doc": ANN_PER_DOC,
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.node()}}
    try:
        with open(os.path.join(ROOT, "tekken-rs_amd", "BUILD_INFO.json")) as f:
            out["build"] = json.load(f).get("git")
    except OSError:
        pass
    parents = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent_runs] if args.parent_runs else None
    if args.bytes_only:
        args.no_torch = True
    if not args.no_torch:
        t_un, t_last1, t_un16, t_last16, t_first = (torch.from_numpy(x).cuda() for x in rank_tables(toks, ns))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for name in args.shapes.split(","):
        kind, D, doc_len = SHAPES[name]
        data, offs = corpus.generate(kind, D, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), True, True, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, D + 1, "<i8"), device="cuda").clone()
        del d_bytes
        if args.bytes_only:
            torch.cuda.synchronize()
            ts = []
            for k in range(args.warmup + args.steps):
                ms, _ = timed(lambda: eng.token_spans_device(ids.data_ptr(), oo.data_ptr(), D, n, 0, 0, 0, sp))
                if k >= args.warmup:
                    ts.append(ms)
            out[name] = {"n_docs": D, "n_ids": n, "bytes_ms": round(float(np.median(ts)), 4), "bytes_min_ms": round(float(np.min(ts)), 4)}
            del ids, oo
            continue
        p_char = eng.token_spans_units_device(ids.data_ptr(), oo.data_ptr(), D, n, tk.UNIT_CHAR, sp)
        chars = torch.as_tensor(tk.DeviceView(p_char, (n, 2), "<i4"), device="cuda").clone()
        # annotations: a start inside the document's characters, up to 40 of them long
        n_char = chars[:, 1][(oo[1:] - 1).clamp(min=0)].to(torch.int64)
        A = D * ANN_PER_DOC
        g = torch.Generator(device="cuda").manual_seed(7)
        ann_doc = torch.arange(D, device="cuda", dtype=torch.int32).repeat_interleave(ANN_PER_DOC)
        a0 = (torch.rand(A, device="cuda", generator=g) * n_char.repeat_interleave(ANN_PER_DOC)).to(torch.int32)
        ann = torch.stack([a0, a0 + torch.randint(1, 41, (A,), device="cuda", generator=g, dtype=torch.int32)], 1).contiguous()
        torch.cuda.synchronize()
        byte_leg = lambda: eng.token_spans_device(ids.data_ptr(), oo.data_ptr(), D, n, 0, 0, 0, sp)
        legs = {"bytes": byte_leg,
                "char": lambda: eng.token_spans_units_device(ids.data_ptr(), oo.data_ptr(), D, n, tk.UNIT_CHAR, sp),
                "utf16": lambda: eng.token_spans_units_device(ids.data_ptr(), oo.data_ptr(), D, n, tk.UNIT_UTF16, sp),
                "bytes_again": byte_leg,
                "locate": lambda: eng.spans_locate_device(chars.data_ptr(), oo.data_ptr(), D, n, ann_doc.data_ptr(), ann.data_ptr(), A, sp)}
        if not args.no_torch:
            legs["torch"] = lambda: torch_char_spans(torch, ids, oo, t_un, t_last1, t_first)
        t = {k: [] for k in legs}
        for k in range(args.warmup + args.steps):
            got = {}
            for leg, fn in legs.items():
                ms, got[leg] = timed(fn)
                if k >= args.warmup:
                    t[leg].append(ms)
                if k == 0 and leg == "utf16" and not args.no_torch:
                    same(torch, torch.as_tensor(tk.DeviceView(got["utf16"], (n, 2), "<i4"), device="cuda"),
                         torch_char_spans(torch, ids, oo, t_un16, t_last16, t_first), oo, name + ": the utf16 kernel against the torch composition")
                if k == 0 and leg == "char":      # (checked here: the utf16 leg writes the same context-owned buffer next)
                    same(torch, torch.as_tensor(tk.DeviceView(got["char"], (n, 2), "<i4"), device="cuda"), chars, oo, name + ": second char call against the first")
            if k == 0:
                if "torch" in got:
                    same(torch, chars, got["torch"], oo, name + ": the kernel against the torch composition")
                rng = torch.as_tensor(tk.DeviceView(got["locate"], (A, 2), "<i4"), device="cuda")
                assert bool((rng[:, 1] >= rng[:, 0]).all()) and bool((rng[:, 1] > rng[:, 0]).any())
            del got
        med = {k: float(np.median(v)) for k, v in t.items()}
        alg = 12 * n
        res = {"n_docs": D, "n_bytes": int(len(data)), "n_ids": n, "n_ann": A, "alg_bytes": alg}
        for leg in legs:
            res[leg + "_ms"] = round(med[leg], 4)
            res[leg + "_min_ms"] = round(float(np.min(t[leg])), 4)
        res["bytes_spread_ms"] = round(abs(med["bytes"] - med["bytes_again"]), 4)
        for leg in ("bytes", "char", "utf16"):
            res[leg + "_frac_hbm"] = round(alg / (med[leg] * 1e-3) / (HBM_TBS * 1e12), 3)
        res["char_over_bytes"] = round(med["char"] / med["bytes"], 3)
        res["utf16_over_bytes"] = round(med["utf16"] / med["bytes"], 3)
        res["locate_ns_per_ann"] = round(med["locate"] * 1e6 / A, 3)
        if parents:
            pm = [p[name]["bytes_ms"] for p in parents]
            res["parent_bytes_ms"] = pm
            res["parent_spread_ms"] = round(abs(pm[0] - pm[1]), 4)
            for leg in ("char", "utf16"):
                res[leg + "_minus_bytes_ms"] = round(med[leg] - med["bytes"], 4)
                res[leg + "_within_parent_spread"] = bool(med[leg] - med["bytes"] <= abs(pm[0] - pm[1]))
        if "torch" in med:
            res["torch_over_char"] = round(med["torch"] / med["char"], 2)
        out[name] = res
        del ids, oo, chars, ann, ann_doc, a0, n_char
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
