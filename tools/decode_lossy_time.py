"""Time lossy decode and the stream step (csrc/tk_decode_lossy.hip) on one MI355X; prints ONE JSON line.

  clean   C2's own ids (1 M x 512 B ASCII): tk_decode_batch_device_lossy against tk_decode_batch_device, interleaved.  The same
          kernels run -- the lossy entry adds nothing where validation finds nothing --, so the two differ by noise only; both
          numbers and the strict entry's own spread are written down.
  dirty   C3's ids (mixed UTF-8, --dirty-docs x 2 KiB) with every 100th document cut after a random id and a run of byte-fallback
          ids spliced into every 1000th: the repair pass alone (events around it), as a fraction of the strict pipeline on the same
          ids, against a device-to-device copy of the same text (the floor: the pass reads the text about twice and writes it
          once), its algorithmic bytes and their fraction of 6.3 TB/s, and against what a caller can do without it: ids and
          offsets to the host, then token-byte joins and errors="replace" over the first --host-docs documents.
  stream  the wall time of one step at 4 096 and 65 536 sequences with 1 and with 8 new ASCII ids each, against
          tk_decode_batch_device on the same ragged ids in the same run (a valid comparator only because the ids are ASCII).

HIP events, warm, median and min, the variants alternating in one process.

    python tools/decode_lossy_time.py [--steps 20] [--warmup 3] [--parts clean,dirty,stream] [--dirty-docs 1000000]
"""
import argparse
import importlib
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

HBM_TBS = 6.3


def med(x):
    return round(float(np.median(x)), 4)


def lo(x):
    return round(float(np.min(x)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="clean,dirty,stream")
    ap.add_argument("--clean-docs", type=int, default=1_000_000)
    ap.add_argument("--dirty-docs", type=int, default=1_000_000)
    ap.add_argument("--host-docs", type=int, default=100_000)
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    P = tk.SpecialTokenPolicy.Ignore
    out = {"tool": "tools/decode_lossy_time.py", "steps": args.steps, "warmup": args.warmup, "hbm_tbs": HBM_TBS,
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

    def encode(kind, n_docs, doc_len):
        data, offs = corpus.generate(kind, n_docs, doc_len, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        d_bytes = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(data), False, False, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_docs + 1, "<i8"), device="cuda").clone()
        torch.cuda.synchronize()
        return d_bytes, ids, oo

    parts = args.parts.split(",")
    if "clean" in parts:
        n_docs = args.clean_docs
        d_bytes, ids, oo = encode("ascii", n_docs, 512)
        t_s, t_l = [], []
        for k in range(args.warmup + args.steps):
            ms_s, rs = timed(lambda: eng.decode_batch_device(ids.data_ptr(), oo.data_ptr(), n_docs, ids.numel(), P, sp))
            ms_l, rl = timed(lambda: eng.decode_batch_device(ids.data_ptr(), oo.data_ptr(), n_docs, ids.numel(), P, sp, errors="replace"))
            if k == 0:
                assert torch.equal(torch.as_tensor(rl[0], device="cuda"), d_bytes) and eng.last_decode_lossy()["repair_launches"] == 0
            if k >= args.warmup:
                t_s.append(ms_s)
                t_l.append(ms_l)
        out["clean"] = {"shape": "C2 ids: %d x 512 B ASCII" % n_docs, "n_ids": int(ids.numel()), "n_bytes": int(d_bytes.numel()),
                        "strict_ms": med(t_s), "strict_min_ms": lo(t_s), "strict_max_ms": round(float(np.max(t_s)), 4),
                        "lossy_ms": med(t_l), "lossy_min_ms": lo(t_l), "lossy_minus_strict_ms": round(med(t_l) - med(t_s), 4),
                        "strict_spread_ms": round(float(np.max(t_s) - np.min(t_s)), 4), "repair_launches": 0}
        print("clean: strict %.3f ms, lossy %.3f ms" % (med(t_s), med(t_l)), file=sys.stderr, flush=True)
        del d_bytes, ids, oo
        torch.cuda.empty_cache()

    if "dirty" in parts:
        n_docs = args.dirty_docs
        d_bytes, ids, oo = encode("mixed", n_docs, 2048)
        del d_bytes
        h_ids, h_oo = ids.cpu().numpy().view(np.uint32), oo.cpu().numpy()
        rng = np.random.default_rng(1)
        lens = h_oo[1:] - h_oo[:-1]
        keep = lens.copy()
        cut = np.arange(0, n_docs, 100)
        keep[cut] = (rng.random(len(cut)) * keep[cut]).astype(np.int64)          # every 100th document: cut after a random id
        doc_of = np.repeat(np.arange(n_docs, dtype=np.int32), lens)
        kept = h_ids[(np.arange(len(h_ids), dtype=np.int64) - h_oo[:-1][doc_of]) < keep[doc_of]]
        del doc_of
        k_oo = np.concatenate([[0], np.cumsum(keep)])
        fallback = np.array([ns + b for b in b"\xf0\x9f\x9a\xe4\xb8\xad\xf0\x9f"], np.uint32)   # a truncated 🚀, 中, a truncated 🚀
        spliced = np.arange(0, n_docs, 1000)                                      # every 1000th: a run of byte-fallback ids spliced in
        at = k_oo[spliced] + keep[spliced] // 2
        new_ids = np.insert(kept, np.repeat(at, len(fallback)), np.tile(fallback, len(spliced)))
        keep[spliced] += len(fallback)
        del kept
        new_oo = np.zeros(n_docs + 1, np.int64)
        new_oo[1:] = np.cumsum(keep)
        assert new_oo[-1] == len(new_ids)
        del ids, oo
        ids = torch.from_numpy(new_ids.view(np.int32)).cuda()
        oo = torch.from_numpy(new_oo).cuda()
        t_rep, t_str, t_all, t_copy = [], [], [], []
        for k in range(args.warmup + args.steps):
            ms_l, rl = timed(lambda: eng.decode_batch_device(ids.data_ptr(), oo.data_ptr(), n_docs, ids.numel(), P, sp, errors="replace"))
            st = eng.last_decode_lossy()
            raw = torch.empty(int(torch.as_tensor(rl[0], device="cuda").numel()), dtype=torch.uint8, device="cuda")
            src = torch.as_tensor(rl[0], device="cuda")
            ms_c, _ = timed(lambda: raw.copy_(src))
            if k >= args.warmup:
                t_all.append(ms_l)
                t_rep.append(st["repair_ms"])
                t_str.append(st["strict_ms"])
                t_copy.append(ms_c)
        n_out = int(src.numel())
        del raw, src
        # the pass reads the raw text twice (counts, write) with its run bits and the old offsets, writes the text and the offsets once
        n_raw = n_out - 2 * st["n_replaced"]           # an upper bound of the raw text (a replacement grows it by at most 2 bytes)
        alg = 2 * (n_raw + n_raw // 8) + n_out + 3 * 8 * (n_docs + 1)
        # what a caller can do today: ids and offsets to the host, token-byte joins, errors="replace"
        nh = min(args.host_docs, n_docs)
        t0 = time.perf_counter()
        c_ids, c_oo = ids.cpu().numpy().view(np.uint32), oo.cpu().numpy()
        t1 = time.perf_counter()
        texts = [b"".join(toks[i - ns] for i in c_ids[int(c_oo[d]):int(c_oo[d + 1])].tolist() if i >= ns).decode("utf-8", "replace") for d in range(nh)]
        t2 = time.perf_counter()
        del texts
        out["dirty"] = {"shape": "C3 ids: %d x 2 KiB mixed UTF-8, every 100th document cut, fallback ids in every 1000th" % n_docs,
                        "n_ids": int(ids.numel()), "n_text_bytes": n_out, "n_replaced": st["n_replaced"], "n_bad_docs": st["n_bad_docs"],
                        "repair_ms": med(t_rep), "repair_min_ms": lo(t_rep), "strict_ms": med(t_str), "strict_min_ms": lo(t_str),
                        "repair_over_strict": round(med(t_rep) / med(t_str), 3), "call_ms": med(t_all),
                        "d2d_copy_ms": med(t_copy), "d2d_copy_min_ms": lo(t_copy), "repair_over_copy": round(med(t_rep) / med(t_copy), 2),
                        "alg_bytes": int(alg), "tb_s": round(alg / (med(t_rep) * 1e-3) / 1e12, 3),
                        "frac_hbm": round(alg / (med(t_rep) * 1e-3) / (HBM_TBS * 1e12), 3),
                        "host_docs": nh, "host_copy_ms": round((t1 - t0) * 1e3, 1), "host_join_replace_ms": round((t2 - t1) * 1e3, 1),
                        "host_ms_per_1000_docs": round((t2 - t1) * 1e3 / nh * 1000, 3),
                        "gpu_call_ms_per_1000_docs": round(med(t_all) / n_docs * 1000, 5)}
        print("dirty: repair %.3f ms, strict %.3f ms, copy %.3f ms" % (med(t_rep), med(t_str), med(t_copy)), file=sys.stderr, flush=True)
        del ids, oo
        torch.cuda.empty_cache()

    if "stream" in parts:
        res = {}
        rng = np.random.default_rng(2)
        for n_seqs in (4096, 65536):
            for per in (1, 8):
                h = (ns + rng.integers(0x20, 0x7F, n_seqs * per)).astype(np.uint32)
                ids = torch.from_numpy(h.view(np.int32)).cuda()
                oo = torch.arange(0, n_seqs * per + 1, per, dtype=torch.int64, device="cuda")
                s = eng.decode_stream(n_seqs, P)
                t_st, t_bt = [], []
                for k in range(args.warmup + args.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    v = s.step_device(ids.data_ptr(), oo.data_ptr(), n_seqs * per, 0, sp)
                    t1 = time.perf_counter()
                    w = eng.decode_batch_device(ids.data_ptr(), oo.data_ptr(), n_seqs, n_seqs * per, P, sp)
                    t2 = time.perf_counter()
                    if k == 0:
                        assert torch.as_tensor(w[0], device="cuda").cpu().numpy().tobytes() == bytes((h - ns).astype(np.uint8))
                        v = s.step_device(ids.data_ptr(), oo.data_ptr(), n_seqs * per, 0, sp)
                        assert torch.as_tensor(v[0], device="cuda").cpu().numpy().tobytes() == bytes((h - ns).astype(np.uint8))
                    if k >= args.warmup:
                        t_st.append((t1 - t0) * 1e3)
                        t_bt.append((t2 - t1) * 1e3)
                res["%d_seqs_x_%d" % (n_seqs, per)] = {"stream_step_wall_ms": med(t_st), "stream_step_wall_min_ms": lo(t_st),
                                                        "strict_batch_wall_ms": med(t_bt), "strict_batch_wall_min_ms": lo(t_bt),
                                                        "stream_over_strict": round(med(t_st) / med(t_bt), 2)}
                print("stream %d x %d: step %.3f ms, strict batch %.3f ms" % (n_seqs, per, med(t_st), med(t_bt)), file=sys.stderr, flush=True)
        out["stream"] = res
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
