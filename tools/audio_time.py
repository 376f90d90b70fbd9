"""Time the audio pass (csrc/tk_audio.hip) on one MI355X; prints ONE JSON line and writes it to
profiles/audio_time.json.

Log-mel, HIP events, warm, the median of --steps, on seeded Gaussian noise:
  chunk1024 / chunk64   1024 and 64 clips of 30 s at the Voxtral config with chunk_length_s = 30 (S x [128, 3000])
  ragged4096            4096 clips of 1 .. 20 s, unchunked
per shape the call, and inside it the product and the clamp kernel as the library's own events see them (tk_last_logmel_ms); the
f32-MFMA floor of the transform as built (its flop count / 157.3 TF) and the fraction reached; the HBM floor (samples read once,
features written once and rewritten by the clamp, at --hbm-tbs); and, for the chunked shapes, the same definition composed from
torch on the same device (torch.stft, abs()**2, a matmul with the f32 filter bank, log10, per-segment max, clamp, scale).
Accuracy record (no assertion): for the jfk excerpt and the chirp, max and RMS deviation from the float64 restatement
(tests/audio_cases.py), beside the same for torch's f32 composition on the CPU.
Splice: C2 (1 M x 512 B ASCII) as parts, every fourth part an audio part of 375 tokens: splice + join beside the plain join.

    python tools/audio_time.py [--steps 10] [--warmup 2] [--shapes chunk1024,chunk64,ragged4096,splice] [--out profiles/audio_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_cases as ac  # noqa: E402
import corpus  # noqa: E402
import synth_vocab as sv  # noqa: E402

PEAK_F32_MFMA_TF = 157.3


def torch_logmel(torch, x, W, H, fb):
    """x [S, L] float32 on the device -> [S, M, T]: the definition composed from torch."""
    st = torch.stft(x, W, H, window=torch.hann_window(W, device=x.device), center=True, pad_mode="reflect", return_complex=True)
    mel = torch.matmul(fb.T, st[..., :-1].abs() ** 2)
    lg = torch.clamp(mel, min=1e-10).log10()
    lg = torch.maximum(lg, lg.amax(dim=(-2, -1), keepdim=True) - 8.0)
    return (lg + 4.0) / 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="chunk1024,chunk64,ragged4096,splice")
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_time.json"))
    args = ap.parse_args()
    import torch
    tk = importlib.import_module("tekken-rs_amd")
    toks, ns, bos, eos = sv.load_tokens(sv.ensure_default())
    eng = tk.Engine(toks, ns, bos, eos, device=0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"tool": "tools/audio_time.py", "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "frame_tile": int(tk.lib().tk_audio_frame_tile()), "peak_f32_mfma_tf": PEAK_F32_MFMA_TF, "hbm_tbs_assumed": args.hbm_tbs}
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
    W, H, M, F = 400, 160, 128, 201
    tile = out["frame_tile"]
    for name in args.shapes.split(","):
        if name == "splice":
            continue
        c = ac.cfg(chunk=30.0) if name.startswith("chunk") else ac.cfg()
        eng.audio_set_config(c)
        g = torch.Generator(device="cuda").manual_seed(1)
        if name.startswith("chunk"):
            n_clips = int(name[5:])
            lens = np.full(n_clips, 480000, np.int64)
        else:
            n_clips = 4096
            lens = np.random.default_rng(1).integers(16000, 20 * 16000 + 1, n_clips).astype(np.int64)
        offs = np.zeros(n_clips + 1, np.int64)
        offs[1:] = np.cumsum(lens)
        n = int(offs[-1])
        x = 0.1 * torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
        d_o = torch.from_numpy(offs).cuda()
        a = (x.data_ptr(), d_o.data_ptr(), n_clips, n)
        t_call, t_st = [], []
        for k in range(args.warmup + args.steps):
            ms, r = timed(lambda: eng.audio_logmel_device(*a, stream=sp))
            if k >= args.warmup:
                t_call.append(ms); t_st.append(eng.last_logmel_ms())
        st = np.median(np.array(t_st), axis=0)
        # the product as built: per tile of `tile` frames, ceil(F / 32) blocks of 32 bins x (real, imaginary) x W samples
        fo = torch.as_tensor(r.views()[1], device="cuda").cpu().numpy()
        tiles = int(sum(-(-int(t) // tile) for t in np.diff(fo)))
        flop = tiles * tile * (-(-F // 32) * 32) * 2 * W * 2
        useful = int(r.n_frames) * F * 2 * W * 2
        hbm = n * 4 + int(r.n_frames) * M * 4 * 3
        rec = {"n_clips": n_clips, "n_samples": n, "n_segments": int(r.n_segments), "n_frames": int(r.n_frames), "call_ms": med(t_call),
               "call_min_ms": round(float(np.min(t_call)), 4), "product_ms": round(float(st[0]), 4), "clamp_ms": round(float(st[1]), 4),
               "product_flop_as_built": flop, "product_flop_useful": useful, "mfma_floor_ms": round(flop / (PEAK_F32_MFMA_TF * 1e12) * 1e3, 4),
               "mfma_fraction": round(flop / (PEAK_F32_MFMA_TF * 1e12) * 1e3 / float(st[0]), 3),
               "product_tflops_as_built": round(flop / (float(st[0]) * 1e-3) / 1e12, 1),
               "hbm_bytes": hbm, "hbm_floor_ms": round(hbm / (args.hbm_tbs * 1e12) * 1e3, 4)}
        if name.startswith("chunk"):
            fb = torch.from_numpy(ac.filter_bank_f32(c).astype(np.float32)).cuda()
            xs = x.reshape(n_clips, 480000)
            ref = torch_logmel(torch, xs[:4], W, H, fb)
            got = torch.as_tensor(r.views()[0], device="cuda").reshape(n_clips, M, 3000)[:4]
            rec["max_abs_vs_torch_first4"] = float((got - ref).abs().max())
            del ref, got
            t_torch = []
            for k in range(args.warmup + args.steps):
                ms, y = timed(lambda: torch_logmel(torch, xs, W, H, fb))
                del y
                if k >= args.warmup:
                    t_torch.append(ms)
            rec["torch_ms"] = med(t_torch)
            rec["torch_over_call"] = round(float(np.median(t_torch)) / float(np.median(t_call)), 3)
        out[name] = rec
        print("%s: %s" % (name, json.dumps(rec)), file=sys.stderr, flush=True)
        del x, d_o
        torch.cuda.empty_cache()

    # ---- accuracy record
    eng.audio_set_config(ac.V)
    acc = {}
    for sig, x in (("jfk", ac.jfk()), ("chirp", ac.signals(32000, 16000)["chirp"])):
        (exp, _, _), = ac.clip_features(ac.V, x)
        h = eng.audio_logmel(x, np.array([0, len(x)], np.uint64))
        got = h["features"].reshape(M, -1).astype(np.float64)
        tcpu = torch_logmel(torch, torch.from_numpy(x)[None], W, H, torch.from_numpy(ac.filter_bank_f32(ac.V).astype(np.float32)))[0].numpy().astype(np.float64)
        acc[sig] = {"hip_max": float(np.abs(got - exp).max()), "hip_rms": float(np.sqrt(((got - exp) ** 2).mean())),
                    "torch_f32_cpu_max": float(np.abs(tcpu - exp).max()), "torch_f32_cpu_rms": float(np.sqrt(((tcpu - exp) ** 2).mean()))}
    out["accuracy_vs_float64"] = acc
    print("accuracy: %s" % json.dumps(acc), file=sys.stderr, flush=True)

    # ---- splice + join against the plain join
    if "splice" in args.shapes.split(","):
        n_parts = 1_000_000
        data, doffs = corpus.generate("ascii", n_parts, 512, seed=corpus.BASE_SEED + 1, threads=min(16, os.cpu_count() or 1))
        d_bytes, d_offs = torch.from_numpy(data).cuda(), torch.from_numpy(doffs.astype(np.int64)).cuda()
        p_ids, p_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, len(data), False, False, sp)
        ids = torch.as_tensor(tk.DeviceView(p_ids, n_ids, "<i4"), device="cuda").clone()
        oo = torch.as_tensor(tk.DeviceView(p_oo, n_parts + 1, "<i8"), device="cuda").clone()
        tokens = np.zeros(n_parts, np.uint32)
        tokens[3::4] = 375
        ctrl = np.full(n_parts, tk.JOIN_NONE, np.uint32)
        ctrl[3::4] = 7
        conv = np.arange(0, n_parts + 1, 4, dtype=np.int64)
        d_tok, d_ctrl, d_conv = (torch.from_numpy(v).cuda() for v in (tokens.view(np.int32), ctrl.view(np.int32), conv))
        t_sp, t_sj, t_j = [], [], []
        for k in range(args.warmup + args.steps):
            ms_s, r = timed(lambda: eng.audio_splice_device(ids.data_ptr(), oo.data_ptr(), n_parts, n_ids, d_tok.data_ptr(), 6, sp))
            ms_a, j = timed(lambda: eng.join_from_ids_device(r.ids_ptr, r.offsets_ptr, n_parts, r.n_ids, d_ctrl.data_ptr(), 0, d_conv.data_ptr(),
                                                             len(conv) - 1, flags=tk.JOIN_LABELS, stream=sp))
            ms_p, jp = timed(lambda: eng.join_from_ids_device(ids.data_ptr(), oo.data_ptr(), n_parts, n_ids, d_ctrl.data_ptr(), 0, d_conv.data_ptr(),
                                                              len(conv) - 1, flags=tk.JOIN_LABELS, stream=sp))
            if k >= args.warmup:
                t_sp.append(ms_s); t_sj.append(ms_s + ms_a); t_j.append(ms_p)
        out["splice"] = {"n_parts": n_parts, "n_ids_in": n_ids, "n_ids_spliced": int(r.n_ids), "splice_ms": med(t_sp), "splice_join_ms": med(t_sj),
                         "plain_join_ms": med(t_j), "splice_gbs": round((n_ids + int(r.n_ids)) * 4 / (float(np.median(t_sp)) * 1e-3) / 1e9, 1),
                         "n_ids_joined": int(j.n_ids), "n_ids_plain": int(jp.n_ids)}
        print("splice: %s" % json.dumps(out["splice"]), file=sys.stderr, flush=True)
    eng.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
