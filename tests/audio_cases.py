"""The audio definitions of include/tekken_hip.h restated in numpy float64: layout arithmetic, filter bank, transform tables,
log-mel features with their derived error bracket, and the splice.  Independent of the C++; shared by test_audio_cpu.py and
test_gpu_audio.py, which compute each reference once."""
import base64
import functools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24          # the unit roundoff of float32


def cfg(sr=16000, fr=12.5, M=128, H=160, W=400, chunk=None):
    return {"sampling_rate": sr, "frame_rate": fr, "num_mel_bins": M, "hop_length": H, "window_size": W, "chunk_length_s": chunk}


V = cfg()
V80 = cfg(M=80)
ODD = cfg(sr=1600, fr=10.0, M=10, H=20, W=50)      # nothing of 400 / 201 / 128 holds here


# ---- layout (audio.rs:439-463, 562-591) ----
def chunk_frames(c):
    return int(c["chunk_length_s"] * float(c["sampling_rate"]))


def per_token(c):
    return int(float(c["sampling_rate"]) / c["frame_rate"] / float(c["hop_length"]))


def padded(c, n):
    if c["chunk_length_s"] is not None:
        cf = chunk_frames(c)
        return -(-n // cf) * cf
    return max(n, c["window_size"])


def frames(c, length):
    H = c["hop_length"]
    if length % H == 0:
        return length // H
    return max(int(math.ceil(float(length) / float(H) - 1.0)), 0)


def layout(c, n):
    """(n', frames of the features, N, segments, frames of a segment, samples of a segment)"""
    npad = padded(c, n)
    N = int(math.ceil(float(frames(c, npad)) / float(per_token(c))))
    if c["chunk_length_s"] is not None:
        cf = chunk_frames(c)
        S, Ts = npad // cf, frames(c, cf)
        return npad, S * Ts, N, S, Ts, cf
    return npad, frames(c, npad), N, 1, frames(c, npad), npad


# ---- tables ----
def hertz_to_mel(f):
    return 15.0 + math.log(f / 1000.0) * (27.0 / math.log(6.4)) if f >= 1000.0 else 3.0 * f / 200.0


def mel_to_hertz(m):
    return 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0)) if m >= 15.0 else 200.0 * m / 3.0


@functools.lru_cache(maxsize=None)
def mel_filter_bank(F, M, sr):
    """mel_filter_bank(F, M, 0, sr / 2, sr) (audio.rs:684-748) in float64: [F, M]."""
    mel_min, mel_max = hertz_to_mel(0.0), hertz_to_mel(sr / 2.0)
    ff = [mel_to_hertz(mel_min + (mel_max - mel_min) * i / (M + 1)) for i in range(M + 2)]
    fft = [i * float(sr) / 2.0 / (F - 1) for i in range(F)]
    fb = np.zeros((F, M))
    for m in range(M):
        lo, ce, hi = ff[m], ff[m + 1], ff[m + 2]
        for k, f in enumerate(fft):
            if lo <= f <= ce:
                v = (f - lo) / (ce - lo)
            elif ce < f <= hi:
                v = (hi - f) / (hi - ce)
            else:
                v = 0.0
            fb[k, m] = max(v, 0.0) * (2.0 / (hi - lo))
    return fb


def filter_bank_f32(c):
    """The filter bank as the engine keeps it: built in double, stored as float32 (here: those values, as float64)."""
    return mel_filter_bank(c["window_size"] // 2 + 1, c["num_mel_bins"], c["sampling_rate"]).astype(np.float32).astype(np.float64)


def hann(W):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


def dft_table(W):
    """[W, 2F]: w[i] cos(2 pi i k / W) | -w[i] sin(2 pi i k / W), the angle reduced as i k mod W, float64."""
    F = W // 2 + 1
    i, k = np.arange(W)[:, None], np.arange(F)[None, :]
    ang = 2.0 * np.pi * ((i * k) % W) / W
    w = hann(W)[:, None]
    return np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1)


# ---- features ----
def feat(mel, mx, log_mel_max=None):
    lg = np.log10(np.maximum(mel, 1e-10))
    top = float(log_mel_max) if log_mel_max is not None else math.log10(max(mx, 1e-10))
    return (np.maximum(lg, top - 8.0) + 4.0) / 4.0


def segment_features(c, x, log_mel_max=None):
    """One segment x (float64, padded to its length L): (features [M, T], lo [M, T], hi [M, T]) -- the features and the bracket
    that every exact-f32 evaluation of the definition lies in:
        S_t = sum_i |p[tH + i] w[i]|, delta_t = (W + 8) 2^-24 S_t   (a W-term f32 fma chain in any order, plus the table's rounding)
        dP_k = 2 sqrt(2) |X_k| delta_t + 2 delta_t^2 + 4 * 2^-24 P_k,   dM = dP . FB + 4 * 2^-24 M
    and the feature increases in both mel and the segment maximum."""
    W, H, M = c["window_size"], c["hop_length"], c["num_mel_bins"]
    L = len(x)
    T = frames(c, L)
    assert L > W // 2
    if T == 0:
        z = np.zeros((M, 0))
        return z, z, z
    p = np.pad(x, (W // 2, W // 2), mode="reflect")
    need = (T - 1) * H + W
    assert need <= len(p)
    fr = np.lib.stride_tricks.sliding_window_view(p, W)[::H][:T] * hann(W)[None, :]      # [T, W]
    X = np.fft.rfft(fr, axis=1)                                                             # [T, F]
    P = X.real ** 2 + X.imag ** 2
    FB = filter_bank_f32(c)
    mel = P @ FB                                                                            # [T, M]
    delta = (W + 8) * U * np.abs(fr).sum(axis=1)[:, None]
    dP = 2.0 * math.sqrt(2.0) * np.abs(X) * delta + 2.0 * delta ** 2 + 4.0 * U * P
    dM = dP @ FB + 4.0 * U * mel
    lo_mel, hi_mel = np.maximum(mel - dM, 0.0), mel + dM
    f = feat(mel, mel.max(), log_mel_max)
    lo = feat(lo_mel, (mel - dM).max(), log_mel_max)
    hi = feat(hi_mel, hi_mel.max(), log_mel_max)
    return f.T.copy(), lo.T.copy(), hi.T.copy()


def clip_features(c, x, log_mel_max=None):
    """A clip (float32 samples) -> the list of its segments' (features, lo, hi), each [M, T_s]."""
    x = np.asarray(x, np.float32).astype(np.float64)
    npad, _, _, S, _, seg = layout(c, len(x))
    xp = np.zeros(npad)
    xp[:len(x)] = x
    return [segment_features(c, xp[k * seg:(k + 1) * seg], log_mel_max) for k in range(S)]


def batch_features(c, clips, log_mel_max=None):
    """(features, lo, hi) flat as the engine lays them out, frame_off [S + 1], clip_seg [n + 1]."""
    fs, los, his, fo, cs = [], [], [], [0], [0]
    for x in clips:
        for f, lo, hi in clip_features(c, x, log_mel_max):
            fs.append(f.reshape(-1)); los.append(lo.reshape(-1)); his.append(hi.reshape(-1))
            fo.append(fo[-1] + f.shape[1])
        cs.append(len(fo) - 1)
    cat = lambda a: np.concatenate(a) if a else np.zeros(0)
    return cat(fs), cat(los), cat(his), np.array(fo, np.uint64), np.array(cs, np.uint64)


# ---- splice ----
def splice(ids, offs, tokens, fill):
    out, oo = [], [0]
    for p in range(len(tokens)):
        out.extend(ids[int(offs[p]):int(offs[p + 1])])
        out.extend([fill] * int(tokens[p]))
        oo.append(len(out))
    return np.array(out, np.uint32), np.array(oo, np.uint64)


# ---- signals ----
def signals(n, sr, seed=7):
    """name -> float32 [n]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    out = {
        "noise_0.1": 0.1 * rng.standard_normal(n),
        "noise_1e-4": 1e-4 * rng.standard_normal(n),
        "chirp": 0.5 * np.sin(2.0 * np.pi * (100.0 * t + 1300.0 * t * t)),
        "tone_silence": np.where(np.arange(n) < n // 2, 0.3 * np.sin(2.0 * np.pi * 440.0 * t), 0.0),
        "zeros": np.zeros(n),
        "impulse_first": np.eye(1, n, 0)[0] if n else np.zeros(0),
        "impulse_last": np.eye(1, n, n - 1)[0] if n else np.zeros(0),
        "dc": np.full(n, 0.25),
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


def jfk():
    """The first 2 s of the reference's tests/assets/jfk.wav (mono, 16 kHz), scaled by 2^15."""
    return (np.fromfile(os.path.join(GOLDEN, "jfk_2s_16k.s16le"), "<i2").astype(np.float64) / 32768.0).astype(np.float32)


def vectors():
    with open(os.path.join(GOLDEN, "audio_vectors.json")) as f:
        return json.load(f)


# ---- a tekken.json small enough to write in a test: 256 byte tokens + two words, the control tokens a chat needs ----
SPECIALS = ["<unk>", "<s>", "</s>", "[INST]", "[/INST]", "<pad>", "[AUDIO]", "[BEGIN_AUDIO]"]


def tekken_json(audio=V, version="v7", n_special=16):
    toks = [bytes([i]) for i in range(256)] + [b"hello", b" world"]
    doc = {"config": {"pattern": "x", "num_vocab_tokens": len(toks), "default_vocab_size": len(toks) + n_special,
                      "default_num_special_tokens": n_special, "version": version},
           "vocab": [{"rank": i, "token_bytes": base64.b64encode(t).decode(), "token_str": None} for i, t in enumerate(toks)],
           "special_tokens": [{"rank": i, "token_str": s, "is_control": True} for i, s in enumerate(SPECIALS)]}
    if audio is not None:
        a = {"sampling_rate": audio["sampling_rate"], "frame_rate": audio["frame_rate"],
             "audio_encoding_config": {"num_mel_bins": audio["num_mel_bins"], "hop_length": audio["hop_length"], "window_size": audio["window_size"]}}
        if audio["chunk_length_s"] is not None:
            a["chunk_length_s"] = audio["chunk_length_s"]
        doc["audio"] = a
    return json.dumps(doc)
