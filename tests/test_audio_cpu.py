"""Audio without a GPU: the loader keeps the audio config (through the model cache too), the tokenizer-level entries, the host layout
arithmetic, the tables header, the float64 restatement pinned against torch.stft, and Audio.from_wav."""
import io
import os
import subprocess
import wave

import numpy as np
import pytest

import audio_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [(176000, None, 176000, 1100, 138), (176000, 30.0, 480000, 3000, 375), (480001, 30.0, 960000, 6000, 750), (0, None, 400, 2, 1),
         (1, None, 400, 2, 1), (0, 30.0, 0, 0, 0)]       # n, chunk, n', T, N at sr = 16000, fr = 12.5, H = 160, W = 400


def load(tk, audio, **kw):
    return tk.Tekkenizer.from_json(ac.tekken_json(audio, **kw), device=-1)


def test_loader_keeps_the_config_and_ids(tk):
    for c in (ac.V, ac.cfg(chunk=30.0), ac.ODD, ac.cfg(sr=44100, fr=12.5, M=80, H=441, W=1023, chunk=0.25)):
        t = load(tk, c)
        assert t.has_audio_support and t.audio_config == c
        assert (t.audio_token_id, t.begin_audio_token_id) == (ac.SPECIALS.index("[AUDIO]"), ac.SPECIALS.index("[BEGIN_AUDIO]"))
        assert t.get_control_token("[AUDIO]") == t.audio_token_id
        t.close()


def test_config_survives_the_model_cache(tk, tmp_path, monkeypatch):
    monkeypatch.setenv("TK_TABLE_CACHE_DIR", str(tmp_path / "cache"))
    os.makedirs(str(tmp_path / "cache"))
    c = ac.cfg(chunk=30.0)
    path = tmp_path / "tekken.json"
    path.write_text(ac.tekken_json(c))
    a = tk.Tekkenizer.from_file(str(path), device=-1)
    b = tk.Tekkenizer.from_file(str(path), device=-1)
    assert not a.from_cache() and b.from_cache()
    for t in (a, b):
        assert t.has_audio_support and t.audio_config == c and t.audio_token_id == 6 and t.begin_audio_token_id == 7
        assert t.encode_audio(tk.Audio(np.zeros(176000, np.float32), 16000))[0] == [7] + [6] * 375
    plain = tmp_path / "plain.json"
    plain.write_text(ac.tekken_json(None))
    p1, p2 = tk.Tekkenizer.from_file(str(plain), device=-1), tk.Tekkenizer.from_file(str(plain), device=-1)
    assert p2.from_cache() and not p1.has_audio_support and not p2.has_audio_support and p2.audio_config is None


@pytest.mark.parametrize("n,chunk,npad,T,N", TABLE)
def test_encode_audio_against_the_table(tk, n, chunk, npad, T, N):
    t = load(tk, ac.cfg(chunk=chunk))
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    ids, padded = t.encode_audio(tk.Audio(x, 16000))
    assert ids == [t.begin_audio_token_id] + [t.audio_token_id] * N
    assert len(padded) == npad and padded.sampling_rate == 16000
    assert np.array_equal(padded.audio_array[:n], x) and not padded.audio_array[n:].any()
    assert ac.layout(ac.cfg(chunk=chunk), n)[:3:2] == (npad, N) and ac.frames(ac.cfg(chunk=chunk), npad) == T
    out = t.encode_audio_batch([tk.Audio(x, 16000)] * 2, return_features=False)
    assert out["ids"].tolist() == ids * 2 and out["offsets"].tolist() == [0, N + 1, 2 * N + 2] and out["tokens_per_clip"].tolist() == [N, N]


def test_audio_errors(tk):
    t = load(tk, ac.V)
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_audio(tk.Audio(np.zeros(100, np.float32), 8000))
    assert e.value.code == tk.TK_ERR_AUDIO and e.value.kind == "Audio" and "Resampling not yet implemented" in str(e.value)
    p = load(tk, None, version="v3")
    assert not p.has_audio_support and p.audio_config is None
    for call in (lambda: p.encode_audio(tk.Audio(np.zeros(100, np.float32), 16000)), lambda: p.audio_token_id, lambda: p.begin_audio_token_id):
        with pytest.raises(tk.TokenizerError) as e:
            call()
        assert e.value.code == tk.TK_ERR_AUDIO and "Audio encoder not configured" in str(e.value)
    # no whole frame per token: the reference would divide by zero
    z = load(tk, ac.cfg(fr=200.0))
    with pytest.raises(tk.TokenizerError) as e:
        z.encode_audio(tk.Audio(np.zeros(100, np.float32), 16000))
    assert e.value.code == tk.TK_ERR_INVALID_CONFIG


CONFIGS = [ac.V, ac.cfg(chunk=0.1), ac.cfg(chunk=30.0), ac.ODD]


@pytest.mark.parametrize("c", CONFIGS, ids=["V", "V-0.1s", "V-30s", "ODD"])
def test_layout_against_the_restatement(tk, c):
    W, H = c["window_size"], c["hop_length"]
    cf = ac.chunk_frames(c) if c["chunk_length_s"] is not None else 1600
    ns = [0, 1, H - 1, H, W - 1, W, W + 1, cf - 1, cf, cf + 1, 2 * cf]
    padded, n_frames, n_tokens, n_seg = tk.audio_layout(c, ns)
    exp = [ac.layout(c, n) for n in ns]
    assert padded.tolist() == [e[0] for e in exp] and n_frames.tolist() == [e[1] for e in exp]
    assert n_tokens.tolist() == [e[2] for e in exp] and n_seg.tolist() == [e[3] for e in exp]
    assert all(len(x) == 0 for x in tk.audio_layout(c, []))


def test_layout_refuses_what_divides_by_zero(tk):
    for bad in (ac.cfg(fr=200.0), ac.cfg(H=0), ac.cfg(sr=0), ac.cfg(fr=0.0), ac.cfg(chunk=0.0), ac.cfg(chunk=1e-6), ac.cfg(M=0), ac.cfg(W=0)):
        with pytest.raises(tk.TokenizerError) as e:
            tk.audio_layout(bad, [100])
        assert e.value.code == tk.TK_ERR_INVALID_CONFIG


def test_float_frame_form_equals_floor():
    # the float expression of audio.rs:572 is what is mirrored; at H = 160 it is floor(n' / H)
    c = ac.V
    assert all(ac.frames(c, n) == n // 160 for n in range(400, 200000))


def test_recorded_vectors():
    v = ac.vectors()
    assert len(v["layout"]) >= 40
    for row in v["layout"]:
        npad, _, N, S, Ts, _ = ac.layout(row["config"], row["n"])
        assert (npad, ac.frames(row["config"], npad), N, S, Ts) == (row["padded"], row["frames"], row["tokens"], row["segments"], row["segment_frames"])
    for b in v["filter_banks"]:
        fb = ac.mel_filter_bank(b["F"], b["M"], b["sr"])
        assert np.allclose(fb.sum(axis=0), b["column_sums"], rtol=1e-12, atol=0)
        for k, m, val in b["spots"]:
            assert abs(fb[k, m] - val) <= 1e-15 + 1e-12 * abs(val)
        # at these configs a bin feeds at most 2 filters
        assert ((fb > 0).sum(axis=1) <= 2).all() and (fb[0] == 0).all()


@pytest.fixture(scope="module")
def tables_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("audio") / "audio_tables_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "audio_tables_check.cpp")])
    return exe


@pytest.mark.parametrize("c", [ac.V, ac.V80, ac.ODD, ac.cfg(chunk=0.1)], ids=["V", "V80", "ODD", "V-0.1s"])
def test_tables_header_against_the_restatement(tables_exe, c):
    ns = [0, 1, 399, 400, 401, 1599, 1600, 1601, 176000]
    chunk = -1.0 if c["chunk_length_s"] is None else c["chunk_length_s"]
    r = subprocess.run([tables_exe] + [repr(c[k]) for k in ("sampling_rate", "frame_rate", "num_mel_bins", "hop_length", "window_size")] +
                       [repr(chunk)] + [str(n) for n in ns], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    raw = r.stdout
    W, F, M, nw = np.frombuffer(raw, "<u4", 4).tolist()
    assert (W, F, M) == (c["window_size"], c["window_size"] // 2 + 1, c["num_mel_bins"])
    at = 16
    dft = np.frombuffer(raw, "<f4", W * 2 * F, at).reshape(W, 2 * F); at += 4 * W * 2 * F
    first, count, start = (np.frombuffer(raw, "<u4", M, at + 4 * M * i) for i in range(3)); at += 12 * M
    weights = np.frombuffer(raw, "<f4", nw, at); at += 4 * nw
    rows = np.frombuffer(raw, "<u8", 3 * len(ns), at).reshape(-1, 3)
    # the DFT matrix: computed in double and rounded once (the libm's last bit of cos / sin may differ from numpy's)
    exp = ac.dft_table(W)
    assert np.abs(dft.astype(np.float64) - exp).max() <= 2.0 ** -24 * 1.001
    assert (dft[0] == 0).all() and (dft[:, F] == 0).all()      # w[0] = 0; the imaginary part of bin 0
    # the filter bank: one run per filter that holds exactly its f32 weights
    fb = ac.mel_filter_bank(F, M, c["sampling_rate"])
    dense = np.zeros((F, M), np.float32)
    for m in range(M):
        assert start[m] + count[m] <= nw and first[m] + count[m] <= F
        dense[first[m]:first[m] + count[m], m] = weights[start[m]:start[m] + count[m]]
        assert count[m] == 0 or (weights[start[m]] != 0 and weights[start[m] + count[m] - 1] != 0)
    assert np.abs(dense.astype(np.float64) - fb).max() <= np.abs(fb).max() * 2.0 ** -23
    assert ((dense != 0) == (fb.astype(np.float32) != 0)).all()
    for n, (npad, fr, ntok) in zip(ns, rows.tolist()):
        e = ac.layout(c, n)
        assert (npad, fr, ntok) == (e[0], ac.frames(c, e[0]), e[2])


@pytest.mark.parametrize("c,name", [(ac.V, "chirp"), (ac.V80, "noise_0.1"), (ac.ODD, "tone_silence"), (ac.cfg(chunk=0.1), "noise_1e-4"), (ac.V, "jfk")])
def test_restatement_against_torch_stft(c, name):
    torch = pytest.importorskip("torch")
    n = 3000 if c is not ac.ODD else 777
    x = ac.jfk()[:8000] if name == "jfk" else ac.signals(n, c["sampling_rate"])[name]
    W, H = c["window_size"], c["hop_length"]
    FB = torch.from_numpy(ac.filter_bank_f32(c))
    for (got, lo, hi), k in zip(ac.clip_features(c, x), range(10 ** 6)):
        npad, _, _, _, Ts, seg = ac.layout(c, len(x))
        xp = np.zeros(npad)
        xp[:len(x)] = x.astype(np.float64)
        s = torch.from_numpy(xp[k * seg:(k + 1) * seg])
        st = torch.stft(s, W, H, window=torch.hann_window(W, dtype=torch.float64), center=True, pad_mode="reflect", return_complex=True)
        mel = (st[:, :-1].abs() ** 2).T @ FB                   # the last frame dropped
        assert mel.shape[0] >= Ts
        lg = torch.clamp(mel[:Ts], min=1e-10).log10()
        lg = torch.maximum(lg, lg.max() - 8.0)
        exp = ((lg + 4.0) / 4.0).T.numpy()
        assert got.shape == exp.shape == (c["num_mel_bins"], Ts)
        assert np.abs(got - exp).max() < 1e-9
        assert (lo <= got).all() and (got <= hi).all()


def test_bracket_is_tight_enough_and_holds_torch_f32():
    torch = pytest.importorskip("torch")
    c = ac.V
    x = ac.jfk()
    (got, lo, hi), = ac.clip_features(c, x)
    assert ((hi - lo) < 0.01).mean() >= 0.92
    st = torch.stft(torch.from_numpy(x), 400, 160, window=torch.hann_window(400), center=True, pad_mode="reflect", return_complex=True)
    mel = (st[:, :-1].abs() ** 2).T @ torch.from_numpy(ac.filter_bank_f32(c).astype(np.float32))
    lg = torch.clamp(mel, min=1e-10).log10()
    f32 = ((torch.maximum(lg, lg.max() - 8.0) + 4.0) / 4.0).T.numpy().astype(np.float64)
    assert (lo - 1e-6 <= f32).all() and (f32 <= hi + 1e-6).all()


def _wav(ch, width, rate, frames):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(ch); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(frames)
    return buf.getvalue()


def test_audio_from_wav(tk, tmp_path):
    a = tk.Audio.from_wav(_wav(1, 1, 8000, bytes([0, 64, 128, 192, 255])))
    assert a.sampling_rate == 8000 and a.audio_array.tolist() == [-1.0, -0.5, 0.0, 0.5, 127.0 / 128.0]
    s16 = np.array([-32768, -16384, 0, 1, 32767], "<i2")
    p = tmp_path / "m16.wav"
    p.write_bytes(_wav(1, 2, 16000, s16.tobytes()))
    b = tk.Audio.from_wav(str(p))
    assert b.sampling_rate == 16000 and b.audio_array.dtype == np.float32
    assert np.array_equal(b.audio_array, (s16.astype(np.float64) / 32768.0).astype(np.float32))
    st = np.array([[1000, 3000], [-32768, 32767], [5, -5]], "<i2")
    c = tk.Audio.from_wav(_wav(2, 2, 44100, st.tobytes()))
    assert c.sampling_rate == 44100 and np.array_equal(c.audio_array, (st.astype(np.float64).mean(axis=1) / 32768.0).astype(np.float32))
    d = tk.Audio.from_wav(_wav(1, 3, 16000, bytes([0, 0, 0x80, 0xFF, 0xFF, 0x7F, 0, 0, 0x40])))
    assert d.audio_array.tolist() == [-1.0, np.float32(8388607.0 / 8388608.0), 0.5]
    e = tk.Audio.from_wav(_wav(1, 4, 16000, np.array([-2 ** 31, 2 ** 30], "<i4").tobytes()))
    assert e.audio_array.tolist() == [-1.0, 0.5]
    with pytest.raises(tk.TokenizerError) as err:
        tk.Audio.from_wav(b"not a wav file")
    assert err.value.code == tk.TK_ERR_AUDIO
