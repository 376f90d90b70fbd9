"""Audio on the GPU: the log-mel features against the float64 restatement (tests/audio_cases.py) inside the derived error bracket,
their exact properties, the splice of audio parts, chat rows with clips, and what the entries refuse."""
import functools

import numpy as np
import pytest

import audio_cases as ac

pytestmark = pytest.mark.gpu

CONFIGS = {"V": ac.V, "V-0.1s": ac.cfg(chunk=0.1), "V-0.4s": ac.cfg(chunk=0.4), "V80": ac.V80, "ODD": ac.ODD}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng(tk, torch):
    e = tk.Engine([bytes([i]) for i in range(256)], 10, 1, 2, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tok(tk, torch):
    t = tk.Tekkenizer.from_json(ac.tekken_json(ac.cfg(chunk=0.4)), device=0)
    yield t
    t.close()


def lengths(tk, c):
    """0, 1, around the window, T around the multiples of the kernel's frame tile, and 2 s"""
    H, W, tile = c["hop_length"], c["window_size"], int(tk.lib().tk_audio_frame_tile())
    return [0, 1, W - 1, W, W + 1] + [H * k for k in (1, tile - 1, tile, tile + 1, 2 * tile + 1)] + [2 * c["sampling_rate"]]


@functools.lru_cache(maxsize=None)
def case_clips(name, ns):
    """signal -> the clips of every length, for config `name`"""
    c = CONFIGS[name]
    sigs = {}
    for n in ns:
        for k, v in ac.signals(n, c["sampling_rate"], seed=n + 1).items():
            sigs.setdefault(k, []).append(v)
    if c["sampling_rate"] == 16000:
        sigs["jfk"] = [ac.jfk()[:n] for n in ns]
    return sigs


@functools.lru_cache(maxsize=None)
def reference(name, ns, signal):
    return ac.batch_features(CONFIGS[name], case_clips(name, ns)[signal])


def logmel(torch, eng, clips, log_mel_max=None, stream=None):
    """One device call over the clips -> (features float32 [M * n_frames], frame_off, clip_seg, the result)"""
    offs = np.zeros(len(clips) + 1, np.int64)
    if clips:
        offs[1:] = np.cumsum([len(x) for x in clips])
    flat = np.concatenate(clips).astype(np.float32) if int(offs[-1]) else np.zeros(1, np.float32)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_x, d_o = torch.from_numpy(flat).cuda(), torch.from_numpy(offs).cuda()
        st.synchronize()
        r = eng.audio_logmel_device(d_x.data_ptr(), d_o.data_ptr(), len(clips), int(offs[-1]), log_mel_max=log_mel_max, checks=1, stream=st.cuda_stream)
        t = r.tensors(copy=True)
    return t["features"].cpu().numpy(), t["frame_off"].cpu().numpy().astype(np.uint64), t["clip_seg"].cpu().numpy().astype(np.uint64), r


@pytest.mark.parametrize("name", list(CONFIGS))
def test_features_lie_in_the_derived_bracket(tk, torch, eng, name):
    c = CONFIGS[name]
    eng.audio_set_config(c)
    ns = tuple(lengths(tk, c))
    for signal, clips in case_clips(name, ns).items():
        exp, lo, hi, fo, cs = reference(name, ns, signal)
        got, gfo, gcs, r = logmel(torch, eng, clips)
        assert np.array_equal(gfo, fo) and np.array_equal(gcs, cs), (name, signal)
        assert (r.n_clips, r.n_segments, r.n_frames, r.n_mel) == (len(clips), len(fo) - 1, int(fo[-1]), c["num_mel_bins"])
        assert got.shape == exp.shape and got.dtype == np.float32
        g = got.astype(np.float64)
        share = float(((hi - lo) < 0.01).mean())
        print("%s %-14s elements %6d  max |got - f64| %.3g  rms %.3g  share of tight brackets %.3f" %
              (name, signal, len(g), np.abs(g - exp).max(), np.sqrt(((g - exp) ** 2).mean()), share))
        bad = np.flatnonzero(~((lo - 1e-6 <= g) & (g <= hi + 1e-6)))
        assert len(bad) == 0, (name, signal, len(bad), bad[:5], g[bad[:5]], lo[bad[:5]], hi[bad[:5]])
        assert share >= 0.70, (name, signal, share)        # the bracket cannot hide a failure
        if signal == "zeros":
            assert (got == np.float32(-1.5)).all()
        # every element is within 2 of its segment's maximum, in f32 (the floor is ((Lmax - 8) + 4) / 4, three f32 roundings
        # of values below 32: 4 ulp of 2^-19 cover them)
        for s in range(len(fo) - 1):
            seg = got[c["num_mel_bins"] * int(fo[s]):c["num_mel_bins"] * int(fo[s + 1])]
            if len(seg):
                assert seg.min() >= np.float32(seg.max() - np.float32(2.0)) - np.float32(4 * 2.0 ** -19)


def test_layout_agrees_with_the_host_and_with_encode_audio(tk, torch, tok):
    c = tok.audio_config
    eng = tok.engine()
    ns = [0, 1, 6399, 6400, 6401, 32000, 12800]
    clips = [ac.signals(n, 16000, seed=n + 3)["noise_0.1"] for n in ns]
    got, fo, cs, r = logmel(torch, eng, clips)
    padded, n_frames, n_tokens, n_seg = tk.audio_layout(c, ns)
    assert np.array_equal(np.diff(cs), n_seg) and r.n_frames == int(n_frames.sum()) == int(fo[-1])
    per = ac.per_token(c)
    for i, x in enumerate(clips):
        ids, pad = tok.encode_audio(tk.Audio(x, 16000))
        T = int(fo[cs[i + 1]] - fo[cs[i]])
        assert T == int(n_frames[i]) and len(pad) == int(padded[i])
        assert len(ids) - 1 == -(-T // per) == int(n_tokens[i])
    out = tok.encode_audio_batch([tk.Audio(x, 16000) for x in clips])
    assert tuple(out["features"].shape) == (int(cs[-1]), 128, 40)
    assert np.array_equal(out["features"].cpu().numpy().reshape(-1), got)
    assert out["tokens_per_clip"].tolist() == n_tokens.tolist() and np.array_equal(out["frame_off"], fo) and np.array_equal(out["clip_seg"], cs)


def test_fixed_log_mel_max_and_the_host_entry(tk, torch, eng):
    c = ac.V
    eng.audio_set_config(c)
    clips = [ac.jfk()[:5000], ac.signals(700, 16000)["chirp"]]
    got, fo, cs, _ = logmel(torch, eng, clips, log_mel_max=30.0)
    assert len(got) and (got == (np.float32(30.0) - np.float32(8.0) + np.float32(4.0)) / np.float32(4.0)).all()
    assert eng.last_logmel_ms()[1] == 0.0                   # the clamp kernel is not launched
    # a fixed maximum inside the data: the restatement with the same value
    exp, lo, hi, _, _ = ac.batch_features(c, clips, log_mel_max=1.5)
    got, _, _, _ = logmel(torch, eng, clips, log_mel_max=1.5)
    assert ((lo - 1e-6 <= got) & (got <= hi + 1e-6)).all() and len(np.unique(got)) > 100
    # host in / host out: the same bits
    dev, fo, cs, _ = logmel(torch, eng, clips)
    offs = np.array([0, 5000, 5700], np.uint64)
    h = eng.audio_logmel(np.concatenate(clips), offs)
    assert np.array_equal(h["features"], dev) and np.array_equal(h["frame_off"], fo) and np.array_equal(h["clip_seg"], cs)
    assert (h["n_clips"], h["n_segments"], h["n_frames"], h["n_mel"]) == (2, 2, int(fo[-1]), 128)
    assert eng.last_logmel_ms()[1] > 0.0


def test_padded_tail_equals_explicit_zeros(tk, torch, eng):
    c = ac.cfg(chunk=0.4)
    eng.audio_set_config(c)
    x = ac.jfk()[:6400 + 1234]
    z = np.concatenate([x, np.zeros(2 * 6400 - len(x), np.float32)])
    a, fo_a, _, _ = logmel(torch, eng, [x])
    b, fo_b, _, _ = logmel(torch, eng, [z])
    assert np.array_equal(fo_a, fo_b) and len(fo_a) == 3 and a.tobytes() == b.tobytes()
    u = ac.cfg()
    eng.audio_set_config(u)
    a, _, _, _ = logmel(torch, eng, [x[:250]])
    b, _, _, _ = logmel(torch, eng, [np.concatenate([x[:250], np.zeros(150, np.float32)])])
    assert a.tobytes() == b.tobytes() and len(a) == 128 * 2


@pytest.mark.parametrize("name", ["V", "V-0.1s"])
def test_a_clip_does_not_depend_on_its_batch_or_stream(tk, torch, eng, name):
    c = CONFIGS[name]
    eng.audio_set_config(c)
    rng = np.random.default_rng(37)
    probe = ac.jfk()[:10240 + 77]
    others = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in rng.integers(0, 12000, 36)]
    alone, fo, _, _ = logmel(torch, eng, [probe])
    M = c["num_mel_bins"]
    for at in (0, 36, 17):
        clips = others[:at] + [probe] + others[at:]
        assert len(clips) == 37
        got, gfo, gcs, _ = logmel(torch, eng, clips, stream=torch.cuda.Stream() if at == 17 else None)
        part = got[M * int(gfo[gcs[at]]):M * int(gfo[gcs[at + 1]])]
        assert part.tobytes() == alone.tobytes(), (name, at)
    again, _, _, _ = logmel(torch, eng, [probe], stream=torch.cuda.Stream())
    assert again.tobytes() == alone.tobytes()


def _splice(torch, eng, ids, offs, tokens, fill):
    n_parts = len(tokens)
    d_ids = torch.from_numpy((ids if len(ids) else np.zeros(1, np.uint32)).view(np.int32)).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_tok = torch.from_numpy((tokens if n_parts else np.zeros(1, np.uint32)).view(np.int32)).cuda()
    torch.cuda.synchronize()
    r = eng.audio_splice_device(d_ids.data_ptr(), d_offs.data_ptr(), n_parts, len(ids), d_tok.data_ptr(), fill, torch.cuda.current_stream().cuda_stream)
    t = r.tensors(copy=True)
    return t["ids"].cpu().numpy().view(np.uint32), t["offsets"].cpu().numpy().astype(np.uint64), r


def test_splice_against_the_restatement(tk, torch, eng):
    rng = np.random.default_rng(5)
    n_parts = 300
    lens = rng.choice([0, 0, 1, 2, 3, 4, 5, 17, 300], n_parts)
    tokens = rng.choice([0, 0, 0, 1, 3, 4, 5, 4097], n_parts).astype(np.uint32)
    lens[:4], tokens[:4] = [0, 0, 5, 0], [0, 7, 0, 4097]       # an empty part, only fill, only ids, only a long fill
    offs = np.zeros(n_parts + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    ids = rng.integers(100, 5000, int(offs[-1])).astype(np.uint32)
    assert {0, 1, 3, 4, 5, 4097} <= set(tokens.tolist())
    got, goffs, r = _splice(torch, eng, ids, offs, tokens, 6)
    exp, eoffs = ac.splice(ids, offs, tokens, 6)
    assert np.array_equal(goffs, eoffs) and np.array_equal(got, exp) and (r.n_parts, r.n_ids) == (n_parts, len(exp))
    got, goffs, r = _splice(torch, eng, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), 6)
    assert len(got) == 0 and goffs.tolist() == [0] and r.n_ids == 0
    got, goffs, _ = _splice(torch, eng, np.zeros(0, np.uint32), np.zeros(3, np.uint64), np.array([3, 0], np.uint32), 9)
    assert got.tolist() == [9, 9, 9] and goffs.tolist() == [0, 3, 3]


def test_conversations_with_audio_parts(tk, torch, tok):
    A, B = tok.audio_token_id, tok.begin_audio_token_id
    clip1, clip2 = tk.Audio(ac.jfk()[:9000], 16000), tk.Audio(ac.signals(700, 16000)["chirp"], 16000)
    convs = [[("<s>", "", False), ("[INST]", "hello", False), (None, clip1, False), (None, " world", False), ("[/INST]", "", False),
              (None, "hello world", True), ("</s>", "", True)],
             [("[INST]", "", False), (None, clip2, True), (None, clip1, False), ("[/INST]", "hi", (False, True))]]
    out = tok.encode_conversations(convs, return_part_index=True, return_tensors="np")
    n1, n2 = len(tok.encode_audio(clip1)[0]) - 1, len(tok.encode_audio(clip2)[0]) - 1
    assert (n1, n2) == (10, 5)                                  # 9000 -> 2 chunks of 0.4 s -> 80 frames / 8; 700 -> 1 chunk -> 40 / 8
    ids, labels, offs, pos = [], [], [0], []
    for conv in convs:
        for k, (ctrl, text, label) in enumerate(conv):
            lc, lt = label if isinstance(label, tuple) else (label, label)
            if isinstance(text, tk.Audio):
                n = n1 if text is clip1 else n2
                pos.append((len(ids) + 1, n))
                new, lab = [B] + [A] * n, [False] * (n + 1)     # an audio part is never labelled
            else:
                own = tok.encode(text)
                new = ([tok.get_control_token(ctrl)] if ctrl else []) + own
                lab = ([lc] if ctrl else []) + [lt] * len(own)
            ids += new
            labels += [i if l else -100 for i, l in zip(new, lab)]
        offs.append(len(ids))
    assert out["input_ids"].tolist() == ids and out["offsets"].tolist() == offs and out["labels"].tolist() == labels
    assert out["audio_positions"] == pos and out["n_labelled"] == sum(l != -100 for l in labels)
    for (start, n) in out["audio_positions"]:
        assert out["input_ids"][start - 1] == B and (out["input_ids"][start:start + n] == A).all()
    assert len(out["part_index"]) == len(ids)
    feats = tok.encode_audio_batch([clip1, clip2, clip1])
    assert out["audio_features"].shape == feats["features"].shape == (5, 128, 40)
    assert torch.equal(out["audio_features"], feats["features"])
    assert np.array_equal(out["audio_clip_seg"], feats["clip_seg"]) and out["audio_clip_seg"].tolist() == [0, 2, 3, 5]
    # encode_chat: a clip where a content item goes
    chat = tok.encode_chat([[{"role": "user", "content": [clip2, "hello"]}, {"role": "assistant", "content": " world"}]], return_tensors="np")
    w = tok.encode(" world")
    assert chat["input_ids"].tolist() == [tok.bos_id(), tok.get_control_token("[INST]"), B] + [A] * n2 + tok.encode("hello") + \
        [tok.get_control_token("[/INST]")] + w + [tok.eos_id()]
    assert chat["audio_positions"] == [(3, n2)] and chat["labels"].tolist()[-len(w) - 1:] == w + [tok.eos_id()]
    assert (chat["labels"][:-len(w) - 1] == -100).all()


def test_conversations_without_audio_are_todays(tk, torch, tok):
    eng = tok.engine()
    convs = [[("<s>", "", False), ("[INST]", "hello world", False), ("[/INST]", "", False), (None, "hello", True), ("</s>", "", True)],
             [("[INST]", "", False), (None, " world hello", (False, True))]]
    before = eng.audio_splice_calls()
    out = tok.encode_conversations(convs, return_tensors="np")
    pt = tok.encode_conversations(convs, return_tensors="pt")
    assert eng.audio_splice_calls() == before               # the splice and its buffers are never touched
    assert "audio_features" not in out and "audio_positions" not in out
    raw = eng.encode_parts_join(*tok._parts_of(convs), ignore_index=-100, flags=tk.JOIN_LABELS)
    assert np.array_equal(out["input_ids"], raw["ids"]) and np.array_equal(out["offsets"], raw["offsets"]) and np.array_equal(out["labels"], raw["labels"])
    assert np.array_equal(pt["input_ids"].cpu().numpy().view(np.uint32), raw["ids"]) and np.array_equal(pt["labels"].cpu().numpy(), raw["labels"])
    ids = [1, 3] + tok.encode("hello world") + [4] + tok.encode("hello") + [2]
    assert out["input_ids"][:len(ids)].tolist() == ids


def test_refusals_leave_the_earlier_result_readable(tk, torch, eng):
    eng.audio_set_config(ac.V)
    clip = ac.jfk()[:4000]
    good, fo, _, r = logmel(torch, eng, [clip])
    keep = torch.as_tensor(r.views()[0], device="cuda")
    for bad in (ac.cfg(W=401), ac.cfg(H=401), ac.cfg(M=257), ac.cfg(chunk=0.0125), ac.cfg(W=2), ac.cfg(W=2050), ac.cfg(H=0), ac.cfg(M=0), ac.cfg(fr=200.0)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.audio_set_config(bad)
        assert e.value.code == tk.TK_ERR_INVALID_CONFIG, bad
    d_x, d_o = torch.from_numpy(clip).cuda(), torch.from_numpy(np.array([0, 4000], np.int64)).cuda()
    bad_o = torch.from_numpy(np.array([0, 3999], np.int64)).cuda()
    torch.cuda.synchronize()
    for kw, offs_t in (({"flags": 1}, d_o), ({"checks": 2}, d_o), ({"checks": 1}, bad_o), ({}, bad_o)):
        with pytest.raises(tk.TokenizerError) as e:
            eng.audio_logmel_device(d_x.data_ptr(), offs_t.data_ptr(), 1, 4000, **kw)
        assert e.value.code == tk.TK_ERR_INVALID_ARG
    with pytest.raises(tk.TokenizerError) as e:
        eng.audio_logmel_device(d_x.data_ptr(), 0, 1, 4000)
    assert e.value.code == tk.TK_ERR_INVALID_ARG
    # the refused config left V in place, and the earlier result is still there
    assert np.array_equal(keep.cpu().numpy(), good)
    again, _, _, _ = logmel(torch, eng, [clip])
    assert np.array_equal(again, good)
    # no config set; a model without audio
    fresh = tk.Engine([bytes([i]) for i in range(256)], 10, 1, 2, device=0)
    with pytest.raises(tk.TokenizerError) as e:
        fresh.audio_logmel_device(d_x.data_ptr(), d_o.data_ptr(), 1, 4000)
    assert e.value.code == tk.TK_ERR_AUDIO and "Audio encoder not configured" in str(e.value)
    fresh.close()
    plain = tk.Tekkenizer.from_json(ac.tekken_json(None), device=0)
    for call in (lambda: plain.encode_audio_batch([tk.Audio(clip, 16000)]),
                 lambda: plain.encode_conversations([[(None, tk.Audio(clip, 16000), False)]])):
        with pytest.raises(tk.TokenizerError) as e:
            call()
        assert e.value.code == tk.TK_ERR_AUDIO
    plain.close()
