"""Writes the audio fixtures of tests/golden/: audio_vectors.json from the float64 restatement (tests/audio_cases.py), and -- given the
reference's tests/assets/jfk.wav -- jfk_2s_16k.s16le, its first 32000 samples as raw int16.

    python tools/gen_golden_audio.py [path/to/jfk.wav]
"""
import json
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_cases as ac  # noqa: E402


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    if len(sys.argv) > 1:
        with wave.open(sys.argv[1], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
            raw = w.readframes(32000)
        with open(os.path.join(gold, "jfk_2s_16k.s16le"), "wb") as f:
            f.write(raw)
    rows = []
    base = dict(sr=16000, fr=12.5, H=160, W=400)
    cfgs = [ac.cfg(**base), ac.cfg(chunk=30.0, **base), ac.cfg(chunk=0.1, **base), ac.cfg(chunk=0.4, **base), ac.ODD,
            ac.cfg(sr=16000, fr=12.5, H=160, W=512), ac.cfg(sr=8000, fr=25.0, H=80, W=200, chunk=1.5), ac.cfg(sr=16000, fr=50.0, H=128, W=400)]
    for c in cfgs:
        cf = ac.chunk_frames(c) if c["chunk_length_s"] is not None else 1600
        W, H = c["window_size"], c["hop_length"]
        for n in sorted({0, 1, H - 1, H, W - 1, W, W + 1, cf - 1, cf, cf + 1, 2 * cf, 176000, 480001}):
            npad, _, N, S, Ts, _ = ac.layout(c, n)
            rows.append({"config": c, "n": n, "padded": npad, "frames": ac.frames(c, npad), "tokens": N, "segments": S, "segment_frames": Ts})
    banks = []
    for F, M in ((201, 128), (201, 80)):
        fb = ac.mel_filter_bank(F, M, 16000)
        spots = [[k, m, fb[k, m]] for k, m in ((1, 0), (2, 1), (10, 8), (50, 40), (100, M // 2), (150, M - 10), (199, M - 1), (200, M - 1), (0, 0))]
        banks.append({"F": F, "M": M, "sr": 16000, "column_sums": fb.sum(axis=0).tolist(), "spots": spots})
    with open(os.path.join(gold, "audio_vectors.json"), "w") as f:
        json.dump({"layout": rows, "filter_banks": banks}, f, indent=0)


if __name__ == "__main__":
    main()
