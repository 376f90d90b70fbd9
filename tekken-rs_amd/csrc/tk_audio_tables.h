// tk_audio_tables.h -- the host arithmetic and the tables of the audio pass (include/tekken_hip.h "audio"; tk_capi_audio.cpp builds
// and uploads them, tk_audio.hip reads them).  Host only, no HIP: tests/audio_tables_check.cpp compiles it alone.
#ifndef TK_AUDIO_TABLES_H
#define TK_AUDIO_TABLES_H
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/tekken_hip.h"

// what the reference's constructors refuse (audio.rs:49-71, 110-140), and the two divisions by zero it would run into
static inline bool tk_audio_config_sane(const tk_audio_config& a) {
    if (a.sampling_rate == 0 || a.hop_length == 0 || a.window_size == 0 || a.num_mel_bins == 0) return false;
    if (!(a.frame_rate > 0.0)) return false;
    if (a.has_chunk_length && !(a.chunk_length_s > 0.0)) return false;
    return true;
}
// AudioConfig::chunk_frames (audio.rs:157-172): (chunk_length * sampling_rate as f64) as usize (a saturating cast)
static inline uint64_t tk_audio_chunk_frames(const tk_audio_config& a) {
    const double v = a.chunk_length_s * (double)a.sampling_rate;
    if (!(v > 0.0)) return 0;
    return v >= 18446744073709551615.0 ? ~0ull : (uint64_t)v;
}
// AudioConfig::audio_length_per_tok (audio.rs:188-199)
static inline uint64_t tk_audio_per_token(const tk_audio_config& a) {
    double f = (double)a.sampling_rate / a.frame_rate;
    f /= (double)a.hop_length;
    if (!(f > 0.0)) return 0;
    return f >= 18446744073709551615.0 ? ~0ull : (uint64_t)f;
}
// Audio::pad (audio.rs:439-463)
static inline uint64_t tk_audio_padded(const tk_audio_config& a, uint64_t cf, uint64_t n) {
    if (a.has_chunk_length) return (n / cf + (n % cf ? 1 : 0)) * cf;
    return n < a.window_size ? a.window_size : n;
}
// the frames of a signal of len samples (audio.rs:562-577): the float expression as the reference writes it
static inline uint64_t tk_audio_frames(const tk_audio_config& a, uint64_t len) {
    if (len % a.hop_length == 0) return len / a.hop_length;
    const double v = ceil((double)len / (double)a.hop_length - 1.0);
    return v > 0.0 ? (uint64_t)v : 0;
}
static inline uint64_t tk_audio_tokens(uint64_t frames, uint64_t per) {
    const double v = ceil((double)frames / (double)per);
    return v > 0.0 ? (uint64_t)v : 0;
}

// hertz_to_mel / mel_to_hertz (audio.rs:611-646: the Slaney scale)
static inline double tk_hertz_to_mel(double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) * (27.0 / log(6.4)) : 3.0 * f / 200.0; }
static inline double tk_mel_to_hertz(double m) { return m >= 15.0 ? 1000.0 * exp((m - 15.0) * (log(6.4) / 27.0)) : 200.0 * m / 3.0; }
// mel_filter_bank(F, M, 0, sr / 2, sr) (audio.rs:684-748), in double: fb[k * M + m]
static inline void tk_mel_filter_bank(uint64_t F, uint64_t M, uint64_t sr, std::vector<double>& fb) {
    const double mel_min = tk_hertz_to_mel(0.0), mel_max = tk_hertz_to_mel((double)sr / 2.0);
    std::vector<double> ff(M + 2);
    for (uint64_t i = 0; i < M + 2; ++i) ff[i] = tk_mel_to_hertz(mel_min + (mel_max - mel_min) * (double)i / (double)(M + 1));
    fb.assign(F * M, 0.0);
    for (uint64_t m = 0; m < M; ++m) {
        const double l = ff[m], c = ff[m + 1], r = ff[m + 2], enorm = 2.0 / (r - l);
        for (uint64_t k = 0; k < F; ++k) {
            const double f = (double)k * (double)sr / 2.0 / (double)(F - 1);
            double v = 0.0;
            if (f >= l && f <= c) v = (f - l) / (c - l);
            else if (f > c && f <= r) v = (r - f) / (r - c);
            if (!(v > 0.0)) v = 0.0;                 // f64::max(0.0): a NaN (a degenerate triangle) becomes 0
            fb[k * M + m] = v * enorm;
        }
    }
}

// The device tables.  dft: [W][2F], column k < F the real part w[i] cos(2 pi i k / W), column F + k the imaginary part
// -w[i] sin(2 pi i k / W), w the periodic Hann window; computed in double (the angle reduced as i k mod W first) and rounded once.
// The filter bank as one run per filter: the bins first[m] .. first[m] + count[m] are the span from its first to its last weight
// that is not 0 as f32 (count 0: a filter without one), their weights at weights[start[m] ..]; a zero inside the span is kept.
struct TkAudioTables {
    uint32_t W = 0, F = 0, M = 0;
    std::vector<float> dft;
    std::vector<uint32_t> first, count, start;
    std::vector<float> weights;
};
static inline void tk_audio_build_tables(const tk_audio_config& a, TkAudioTables& t) {
    const uint32_t W = (uint32_t)a.window_size, F = W / 2 + 1, M = (uint32_t)a.num_mel_bins;
    const double two_pi = 6.283185307179586476925286766559;
    t.W = W; t.F = F; t.M = M;
    t.dft.assign((size_t)W * 2 * F, 0.f);
    for (uint32_t i = 0; i < W; ++i) {
        const double w = 0.5 - 0.5 * cos(two_pi * (double)i / (double)W);
        for (uint32_t k = 0; k < F; ++k) {
            const double ang = two_pi * (double)(((uint64_t)i * k) % W) / (double)W;
            t.dft[(size_t)i * 2 * F + k] = (float)(w * cos(ang));
            t.dft[(size_t)i * 2 * F + F + k] = (float)(-w * sin(ang));
        }
    }
    std::vector<double> fb;
    tk_mel_filter_bank(F, M, a.sampling_rate, fb);
    t.first.assign(M, 0); t.count.assign(M, 0); t.start.assign(M, 0);
    t.weights.clear();
    for (uint32_t m = 0; m < M; ++m) {
        uint32_t lo = F, hi = 0;
        for (uint32_t k = 0; k < F; ++k)
            if ((float)fb[(size_t)k * M + m] != 0.f) { if (lo == F) lo = k; hi = k + 1; }
        t.start[m] = (uint32_t)t.weights.size();
        if (lo == F) continue;
        t.first[m] = lo;
        t.count[m] = hi - lo;
        for (uint32_t k = lo; k < hi; ++k) t.weights.push_back((float)fb[(size_t)k * M + m]);
    }
}
#endif
