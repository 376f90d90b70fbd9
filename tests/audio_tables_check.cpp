// Stand-alone driver of csrc/tk_audio_tables.h for tests/test_audio_cpu.py: builds the audio pass's tables for the config on the
// command line (sr fr M H W) and writes them to stdout as raw little-endian words:
//   u32 W, F, M, n_weights | f32 dft[W * 2F] | u32 first[M] | u32 count[M] | u32 start[M] | f32 weights[n_weights]
// and the host arithmetic for the sample counts that follow (chunk_length_s as the sixth argument, a negative one: none):
//   u64 padded, frames, tokens per count
#include <stdio.h>
#include <stdlib.h>

#include "../tekken-rs_amd/csrc/tk_audio_tables.h"

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    tk_audio_config a = {};
    a.sampling_rate = strtoull(argv[1], nullptr, 10);
    a.frame_rate = atof(argv[2]);
    a.num_mel_bins = strtoull(argv[3], nullptr, 10);
    a.hop_length = strtoull(argv[4], nullptr, 10);
    a.window_size = strtoull(argv[5], nullptr, 10);
    const double chunk = atof(argv[6]);
    a.has_chunk_length = chunk >= 0.0;
    a.chunk_length_s = chunk >= 0.0 ? chunk : 0.0;
    if (!tk_audio_config_sane(a)) return 3;
    TkAudioTables t;
    tk_audio_build_tables(a, t);
    const uint32_t head[4] = {t.W, t.F, t.M, (uint32_t)t.weights.size()};
    fwrite(head, 4, 4, stdout);
    fwrite(t.dft.data(), 4, t.dft.size(), stdout);
    fwrite(t.first.data(), 4, t.first.size(), stdout);
    fwrite(t.count.data(), 4, t.count.size(), stdout);
    fwrite(t.start.data(), 4, t.start.size(), stdout);
    fwrite(t.weights.data(), 4, t.weights.size(), stdout);
    const uint64_t cf = a.has_chunk_length ? tk_audio_chunk_frames(a) : 0, per = tk_audio_per_token(a);
    for (int i = 7; i < argc; ++i) {
        const uint64_t n = strtoull(argv[i], nullptr, 10), np = tk_audio_padded(a, cf, n), fr = tk_audio_frames(a, np);
        const uint64_t row[3] = {np, fr, tk_audio_tokens(fr, per)};
        fwrite(row, 8, 3, stdout);
    }
    return 0;
}
