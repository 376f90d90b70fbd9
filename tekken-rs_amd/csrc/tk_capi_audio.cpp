// tk_capi_audio.cpp -- the audio entries of the C ABI (include/tekken_hip.h "audio"; csrc/tk_audio.hip, csrc/tk_audio_tables.h):
// the host arithmetic of a clip's layout, the transform's tables, the log-mel features and the splice of audio parts.
#include <math.h>

#include "tk_audio_tables.h"
#include "tk_capi_layout.h"

#define TKA_MAX_WINDOW 2048u
#define TKA_MAX_MEL 256u

extern "C" int tk_audio_layout(const tk_audio_config* cfg, const uint64_t* n_samples, uint64_t n_clips, uint64_t* padded, uint64_t* n_frames,
                               uint64_t* n_tokens, uint64_t* n_segments) {
    if (!cfg || (!n_samples && n_clips)) return TK_ERR_INVALID_ARG;
    if (!tk_audio_config_sane(*cfg)) return TK_ERR_INVALID_CONFIG;
    const uint64_t per = tk_audio_per_token(*cfg), cf = cfg->has_chunk_length ? tk_audio_chunk_frames(*cfg) : 0;
    if (per == 0 || (cfg->has_chunk_length && cf == 0)) return TK_ERR_INVALID_CONFIG;
    const uint64_t chunk_frames = cfg->has_chunk_length ? tk_audio_frames(*cfg, cf) : 0;
    for (uint64_t c = 0; c < n_clips; ++c) {
        const uint64_t np = tk_audio_padded(*cfg, cf, n_samples[c]);
        const uint64_t segs = cfg->has_chunk_length ? np / cf : 1;
        if (padded) padded[c] = np;
        if (n_frames) n_frames[c] = cfg->has_chunk_length ? segs * chunk_frames : tk_audio_frames(*cfg, np);
        if (n_tokens) n_tokens[c] = tk_audio_tokens(tk_audio_frames(*cfg, np), per);   // (the reference counts over the whole padded clip)
        if (n_segments) n_segments[c] = segs;
    }
    return TK_OK;
}

extern "C" uint32_t tk_audio_frame_tile(void) { return TKA_FRAMES; }

// what the transform cannot do (step 8 of the definition)
static int audio_check_config(tk_ctx* c, const tk_audio_config* a) {
    const char* why = nullptr;
    if (!tk_audio_config_sane(*a)) why = "a zero or negative field";
    else if (a->window_size % 2) why = "window_size is odd";
    else if (a->window_size < 4 || a->window_size > TKA_MAX_WINDOW) why = "window_size is outside 4 .. 2048";
    else if (a->hop_length > a->window_size) why = "hop_length exceeds window_size";
    else if (a->num_mel_bins > TKA_MAX_MEL) why = "num_mel_bins exceeds 256";
    else if (a->sampling_rate > 0xFFFFFFFFull) why = "sampling_rate is beyond 2^32";
    else if (tk_audio_per_token(*a) == 0) why = "no whole frame per token";
    else if (a->has_chunk_length && tk_audio_chunk_frames(*a) <= a->window_size / 2) why = "a chunk is no longer than half a window";
    if (!why) return TK_OK;
    c->err = std::string("audio config: ") + why;
    return TK_ERR_INVALID_CONFIG;
}

extern "C" int tk_audio_set_config(tk_ctx* c, const tk_audio_config* cfg) {
    TK_ENTRY(c);
    if (!cfg) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    int rc = audio_check_config(c, cfg);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    TkAudioTables t;
    tk_audio_build_tables(*cfg, t);
    if (t.weights.empty()) t.weights.push_back(0.f);
    AudioBufs& b = c->audio;
    // (an earlier call's kernels have drained: every log-mel entry waits for its stream)
    b.have_config = false;
    if ((rc = upload(c, b.dft, t.dft.data(), t.dft.size() * 4)) != TK_OK) return rc;
    if ((rc = upload(c, b.fb_first, t.first.data(), t.first.size() * 4)) != TK_OK) return rc;
    if ((rc = upload(c, b.fb_count, t.count.data(), t.count.size() * 4)) != TK_OK) return rc;
    if ((rc = upload(c, b.fb_start, t.start.data(), t.start.size() * 4)) != TK_OK) return rc;
    if ((rc = upload(c, b.fb_weights, t.weights.data(), t.weights.size() * 4)) != TK_OK) return rc;
    b.cfg = *cfg;
    b.W = t.W; b.F = t.F; b.M = t.M;
    b.have_config = true;
    return TK_OK;
}

// The log-mel pass over samples on the device into c->audio; *out gets the device pointers.  h_offs: the sample offsets on the
// host, checked here.  Everything that can be refused is refused before a buffer of an earlier result is touched.
static int run_logmel(tk_ctx* c, const float* d_samples, const uint64_t* h_offs, uint64_t n_clips, uint64_t n_samples,
                      const tk_logmel_opts* opts, hipStream_t s, tk_logmel* out) {
    AudioBufs& b = c->audio;
    if (h_offs[0] != 0 || h_offs[n_clips] != n_samples) { c->err = "logmel: the sample offsets do not span the samples"; return TK_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n_clips; ++i)
        if (h_offs[i + 1] < h_offs[i]) { c->err = "logmel: the sample offsets decrease at clip " + std::to_string(i); return TK_ERR_INVALID_ARG; }
    const tk_audio_config& a = b.cfg;
    const uint64_t cf = a.has_chunk_length ? tk_audio_chunk_frames(a) : 0, M = b.M, H = a.hop_length;
    std::vector<TkaSegment> segs;
    std::vector<TkaTile> tiles;
    std::vector<uint64_t> frame_off(1, 0), clip_seg(n_clips + 1, 0);
    for (uint64_t i = 0; i < n_clips; ++i) {
        const uint64_t n = h_offs[i + 1] - h_offs[i], np = tk_audio_padded(a, cf, n);
        const uint64_t seg_len = a.has_chunk_length ? cf : np, n_seg = a.has_chunk_length ? np / cf : 1;
        const uint64_t T = tk_audio_frames(a, seg_len);
        // (frame t reads up to sample t H + W / 2 - 1 + W / 2 of the segment, reflected: T H <= L keeps the reflection inside it)
        if (T > 0xFFFFFFF0ull / (H ? H : 1) || T * H > seg_len) { c->err = "logmel: clip " + std::to_string(i) + " is too long"; return TK_ERR_INVALID_ARG; }
        if (segs.size() + n_seg > 0xFFFFFFF0ull) { c->err = "logmel: too many segments"; return TK_ERR_INVALID_ARG; }
        for (uint64_t k = 0; k < n_seg; ++k) {
            TkaSegment g;
            memset(&g, 0, sizeof(g));
            const uint64_t first = k * seg_len;
            g.start = h_offs[i] + (first < n ? first : n);
            g.valid = first < n ? (n - first < seg_len ? n - first : seg_len) : 0;
            g.len = seg_len;
            g.out = M * frame_off.back();
            g.frames = (uint32_t)T;
            for (uint64_t t0 = 0; t0 < T; t0 += TKA_FRAMES) tiles.push_back(TkaTile{(uint32_t)segs.size(), (uint32_t)t0});
            segs.push_back(g);
            frame_off.push_back(frame_off.back() + T);
            if (frame_off.back() > TK_LAYOUT_MAX_ELEMS / M) return layout_too_large(c, "logmel", frame_off.back(), M);
        }
        clip_seg[i + 1] = segs.size();
    }
    if (tiles.size() > 0x7FFFFFFFull) return layout_too_large(c, "logmel", frame_off.back(), M);
    const uint64_t S = segs.size(), n_frames = frame_off.back(), n_elems = M * n_frames;
    const bool fixed = opts && isfinite(opts->log_mel_max);

    for (Event& ev : b.ev)
        if (!ev.h) TK_HIP(c, hipEventCreate(&ev.h));
    TK_HIP(c, b.feat.reserve(n_elems * 4 + 16));
    TK_HIP(c, b.frame_off.reserve((S + 1) * 8));
    TK_HIP(c, b.clip_seg.reserve((n_clips + 1) * 8));
    TK_HIP(c, b.segs.reserve(S * sizeof(TkaSegment) + 16));
    TK_HIP(c, b.tiles.reserve(tiles.size() * sizeof(TkaTile) + 16));
    TK_HIP(c, b.seg_max.reserve(S * 4 + 16));
    TK_HIP(c, hipMemcpyAsync(b.frame_off.p, frame_off.data(), (S + 1) * 8, hipMemcpyHostToDevice, s));
    TK_HIP(c, hipMemcpyAsync(b.clip_seg.p, clip_seg.data(), (n_clips + 1) * 8, hipMemcpyHostToDevice, s));
    if (S) TK_HIP(c, hipMemcpyAsync(b.segs.p, segs.data(), S * sizeof(TkaSegment), hipMemcpyHostToDevice, s));
    if (!tiles.empty()) TK_HIP(c, hipMemcpyAsync(b.tiles.p, tiles.data(), tiles.size() * sizeof(TkaTile), hipMemcpyHostToDevice, s));
    if (S && !fixed) TK_HIP(c, hipMemsetAsync(b.seg_max.p, 0, S * 4, s));
    TkLogmelArgs k;
    memset(&k, 0, sizeof(k));
    k.samples = d_samples;
    k.segs = (const TkaSegment*)b.segs.p;
    k.tiles = (const TkaTile*)b.tiles.p;
    k.n_tiles = (uint32_t)tiles.size();
    k.n_segs = (uint32_t)S;
    k.W = b.W; k.H = (uint32_t)H; k.F = b.F; k.M = b.M;
    k.dft = (const float*)b.dft.p;
    k.fb_first = (const uint32_t*)b.fb_first.p;
    k.fb_count = (const uint32_t*)b.fb_count.p;
    k.fb_start = (const uint32_t*)b.fb_start.p;
    k.fb_weights = (const float*)b.fb_weights.p;
    k.out = (float*)b.feat.p;
    k.seg_max = fixed ? nullptr : (uint32_t*)b.seg_max.p;
    k.fixed_max = fixed ? opts->log_mel_max : 0.f;
    k.frame_off = (const uint64_t*)b.frame_off.p;
    k.n_elems = n_elems;
    b.ms[0] = b.ms[1] = 0.f;
    TK_HIP(c, hipEventRecord(b.ev[0], s));
    TK_HIP(c, tk_launch_logmel(k, s));
    TK_HIP(c, hipEventRecord(b.ev[1], s));
    if (!fixed) TK_HIP(c, tk_launch_logmel_clamp(k, s));
    TK_HIP(c, hipEventRecord(b.ev[2], s));
    TK_HIP(c, hipStreamSynchronize(s));                   // (segs, tiles, frame_off and clip_seg live until here)
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    if (!fixed) (void)hipEventElapsedTime(&b.ms[1], b.ev[1], b.ev[2]);
    out->features = (float*)b.feat.p;
    out->frame_off = (uint64_t*)b.frame_off.p;
    out->clip_seg = (uint64_t*)b.clip_seg.p;
    out->n_clips = n_clips;
    out->n_segments = S;
    out->n_frames = n_frames;
    out->n_mel = M;
    return TK_OK;
}

// what both log-mel entries refuse before anything else
static int logmel_check(tk_ctx* c, int checks, const tk_logmel_opts* opts, bool null_arg, uint64_t n_clips) {
    int rc = check_flags_and_args(c, checks, TK_CHECK_OFFSETS, null_arg);
    if (rc != TK_OK) return rc;
    if (opts && opts->flags) { c->err = "unknown logmel flag"; return TK_ERR_INVALID_ARG; }
    if (n_clips > 0xFFFFFFF0ull) { c->err = "logmel: too many clips"; return TK_ERR_INVALID_ARG; }
    if (!c->audio.have_config) { c->err = "Audio encoder not configured"; return TK_ERR_AUDIO; }
    return TK_OK;
}

extern "C" int tk_audio_logmel_device(tk_ctx* c, const void* d_samples, const void* d_sample_offsets, uint64_t n_clips, uint64_t n_samples,
                                      int checks, const tk_logmel_opts* opts, void* hip_stream, tk_logmel* out) {
    TK_ENTRY(c);
    int rc = logmel_check(c, checks, opts, !d_sample_offsets || (!d_samples && n_samples) || !out, n_clips);
    if (rc != TK_OK) return rc;
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    std::vector<uint64_t> h_offs(n_clips + 1);
    TK_HIP(c, hipMemcpyAsync(h_offs.data(), d_sample_offsets, (n_clips + 1) * 8, hipMemcpyDeviceToHost, s));
    TK_HIP(c, hipStreamSynchronize(s));
    return run_logmel(c, (const float*)d_samples, h_offs.data(), n_clips, n_samples, opts, s, out);
}

extern "C" int tk_audio_logmel(tk_ctx* c, const float* samples, const uint64_t* sample_offsets, uint64_t n_clips, const tk_logmel_opts* opts,
                               tk_logmel* out) {
    TK_ENTRY(c);
    int rc = logmel_check(c, 0, opts, !sample_offsets || !out, n_clips);
    if (rc != TK_OK) return rc;
    memset(out, 0, sizeof(*out));
    const uint64_t n_samples = sample_offsets[n_clips];
    if (!samples && n_samples) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    TK_HIP(c, c->audio.in_samples.reserve(n_samples * 4 + 16));
    if (n_samples) TK_HIP(c, hipMemcpyAsync(c->audio.in_samples.p, samples, n_samples * 4, hipMemcpyHostToDevice, c->stream));
    tk_logmel r;
    if ((rc = run_logmel(c, (const float*)c->audio.in_samples.p, sample_offsets, n_clips, n_samples, opts, c->stream, &r)) != TK_OK) return rc;
    return layout_copy_out(c, r, 4, 0, "logmel", out);
}

extern "C" void tk_free_logmel(tk_logmel* r) { layout_free(r); }

extern "C" void tk_last_logmel_ms(const tk_ctx* c, float ms[2]) {
    std::unique_lock<std::mutex> lock;
    if (c) lock = std::unique_lock<std::mutex>(const_cast<tk_ctx*>(c)->mu);   // (a call on another thread writes them under it)
    for (int i = 0; ms && i < 2; ++i) ms[i] = c ? c->audio.ms[i] : 0.f;
}

// ---- the splice: counts, one scan, the fill ----
extern "C" int tk_audio_splice_device(tk_ctx* c, const void* d_ids, const void* d_id_offsets, uint64_t n_parts, uint64_t n_ids,
                                      const void* d_part_tokens, uint32_t fill_id, void* hip_stream, tk_ragged* out) {
    TK_ENTRY(c);
    if (!d_id_offsets || (!d_ids && n_ids) || (!d_part_tokens && n_parts) || !out) { c->err = "null argument"; return TK_ERR_INVALID_ARG; }
    if (n_parts >= 0xFFFFFFF0ull) { c->err = "splice: too many parts"; return TK_ERR_INVALID_ARG; }
    TK_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    AudioBufs& b = c->audio;
    ++b.n_splice_calls;
    TK_HIP(c, b.sp_cnt.reserve(n_parts * 4 + 16));
    TK_HIP(c, b.sp_offs.reserve((n_parts + 1) * 8));
    TK_HIP(c, b.sp_bsum.reserve(scan_workspace_bytes(n_parts)));
    TkSpliceArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = (const uint32_t*)d_ids;
    a.id_offs = (const uint64_t*)d_id_offsets;
    a.part_tokens = (const uint32_t*)d_part_tokens;
    a.n_parts = n_parts;
    a.n_ids = n_ids;
    a.fill_id = fill_id;
    a.counts = (uint32_t*)b.sp_cnt.p;
    a.out_offs = (const uint64_t*)b.sp_offs.p;
    uint64_t total = 0;
    if (n_parts == 0) {
        TK_HIP(c, hipMemsetAsync(b.sp_offs.p, 0, 8, s));
    } else {
        TK_HIP(c, tk_launch_splice_counts(a, s));
        const int rc = scan_u32(c, b.sp_bsum, a.counts, n_parts, (uint64_t*)b.sp_offs.p, s);
        if (rc != TK_OK) return rc;
        TK_HIP(c, hipMemcpyAsync(&total, (const uint64_t*)b.sp_offs.p + n_parts, 8, hipMemcpyDeviceToHost, s));
    }
    TK_HIP(c, hipStreamSynchronize(s));
    TK_HIP(c, b.sp_ids.reserve(total * 4 + 16));
    a.out_ids = (uint32_t*)b.sp_ids.p;
    a.n_out = total;
    TK_HIP(c, tk_launch_splice_fill(a, s));
    TK_HIP(c, hipStreamSynchronize(s));
    out->ids = (uint32_t*)b.sp_ids.p;
    out->offsets = (uint64_t*)b.sp_offs.p;
    out->n_parts = n_parts;
    out->n_ids = total;
    return TK_OK;
}

extern "C" uint64_t tk_audio_splice_calls(const tk_ctx* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lock(const_cast<tk_ctx*>(c)->mu);
    return c->audio.n_splice_calls;
}
