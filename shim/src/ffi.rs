//! The C ABI of tekken-rs_amd/libtekken_hip.so, one declaration per entry of include/tekken_hip.h that a Rust host needs.
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct TkCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct TkNode {
    _p: [u8; 0],
}
#[repr(C)]
pub struct TkTokenizer {
    _p: [u8; 0],
}
#[repr(C)]
pub struct TkResult {
    pub ids: *mut u32,
    pub offsets: *mut u64,
    pub n_ids: u64,
    pub n_docs: u64,
}
#[repr(C)]
pub struct TkTextResult {
    pub bytes: *mut u8,
    pub offsets: *mut u64,
    pub n_bytes: u64,
    pub n_docs: u64,
}

pub const TK_OK: c_int = 0;
pub const TK_ERR_INVALID_CONFIG: c_int = -1;
pub const TK_ERR_RUNTIME: c_int = -2;
pub const TK_ERR_INVALID_UTF8: c_int = -3;
pub const TK_ERR_NO_DEVICE: c_int = -4;
pub const TK_ERR_INVALID_ARG: c_int = -5;
pub const TK_ERR_TOKEN_NOT_FOUND: c_int = -9;
pub const TK_ERR_SPECIAL_POLICY: c_int = -10;
pub const TK_ERR_AUDIO: c_int = -11;

// the checks of the spans entries (above TK_CHECK_OFFSETS = 1 / TK_CHECK_UTF8 = 2: one word can carry all four)
pub const TK_STREAM_FINAL: c_int = 1;
pub const TK_SPANS_CHECK_COVER: c_int = 4;
pub const TK_SPANS_CHECK_BYTES: c_int = 8;
// the unit of the units entries' spans
pub const TK_UNIT_BYTE: c_int = 0;
pub const TK_UNIT_CHAR: c_int = 1;
pub const TK_UNIT_UTF16: c_int = 2;

// model-ready dense batches (tk_dense_opts.flags; include/tekken_hip.h has the definition)
pub const TK_DENSE_PAD_LEFT: u32 = 1;
pub const TK_DENSE_TRUNC_LEFT: u32 = 2;
pub const TK_DENSE_FIXED: u32 = 4;
pub const TK_DENSE_I64: u32 = 8;
pub const TK_DENSE_MASK: u32 = 16;
// audio (include/tekken_hip.h "audio"): the config of the tekken.json, the log-mel options and result, a ragged result
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct TkAudioConfig {
    pub sampling_rate: u64,
    pub frame_rate: f64,
    pub num_mel_bins: u64,
    pub hop_length: u64,
    pub window_size: u64,
    pub chunk_length_s: f64, // valid where has_chunk_length != 0
    pub has_chunk_length: u32,
    pub pad: u32,
}
#[repr(C)]
pub struct TkLogmelOpts {
    pub log_mel_max: f32, // NaN: the per-segment maximum
    pub flags: u32,
}
#[repr(C)]
pub struct TkLogmel {
    pub features: *mut f32,
    pub frame_off: *mut u64, // n_segments + 1
    pub clip_seg: *mut u64,  // n_clips + 1
    pub n_clips: u64,
    pub n_segments: u64,
    pub n_frames: u64,
    pub n_mel: u64,
}
#[repr(C)]
pub struct TkRagged {
    pub ids: *mut u32,
    pub offsets: *mut u64,
    pub n_parts: u64,
    pub n_ids: u64,
}

#[repr(C)]
pub struct TkDenseOpts {
    pub max_length: u32,
    pub multiple_of: u32,
    pub pad_id: u32,
    pub keep_head: u32,
    pub keep_tail: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkDense {
    pub ids: *mut c_void,
    pub mask: *mut u8,
    pub lengths: *mut u32,
    pub n_docs: u64,
    pub row_len: u64,
    pub n_truncated: u64,
}
// packed fixed-length training rows (tk_seqpack_opts.flags; include/tekken_hip.h has the definition)
pub const TK_SEQPACK_I64: u32 = 1;
pub const TK_SEQPACK_POSITIONS: u32 = 2;
pub const TK_SEQPACK_SEGMENTS: u32 = 4;
pub const TK_SEQPACK_CU_SEQLENS: u32 = 8;
pub const TK_SEQPACK_DROP_LAST: u32 = 16;
#[repr(C)]
pub struct TkSeqpackOpts {
    pub seq_len: u32,
    pub pad_id: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkSeqpack {
    pub input_ids: *mut c_void,
    pub position_ids: *mut c_void,
    pub segment_ids: *mut c_void,
    pub cu_seqlens: *mut i32,
    pub n_rows: u64,
    pub row_len: u64,
    pub n_used: u64,
    pub n_left: u64,
    pub n_segments: u64,
    pub max_seqlen: u64,
}
// sentence-pair rows (tk_pair_opts.strategy / .flags; include/tekken_hip.h has the definition)
pub const TK_PAIR_LONGEST_FIRST: u32 = 0;
pub const TK_PAIR_ONLY_FIRST: u32 = 1;
pub const TK_PAIR_ONLY_SECOND: u32 = 2;
pub const TK_PAIR_FIXED: u32 = 1;
pub const TK_PAIR_I64: u32 = 2;
pub const TK_PAIR_MASK: u32 = 4;
pub const TK_PAIR_SPANS: u32 = 8;
pub const TK_PAIR_TYPE_IDS: u32 = 16;
pub const TK_PAIR_SEQUENCE_IDS: u32 = 32;
pub const TK_PAIR_OVERFLOW: u32 = 64;
pub const TK_PAIR_SEQ_NONE: u8 = 255;
#[repr(C)]
pub struct TkPairOpts {
    pub max_length: u32,
    pub strategy: u32,
    pub stride: u32,
    pub max_fixed: u32,
    pub multiple_of: u32,
    pub pad_id: u32,
    pub n_head: u32,
    pub n_sep: u32,
    pub n_tail: u32,
    pub head: [u32; 4],
    pub sep: [u32; 4],
    pub tail: [u32; 4],
    pub flags: u32,
}
#[repr(C)]
pub struct TkPair {
    pub input_ids: *mut c_void,
    pub mask: *mut u8,
    pub type_ids: *mut u8,
    pub sequence_ids: *mut u8,
    pub lengths: *mut u32,
    pub window_pair: *mut u32,
    pub window_start: *mut u32,
    pub second_start: *mut u32,
    pub spans: *mut u32,
    pub pair_windows: *mut u64,
    pub n_pairs: u64,
    pub n_windows: u64,
    pub row_len: u64,
    pub n_truncated: u64,
    pub n_split: u64,
    pub n_fixed_cut: u64,
}
// overlapping windows for long documents (tk_window_opts.flags; include/tekken_hip.h has the definition)
pub const TK_WINDOW_FIXED: u32 = 1;
pub const TK_WINDOW_I64: u32 = 2;
pub const TK_WINDOW_MASK: u32 = 4;
pub const TK_WINDOW_SPANS: u32 = 8;
#[repr(C)]
pub struct TkWindowOpts {
    pub max_length: u32,
    pub stride: u32,
    pub multiple_of: u32,
    pub pad_id: u32,
    pub keep_head: u32,
    pub keep_tail: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkWindow {
    pub input_ids: *mut c_void,
    pub mask: *mut u8,
    pub lengths: *mut u32,
    pub window_doc: *mut u32,
    pub window_start: *mut u32,
    pub doc_windows: *mut u64,
    pub spans: *mut u32,
    pub n_docs: u64,
    pub n_windows: u64,
    pub row_len: u64,
    pub n_split: u64,
}
// boundary-aware token-budget chunks (tk_chunk_opts.flags, the level bytes, tk_chunk_opts.levels; include/tekken_hip.h has the
// definition)
pub const TK_CHUNK_FIXED: u32 = 1;
pub const TK_CHUNK_I64: u32 = 2;
pub const TK_CHUNK_MASK: u32 = 4;
pub const TK_CHUNK_SPANS: u32 = 8;
pub const TK_CHUNK_BYTES: u32 = 16;
pub const TK_CHUNK_LEVEL_NONE: u8 = 0;
pub const TK_CHUNK_LEVEL_TOKEN: u8 = 1;
pub const TK_CHUNK_LEVEL_WORD: u8 = 2;
pub const TK_CHUNK_LEVEL_SENTENCE: u8 = 3;
pub const TK_CHUNK_LEVEL_LINE: u8 = 4;
pub const TK_CHUNK_LEVEL_PARAGRAPH: u8 = 5;
pub const TK_CHUNK_LEVELS_ALL: u32 = 60;
pub const TK_CHUNK_CUT_LAST: u8 = 255;
#[repr(C)]
pub struct TkChunkOpts {
    pub max_length: u32,
    pub min_length: u32,
    pub overlap: u32,
    pub multiple_of: u32,
    pub pad_id: u32,
    pub keep_head: u32,
    pub keep_tail: u32,
    pub levels: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkChunk {
    pub input_ids: *mut c_void,
    pub mask: *mut u8,
    pub lengths: *mut u32,
    pub window_doc: *mut u32,
    pub window_start: *mut u32,
    pub doc_windows: *mut u64,
    pub spans: *mut u32,
    pub cut_level: *mut u8,
    pub chunk_bytes: *mut u32,
    pub level_counts: *mut u64,
    pub n_docs: u64,
    pub n_windows: u64,
    pub row_len: u64,
    pub n_split: u64,
}
// chat batches: parts joined with control ids, plus labels (include/tekken_hip.h has the definition)
pub const TK_CHECK_PARTS: c_int = 16;
pub const TK_JOIN_NONE: u32 = 0xFFFF_FFFF;
pub const TK_PART_LABEL_CTRL: u32 = 1;
pub const TK_PART_LABEL_TEXT: u32 = 2;
pub const TK_JOIN_LABELS: u32 = 1;
pub const TK_JOIN_PART_INDEX: u32 = 2;
#[repr(C)]
pub struct TkJoinOpts {
    pub ignore_index: i32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkJoin {
    pub ids: *mut u32,
    pub offsets: *mut u64,
    pub labels: *mut i32,
    pub part_index: *mut u32,
    pub n_convs: u64,
    pub n_parts: u64,
    pub n_ids: u64,
    pub n_ctrl: u64,
    pub n_labelled: u64,
}
// whole documents packed into rows without cutting them (tk_rowfit_opts.flags; include/tekken_hip.h has the definition)
pub const TK_ROWFIT_I64: u32 = 1;
pub const TK_ROWFIT_POSITIONS: u32 = 2;
pub const TK_ROWFIT_SEGMENTS: u32 = 4;
pub const TK_ROWFIT_CU_SEQLENS: u32 = 8;
pub const TK_ROWFIT_LABELS: u32 = 16;
pub const TK_ROWFIT_DOC_START: u32 = 32;
#[repr(C)]
pub struct TkRowfitOpts {
    pub seq_len: u32,
    pub pad_id: u32,
    pub keep_tail: u32,
    pub flags: u32,
    pub ignore_index: i32,
}
#[repr(C)]
pub struct TkRowfit {
    pub input_ids: *mut c_void,
    pub labels: *mut i32,
    pub position_ids: *mut c_void,
    pub segment_ids: *mut c_void,
    pub cu_seqlens: *mut i32,
    pub doc_start: *mut u64,
    pub n_rows: u64,
    pub row_len: u64,
    pub n_segments: u64,
    pub max_seqlen: u64,
    pub n_truncated: u64,
    pub n_pad: u64,
}
// documents selected, reordered and cut into batches (tk_regroup_opts.order / .flags; include/tekken_hip.h has the definition)
pub const TK_REGROUP_ORDER_KEEP: u32 = 0;
pub const TK_REGROUP_ORDER_LENGTH: u32 = 1;
pub const TK_REGROUP_ORDER_SHUFFLE: u32 = 2;
pub const TK_REGROUP_ORDER_GROUPED: u32 = 3;
pub const TK_REGROUP_DESC: u32 = 1;
pub const TK_REGROUP_LABELS: u32 = 2;
pub const TK_REGROUP_PERM: u32 = 4;
pub const TK_REGROUP_BATCHES: u32 = 8;
pub const TK_REGROUP_BATCH_OFFSETS: u32 = 16;
pub const TK_REGROUP_BATCH_ROWLEN: u32 = 32;
#[repr(C)]
pub struct TkRegroupOpts {
    pub max_tokens: u64,
    pub min_length: u32,
    pub max_length: u32,
    pub order: u32,
    pub seed: u32,
    pub window: u32,
    pub max_docs: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkRegroup {
    pub ids: *mut u32,
    pub offsets: *mut u64,
    pub labels: *mut i32,
    pub perm: *mut u32,
    pub batch_offsets: *mut u64,
    pub batch_rowlen: *mut u32,
    pub n_docs: u64,
    pub n_ids: u64,
    pub n_masked: u64,
    pub n_short: u64,
    pub n_long: u64,
    pub n_batches: u64,
    pub n_oversize: u64,
    pub n_batch_pad: u64,
}
// word ids: the pre-tokenization piece of every id (tk_words_opts.flags, the check bit; include/tekken_hip.h has the definition)
pub const TK_WORD_NONE: u32 = 0xFFFF_FFFF;
pub const TK_WORDS_FIRST: u32 = 1;
pub const TK_WORDS_CHECK_ALIGNED: c_int = 32;
#[repr(C)]
pub struct TkWordsOpts {
    pub flags: u32,
}
#[repr(C)]
pub struct TkWords {
    pub word_ids: *mut u32,
    pub doc_words: *mut u64,
    pub word_first: *mut u32,
    pub n_docs: u64,
    pub n_ids: u64,
    pub n_words: u64,
}
// special-token strings parsed out of text (tk_specials_opts.modes / .flags; include/tekken_hip.h has the definition)
pub const TK_SPECIAL_TEXT: u8 = 0;
pub const TK_SPECIAL_PARSE: u8 = 1;
pub const TK_SPECIAL_RAISE: u8 = 2;
pub const TK_SPECIALS_BOS: u32 = 1;
pub const TK_SPECIALS_EOS: u32 = 2;
pub const TK_SPECIALS_PART_SRC: u32 = 4;
#[repr(C)]
pub struct TkSpecialsOpts {
    pub modes: *const u8,
    pub n_modes: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkSpecials {
    pub bytes: *mut u8,
    pub part_offsets: *mut u64,
    pub part_ctrl: *mut u32,
    pub conv_offsets: *mut u64,
    pub part_src: *mut u64,
    pub n_docs: u64,
    pub n_parts: u64,
    pub n_bytes: u64,
    pub n_matches: u64,
    pub n_removed: u64,
}
// fill-in-the-middle rows (tk_fim_opts.flags, tk_fim.cuts / .mode; include/tekken_hip.h has the definition)
pub const TK_FIM_NO_CUT: u64 = !0;
pub const TK_FIM_SNAP: u32 = 1;
pub const TK_FIM_BOS: u32 = 2;
pub const TK_FIM_EOS: u32 = 4;
pub const TK_FIM_PART_SRC: u32 = 8;
pub const TK_FIM_LABEL_MIDDLE: u32 = 16;
#[repr(C)]
pub struct TkFimOpts {
    pub rate_q32: u64,
    pub spm_q32: u64,
    pub seed: u32,
    pub prefix_id: u32,
    pub suffix_id: u32,
    pub middle_id: u32,
    pub head: u32,
    pub tail: u32,
    pub min_units: u32,
    pub flags: u32,
}
#[repr(C)]
pub struct TkFim {
    pub units: *mut c_void,
    pub part_offsets: *mut u64,
    pub part_ctrl: *mut u32,
    pub part_flags: *mut u32,
    pub conv_offsets: *mut u64,
    pub part_src: *mut u64,
    pub cuts: *mut u64,
    pub mode: *mut u8,
    pub n_docs: u64,
    pub n_parts: u64,
    pub n_units: u64,
    pub n_transformed: u64,
    pub n_spm: u64,
    pub n_skipped: u64,
}
// masked-LM and span-corruption rows (tk_noise_opts.unit / .flags; include/tekken_hip.h has the definition)
pub const TK_NOISE_UNIT_TOKEN: u32 = 0;
pub const TK_NOISE_UNIT_WORD: u32 = 1;
pub const TK_NOISE_SELECTED: u32 = 1;
pub const TK_NOISE_DESC: u32 = 2;
pub const TK_NOISE_SPLIT: u32 = 4;
pub const TK_NOISE_JOINED: u32 = 8;
pub const TK_NOISE_SPAN_LIMIT: u32 = 64;
#[repr(C)]
pub struct TkNoiseOpts {
    pub start_q32: u64,
    pub mask_q32: u64,
    pub random_q32: u64,
    pub seed: u32,
    pub unit: u32,
    pub span_min: u32,
    pub span_max: u32,
    pub mask_id: u32,
    pub n_sentinels: u32,
    pub sentinel_first: u32,
    pub final_id: u32,
    pub flags: u32,
    pub ignore_index: i32,
}
#[repr(C)]
pub struct TkNoiseReplace {
    pub input_ids: *mut u32,
    pub labels: *mut i32,
    pub selected: *mut u8,
    pub n_docs: u64,
    pub n_ids: u64,
    pub n_selected: u64,
    pub n_masked: u64,
    pub n_random: u64,
}
#[repr(C)]
pub struct TkNoiseSpans {
    pub inputs: *mut u32,
    pub input_offsets: *mut u64,
    pub targets: *mut u32,
    pub target_offsets: *mut u64,
    pub joined: *mut u32,
    pub joined_offsets: *mut u64,
    pub joined_labels: *mut i32,
    pub n_docs: u64,
    pub n_selected: u64,
    pub n_runs: u64,
    pub n_runs_dropped: u64,
    pub n_inputs: u64,
    pub n_targets: u64,
}

extern "C" {
    // engine level: replaces CoreBPE::new / CoreBPE::encode (src/tekkenizer.rs:125, :384-386)
    pub fn tk_ctx_create(token_bytes: *const u8, token_offsets: *const u32, n_ranks: u32, num_special_tokens: u32, bos_id: u32,
                         eos_id: u32, device_id: c_int, out_ctx: *mut *mut TkCtx) -> c_int;
    pub fn tk_ctx_destroy(ctx: *mut TkCtx);
    pub fn tk_last_error(ctx: *const TkCtx) -> *const c_char;
    pub fn tk_encode_batch(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                           validate_utf8: c_int, out: *mut TkResult) -> c_int;
    pub fn tk_free_result(r: *mut TkResult);
    // one document, caller-owned output (the reference's own call shape; no allocation per call)
    pub fn tk_encode_one(ctx: *mut TkCtx, text: *const u8, len: u64, add_bos: c_int, add_eos: c_int, ids_out: *mut u32,
                         ids_capacity: u64, n_ids: *mut u64) -> c_int;
    pub fn tk_encode_batch_device(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                  add_bos: c_int, add_eos: c_int, hip_stream: *mut c_void, d_ids: *mut *mut c_void,
                                  d_out_offsets: *mut *mut c_void, n_ids: *mut u64) -> c_int;
    // the same with the checks tk_encode_batch makes for host callers, on the device: TK_CHECK_OFFSETS = 1, TK_CHECK_UTF8 = 2
    pub fn tk_encode_batch_device_ex(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                     add_bos: c_int, add_eos: c_int, checks: c_int, hip_stream: *mut c_void, d_ids: *mut *mut c_void,
                                     d_out_offsets: *mut *mut c_void, n_ids: *mut u64) -> c_int;
    // per-token byte spans: (start, end) of every id, u32 byte offsets relative to the start of its document
    pub fn tk_token_spans_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                 d_doc_offsets: *const c_void, d_bytes: *const c_void, checks: c_int, hip_stream: *mut c_void,
                                 d_spans: *mut *mut c_void, bad_doc: *mut u64) -> c_int;
    pub fn tk_encode_batch_device_spans(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                        add_bos: c_int, add_eos: c_int, checks: c_int, hip_stream: *mut c_void, d_ids: *mut *mut c_void,
                                        d_out_offsets: *mut *mut c_void, d_spans: *mut *mut c_void, n_ids: *mut u64, bad_doc: *mut u64) -> c_int;
    pub fn tk_encode_batch_spans(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                 validate_utf8: c_int, checks: c_int, out: *mut TkResult, spans: *mut *mut u32, bad_doc: *mut u64) -> c_int;
    pub fn tk_free_spans(spans: *mut u32);
    // the same spans in code points or UTF-16 units (unit: TK_UNIT_*), in a context-owned buffer of their own
    pub fn tk_token_spans_units_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                       unit: c_int, hip_stream: *mut c_void, d_spans: *mut *mut c_void) -> c_int;
    pub fn tk_encode_batch_device_spans_units(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                              add_bos: c_int, add_eos: c_int, checks: c_int, unit: c_int, hip_stream: *mut c_void,
                                              d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, d_spans: *mut *mut c_void,
                                              n_ids: *mut u64) -> c_int;
    pub fn tk_encode_batch_spans_units(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                       validate_utf8: c_int, unit: c_int, out: *mut TkResult, spans: *mut *mut u32) -> c_int;
    // annotation (as, ae) of document ann_doc -> the document-relative id range (lo, hi) its span covers
    pub fn tk_spans_locate_device(ctx: *mut TkCtx, d_spans: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                  d_ann_doc: *const c_void, d_ann: *const c_void, n_ann: u64, hip_stream: *mut c_void,
                                  d_tok_range: *mut *mut c_void, bad_ann: *mut u64) -> c_int;
    // tokenizer level, one string: Tekkenizer::encode + offsets (*ids and *spans malloc'ed, both freed with tk_free_ids)
    pub fn tk_tokenizer_encode_with_spans(t: *mut TkTokenizer, text: *const c_char, len: usize, add_bos: c_int, add_eos: c_int,
                                          ids: *mut *mut u32, spans: *mut *mut u32, n_ids: *mut usize) -> c_int;
    pub fn tk_free_ids(ids: *mut u32);
    // dense batches: ragged ids -> dense[D, L] (+ mask, lengths, truncated count), fused with encode, host form, and the inverse
    pub fn tk_dense_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                    opts: *const TkDenseOpts, hip_stream: *mut c_void, out: *mut TkDense) -> c_int;
    pub fn tk_encode_batch_device_dense(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                        add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkDenseOpts, hip_stream: *mut c_void,
                                        d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkDense) -> c_int;
    pub fn tk_encode_batch_dense(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                 validate_utf8: c_int, opts: *const TkDenseOpts, out: *mut TkDense) -> c_int;
    pub fn tk_free_dense(out: *mut TkDense);
    pub fn tk_ragged_from_dense_device(ctx: *mut TkCtx, d_dense: *const c_void, n_docs: u64, row_len: u64, flags: c_int,
                                       d_lengths: *const c_void, pad_id: u32, hip_stream: *mut c_void, d_ids: *mut *mut c_void,
                                       d_id_offsets: *mut *mut c_void, n_ids: *mut u64) -> c_int;
    // packed training rows: the id stream cut into rows of seq_len (+ position_ids, segment_ids, cu_seqlens), fused with encode, host form
    pub fn tk_seqpack_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                      opts: *const TkSeqpackOpts, hip_stream: *mut c_void, out: *mut TkSeqpack) -> c_int;
    pub fn tk_encode_batch_device_seqpack(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                          add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkSeqpackOpts, hip_stream: *mut c_void,
                                          d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkSeqpack) -> c_int;
    pub fn tk_encode_batch_seqpack(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                   validate_utf8: c_int, opts: *const TkSeqpackOpts, out: *mut TkSeqpack) -> c_int;
    pub fn tk_free_seqpack(out: *mut TkSeqpack);
    // overlapping windows: documents longer than max_length split into windows that share `stride` ids (+ mask, spans, the mapping
    // back to the documents), fused with encode, host form
    pub fn tk_window_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                     d_spans: *const c_void, opts: *const TkWindowOpts, hip_stream: *mut c_void, out: *mut TkWindow) -> c_int;
    pub fn tk_encode_batch_device_window(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                         add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkWindowOpts, hip_stream: *mut c_void,
                                         d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkWindow) -> c_int;
    pub fn tk_encode_batch_window(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                  validate_utf8: c_int, opts: *const TkWindowOpts, out: *mut TkWindow) -> c_int;
    pub fn tk_free_window(out: *mut TkWindow);
    // boundary-aware chunks: the level byte of every id from text and spans; long documents cut at the strongest break a chunk can
    // end at (+ cut_level, chunk_bytes, level_counts), fused with encode, host form; the stage times of the last call
    pub fn tk_chunk_levels_device(ctx: *mut TkCtx, d_spans: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                  d_bytes: *const c_void, d_doc_offsets: *const c_void, n_bytes: u64, levels: u32, hip_stream: *mut c_void,
                                  d_levels: *mut *mut c_void) -> c_int;
    pub fn tk_chunk_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                    d_levels: *const c_void, d_spans: *const c_void, opts: *const TkChunkOpts, hip_stream: *mut c_void,
                                    out: *mut TkChunk) -> c_int;
    pub fn tk_encode_batch_device_chunk(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                        add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkChunkOpts, hip_stream: *mut c_void,
                                        d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkChunk) -> c_int;
    pub fn tk_encode_batch_chunk(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                 validate_utf8: c_int, opts: *const TkChunkOpts, out: *mut TkChunk) -> c_int;
    pub fn tk_free_chunk(out: *mut TkChunk);
    pub fn tk_last_chunk_ms(ctx: *const TkCtx, ms: *mut f32);
    // sentence-pair rows: the ids of 2P parts (first text, second text) as rows head + A + sep + B + tail, cut or split into
    // overlapping windows (+ mask, type ids, sequence ids, spans, the mapping back to the pairs), fused with encode, host form
    pub fn tk_pair_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_parts: u64, n_ids: u64,
                                   d_spans: *const c_void, opts: *const TkPairOpts, hip_stream: *mut c_void, out: *mut TkPair) -> c_int;
    pub fn tk_encode_pairs_device(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_parts: u64, n_bytes: u64,
                                  checks: c_int, opts: *const TkPairOpts, hip_stream: *mut c_void, d_ids: *mut *mut c_void,
                                  d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkPair) -> c_int;
    pub fn tk_encode_pairs(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_parts: u64, validate_utf8: c_int,
                           opts: *const TkPairOpts, out: *mut TkPair) -> c_int;
    pub fn tk_free_pair(out: *mut TkPair);
    // chat batches: the ids of text parts joined with control ids per conversation (+ labels, part_index), fused with encode, host form
    pub fn tk_join_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_parts: u64, n_ids: u64,
                                   d_part_ctrl: *const c_void, d_part_flags: *const c_void, d_conv_offsets: *const c_void, n_convs: u64,
                                   checks: c_int, opts: *const TkJoinOpts, hip_stream: *mut c_void, out: *mut TkJoin) -> c_int;
    pub fn tk_encode_parts_device_join(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_parts: u64, n_bytes: u64,
                                       d_part_ctrl: *const c_void, d_part_flags: *const c_void, d_conv_offsets: *const c_void, n_convs: u64,
                                       checks: c_int, opts: *const TkJoinOpts, hip_stream: *mut c_void, out: *mut TkJoin) -> c_int;
    pub fn tk_encode_parts_join(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_parts: u64, part_ctrl: *const u32,
                                part_flags: *const u32, conv_offsets: *const u64, n_convs: u64, validate_utf8: c_int,
                                opts: *const TkJoinOpts, out: *mut TkJoin) -> c_int;
    pub fn tk_free_join(out: *mut TkJoin);
    // whole-document rows (next-fit, never cut) behind encode or a join: ids, labels, positions, segments, cu_seqlens, doc_start
    pub fn tk_rowfit_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                     d_labels: *const c_void, opts: *const TkRowfitOpts, hip_stream: *mut c_void, out: *mut TkRowfit) -> c_int;
    pub fn tk_encode_batch_device_rowfit(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                         add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkRowfitOpts, hip_stream: *mut c_void,
                                         d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkRowfit) -> c_int;
    pub fn tk_encode_parts_device_rowfit(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_parts: u64, n_bytes: u64,
                                         d_part_ctrl: *const c_void, d_part_flags: *const c_void, d_conv_offsets: *const c_void, n_convs: u64,
                                         checks: c_int, join_opts: *const TkJoinOpts, opts: *const TkRowfitOpts, hip_stream: *mut c_void,
                                         joined: *mut TkJoin, out: *mut TkRowfit) -> c_int;
    pub fn tk_encode_batch_rowfit(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                  validate_utf8: c_int, opts: *const TkRowfitOpts, out: *mut TkRowfit) -> c_int;
    pub fn tk_free_rowfit(out: *mut TkRowfit);
    pub fn tk_last_rowfit_ms(ctx: *const TkCtx, placement_ms: *mut f32, fill_ms: *mut f32, cu_ms: *mut f32);
    pub fn tk_regroup_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                      d_labels: *const c_void, d_keep: *const c_void, opts: *const TkRegroupOpts, hip_stream: *mut c_void,
                                      out: *mut TkRegroup) -> c_int;
    pub fn tk_encode_batch_device_regroup(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                          add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkRegroupOpts, hip_stream: *mut c_void,
                                          d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkRegroup) -> c_int;
    pub fn tk_encode_batch_regroup(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                   validate_utf8: c_int, opts: *const TkRegroupOpts, out: *mut TkRegroup) -> c_int;
    pub fn tk_free_regroup(out: *mut TkRegroup);
    pub fn tk_last_regroup_ms(ctx: *const TkCtx, ms: *mut f32);
    pub fn tk_specials_split_device(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                    checks: c_int, opts: *const TkSpecialsOpts, hip_stream: *mut c_void, out: *mut TkSpecials,
                                    bad: *mut u64) -> c_int;
    pub fn tk_encode_batch_device_parsed(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                         checks: c_int, opts: *const TkSpecialsOpts, jopts: *const TkJoinOpts, hip_stream: *mut c_void,
                                         parts: *mut TkSpecials, out: *mut TkJoin, bad: *mut u64) -> c_int;
    pub fn tk_encode_batch_parsed(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, validate_utf8: c_int,
                                  opts: *const TkSpecialsOpts, jopts: *const TkJoinOpts, parts: *mut TkSpecials, out: *mut TkJoin,
                                  bad: *mut u64) -> c_int;
    pub fn tk_free_specials(out: *mut TkSpecials);
    pub fn tk_last_specials_ms(ctx: *const TkCtx, ms: *mut f32);
    pub fn tk_specials_tile() -> u32;
    pub fn tk_tokenizer_encode_parsed(t: *mut TkTokenizer, text: *const c_char, len: usize, add_bos: c_int, add_eos: c_int, modes: *const u8,
                                      n_modes: u32, ids: *mut *mut u32, n_ids: *mut usize) -> c_int;
    pub fn tk_fim_split_device(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                               d_cuts: *const c_void, checks: c_int, opts: *const TkFimOpts, hip_stream: *mut c_void, out: *mut TkFim) -> c_int;
    pub fn tk_fim_split_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                   d_cuts: *const c_void, opts: *const TkFimOpts, hip_stream: *mut c_void, out: *mut TkFim) -> c_int;
    pub fn tk_encode_batch_device_fim(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                      d_cuts: *const c_void, checks: c_int, opts: *const TkFimOpts, jopts: *const TkJoinOpts,
                                      hip_stream: *mut c_void, parts: *mut TkFim, out: *mut TkJoin) -> c_int;
    pub fn tk_fim_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                  d_cuts: *const c_void, opts: *const TkFimOpts, jopts: *const TkJoinOpts, hip_stream: *mut c_void,
                                  parts: *mut TkFim, out: *mut TkJoin) -> c_int;
    pub fn tk_encode_batch_fim(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, cuts: *const u64,
                               validate_utf8: c_int, opts: *const TkFimOpts, jopts: *const TkJoinOpts, parts: *mut TkFim,
                               out: *mut TkJoin) -> c_int;
    pub fn tk_free_fim(out: *mut TkFim);
    pub fn tk_last_fim_ms(ctx: *const TkCtx, ms: *mut f32);
    pub fn tk_fim_tile(unit_bytes: c_int) -> u32;
    pub fn tk_noise_replace_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                   d_word_ids: *const c_void, d_sel: *const c_void, opts: *const TkNoiseOpts, hip_stream: *mut c_void,
                                   out: *mut TkNoiseReplace) -> c_int;
    pub fn tk_noise_spans_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                 d_word_ids: *const c_void, d_sel: *const c_void, opts: *const TkNoiseOpts, hip_stream: *mut c_void,
                                 out: *mut TkNoiseSpans) -> c_int;
    pub fn tk_encode_batch_device_noise_replace(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64,
                                                n_bytes: u64, add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkNoiseOpts,
                                                hip_stream: *mut c_void, d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void,
                                                n_ids: *mut u64, out: *mut TkNoiseReplace) -> c_int;
    pub fn tk_encode_batch_device_noise_spans(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                              add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkNoiseOpts, hip_stream: *mut c_void,
                                              d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64,
                                              out: *mut TkNoiseSpans) -> c_int;
    pub fn tk_encode_batch_noise_replace(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int,
                                         add_eos: c_int, validate_utf8: c_int, opts: *const TkNoiseOpts, ids_out: *mut TkResult,
                                         out: *mut TkNoiseReplace) -> c_int;
    pub fn tk_encode_batch_noise_spans(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                       validate_utf8: c_int, opts: *const TkNoiseOpts, ids_out: *mut TkResult, out: *mut TkNoiseSpans) -> c_int;
    pub fn tk_free_noise_replace(out: *mut TkNoiseReplace);
    pub fn tk_free_noise_spans(out: *mut TkNoiseSpans);
    pub fn tk_last_noise_ms(ctx: *const TkCtx, ms: *mut f32);
    pub fn tk_noise_tile() -> u32;
    pub fn tk_words_from_ids_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                    d_bytes: *const c_void, d_doc_offsets: *const c_void, n_bytes: u64, checks: c_int,
                                    opts: *const TkWordsOpts, hip_stream: *mut c_void, out: *mut TkWords, bad: *mut u64) -> c_int;
    pub fn tk_encode_batch_device_words(ctx: *mut TkCtx, d_bytes: *const c_void, d_doc_offsets: *const c_void, n_docs: u64, n_bytes: u64,
                                        add_bos: c_int, add_eos: c_int, checks: c_int, opts: *const TkWordsOpts, hip_stream: *mut c_void,
                                        d_ids: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_ids: *mut u64, out: *mut TkWords,
                                        bad: *mut u64) -> c_int;
    pub fn tk_encode_batch_words(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int, add_eos: c_int,
                                 validate_utf8: c_int, checks: c_int, opts: *const TkWordsOpts, ids_out: *mut TkResult, out: *mut TkWords,
                                 bad: *mut u64) -> c_int;
    pub fn tk_free_words(out: *mut TkWords);
    pub fn tk_last_words_ms(ctx: *const TkCtx, ms: *mut f32);
    // memo of merged pieces (round 4): a device table {unknown piece of 2..16 bytes -> its <= 4 ids}; never changes an id
    pub fn tk_ctx_set_memo(ctx: *mut TkCtx, log2_entries: c_int, policy: c_int) -> c_int;
    pub fn tk_ctx_memo_clear(ctx: *mut TkCtx) -> c_int;
    pub fn tk_memo_stats(ctx: *const TkCtx, lookups_last: *mut u64, hits_last: *mut u64, lookups_total: *mut u64, hits_total: *mut u64,
                         active_last: *mut c_int) -> c_int;
    pub fn tk_host_alloc(bytes: usize) -> *mut c_void;
    pub fn tk_host_free(p: *mut c_void);
    pub fn tk_encode_batch_pipelined(ctx: *mut TkCtx, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int,
                                     add_eos: c_int, slice_bytes: u64, ids_out: *mut u32, ids_capacity: u64, offsets_out: *mut u64,
                                     n_ids: *mut u64) -> c_int;
    pub fn tk_ctx_set_special_tokens(ctx: *mut TkCtx, strings_blob: *const u8, string_offsets: *const u32, n: u32) -> c_int;
    pub fn tk_decode_batch(ctx: *mut TkCtx, ids: *const u32, id_offsets: *const u64, n_docs: u64, policy: c_int,
                           out: *mut TkTextResult, bad_doc: *mut u64) -> c_int;
    pub fn tk_free_text_result(r: *mut TkTextResult);
    // lossy decode (invalid UTF-8 -> U+FFFD, a run of non-special ids at a time) and the stream step for generation
    // (state: one u32 per sequence, bytes 0..2 the pending bytes, byte 3 their count; TK_STREAM_FINAL flushes)
    pub fn tk_decode_batch_lossy(ctx: *mut TkCtx, ids: *const u32, id_offsets: *const u64, n_docs: u64, policy: c_int,
                                 out: *mut TkTextResult, bad_doc: *mut u64, n_replaced: *mut u64, first_bad_doc: *mut u64) -> c_int;
    pub fn tk_decode_batch_device_lossy(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_docs: u64, n_ids: u64,
                                        policy: c_int, hip_stream: *mut c_void, d_bytes: *mut *mut c_void,
                                        d_out_offsets: *mut *mut c_void, n_bytes: *mut u64, bad_doc: *mut u64,
                                        n_replaced: *mut u64, first_bad_doc: *mut u64) -> c_int;
    pub fn tk_decode_stream_step_device(ctx: *mut TkCtx, d_state: *mut c_void, d_ids: *const c_void, d_id_offsets: *const c_void,
                                        n_seqs: u64, n_ids: u64, policy: c_int, flags: c_int, hip_stream: *mut c_void,
                                        d_bytes: *mut *mut c_void, d_out_offsets: *mut *mut c_void, n_bytes: *mut u64,
                                        bad_seq: *mut u64) -> c_int;
    pub fn tk_decode_stream_step(ctx: *mut TkCtx, state: *mut u32, ids: *const u32, id_offsets: *const u64, n_seqs: u64,
                                 policy: c_int, flags: c_int, out: *mut TkTextResult, bad_seq: *mut u64) -> c_int;
    pub fn tk_last_decode_lossy_ms(ctx: *const TkCtx, strict_ms: *mut f32, repair_ms: *mut f32);
    pub fn tk_last_decode_lossy_stats(ctx: *const TkCtx, n_replaced: *mut u64, n_bad_docs: *mut u64, n_repair_launches: *mut u64);
    pub fn tk_ctx_set_pattern(ctx: *mut TkCtx, mode: c_int) -> c_int;
    // audio: the ids of a clip ([BEGIN_AUDIO] + [AUDIO] * N), the log-mel features of a batch of clips, the splice of audio parts
    pub fn tk_tokenizer_from_file(path: *const c_char, device_id: c_int, out: *mut *mut TkTokenizer) -> c_int;
    pub fn tk_tokenizer_destroy(t: *mut TkTokenizer);
    pub fn tk_tokenizer_last_error(t: *const TkTokenizer) -> *const c_char;
    pub fn tk_tokenizer_ctx(t: *mut TkTokenizer) -> *mut TkCtx;
    pub fn tk_tokenizer_has_audio(t: *const TkTokenizer) -> c_int;
    pub fn tk_tokenizer_audio_config(t: *mut TkTokenizer, out: *mut TkAudioConfig) -> c_int;
    pub fn tk_tokenizer_audio_ids(t: *mut TkTokenizer, audio_id: *mut u32, begin_audio_id: *mut u32) -> c_int;
    pub fn tk_tokenizer_encode_audio(t: *mut TkTokenizer, n_samples: u64, clip_rate: u64, ids: *mut *mut u32, n_ids: *mut usize,
                                     padded_samples: *mut u64) -> c_int;
    pub fn tk_audio_layout(cfg: *const TkAudioConfig, n_samples: *const u64, n_clips: u64, padded: *mut u64, n_frames: *mut u64,
                           n_tokens: *mut u64, n_segments: *mut u64) -> c_int;
    pub fn tk_audio_set_config(ctx: *mut TkCtx, cfg: *const TkAudioConfig) -> c_int;
    pub fn tk_audio_logmel_device(ctx: *mut TkCtx, d_samples: *const c_void, d_sample_offsets: *const c_void, n_clips: u64, n_samples: u64,
                                  checks: c_int, opts: *const TkLogmelOpts, hip_stream: *mut c_void, out: *mut TkLogmel) -> c_int;
    pub fn tk_audio_logmel(ctx: *mut TkCtx, samples: *const f32, sample_offsets: *const u64, n_clips: u64, opts: *const TkLogmelOpts,
                           out: *mut TkLogmel) -> c_int;
    pub fn tk_free_logmel(out: *mut TkLogmel);
    pub fn tk_audio_frame_tile() -> u32;
    pub fn tk_last_logmel_ms(ctx: *const TkCtx, ms: *mut f32);
    pub fn tk_audio_splice_device(ctx: *mut TkCtx, d_ids: *const c_void, d_id_offsets: *const c_void, n_parts: u64, n_ids: u64,
                                  d_part_tokens: *const c_void, fill_id: u32, hip_stream: *mut c_void, out: *mut TkRagged) -> c_int;
    pub fn tk_audio_splice_calls(ctx: *const TkCtx) -> u64;

    // node level: every GPU of the node behind one call (north star: documents sharded across the GPUs, one RCCL
    // gather of the id buffers over xGMI); SURVEY section 8b `ctx_create(.., device_ids[], n_devices, ..)`
    pub fn tk_node_create(token_bytes: *const u8, token_offsets: *const u32, n_ranks: u32, num_special_tokens: u32, bos_id: u32,
                          eos_id: u32, device_ids: *const c_int, n_devices: c_int, out_node: *mut *mut TkNode) -> c_int;
    pub fn tk_node_destroy(node: *mut TkNode);
    pub fn tk_node_last_error(node: *const TkNode) -> *const c_char;
    pub fn tk_node_encode_batch(node: *mut TkNode, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int,
                                add_eos: c_int, out: *mut TkResult) -> c_int;
    // caller-owned host buffers (tk_host_alloc: pinned -- nothing allocated, pinned or copied on the host per call)
    pub fn tk_node_encode_batch_pinned(node: *mut TkNode, bytes: *const u8, doc_offsets: *const u64, n_docs: u64, add_bos: c_int,
                                       add_eos: c_int, ids_out: *mut u32, ids_capacity: u64, offsets_out: *mut u64, n_ids_out: *mut u64) -> c_int;
    // how the last batch was cut: text bytes and ids of every device's run
    pub fn tk_node_last_shards(node: *const TkNode, shard_bytes: *mut u64, shard_ids: *mut u64, cap: c_int) -> c_int;
}
