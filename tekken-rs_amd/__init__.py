"""tekken-rs_amd -- MI355X-native batch tokenization behind tekken-rs's `Tekkenizer::encode`.

Python is plumbing here: this module only loads the in-tree C-ABI library
(`libtekken_hip.so`, built from csrc/ by `make -C tekken-rs_amd`) with ctypes and mirrors the
reference's public surface for this path --

    Tekkenizer.from_file / encode / decode / SpecialTokenPolicy     (reference src/tekkenizer.rs:222,378,436;
                                                                     src/special_tokens.rs:128-136)

plus the batch and device-resident entry points that the GPU path adds.  There is no CPU
fallback: if the library or a HIP device is missing, calls raise.

The directory name contains a hyphen, so import it with
`importlib.import_module("tekken-rs_amd")`.
"""
import ctypes
import enum
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (TK_HIP_LIB: another build of the same library -- the development build with the timing ablations, `make ablate`, or an A / B
# variant --, so that no tool ever has to copy a variant over the shipped file)
LIB_PATH = os.environ.get("TK_HIP_LIB") or os.path.join(_HERE, "libtekken_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

TK_OK = 0
CHECK_OFFSETS, CHECK_UTF8 = 1, 2   # tk_encode_batch_device_ex
SPANS_CHECK_COVER, SPANS_CHECK_BYTES = 4, 8   # the spans entries (tk_token_spans_device, tk_encode_batch_*spans)
UNIT_BYTE, UNIT_CHAR, UNIT_UTF16 = 0, 1, 2   # the unit of the units entries' spans (tk_token_spans_units_device)
_UNITS = {"byte": UNIT_BYTE, "char": UNIT_CHAR, "utf16": UNIT_UTF16}   # the offsets_unit keyword of the Tekkenizer methods
STREAM_FINAL = 1   # tk_decode_stream_step[_device] flags: write every open prefix as U+FFFD, leave the states 0
DENSE_PAD_LEFT, DENSE_TRUNC_LEFT, DENSE_FIXED, DENSE_I64, DENSE_MASK = 1, 2, 4, 8, 16   # tk_dense_opts.flags (the dense entries)
SEQPACK_I64, SEQPACK_POSITIONS, SEQPACK_SEGMENTS, SEQPACK_CU_SEQLENS, SEQPACK_DROP_LAST = 1, 2, 4, 8, 16   # tk_seqpack_opts.flags (the packed entries)
WINDOW_FIXED, WINDOW_I64, WINDOW_MASK, WINDOW_SPANS = 1, 2, 4, 8   # tk_window_opts.flags (the window entries)
CHUNK_FIXED, CHUNK_I64, CHUNK_MASK, CHUNK_SPANS, CHUNK_BYTES = 1, 2, 4, 8, 16   # tk_chunk_opts.flags (the chunk entries)
CHUNK_LEVEL_NONE, CHUNK_LEVEL_TOKEN, CHUNK_LEVEL_WORD, CHUNK_LEVEL_SENTENCE, CHUNK_LEVEL_LINE, CHUNK_LEVEL_PARAGRAPH = 0, 1, 2, 3, 4, 5   # the level bytes
CHUNK_LEVELS_ALL = 60   # tk_chunk_opts.levels: bit 1 << level of every level that can be disabled
CHUNK_CUT_LAST = 255   # cut_level: a document's last chunk
_LEVELS = {"word": CHUNK_LEVEL_WORD, "sentence": CHUNK_LEVEL_SENTENCE, "line": CHUNK_LEVEL_LINE, "paragraph": CHUNK_LEVEL_PARAGRAPH}   # the levels keyword of encode_batch_chunks
PAIR_LONGEST_FIRST, PAIR_ONLY_FIRST, PAIR_ONLY_SECOND = 0, 1, 2   # tk_pair_opts.strategy
PAIR_FIXED, PAIR_I64, PAIR_MASK, PAIR_SPANS, PAIR_TYPE_IDS, PAIR_SEQUENCE_IDS, PAIR_OVERFLOW = 1, 2, 4, 8, 16, 32, 64   # tk_pair_opts.flags (the pair entries)
PAIR_SEQ_NONE = 255   # sequence_ids: a fixed id or a pad (HF's None)
_STRATEGIES = {"longest_first": PAIR_LONGEST_FIRST, "only_first": PAIR_ONLY_FIRST, "only_second": PAIR_ONLY_SECOND}   # the truncation keyword of encode_pairs
CHECK_PARTS = 16   # the join entries: conv_offsets and the control ids are checked (beside CHECK_OFFSETS / CHECK_UTF8 in one word)
JOIN_NONE = 0xFFFFFFFF   # part_ctrl: the part has no control id
PART_LABEL_CTRL, PART_LABEL_TEXT = 1, 2   # part_flags
JOIN_LABELS, JOIN_PART_INDEX = 1, 2   # tk_join_opts.flags (the join entries)
ROWFIT_I64, ROWFIT_POSITIONS, ROWFIT_SEGMENTS, ROWFIT_CU_SEQLENS, ROWFIT_LABELS, ROWFIT_DOC_START = 1, 2, 4, 8, 16, 32   # tk_rowfit_opts.flags (the rowfit entries)
REGROUP_ORDER_KEEP, REGROUP_ORDER_LENGTH, REGROUP_ORDER_SHUFFLE, REGROUP_ORDER_GROUPED = 0, 1, 2, 3   # tk_regroup_opts.order
REGROUP_DESC, REGROUP_LABELS, REGROUP_PERM, REGROUP_BATCHES, REGROUP_BATCH_OFFSETS, REGROUP_BATCH_ROWLEN = 1, 2, 4, 8, 16, 32   # tk_regroup_opts.flags (the regroup entries)
WORD_NONE = 0xFFFFFFFF   # word_ids: a special id (HF's None)
WORDS_FIRST = 1   # tk_words_opts.flags (the words entries)
WORDS_CHECK_ALIGNED = 32   # the words entries' check (beside CHECK_OFFSETS / CHECK_UTF8 in one word)
SPECIAL_TEXT, SPECIAL_PARSE, SPECIAL_RAISE = 0, 1, 2   # tk_specials_opts.modes: what a special-token string found in text becomes
SPECIALS_BOS, SPECIALS_EOS, SPECIALS_PART_SRC = 1, 2, 4   # tk_specials_opts.flags (the specials entries)
FIM_NO_CUT = 0xFFFFFFFFFFFFFFFF   # cuts[d][0]: leave document d alone; cuts out: the document was not transformed
FIM_SNAP, FIM_BOS, FIM_EOS, FIM_PART_SRC, FIM_LABEL_MIDDLE = 1, 2, 4, 8, 16   # tk_fim_opts.flags (the fill-in-the-middle entries)
FIM_NONE, FIM_PSM, FIM_SPM = 0, 1, 2   # tk_fim.mode
NOISE_UNIT_TOKEN, NOISE_UNIT_WORD = 0, 1   # tk_noise_opts.unit (the noise entries: masked-LM and span-corruption rows)
NOISE_SELECTED, NOISE_DESC, NOISE_SPLIT, NOISE_JOINED = 1, 2, 4, 8   # tk_noise_opts.flags
NOISE_SPAN_LIMIT = 64   # the largest span_max
_NOISE_UNITS = {"token": NOISE_UNIT_TOKEN, "word": NOISE_UNIT_WORD}   # the unit keyword of encode_batch_mlm / encode_batch_span_corruption
_ORDERS = {"keep": REGROUP_ORDER_KEEP, "length": REGROUP_ORDER_LENGTH, "shuffle": REGROUP_ORDER_SHUFFLE, "grouped": REGROUP_ORDER_GROUPED}   # the order keyword of encode_batch_regrouped
TK_ERR_INVALID_CONFIG = -1
TK_ERR_RUNTIME = -2
TK_ERR_INVALID_UTF8 = -3
TK_ERR_NO_DEVICE = -4
TK_ERR_INVALID_ARG = -5
TK_ERR_IO = -6
TK_ERR_JSON = -7
TK_ERR_BASE64 = -8
TK_ERR_TOKEN_NOT_FOUND = -9
TK_ERR_SPECIAL_POLICY = -10
TK_ERR_AUDIO = -11


class TokenizerError(Exception):
    """Mirror of tekken::errors::TokenizerError (reference src/errors.rs:23-59)."""
    KIND = {TK_ERR_INVALID_CONFIG: "InvalidConfig", TK_ERR_RUNTIME: "Tokenizers", TK_ERR_INVALID_UTF8: "Tokenizers",
            TK_ERR_NO_DEVICE: "Tokenizers", TK_ERR_INVALID_ARG: "InvalidConfig", TK_ERR_IO: "Io", TK_ERR_JSON: "Json",
            TK_ERR_BASE64: "Base64", TK_ERR_TOKEN_NOT_FOUND: "TokenNotFound",
            TK_ERR_SPECIAL_POLICY: "SpecialTokenPolicy", TK_ERR_AUDIO: "Audio"}

    def __init__(self, code, message):
        self.code = code
        self.kind = self.KIND.get(code, "Tokenizers")
        super().__init__("%s: %s" % (self.kind, message))


class SpecialTokenPolicy(enum.IntEnum):
    """reference src/special_tokens.rs:128-136"""
    Ignore = 0
    Keep = 1
    Raise = 2


class _TextResult(ctypes.Structure):
    _fields_ = [("bytes", ctypes.POINTER(ctypes.c_uint8)), ("offsets", ctypes.POINTER(ctypes.c_uint64)),
                ("n_bytes", ctypes.c_uint64), ("n_docs", ctypes.c_uint64)]


class _Result(ctypes.Structure):
    _fields_ = [("ids", ctypes.POINTER(ctypes.c_uint32)), ("offsets", ctypes.POINTER(ctypes.c_uint64)),
                ("n_ids", ctypes.c_uint64), ("n_docs", ctypes.c_uint64)]


class _DenseOpts(ctypes.Structure):
    _fields_ = [("max_length", ctypes.c_uint32), ("multiple_of", ctypes.c_uint32), ("pad_id", ctypes.c_uint32),
                ("keep_head", ctypes.c_uint32), ("keep_tail", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Dense(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("lengths", ctypes.c_void_p),
                ("n_docs", ctypes.c_uint64), ("row_len", ctypes.c_uint64), ("n_truncated", ctypes.c_uint64)]


class _SeqpackOpts(ctypes.Structure):
    _fields_ = [("seq_len", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Seqpack(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("position_ids", ctypes.c_void_p), ("segment_ids", ctypes.c_void_p),
                ("cu_seqlens", ctypes.c_void_p), ("n_rows", ctypes.c_uint64), ("row_len", ctypes.c_uint64), ("n_used", ctypes.c_uint64),
                ("n_left", ctypes.c_uint64), ("n_segments", ctypes.c_uint64), ("max_seqlen", ctypes.c_uint64)]


class _WindowOpts(ctypes.Structure):
    _fields_ = [("max_length", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("multiple_of", ctypes.c_uint32), ("pad_id", ctypes.c_uint32),
                ("keep_head", ctypes.c_uint32), ("keep_tail", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Window(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("window_doc", ctypes.c_void_p),
                ("window_start", ctypes.c_void_p), ("doc_windows", ctypes.c_void_p), ("spans", ctypes.c_void_p),
                ("n_docs", ctypes.c_uint64), ("n_windows", ctypes.c_uint64), ("row_len", ctypes.c_uint64), ("n_split", ctypes.c_uint64)]


class _ChunkOpts(ctypes.Structure):
    _fields_ = [("max_length", ctypes.c_uint32), ("min_length", ctypes.c_uint32), ("overlap", ctypes.c_uint32), ("multiple_of", ctypes.c_uint32),
                ("pad_id", ctypes.c_uint32), ("keep_head", ctypes.c_uint32), ("keep_tail", ctypes.c_uint32), ("levels", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class _Chunk(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("window_doc", ctypes.c_void_p),
                ("window_start", ctypes.c_void_p), ("doc_windows", ctypes.c_void_p), ("spans", ctypes.c_void_p),
                ("cut_level", ctypes.c_void_p), ("chunk_bytes", ctypes.c_void_p), ("level_counts", ctypes.c_void_p),
                ("n_docs", ctypes.c_uint64), ("n_windows", ctypes.c_uint64), ("row_len", ctypes.c_uint64), ("n_split", ctypes.c_uint64)]


class _PairOpts(ctypes.Structure):
    _fields_ = [("max_length", ctypes.c_uint32), ("strategy", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("max_fixed", ctypes.c_uint32),
                ("multiple_of", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("n_head", ctypes.c_uint32), ("n_sep", ctypes.c_uint32),
                ("n_tail", ctypes.c_uint32), ("head", ctypes.c_uint32 * 4), ("sep", ctypes.c_uint32 * 4), ("tail", ctypes.c_uint32 * 4),
                ("flags", ctypes.c_uint32)]


class _Pair(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("type_ids", ctypes.c_void_p), ("sequence_ids", ctypes.c_void_p),
                ("lengths", ctypes.c_void_p), ("window_pair", ctypes.c_void_p), ("window_start", ctypes.c_void_p),
                ("second_start", ctypes.c_void_p), ("spans", ctypes.c_void_p), ("pair_windows", ctypes.c_void_p),
                ("n_pairs", ctypes.c_uint64), ("n_windows", ctypes.c_uint64), ("row_len", ctypes.c_uint64), ("n_truncated", ctypes.c_uint64),
                ("n_split", ctypes.c_uint64), ("n_fixed_cut", ctypes.c_uint64)]


class _JoinOpts(ctypes.Structure):
    _fields_ = [("ignore_index", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class _Join(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("part_index", ctypes.c_void_p),
                ("n_convs", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_ids", ctypes.c_uint64), ("n_ctrl", ctypes.c_uint64),
                ("n_labelled", ctypes.c_uint64)]


class _RowfitOpts(ctypes.Structure):
    _fields_ = [("seq_len", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("keep_tail", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("ignore_index", ctypes.c_int32)]


class _Rowfit(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("position_ids", ctypes.c_void_p), ("segment_ids", ctypes.c_void_p),
                ("cu_seqlens", ctypes.c_void_p), ("doc_start", ctypes.c_void_p), ("n_rows", ctypes.c_uint64), ("row_len", ctypes.c_uint64),
                ("n_segments", ctypes.c_uint64), ("max_seqlen", ctypes.c_uint64), ("n_truncated", ctypes.c_uint64), ("n_pad", ctypes.c_uint64)]


class _RegroupOpts(ctypes.Structure):
    _fields_ = [("max_tokens", ctypes.c_uint64), ("min_length", ctypes.c_uint32), ("max_length", ctypes.c_uint32), ("order", ctypes.c_uint32),
                ("seed", ctypes.c_uint32), ("window", ctypes.c_uint32), ("max_docs", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Regroup(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("perm", ctypes.c_void_p),
                ("batch_offsets", ctypes.c_void_p), ("batch_rowlen", ctypes.c_void_p), ("n_docs", ctypes.c_uint64), ("n_ids", ctypes.c_uint64),
                ("n_masked", ctypes.c_uint64), ("n_short", ctypes.c_uint64), ("n_long", ctypes.c_uint64), ("n_batches", ctypes.c_uint64),
                ("n_oversize", ctypes.c_uint64), ("n_batch_pad", ctypes.c_uint64)]


class _SpecialsOpts(ctypes.Structure):
    _fields_ = [("modes", ctypes.POINTER(ctypes.c_uint8)), ("n_modes", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Specials(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_void_p), ("part_offsets", ctypes.c_void_p), ("part_ctrl", ctypes.c_void_p), ("conv_offsets", ctypes.c_void_p),
                ("part_src", ctypes.c_void_p), ("n_docs", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64),
                ("n_matches", ctypes.c_uint64), ("n_removed", ctypes.c_uint64)]


class _FimOpts(ctypes.Structure):
    _fields_ = [("rate_q32", ctypes.c_uint64), ("spm_q32", ctypes.c_uint64), ("seed", ctypes.c_uint32), ("prefix_id", ctypes.c_uint32),
                ("suffix_id", ctypes.c_uint32), ("middle_id", ctypes.c_uint32), ("head", ctypes.c_uint32), ("tail", ctypes.c_uint32),
                ("min_units", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Fim(ctypes.Structure):
    _fields_ = [("units", ctypes.c_void_p), ("part_offsets", ctypes.c_void_p), ("part_ctrl", ctypes.c_void_p), ("part_flags", ctypes.c_void_p),
                ("conv_offsets", ctypes.c_void_p), ("part_src", ctypes.c_void_p), ("cuts", ctypes.c_void_p), ("mode", ctypes.c_void_p),
                ("n_docs", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_units", ctypes.c_uint64), ("n_transformed", ctypes.c_uint64),
                ("n_spm", ctypes.c_uint64), ("n_skipped", ctypes.c_uint64)]


class _NoiseOpts(ctypes.Structure):
    _fields_ = [("start_q32", ctypes.c_uint64), ("mask_q32", ctypes.c_uint64), ("random_q32", ctypes.c_uint64), ("seed", ctypes.c_uint32),
                ("unit", ctypes.c_uint32), ("span_min", ctypes.c_uint32), ("span_max", ctypes.c_uint32), ("mask_id", ctypes.c_uint32),
                ("n_sentinels", ctypes.c_uint32), ("sentinel_first", ctypes.c_uint32), ("final_id", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("ignore_index", ctypes.c_int32)]


class _NoiseReplace(ctypes.Structure):
    _fields_ = [("input_ids", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("selected", ctypes.c_void_p), ("n_docs", ctypes.c_uint64),
                ("n_ids", ctypes.c_uint64), ("n_selected", ctypes.c_uint64), ("n_masked", ctypes.c_uint64), ("n_random", ctypes.c_uint64)]


class _NoiseSpans(ctypes.Structure):
    _fields_ = [("inputs", ctypes.c_void_p), ("input_offsets", ctypes.c_void_p), ("targets", ctypes.c_void_p), ("target_offsets", ctypes.c_void_p),
                ("joined", ctypes.c_void_p), ("joined_offsets", ctypes.c_void_p), ("joined_labels", ctypes.c_void_p), ("n_docs", ctypes.c_uint64),
                ("n_selected", ctypes.c_uint64), ("n_runs", ctypes.c_uint64), ("n_runs_dropped", ctypes.c_uint64), ("n_inputs", ctypes.c_uint64),
                ("n_targets", ctypes.c_uint64)]


class _WordsOpts(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32)]


class _Words(ctypes.Structure):
    _fields_ = [("word_ids", ctypes.c_void_p), ("doc_words", ctypes.c_void_p), ("word_first", ctypes.c_void_p),
                ("n_docs", ctypes.c_uint64), ("n_ids", ctypes.c_uint64), ("n_words", ctypes.c_uint64)]


_LIB = None


class _AudioConfig(ctypes.Structure):
    _fields_ = [("sampling_rate", ctypes.c_uint64), ("frame_rate", ctypes.c_double), ("num_mel_bins", ctypes.c_uint64),
                ("hop_length", ctypes.c_uint64), ("window_size", ctypes.c_uint64), ("chunk_length_s", ctypes.c_double),
                ("has_chunk_length", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class _LogmelOpts(ctypes.Structure):
    _fields_ = [("log_mel_max", ctypes.c_float), ("flags", ctypes.c_uint32)]


class _Logmel(ctypes.Structure):
    _fields_ = [("features", ctypes.c_void_p), ("frame_off", ctypes.c_void_p), ("clip_seg", ctypes.c_void_p), ("n_clips", ctypes.c_uint64),
                ("n_segments", ctypes.c_uint64), ("n_frames", ctypes.c_uint64), ("n_mel", ctypes.c_uint64)]


class _Ragged(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("n_parts", ctypes.c_uint64), ("n_ids", ctypes.c_uint64)]


def build(force=False):
    """Compile libtekken_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _HERE, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", _HERE, "libtekken_hip.so"])
    return LIB_PATH


def lib():
    """The C-ABI library.  Raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libtekken_hip.so is missing: run `make -C tekken-rs_amd` (or __graft_entry__.build())")
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.
    # If torch is going to live in this process it must be loaded FIRST so that our DT_NEEDED
    # libamdhip64.so.7 resolves to the copy torch already mapped (two runtimes cannot both open the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    L.tk_ctx_create.restype = ctypes.c_int
    L.tk_ctx_create.argtypes = [u8p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                ctypes.c_int, ctypes.POINTER(vp)]
    L.tk_ctx_destroy.argtypes = [vp]
    L.tk_last_error.restype = ctypes.c_char_p
    L.tk_last_error.argtypes = [vp]
    L.tk_encode_batch.restype = ctypes.c_int
    L.tk_encode_batch.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(_Result)]
    L.tk_free_result.argtypes = [ctypes.POINTER(_Result)]
    L.tk_encode_one.restype = ctypes.c_int
    L.tk_encode_one.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u32p, ctypes.c_uint64, u64p]
    L.tk_small_path_calls.restype = ctypes.c_uint64
    L.tk_small_path_calls.argtypes = [vp]
    L.tk_round_path_docs.restype = ctypes.c_uint64
    L.tk_round_path_docs.argtypes = [vp]
    L.tk_long_piece_records.restype = ctypes.c_uint64
    L.tk_long_piece_records.argtypes = [vp]
    if hasattr(L, "tk_ctx_set_memo"):   # (memo of merged pieces: libraries built before it have neither)
        L.tk_ctx_set_memo.restype = ctypes.c_int
        L.tk_ctx_set_memo.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.tk_ctx_memo_clear.restype = ctypes.c_int
        L.tk_ctx_memo_clear.argtypes = [vp]
        L.tk_memo_stats.restype = ctypes.c_int
        L.tk_memo_stats.argtypes = [vp, u64p, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "tk_last_host_syncs"):
        L.tk_last_host_syncs.restype = ctypes.c_uint64
        L.tk_last_host_syncs.argtypes = [vp]
    if hasattr(L, "tk_cut_chunks"):   # (diagnostics only; tools/ab_bench.sh also loads libraries built before it existed)
        L.tk_cut_chunks.restype = ctypes.c_uint64
        L.tk_cut_chunks.argtypes = [vp]
    L.tk_encode_batch_device.restype = ctypes.c_int
    L.tk_encode_batch_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, vp,
                                         ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64)]
    L.tk_encode_batch_device_ex.restype = ctypes.c_int
    L.tk_encode_batch_device_ex.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                            ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64)]
    L.tk_host_alloc.restype = ctypes.c_void_p
    L.tk_host_alloc.argtypes = [ctypes.c_size_t]
    L.tk_host_free.argtypes = [ctypes.c_void_p]
    L.tk_encode_batch_pipelined.restype = ctypes.c_int
    L.tk_encode_batch_pipelined.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, u32p,
                                            ctypes.c_uint64, u64p, u64p]
    L.tk_ids18_bytes.restype = ctypes.c_uint64
    L.tk_ids18_bytes.argtypes = [ctypes.c_uint64]
    L.tk_pack_ids18_device.restype = ctypes.c_int
    L.tk_pack_ids18_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp]
    L.tk_unpack_ids18_device.restype = ctypes.c_int
    L.tk_unpack_ids18_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp]
    L.tk_ctx_set_pattern.restype = ctypes.c_int
    L.tk_ctx_set_pattern.argtypes = [vp, ctypes.c_int]
    L.tk_tokenizer_set_honour_pattern.restype = ctypes.c_int
    L.tk_tokenizer_set_honour_pattern.argtypes = [vp, ctypes.c_int]
    L.tk_ctx_set_special_tokens.restype = ctypes.c_int
    L.tk_ctx_set_special_tokens.argtypes = [vp, u8p, u32p, ctypes.c_uint32]
    L.tk_decode_batch.restype = ctypes.c_int
    L.tk_decode_batch.argtypes = [vp, u32p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(_TextResult), u64p]
    L.tk_free_text_result.argtypes = [ctypes.POINTER(_TextResult)]
    L.tk_decode_batch_device.restype = ctypes.c_int
    L.tk_decode_batch_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, vp, ctypes.POINTER(vp),
                                         ctypes.POINTER(vp), u64p, u64p]
    if hasattr(L, "tk_decode_batch_lossy"):   # lossy decode and the stream step (a library built before them lacks all six)
        L.tk_decode_batch_lossy.restype = ctypes.c_int
        L.tk_decode_batch_lossy.argtypes = [vp, u32p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(_TextResult), u64p, u64p, u64p]
        L.tk_decode_batch_device_lossy.restype = ctypes.c_int
        L.tk_decode_batch_device_lossy.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, vp, ctypes.POINTER(vp),
                                                   ctypes.POINTER(vp), u64p, u64p, u64p, u64p]
        L.tk_decode_stream_step_device.restype = ctypes.c_int
        L.tk_decode_stream_step_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, vp,
                                                   ctypes.POINTER(vp), ctypes.POINTER(vp), u64p, u64p]
        L.tk_decode_stream_step.restype = ctypes.c_int
        L.tk_decode_stream_step.argtypes = [vp, u32p, u32p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_TextResult), u64p]
        L.tk_last_decode_lossy_ms.restype = None
        L.tk_last_decode_lossy_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.tk_last_decode_lossy_stats.restype = None
        L.tk_last_decode_lossy_stats.argtypes = [vp, u64p, u64p, u64p]
    L.tk_tokenizer_decode_batch.restype = ctypes.c_int
    L.tk_tokenizer_decode_batch.argtypes = [vp, u32p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(_TextResult), u64p]
    L.tk_last_timing.restype = ctypes.c_int
    if hasattr(L, "tk_last_merge_ms"):   # (like tk_cut_chunks: a diagnostic that older builds of the library lack)
        L.tk_last_merge_ms.restype = ctypes.c_float
        L.tk_last_merge_ms.argtypes = [vp]
    L.tk_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.tk_last_stats.restype = ctypes.c_int
    L.tk_last_stats.argtypes = [vp, u64p, u64p]
    L.tk_split_batch.restype = ctypes.c_int
    L.tk_split_batch.argtypes = [vp, u8p, u64p, ctypes.c_uint64, u8p]
    L.tk_tokenizer_from_file.restype = ctypes.c_int
    L.tk_tokenizer_from_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(vp)]
    L.tk_tokenizer_from_json.restype = ctypes.c_int
    L.tk_tokenizer_from_json.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
    L.tk_tokenizer_destroy.argtypes = [vp]
    L.tk_tokenizer_last_error.restype = ctypes.c_char_p
    L.tk_tokenizer_last_error.argtypes = [vp]
    L.tk_tokenizer_encode.restype = ctypes.c_int
    L.tk_tokenizer_encode.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(u32p), ctypes.POINTER(ctypes.c_size_t)]
    L.tk_tokenizer_encode_batch.restype = ctypes.c_int
    L.tk_tokenizer_encode_batch.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(_Result)]
    L.tk_free_ids.argtypes = [u32p]
    L.tk_tokenizer_decode.restype = ctypes.c_int
    L.tk_tokenizer_decode.argtypes = [vp, u32p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_size_t)]
    L.tk_free_text.argtypes = [ctypes.c_void_p]
    u64pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64))
    L.tk_free_offsets.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.tk_free_offsets.restype = None
    L.tk_tokenizer_decode_all.restype = ctypes.c_int
    L.tk_tokenizer_decode_all.argtypes = [vp, u32p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), u64pp,
                                          ctypes.POINTER(ctypes.c_size_t)]
    L.tk_tokenizer_vocab.restype = ctypes.c_int
    L.tk_tokenizer_vocab.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), u64pp, ctypes.POINTER(ctypes.c_size_t)]
    L.tk_tokenizer_vocab_size.restype = ctypes.c_uint32
    L.tk_tokenizer_vocab_size.argtypes = [vp]
    L.tk_tokenizer_num_special_tokens.restype = ctypes.c_uint32
    L.tk_tokenizer_num_special_tokens.argtypes = [vp]
    L.tk_tokenizer_version.restype = ctypes.c_char_p
    L.tk_tokenizer_version.argtypes = [vp]
    L.tk_tokenizer_control_token.restype = ctypes.c_int
    L.tk_tokenizer_control_token.argtypes = [vp, ctypes.c_char_p, u32p]
    L.tk_tokenizer_is_special.restype = ctypes.c_int
    L.tk_tokenizer_is_special.argtypes = [vp, ctypes.c_uint32]
    L.tk_tokenizer_is_byte.restype = ctypes.c_int
    L.tk_tokenizer_is_byte.argtypes = [vp, ctypes.c_uint32]
    L.tk_tokenizer_id_to_piece.restype = ctypes.c_int
    L.tk_tokenizer_id_to_piece.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.POINTER(ctypes.c_size_t)]
    L.tk_tokenizer_id_to_byte_piece.restype = ctypes.c_int
    L.tk_tokenizer_id_to_byte_piece.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                ctypes.POINTER(ctypes.c_size_t)]
    L.tk_tokenizer_ctx.restype = vp
    L.tk_tokenizer_ctx.argtypes = [vp]
    L.tk_node_create.restype = ctypes.c_int
    L.tk_node_create.argtypes = [u8p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(vp)]
    L.tk_node_destroy.argtypes = [vp]
    L.tk_node_last_error.restype = ctypes.c_char_p
    L.tk_node_last_error.argtypes = [vp]
    L.tk_node_encode_batch.restype = ctypes.c_int
    L.tk_node_encode_batch.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_Result)]
    L.tk_node_encode_batch_pinned.restype = ctypes.c_int
    L.tk_node_encode_batch_pinned.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u32p, ctypes.c_uint64, u64p, u64p]
    L.tk_node_n_devices.restype = ctypes.c_int
    L.tk_node_n_devices.argtypes = [vp]
    L.tk_node_last_shards.restype = ctypes.c_int
    L.tk_node_last_shards.argtypes = [vp, u64p, u64p, ctypes.c_int]
    L.tk_node_last_timing.restype = ctypes.c_int
    L.tk_node_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.tk_tokenizer_json_pattern.restype = ctypes.c_char_p
    L.tk_tokenizer_json_pattern.argtypes = [vp]
    L.tk_tokenizer_from_cache.restype = ctypes.c_int
    L.tk_tokenizer_from_cache.argtypes = [vp]
    if hasattr(L, "tk_token_spans_device"):   # (per-token byte spans: libraries built before them still load through TK_HIP_LIB)
        L.tk_token_spans_device.restype = ctypes.c_int
        L.tk_token_spans_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp, vp, ctypes.c_int, vp, ctypes.POINTER(vp), u64p]
        L.tk_encode_batch_device_spans.restype = ctypes.c_int
        L.tk_encode_batch_device_spans.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), u64p, u64p]
        L.tk_encode_batch_spans.restype = ctypes.c_int
        L.tk_encode_batch_spans.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(_Result), ctypes.POINTER(u32p), u64p]
        L.tk_free_spans.restype = None
        L.tk_free_spans.argtypes = [u32p]
        L.tk_tokenizer_encode_with_spans.restype = ctypes.c_int
        L.tk_tokenizer_encode_with_spans.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u32p),
                                                     ctypes.POINTER(u32p), ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(L, "tk_token_spans_units_device"):   # (spans in code points / UTF-16 units, annotation -> token range)
        L.tk_token_spans_units_device.restype = ctypes.c_int
        L.tk_token_spans_units_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, vp, ctypes.POINTER(vp)]
        L.tk_encode_batch_device_spans_units.restype = ctypes.c_int
        L.tk_encode_batch_device_spans_units.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), u64p]
        L.tk_encode_batch_spans_units.restype = ctypes.c_int
        L.tk_encode_batch_spans_units.argtypes = [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.POINTER(_Result), ctypes.POINTER(u32p)]
        L.tk_spans_locate_device.restype = ctypes.c_int
        L.tk_spans_locate_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp, ctypes.POINTER(vp), u64p]
    # the layout passes whose three entries take the same arguments (extra: the second input stream of the pass over ids).  A
    # library built before a pass still loads through TK_HIP_LIB
    u64, ci, vpp = ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(vp)
    for R, opts, extra in ((DenseResult, _DenseOpts, []), (SeqpackResult, _SeqpackOpts, []), (WindowResult, _WindowOpts, [vp]),
                           (RowfitResult, _RowfitOpts, [vp]), (RegroupResult, _RegroupOpts, [vp, vp]), (ChunkResult, _ChunkOpts, [vp, vp])):
        if not hasattr(L, "tk_%s_from_ids_device" % R.PASS):
            continue
        op, rp = ctypes.POINTER(opts), ctypes.POINTER(R.STRUCT)
        for name, args in (("tk_%s_from_ids_device", [vp, vp, vp, u64, u64] + extra + [op, vp, rp]),
                           ("tk_encode_batch_device_%s", [vp, vp, vp, u64, u64, ci, ci, ci, op, vp, vpp, vpp, u64p, rp]),
                           ("tk_encode_batch_%s", [vp, u8p, u64p, u64, ci, ci, ci, op, rp]), ("tk_free_%s", [rp])):
            fn = getattr(L, name % R.PASS)
            fn.restype, fn.argtypes = (None if name == "tk_free_%s" else ci), args
    if hasattr(L, "tk_chunk_levels_device"):   # (boundary-aware chunks: libraries built before them still load through TK_HIP_LIB)
        L.tk_chunk_levels_device.restype = ci
        L.tk_chunk_levels_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64, ctypes.c_uint32, vp, vpp]
        L.tk_last_chunk_ms.restype = None
        L.tk_last_chunk_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 3)]
    if hasattr(L, "tk_pair_from_ids_device"):   # (sentence-pair rows: libraries built before them still load through TK_HIP_LIB)
        pop, pp = ctypes.POINTER(_PairOpts), ctypes.POINTER(_Pair)
        L.tk_pair_from_ids_device.restype = ci
        L.tk_pair_from_ids_device.argtypes = [vp, vp, vp, u64, u64, vp, pop, vp, pp]
        L.tk_encode_pairs_device.restype = ci
        L.tk_encode_pairs_device.argtypes = [vp, vp, vp, u64, u64, ci, pop, vp, vpp, vpp, u64p, pp]
        L.tk_encode_pairs.restype = ci
        L.tk_encode_pairs.argtypes = [vp, u8p, u64p, u64, ci, pop, pp]
        L.tk_free_pair.restype = None
        L.tk_free_pair.argtypes = [pp]
    jop, jp = ctypes.POINTER(_JoinOpts), ctypes.POINTER(_Join)
    if hasattr(L, "tk_ragged_from_dense_device"):
        L.tk_ragged_from_dense_device.restype = ci
        L.tk_ragged_from_dense_device.argtypes = [vp, vp, u64, u64, ci, vp, ctypes.c_uint32, vp, vpp, vpp, u64p]
    if hasattr(L, "tk_join_from_ids_device"):   # (chat batches: libraries built before them still load through TK_HIP_LIB)
        L.tk_join_from_ids_device.restype = ci
        L.tk_join_from_ids_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, ci, jop, vp, jp]
        L.tk_encode_parts_device_join.restype = ci
        L.tk_encode_parts_device_join.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, ci, jop, vp, jp]
        L.tk_encode_parts_join.restype = ci
        L.tk_encode_parts_join.argtypes = [vp, u8p, u64p, u64, u32p, u32p, u64p, u64, ci, jop, jp]
        L.tk_free_join.restype = None
        L.tk_free_join.argtypes = [jp]
    if hasattr(L, "tk_encode_parts_device_rowfit"):
        L.tk_encode_parts_device_rowfit.restype = ci
        L.tk_encode_parts_device_rowfit.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, ci, jop, ctypes.POINTER(_RowfitOpts), vp, jp,
                                                    ctypes.POINTER(_Rowfit)]
        L.tk_last_rowfit_ms.restype = None
        L.tk_last_rowfit_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    if hasattr(L, "tk_last_regroup_ms"):
        L.tk_last_regroup_ms.restype = None
        L.tk_last_regroup_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 4)]
    if hasattr(L, "tk_words_from_ids_device"):   # (word ids: libraries built before them still load through TK_HIP_LIB)
        wop, wp = ctypes.POINTER(_WordsOpts), ctypes.POINTER(_Words)
        L.tk_words_from_ids_device.restype = ci
        L.tk_words_from_ids_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64, ci, wop, vp, wp, u64p]
        L.tk_encode_batch_device_words.restype = ci
        L.tk_encode_batch_device_words.argtypes = [vp, vp, vp, u64, u64, ci, ci, ci, wop, vp, vpp, vpp, u64p, wp, u64p]
        L.tk_encode_batch_words.restype = ci
        L.tk_encode_batch_words.argtypes = [vp, u8p, u64p, u64, ci, ci, ci, ci, wop, ctypes.POINTER(_Result), wp, u64p]
        L.tk_free_words.restype = None
        L.tk_free_words.argtypes = [wp]
        L.tk_last_words_ms.restype = None
        L.tk_last_words_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 4)]
    if hasattr(L, "tk_specials_split_device"):   # (special strings parsed out of text: libraries built before it still load through TK_HIP_LIB)
        sop, sp = ctypes.POINTER(_SpecialsOpts), ctypes.POINTER(_Specials)
        L.tk_specials_split_device.restype = ci
        L.tk_specials_split_device.argtypes = [vp, vp, vp, u64, u64, ci, sop, vp, sp, u64p]
        L.tk_encode_batch_device_parsed.restype = ci
        L.tk_encode_batch_device_parsed.argtypes = [vp, vp, vp, u64, u64, ci, sop, jop, vp, sp, jp, u64p]
        L.tk_encode_batch_parsed.restype = ci
        L.tk_encode_batch_parsed.argtypes = [vp, u8p, u64p, u64, ci, sop, jop, sp, jp, u64p]
        L.tk_free_specials.restype = None
        L.tk_free_specials.argtypes = [sp]
        L.tk_last_specials_ms.restype = None
        L.tk_last_specials_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 4)]
        L.tk_specials_tile.restype = ctypes.c_uint32
        L.tk_specials_tile.argtypes = []
        L.tk_tokenizer_encode_parsed.restype = ci
        L.tk_tokenizer_encode_parsed.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ci, ci, u8p, ctypes.c_uint32, ctypes.POINTER(u32p),
                                                 ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(L, "tk_fim_split_device"):   # (fill-in-the-middle rows: libraries built before them still load through TK_HIP_LIB)
        fop, fp = ctypes.POINTER(_FimOpts), ctypes.POINTER(_Fim)
        L.tk_fim_split_device.restype = ci
        L.tk_fim_split_device.argtypes = [vp, vp, vp, u64, u64, vp, ci, fop, vp, fp]
        L.tk_fim_split_ids_device.restype = ci
        L.tk_fim_split_ids_device.argtypes = [vp, vp, vp, u64, u64, vp, fop, vp, fp]
        L.tk_encode_batch_device_fim.restype = ci
        L.tk_encode_batch_device_fim.argtypes = [vp, vp, vp, u64, u64, vp, ci, fop, jop, vp, fp, jp]
        L.tk_fim_from_ids_device.restype = ci
        L.tk_fim_from_ids_device.argtypes = [vp, vp, vp, u64, u64, vp, fop, jop, vp, fp, jp]
        L.tk_encode_batch_fim.restype = ci
        L.tk_encode_batch_fim.argtypes = [vp, u8p, u64p, u64, u64p, ci, fop, jop, fp, jp]
        L.tk_free_fim.restype = None
        L.tk_free_fim.argtypes = [fp]
        L.tk_last_fim_ms.restype = None
        L.tk_last_fim_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 2)]
        L.tk_fim_tile.restype = ctypes.c_uint32
        L.tk_fim_tile.argtypes = [ci]
    L.tk_tokenizer_rank_table.restype = ctypes.c_int
    L.tk_tokenizer_rank_table.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(u32p), u32p]
    _LIB = L
    if hasattr(L, "tk_audio_logmel_device"):   # (audio: libraries built before it still load through TK_HIP_LIB)
        acp, lop, lmp, rgp = ctypes.POINTER(_AudioConfig), ctypes.POINTER(_LogmelOpts), ctypes.POINTER(_Logmel), ctypes.POINTER(_Ragged)
        L.tk_audio_layout.restype = ci
        L.tk_audio_layout.argtypes = [acp, u64p, u64, u64p, u64p, u64p, u64p]
        L.tk_audio_set_config.restype = ci
        L.tk_audio_set_config.argtypes = [vp, acp]
        L.tk_audio_logmel_device.restype = ci
        L.tk_audio_logmel_device.argtypes = [vp, vp, vp, u64, u64, ci, lop, vp, lmp]
        L.tk_audio_logmel.restype = ci
        L.tk_audio_logmel.argtypes = [vp, ctypes.POINTER(ctypes.c_float), u64p, u64, lop, lmp]
        L.tk_free_logmel.restype = None
        L.tk_free_logmel.argtypes = [lmp]
        L.tk_audio_frame_tile.restype = ctypes.c_uint32
        L.tk_audio_frame_tile.argtypes = []
        L.tk_last_logmel_ms.restype = None
        L.tk_last_logmel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 2)]
        L.tk_audio_splice_device.restype = ci
        L.tk_audio_splice_device.argtypes = [vp, vp, vp, u64, u64, vp, ctypes.c_uint32, vp, rgp]
        L.tk_audio_splice_calls.restype = u64
        L.tk_audio_splice_calls.argtypes = [vp]
        L.tk_tokenizer_has_audio.restype = ci
        L.tk_tokenizer_has_audio.argtypes = [vp]
        L.tk_tokenizer_audio_config.restype = ci
        L.tk_tokenizer_audio_config.argtypes = [vp, acp]
        L.tk_tokenizer_audio_ids.restype = ci
        L.tk_tokenizer_audio_ids.argtypes = [vp, u32p, u32p]
        L.tk_tokenizer_encode_audio.restype = ci
        L.tk_tokenizer_encode_audio.argtypes = [vp, u64, u64, ctypes.POINTER(u32p), ctypes.POINTER(ctypes.c_size_t), u64p]
    if hasattr(L, "tk_noise_replace_device"):   # (masked-LM and span-corruption rows: libraries built before them still load through TK_HIP_LIB)
        nop = ctypes.POINTER(_NoiseOpts)
        for mode, st in (("replace", _NoiseReplace), ("spans", _NoiseSpans)):
            np_ = ctypes.POINTER(st)
            fn = getattr(L, "tk_noise_%s_device" % mode)
            fn.restype = ci
            fn.argtypes = [vp, vp, vp, u64, u64, vp, vp, nop, vp, np_]
            fn = getattr(L, "tk_encode_batch_device_noise_" + mode)
            fn.restype = ci
            fn.argtypes = [vp, vp, vp, u64, u64, ci, ci, ci, nop, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), u64p, np_]
            fn = getattr(L, "tk_encode_batch_noise_" + mode)
            fn.restype = ci
            fn.argtypes = [vp, u8p, u64p, u64, ci, ci, ci, nop, ctypes.POINTER(_Result), np_]
            fn = getattr(L, "tk_free_noise_" + mode)
            fn.restype = None
            fn.argtypes = [np_]
        L.tk_last_noise_ms.restype = None
        L.tk_last_noise_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 3)]
        L.tk_noise_tile.restype = ctypes.c_uint32
        L.tk_noise_tile.argtypes = []
    return L


def _p(arr, ct):
    return arr.ctypes.data_as(ctypes.POINTER(ct))


def pack_docs(docs):
    """list[bytes] -> (uint8[n_bytes], uint64[D+1]) packed byte buffer + doc-offset array."""
    offs = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    joined = b"".join(docs)
    data = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(0, np.uint8)
    return data, offs


def _need(name):
    """The bound C symbol `name`; a library built before it existed raises instead of failing on a missing attribute."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise TokenizerError(TK_ERR_RUNTIME, "%s: the loaded library (%s) predates this entry" % (name, LIB_PATH))
    return fn


def _take(ptr, n, dtype):
    """A numpy copy of the n elements of dtype at the host address ptr."""
    if n == 0:
        return np.zeros(0, dtype)
    raw = (ctypes.c_uint8 * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(raw, dtype=dtype, count=n).copy()


def _torch_wrap(view, copy):
    """A DeviceView as a torch tensor on the GPU (copy: a clone of it); an unselected output (None) stays None."""
    import torch
    if view is None:
        return None
    cai = view.__cuda_array_interface__
    if 0 in cai["shape"]:     # (nothing behind the pointer to look at)
        return torch.empty(cai["shape"], dtype={"<i4": torch.int32, "<i8": torch.int64, "|u1": torch.uint8, "<f4": torch.float32}[cai["typestr"]], device="cuda")
    t = torch.as_tensor(view, device="cuda")
    return t.clone() if copy else t


def _upload(data, offs):
    """The packed text and its offsets go up once: (uint8 tensor, int64 tensor) on the GPU and the current stream."""
    import torch
    return (torch.from_numpy(data if len(data) else np.zeros(1, np.uint8)).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
            torch.cuda.current_stream().cuda_stream)


def _take_result(res):
    n, D = int(res.n_ids), int(res.n_docs)
    ids = np.ctypeslib.as_array(res.ids, shape=(max(n, 1),))[:n].copy()
    offs = np.ctypeslib.as_array(res.offsets, shape=(D + 1,)).copy()
    lib().tk_free_result(ctypes.byref(res))
    return ids, offs


class DecodeStream:
    """Streaming decode for generation (tk_decode_stream_step_device): n_seqs running sequences, one uint32 state word each in a
    device buffer (.state: a torch int32 tensor; bytes 0..2 up to three pending bytes, byte 3 their count).  A step takes the new
    ids of every sequence (a sequence may have none) and returns only complete characters: the open tail of a character waits in
    the state for the next step, invalid bytes become U+FFFD as in decode_batch(errors="replace").  One lane walks one sequence:
    prefill-sized input belongs in decode_batch."""

    def __init__(self, engine, n_seqs, policy=SpecialTokenPolicy.Ignore, text=False):
        import torch
        self._eng, self.n_seqs, self.policy, self._text = engine, int(n_seqs), policy, text
        self.state = torch.zeros(max(self.n_seqs, 1), dtype=torch.int32, device="cuda")[:self.n_seqs]

    def step_device(self, ids_ptr, offs_ptr, n_ids, flags=0, stream=None):
        """The new ids (uint32) and their offsets (uint64[n_seqs + 1]) in HBM -> (bytes view, offsets view), context-owned."""
        import torch
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return self._eng.decode_stream_step_device(self.state.data_ptr() if self.n_seqs else 0, ids_ptr, offs_ptr, self.n_seqs, n_ids,
                                                   self.policy, flags, st)

    def step(self, id_lists, flags=0):
        """The new ids of every sequence (n_seqs lists) -> list of bytes (str with text=True)."""
        import torch
        if len(id_lists) != self.n_seqs:
            raise TokenizerError(TK_ERR_INVALID_ARG, "DecodeStream.step: one id list per sequence (%d)" % self.n_seqs)
        offs = np.zeros(self.n_seqs + 1, np.int64)
        if id_lists:
            offs[1:] = np.cumsum([len(x) for x in id_lists])
        flat = [i for x in id_lists for i in x]
        n_ids = len(flat)
        d_ids = torch.from_numpy(np.array(flat or [0], dtype=np.uint32).view(np.int32)).cuda()
        d_offs = torch.from_numpy(offs).cuda()
        v_b, v_o = self.step_device(d_ids.data_ptr(), d_offs.data_ptr(), n_ids, flags)
        oo = torch.as_tensor(v_o, device="cuda").cpu().numpy()
        raw = torch.as_tensor(v_b, device="cuda").cpu().numpy().tobytes() if int(oo[-1]) else b""
        out = [raw[int(oo[d]):int(oo[d + 1])] for d in range(self.n_seqs)]
        return [b.decode("utf-8", "replace") for b in out] if self._text else out

    def finish(self):
        """Flushes every open prefix as U+FFFD (TK_STREAM_FINAL) and leaves the states 0."""
        return self.step([[] for _ in range(self.n_seqs)], STREAM_FINAL)

    def reset(self, rows=None):
        """Zeroes the state of the given slots (None: all): a slot reused in continuous batching starts fresh."""
        if rows is None:
            self.state.zero_()
        elif len(rows):
            import torch
            self.state[torch.as_tensor(list(rows), dtype=torch.long, device="cuda")] = 0


class DeviceView:
    """Zero-copy view of a context-owned device buffer for array libraries that understand
    `__cuda_array_interface__` (e.g. `torch.as_tensor(view, device="cuda")`).  Valid until the next
    call on the owning context.  n: the number of elements, or a shape (C-contiguous; the dense entries' [D, L])."""

    def __init__(self, ptr, n, typestr):
        shape = tuple(int(x) for x in n) if isinstance(n, (tuple, list)) else (int(n),)
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def _dense_opts(max_length=0, multiple_of=0, pad_id=0, keep_head=0, keep_tail=0, flags=0):
    return _DenseOpts(int(max_length or 0), int(multiple_of or 0), int(pad_id), int(keep_head), int(keep_tail), int(flags))


class _LayoutResult:
    """What the six layout results share.  A result class declares its outputs ONCE, in the order of the C struct's pointer
    fields (tests/test_layout_binding_cpu.py holds them against include/tekken_hip.h), and everything that walks them is here:
    the *_ptr attributes, views(), tensors() and the host copy.
    OUTPUTS: (name, typestr of views() -- None: the tensors' dtype, self.typestr --, shape(self), numpy dtype of the host entry's
    array -- None: the tensors' dtype --, optional: an unselected one is None) per output; COUNTS: the uint64 members of the
    struct, attributes of the same name; DICT_COUNTS: the ones the dicts of the host entries and tensors() carry; STRUCT / PASS /
    I64: the ctypes struct, the name in the C entries, the flag that widens the tensors (None: no tensor of the pass has a dtype
    to choose, and no typestr attribute)."""
    OUTPUTS, COUNTS, DICT_COUNTS, STRUCT, PASS, I64 = (), (), (), None, "", None

    def __init__(self, st, flags=0, n_docs=None):
        """n_docs: only for the result whose struct does not carry it (RowfitResult)."""
        for name, _, _, _, optional in self.OUTPUTS:
            setattr(self, name + "_ptr", getattr(st, name) or (None if optional else 0))
        for k in self.COUNTS:
            setattr(self, k, int(getattr(st, k)))
        if self.I64 is not None:
            self.typestr = "<i8" if flags & self.I64 else "<i4"

    def _ptrs(self):
        return [getattr(self, o[0] + "_ptr") for o in self.OUTPUTS]

    def views(self):
        """One DeviceView per output, in the order of OUTPUTS (an unselected one: None)."""
        return tuple(None if p is None else DeviceView(p, shape(self), ts or self.typestr)
                     for p, (_, ts, shape, _, _) in zip(self._ptrs(), self.OUTPUTS))

    def _counts(self):
        return {k: getattr(self, k) for k in self.DICT_COUNTS}

    def tensors(self, copy=True):
        """The views as torch tensors on the GPU (copy: clones of them) by output name, and the counts, as the Tekkenizer methods
        return them."""
        out = {o[0]: _torch_wrap(v, copy) for o, v in zip(self.OUTPUTS, self.views())}
        out.update(self._counts())
        return out

    @classmethod
    def take(cls, st, flags=0, n_docs=None):
        """The result of a host entry (pinned host blocks) as numpy copies by output name, and the counts; st is freed."""
        r = cls(st, flags, n_docs)
        out = {}
        for p, (name, _, shape, hdt, _) in zip(r._ptrs(), cls.OUTPUTS):
            out[name] = None if p is None else _take(p, int(np.prod(shape(r))), hdt or (np.int64 if r.typestr == "<i8" else np.int32)).reshape(shape(r))
        out.update(r._counts())
        getattr(lib(), "tk_free_" + cls.PASS)(ctypes.byref(st))
        return r, out


def _rows(r):
    return (r.n_rows, r.row_len)


class DenseResult(_LayoutResult):
    """What the device dense entries return (tk_dense): raw device pointers of context-owned buffers, valid until the next dense
    call on the context.  ids_ptr: int32 or int64 [n_docs, row_len]; mask_ptr: uint8 [n_docs, row_len] or None;
    lengths_ptr: uint32 [n_docs] (views() shows it as int32: a length is at most row_len < 2^31).
    views(): (ids view [n_docs, row_len], mask view or None, lengths view as int32 [n_docs])."""
    STRUCT, PASS, I64 = _Dense, "dense", DENSE_I64
    OUTPUTS = (("ids", None, lambda r: (r.n_docs, r.row_len), None, False),
               ("mask", "|u1", lambda r: (r.n_docs, r.row_len), np.uint8, True),
               ("lengths", "<i4", lambda r: (r.n_docs,), np.uint32, False))
    COUNTS = ("n_docs", "row_len", "n_truncated")
    DICT_COUNTS = ("n_truncated",)


class SeqpackResult(_LayoutResult):
    """What the device packed entries return (tk_seqpack): raw device pointers of context-owned buffers, valid until the next
    packed call on the context.  input_ids_ptr / position_ids_ptr / segment_ids_ptr: int32 or int64 [n_rows, row_len] (an
    unselected one: None); cu_seqlens_ptr: int32 [n_segments + 1] or None.
    views(): (input_ids, position_ids or None, segment_ids or None -- views [n_rows, row_len] --, cu_seqlens view
    [n_segments + 1] or None)."""
    STRUCT, PASS, I64 = _Seqpack, "seqpack", SEQPACK_I64
    OUTPUTS = (("input_ids", None, _rows, None, False), ("position_ids", None, _rows, None, True), ("segment_ids", None, _rows, None, True),
               ("cu_seqlens", "<i4", lambda r: (r.n_segments + 1,), np.int32, True))
    COUNTS = ("n_rows", "row_len", "n_used", "n_left", "n_segments", "max_seqlen")
    DICT_COUNTS = ("max_seqlen", "n_rows", "n_used", "n_left", "n_segments")


def _window_opts(max_length, stride=0, multiple_of=0, pad_id=0, keep_head=0, keep_tail=0, flags=0):
    return _WindowOpts(int(max_length or 0), int(stride or 0), int(multiple_of or 0), int(pad_id), int(keep_head), int(keep_tail), int(flags))


class WindowResult(_LayoutResult):
    """What the device window entries return (tk_window): raw device pointers of context-owned buffers, valid until the next
    window call on the context.  input_ids_ptr: int32 or int64 [n_windows, row_len]; mask_ptr: uint8 [n_windows, row_len] or None;
    lengths_ptr / window_doc_ptr / window_start_ptr: uint32 [n_windows] (views() shows them as int32: each is below 2^31 for every
    batch a tensor can hold); doc_windows_ptr: uint64 [n_docs + 1]; spans_ptr: uint32 [n_windows, row_len, 2] or None.
    views(): (input_ids [n_windows, row_len], mask or None, lengths, window_doc, window_start as int32 [n_windows], doc_windows as
    int64 [n_docs + 1], spans as int32 [n_windows, row_len, 2] or None)."""
    STRUCT, PASS, I64 = _Window, "window", WINDOW_I64
    OUTPUTS = (("input_ids", None, lambda r: (r.n_windows, r.row_len), None, False),
               ("mask", "|u1", lambda r: (r.n_windows, r.row_len), np.uint8, True),
               ("lengths", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("window_doc", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("window_start", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("doc_windows", "<i8", lambda r: (r.n_docs + 1,), np.uint64, False),
               ("spans", "<i4", lambda r: (r.n_windows, r.row_len, 2), np.uint32, True))
    COUNTS = ("n_docs", "n_windows", "row_len", "n_split")
    DICT_COUNTS = ("n_windows", "n_split")


def _chunk_opts(max_length, min_length, overlap=0, multiple_of=0, pad_id=0, keep_head=0, keep_tail=0, levels=CHUNK_LEVELS_ALL, flags=0):
    return _ChunkOpts(int(max_length or 0), int(min_length or 0), int(overlap or 0), int(multiple_of or 0), int(pad_id), int(keep_head),
                      int(keep_tail), int(levels), int(flags))


class ChunkResult(_LayoutResult):
    """What the device chunk entries return (tk_chunk): raw device pointers of context-owned buffers, valid until the next chunk
    call on the context.  The first seven outputs are WindowResult's; cut_level_ptr: uint8 [n_windows] (CHUNK_CUT_LAST for a
    document's last chunk); chunk_bytes_ptr: uint32 [n_windows, 2] or None (with CHUNK_BYTES); level_counts_ptr: uint64 [6], the cuts
    made at every level.
    views(): WindowResult's seven, then cut_level as uint8 [n_windows], chunk_bytes as int32 [n_windows, 2] or None, level_counts as
    int64 [6]."""
    STRUCT, PASS, I64 = _Chunk, "chunk", CHUNK_I64
    OUTPUTS = WindowResult.OUTPUTS + (("cut_level", "|u1", lambda r: (r.n_windows,), np.uint8, False),
                                      ("chunk_bytes", "<i4", lambda r: (r.n_windows, 2), np.uint32, True),
                                      ("level_counts", "<i8", lambda r: (6,), np.uint64, False))
    COUNTS = ("n_docs", "n_windows", "row_len", "n_split")
    DICT_COUNTS = ("n_windows", "n_split")


def _pair_opts(max_length, strategy=PAIR_LONGEST_FIRST, stride=0, max_fixed=0, multiple_of=0, pad_id=0, head=(), sep=(), tail=(), flags=0):
    # (a list of more than 4 ids keeps its count and its first 4 ids: the entry refuses the count)
    lists = [(ctypes.c_uint32 * 4)(*[int(x) for x in list(l)[:4]]) for l in (head, sep, tail)]
    return _PairOpts(int(max_length or 0), int(strategy), int(stride or 0), int(max_fixed or 0), int(multiple_of or 0), int(pad_id),
                     len(head), len(sep), len(tail), lists[0], lists[1], lists[2], int(flags))


def _windows(r):
    return (r.n_windows, r.row_len)


def _window_dict(r, **own):
    """What encode_batch_windows returns, from the engine's numpy result (uint32 / uint64 arrays: shown as int32 / int64) or from
    the tensors of a device result; own: the keys a pass adds in front of the counts (encode_batch_chunks)."""
    as_ = (lambda v, dt: v.astype(dt)) if isinstance(r["lengths"], np.ndarray) else (lambda v, dt: v)
    out = {"input_ids": r["input_ids"], "attention_mask": r["mask"], "lengths": as_(r["lengths"], np.int32),
           "overflow_to_sample_mapping": as_(r["window_doc"], np.int32), "window_start": as_(r["window_start"], np.int32),
           "doc_windows": as_(r["doc_windows"], np.int64),
           "offset_mapping": as_(r["spans"], np.int32) if r["spans"] is not None else None}
    out.update(own)
    out["n_windows"], out["n_split"] = r["n_windows"], r["n_split"]
    return out


class PairResult(_LayoutResult):
    """What the device pair entries return (tk_pair): raw device pointers of context-owned buffers, valid until the next pair call
    on the context.  input_ids_ptr: int32 or int64 [n_windows, row_len]; mask_ptr / type_ids_ptr / sequence_ids_ptr: uint8
    [n_windows, row_len] or None (sequence_ids: PAIR_SEQ_NONE under a fixed id or a pad); lengths_ptr / window_pair_ptr /
    window_start_ptr / second_start_ptr: uint32 [n_windows] (views() shows them as int32: each is below 2^31 for every batch a
    tensor can hold); spans_ptr: uint32 [n_windows, row_len, 2] or None; pair_windows_ptr: uint64 [n_pairs + 1].
    views(): one view per output in this order, an unselected one None."""
    STRUCT, PASS, I64 = _Pair, "pair", PAIR_I64
    OUTPUTS = (("input_ids", None, _windows, None, False), ("mask", "|u1", _windows, np.uint8, True),
               ("type_ids", "|u1", _windows, np.uint8, True), ("sequence_ids", "|u1", _windows, np.uint8, True),
               ("lengths", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("window_pair", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("window_start", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("second_start", "<i4", lambda r: (r.n_windows,), np.uint32, False),
               ("spans", "<i4", lambda r: (r.n_windows, r.row_len, 2), np.uint32, True),
               ("pair_windows", "<i8", lambda r: (r.n_pairs + 1,), np.uint64, False))
    COUNTS = ("n_pairs", "n_windows", "row_len", "n_truncated", "n_split", "n_fixed_cut")
    DICT_COUNTS = ("n_windows", "n_truncated", "n_split", "n_fixed_cut")


class JoinResult(_LayoutResult):
    """What the device join entries return (tk_join): raw device pointers of context-owned buffers, valid until the next join call
    on the context.  ids_ptr: uint32 [n_ids]; offsets_ptr: uint64 [n_convs + 1]; labels_ptr: int32 [n_ids] or None;
    part_index_ptr: uint32 [n_ids] or None.
    views(): (ids as int32 [n_ids], offsets as int64 [n_convs + 1], labels int32 [n_ids] or None, part_index as int32 [n_ids] or
    None)."""
    STRUCT, PASS = _Join, "join"
    OUTPUTS = (("ids", "<i4", lambda r: (r.n_ids,), np.uint32, False), ("offsets", "<i8", lambda r: (r.n_convs + 1,), np.uint64, False),
               ("labels", "<i4", lambda r: (r.n_ids,), np.int32, True), ("part_index", "<i4", lambda r: (r.n_ids,), np.uint32, True))
    COUNTS = ("n_convs", "n_parts", "n_ids", "n_ctrl", "n_labelled")
    DICT_COUNTS = ("n_ids", "n_ctrl", "n_labelled")


class RowfitResult(_LayoutResult):
    """What the device rowfit entries return (tk_rowfit): raw device pointers of context-owned buffers, valid until the next
    rowfit call on the context.  input_ids_ptr / position_ids_ptr / segment_ids_ptr: int32 or int64 [n_rows, row_len];
    labels_ptr: int32 [n_rows, row_len]; cu_seqlens_ptr: int32 [n_segments + 1]; doc_start_ptr: uint64 [n_docs] (an unselected
    one: None).  n_docs is the caller's: the struct does not carry it.
    views(): (input_ids, labels (int32) or None, position_ids or None, segment_ids or None -- views [n_rows, row_len] --,
    cu_seqlens view [n_segments + 1] or None, doc_start view as int64 [n_docs] or None)."""
    STRUCT, PASS, I64 = _Rowfit, "rowfit", ROWFIT_I64
    OUTPUTS = (("input_ids", None, _rows, None, False), ("labels", "<i4", _rows, np.int32, True), ("position_ids", None, _rows, None, True),
               ("segment_ids", None, _rows, None, True), ("cu_seqlens", "<i4", lambda r: (r.n_segments + 1,), np.int32, True),
               ("doc_start", "<i8", lambda r: (r.n_docs,), np.uint64, True))
    COUNTS = ("n_rows", "row_len", "n_segments", "max_seqlen", "n_truncated", "n_pad")
    DICT_COUNTS = ("max_seqlen", "n_rows", "n_segments", "n_truncated", "n_pad")

    def __init__(self, st, flags=0, n_docs=0):
        super().__init__(st, flags)
        self.n_docs = int(n_docs)

    def counts(self):
        return self._counts()


def _regroup_opts(order=REGROUP_ORDER_KEEP, min_length=0, max_length=0, seed=0, window=0, max_tokens=0, max_docs=0, flags=0):
    return _RegroupOpts(int(max_tokens or 0), int(min_length or 0), int(max_length or 0), int(order), int(seed), int(window or 0),
                        int(max_docs or 0), int(flags))


class RegroupResult(_LayoutResult):
    """What the device regroup entries return (tk_regroup): raw device pointers of context-owned buffers, valid until the next
    regroup call on the context.  ids_ptr: uint32 [n_ids]; offsets_ptr: uint64 [n_docs + 1] (n_docs: the KEPT documents);
    labels_ptr: int32 [n_ids]; perm_ptr: uint32 [n_docs]; batch_offsets_ptr: uint64 [n_batches + 1]; batch_rowlen_ptr: uint32
    [n_batches] (an unselected one: None).
    views(): (ids as int32 [n_ids], offsets as int64 [n_docs + 1], labels or None, perm as int32 or None, batch_offsets as int64
    or None, batch_rowlen as int32 or None)."""
    STRUCT, PASS = _Regroup, "regroup"
    OUTPUTS = (("ids", "<i4", lambda r: (r.n_ids,), np.uint32, False), ("offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, False),
               ("labels", "<i4", lambda r: (r.n_ids,), np.int32, True), ("perm", "<i4", lambda r: (r.n_docs,), np.uint32, True),
               ("batch_offsets", "<i8", lambda r: (r.n_batches + 1,), np.uint64, True),
               ("batch_rowlen", "<i4", lambda r: (r.n_batches,), np.uint32, True))
    COUNTS = ("n_docs", "n_ids", "n_masked", "n_short", "n_long", "n_batches", "n_oversize", "n_batch_pad")
    DICT_COUNTS = COUNTS

    def batches(self):
        """(first_doc, end_doc, rowlen) of every batch, from one host copy of batch_offsets and batch_rowlen (both selected)."""
        if self.batch_offsets_ptr is None or self.batch_rowlen_ptr is None:
            raise TokenizerError(TK_ERR_INVALID_ARG, "batches(): REGROUP_BATCHES | REGROUP_BATCH_OFFSETS | REGROUP_BATCH_ROWLEN were not selected")
        v = self.views()
        bo, rl = (_torch_wrap(x, False).cpu().tolist() for x in (v[4], v[5]))
        for b in range(self.n_batches):
            yield bo[b], bo[b + 1], rl[b]


class WordsResult(_LayoutResult):
    """What the device words entries return (tk_words): raw device pointers of context-owned buffers, valid until the next words
    call on the context.  word_ids_ptr: uint32 [n_ids] (WORD_NONE for a special id; views() shows it as int32: -1);
    doc_words_ptr: uint64 [n_docs + 1]; word_first_ptr: uint32 [n_words] or None (WORDS_FIRST).
    views(): (word_ids as int32 [n_ids], doc_words as int64 [n_docs + 1], word_first as int32 [n_words] or None)."""
    STRUCT, PASS = _Words, "words"
    OUTPUTS = (("word_ids", "<i4", lambda r: (r.n_ids,), np.uint32, False), ("doc_words", "<i8", lambda r: (r.n_docs + 1,), np.uint64, False),
               ("word_first", "<i4", lambda r: (r.n_words,), np.uint32, True))
    COUNTS = ("n_docs", "n_ids", "n_words")
    DICT_COUNTS = ("n_words",)


def _specials_opts(modes, flags):
    """(tk_specials_opts, the array it points into -- to be kept alive through the call).  modes None: every string is parsed."""
    if modes is None:
        return _SpecialsOpts(None, 0, int(flags)), None
    m = np.ascontiguousarray(modes, dtype=np.uint8)
    buf = m if len(m) else np.zeros(1, np.uint8)
    return _SpecialsOpts(_p(buf, ctypes.c_uint8), len(m), int(flags)), buf


class SpecialsResult(_LayoutResult):
    """What the device specials entries return (tk_specials): raw device pointers of context-owned buffers, valid until the next
    specials call on the context.  bytes_ptr: uint8 [n_bytes], the text without the matched strings (the caller's own buffer where
    n_removed == 0); part_offsets_ptr: uint64 [n_parts + 1]; part_ctrl_ptr: uint32 [n_parts] (JOIN_NONE: views() shows it as
    int32, -1); conv_offsets_ptr: uint64 [n_docs + 1]; part_src_ptr: uint64 [n_parts] or None (SPECIALS_PART_SRC).
    views(): one view per output in this order, the offsets as int64."""
    STRUCT, PASS = _Specials, "specials"
    OUTPUTS = (("bytes", "|u1", lambda r: (r.n_bytes,), np.uint8, False),
               ("part_offsets", "<i8", lambda r: (r.n_parts + 1,), np.uint64, False),
               ("part_ctrl", "<i4", lambda r: (r.n_parts,), np.uint32, False),
               ("conv_offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, False),
               ("part_src", "<i8", lambda r: (r.n_parts,), np.uint64, True))
    COUNTS = ("n_docs", "n_parts", "n_bytes", "n_matches", "n_removed")
    DICT_COUNTS = ("n_parts", "n_bytes", "n_matches", "n_removed")


def fim_q32(rate):
    """A probability as tk_fim_opts carries it: min(2^32, round(rate * 2^32))."""
    if not 0.0 <= float(rate) <= 1.0:
        raise TokenizerError(TK_ERR_INVALID_ARG, "fim: a rate of %r is not in [0, 1]" % (rate,))
    return min(1 << 32, int(round(float(rate) * (1 << 32))))


def _fim_opts(rate_q32=0, spm_q32=0, seed=0, prefix_id=JOIN_NONE, suffix_id=JOIN_NONE, middle_id=JOIN_NONE, head=0, tail=0, min_units=0, flags=0):
    return _FimOpts(int(rate_q32), int(spm_q32), int(seed) & 0xFFFFFFFF, int(prefix_id), int(suffix_id), int(middle_id), int(head), int(tail),
                    int(min_units), int(flags))


class FimResult(_LayoutResult):
    """What the device fill-in-the-middle entries return (tk_fim): raw device pointers of context-owned buffers, valid until the
    next FIM call on the context.  units_ptr: uint8 [n_units] (text entries) or uint32 [n_units] (ids entries; views() shows them
    as int32), each document's units in part order -- the caller's own buffer where nothing could be transformed;
    part_offsets_ptr: uint64 [n_parts + 1]; part_ctrl_ptr / part_flags_ptr: uint32 [n_parts] (JOIN_NONE: -1 in views());
    conv_offsets_ptr: uint64 [n_docs + 1]; part_src_ptr: uint64 [n_parts] or None (FIM_PART_SRC); cuts_ptr: uint64 [n_docs, 2]
    ((lo, hi), FIM_NO_CUT twice for an untransformed document: -1 in views()); mode_ptr: uint8 [n_docs].
    views(): one view per output in this order, the offsets as int64.  unit_bytes: 1 or 4."""
    STRUCT, PASS = _Fim, "fim"
    OUTPUTS = (("units", None, lambda r: (r.n_units,), np.uint8, False),
               ("part_offsets", "<i8", lambda r: (r.n_parts + 1,), np.uint64, False),
               ("part_ctrl", "<i4", lambda r: (r.n_parts,), np.uint32, False),
               ("part_flags", "<i4", lambda r: (r.n_parts,), np.uint32, False),
               ("conv_offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, False),
               ("part_src", "<i8", lambda r: (r.n_parts,), np.uint64, True),
               ("cuts", "<i8", lambda r: (r.n_docs, 2), np.uint64, False),
               ("mode", "|u1", lambda r: (r.n_docs,), np.uint8, False))
    COUNTS = ("n_docs", "n_parts", "n_units", "n_transformed", "n_spm", "n_skipped")
    DICT_COUNTS = ("n_parts", "n_units", "n_transformed", "n_spm", "n_skipped")

    def __init__(self, st, flags=0, n_docs=None, unit_bytes=1):
        super().__init__(st, flags)
        self.unit_bytes = int(unit_bytes)
        self.typestr = "|u1" if self.unit_bytes == 1 else "<i4"   # (of units: the host entry takes text, so its array is uint8)


def noise_start_q32(rate, span_min=1, span_max=1):
    """The start_q32 of tk_noise_opts under which the expected covered fraction of the units is `rate`.  A unit x is left alone iff
    none of the span_max units q = x - j, j = 0 .. span_max - 1, starts a span longer than j; starts are independent with
    probability s and len is uniform over span_min .. span_max, so P(len > j) = 1 for j < span_min, (span_max - j) / (span_max -
    span_min + 1) behind it, and  1 - prod_j (1 - s P(len > j)) = rate  is solved for s by bisection (the left side grows with s)."""
    rate, lo_n, hi_n = float(rate), int(span_min), int(span_max)
    if not 0.0 <= rate <= 1.0 or not 1 <= lo_n <= hi_n <= NOISE_SPAN_LIMIT:
        raise TokenizerError(TK_ERR_INVALID_ARG, "noise: rate %r / span (%r, %r) out of range" % (rate, span_min, span_max))
    longer = [1.0 if j < lo_n else (hi_n - j) / (hi_n - lo_n + 1.0) for j in range(hi_n)]

    def covered(s):
        left = 1.0
        for pj in longer:
            left *= 1.0 - s * pj
        return 1.0 - left

    if rate in (0.0, 1.0):                              # (exactly none, exactly all)
        return int(rate) << 32
    lo, hi = 0.0, 1.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if covered(mid) < rate:
            lo = mid
        else:
            hi = mid
    return min(1 << 32, int(round(hi * (1 << 32))))


def _noise_opts(start_q32=0, mask_q32=0, random_q32=0, seed=0, unit=NOISE_UNIT_TOKEN, span_min=1, span_max=1, mask_id=0, n_sentinels=0,
                sentinel_first=0, final_id=JOIN_NONE, flags=0, ignore_index=-100):
    return _NoiseOpts(int(start_q32), int(mask_q32), int(random_q32), int(seed) & 0xFFFFFFFF, int(unit), int(span_min), int(span_max), int(mask_id),
                      int(n_sentinels), int(sentinel_first), int(final_id), int(flags), int(ignore_index))


class NoiseReplaceResult(_LayoutResult):
    """What the device replace-mode noise entries return (tk_noise_replace): raw device pointers of context-owned buffers, valid
    until the next noise call on the context.  input_ids_ptr: uint32 [n_ids] (views(): int32); labels_ptr: int32 [n_ids];
    selected_ptr: uint8 [n_ids] or None (NOISE_SELECTED).  The offsets are the input's."""
    STRUCT, PASS = _NoiseReplace, "noise_replace"
    OUTPUTS = (("input_ids", "<i4", lambda r: (r.n_ids,), np.uint32, False), ("labels", "<i4", lambda r: (r.n_ids,), np.int32, False),
               ("selected", "|u1", lambda r: (r.n_ids,), np.uint8, True))
    COUNTS = ("n_docs", "n_ids", "n_selected", "n_masked", "n_random")
    DICT_COUNTS = ("n_selected", "n_masked", "n_random")


class NoiseSpansResult(_LayoutResult):
    """What the device spans-mode noise entries return (tk_noise_spans): raw device pointers of context-owned buffers, valid until
    the next noise call on the context.  inputs_ptr / targets_ptr: uint32 [n_inputs] / [n_targets] with input_offsets_ptr /
    target_offsets_ptr: uint64 [n_docs + 1] (NOISE_SPLIT, else None); joined_ptr: uint32 [n_inputs + n_targets], joined_offsets_ptr:
    uint64 [n_docs + 1], joined_labels_ptr: int32 [n_inputs + n_targets] (NOISE_JOINED, else None).  views(): ids as int32,
    offsets as int64."""
    STRUCT, PASS = _NoiseSpans, "noise_spans"
    OUTPUTS = (("inputs", "<i4", lambda r: (r.n_inputs,), np.uint32, True), ("input_offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, True),
               ("targets", "<i4", lambda r: (r.n_targets,), np.uint32, True), ("target_offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, True),
               ("joined", "<i4", lambda r: (r.n_inputs + r.n_targets,), np.uint32, True),
               ("joined_offsets", "<i8", lambda r: (r.n_docs + 1,), np.uint64, True),
               ("joined_labels", "<i4", lambda r: (r.n_inputs + r.n_targets,), np.int32, True))
    COUNTS = ("n_docs", "n_selected", "n_runs", "n_runs_dropped", "n_inputs", "n_targets")
    DICT_COUNTS = ("n_selected", "n_runs", "n_runs_dropped", "n_inputs", "n_targets")


_NOISE = {"replace": (_NoiseReplace, NoiseReplaceResult), "spans": (_NoiseSpans, NoiseSpansResult)}


class LogmelResult(_LayoutResult):
    """What tk_audio_logmel_device returns (tk_logmel): raw device pointers of context-owned buffers, valid until the next log-mel
    call on the context.  features_ptr: float32, segment s is [n_mel, T_s] at element n_mel * frame_off[s]; frame_off_ptr: uint64
    [n_segments + 1]; clip_seg_ptr: uint64 [n_clips + 1].  views(): (features float32 [n_mel * n_frames], frame_off as int64,
    clip_seg as int64)."""
    STRUCT, PASS = _Logmel, "logmel"
    OUTPUTS = (("features", "<f4", lambda r: (r.n_mel * r.n_frames,), np.float32, False),
               ("frame_off", "<i8", lambda r: (r.n_segments + 1,), np.uint64, False),
               ("clip_seg", "<i8", lambda r: (r.n_clips + 1,), np.uint64, False))
    COUNTS = ("n_clips", "n_segments", "n_frames", "n_mel")
    DICT_COUNTS = ("n_clips", "n_segments", "n_frames", "n_mel")


class RaggedResult(_LayoutResult):
    """What tk_audio_splice_device returns (tk_ragged): ids_ptr uint32 [n_ids], offsets_ptr uint64 [n_parts + 1], context-owned, valid
    until the next splice on the context.  views(): (ids as int32, offsets as int64)."""
    STRUCT, PASS = _Ragged, "ragged"
    OUTPUTS = (("ids", "<i4", lambda r: (r.n_ids,), np.uint32, False), ("offsets", "<i8", lambda r: (r.n_parts + 1,), np.uint64, False))
    COUNTS = ("n_parts", "n_ids")
    DICT_COUNTS = ("n_ids",)


class Audio:
    """A clip: .audio_array float32 [n] and .sampling_rate (reference src/audio.rs:212-217)."""

    def __init__(self, samples, sampling_rate):
        self.audio_array = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        self.sampling_rate = int(sampling_rate)

    def __len__(self):
        return len(self.audio_array)

    @classmethod
    def from_wav(cls, path_or_bytes):
        """A PCM WAV file (a path, or its bytes) through the stdlib `wave` module: 8 / 16 / 24 / 32-bit samples scaled by
        2^(bits - 1) (8-bit is unsigned around 128), the channels averaged.  Deviation from the reference: it divides integer PCM
        by i32::MAX whatever the bit depth (audio.rs Audio::from_file), which scales 16-bit audio by 2^-16 and pushes speech under
        the 1e-10 floor of the log-mel features."""
        import io
        import wave
        src = io.BytesIO(bytes(path_or_bytes)) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else os.fspath(path_or_bytes)
        try:
            with wave.open(src, "rb") as w:
                ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
                raw = w.readframes(n)
        except (wave.Error, EOFError) as e:
            raise TokenizerError(TK_ERR_AUDIO, "WAV: %s" % (e,))
        if width == 1:
            x = (np.frombuffer(raw, np.uint8).astype(np.float64) - 128.0) / 128.0
        elif width == 2:
            x = np.frombuffer(raw, "<i2").astype(np.float64) / 32768.0
        elif width == 3:
            b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            x = (v - ((v & 0x800000) << 1)).astype(np.float64) / 8388608.0
        elif width == 4:
            x = np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0
        else:
            raise TokenizerError(TK_ERR_AUDIO, "WAV: %d-byte samples" % width)
        x = x[:len(x) // ch * ch].reshape(-1, ch).mean(axis=1) if ch > 1 else x
        return cls(x.astype(np.float32), rate)


def _audio_config_struct(cfg):
    """An audio config (a dict with the fields of tk_audio_config; chunk_length_s None or absent: none) as the C struct."""
    if isinstance(cfg, _AudioConfig):
        return cfg
    cl = cfg.get("chunk_length_s")
    return _AudioConfig(int(cfg["sampling_rate"]), float(cfg["frame_rate"]), int(cfg["num_mel_bins"]), int(cfg["hop_length"]),
                        int(cfg["window_size"]), float(cl) if cl is not None else 0.0, 1 if cl is not None else 0, 0)


def audio_layout(cfg, n_samples):
    """tk_audio_layout: the host arithmetic of a batch of clips -> (padded, n_frames, n_tokens, n_segments), uint64 [n_clips] each."""
    st = _audio_config_struct(cfg)
    n = np.ascontiguousarray(n_samples, dtype=np.uint64).reshape(-1)
    out = [np.zeros(max(len(n), 1), np.uint64) for _ in range(4)]
    nb = n if len(n) else np.zeros(1, np.uint64)
    rc = _need("tk_audio_layout")(ctypes.byref(st), _p(nb, ctypes.c_uint64), len(n), *[_p(o, ctypes.c_uint64) for o in out])
    if rc != TK_OK:
        raise TokenizerError(rc, "audio config: a zero or negative field, or no whole frame per token")
    return tuple(o[:len(n)] for o in out)


class Engine:
    """Engine-level context: the replacement for CoreBPE (reference src/tekkenizer.rs:125, 384-386)."""

    def __init__(self, token_bytes, num_special, bos_id, eos_id, device=0, _borrowed=None):
        self._own = _borrowed is None
        if _borrowed is not None:
            self._h = _borrowed
            return
        toks = list(token_bytes)
        offs = np.zeros(len(toks) + 1, np.uint32)
        offs[1:] = np.cumsum([len(t) for t in toks], dtype=np.uint64).astype(np.uint32)
        blob = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8).copy()
        h = ctypes.c_void_p()
        rc = lib().tk_ctx_create(_p(blob, ctypes.c_uint8), _p(offs, ctypes.c_uint32), len(toks), num_special, bos_id,
                                 eos_id, device, ctypes.byref(h))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self._own:
            lib().tk_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc):
        return TokenizerError(rc, lib().tk_last_error(self._h).decode())

    def _call(self, name, *args):
        """The C entry `name` on this context; anything but TK_OK raises with tk_last_error."""
        rc = _need(name)(self._h, *args)
        if rc != TK_OK:
            raise self._err(rc)

    def audio_set_config(self, cfg):
        """tk_audio_set_config: builds and uploads the log-mel tables for cfg (a dict with the fields of tk_audio_config)."""
        st = _audio_config_struct(cfg)
        self._call("tk_audio_set_config", ctypes.byref(st))

    @staticmethod
    def _logmel_opts(log_mel_max, flags):
        return _LogmelOpts(float("nan") if log_mel_max is None else float(log_mel_max), int(flags))

    def audio_logmel_device(self, d_samples_ptr, d_offs_ptr, n_clips, n_samples, log_mel_max=None, checks=0, stream=0, flags=0):
        """tk_audio_logmel_device: float32 samples of all clips back to back (unpadded) and their uint64 offsets [n_clips + 1] in
        HBM -> a LogmelResult (context-owned device buffers); the definition is in include/tekken_hip.h.  log_mel_max None: the
        per-segment maximum."""
        o, r = self._logmel_opts(log_mel_max, flags), _Logmel()
        self._call("tk_audio_logmel_device", ctypes.c_void_p(d_samples_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_clips, n_samples,
                   int(checks), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(r))
        return LogmelResult(r)

    def audio_logmel(self, samples, offs, log_mel_max=None, flags=0):
        """tk_audio_logmel, host in / host out: a dict of numpy arrays (features float32 [n_mel * n_frames], frame_off uint64,
        clip_seg uint64) and the counts."""
        x = np.ascontiguousarray(samples, dtype=np.float32)
        oo = np.ascontiguousarray(offs, dtype=np.uint64)
        o, r = self._logmel_opts(log_mel_max, flags), _Logmel()
        xb = x if len(x) else np.zeros(1, np.float32)
        self._call("tk_audio_logmel", _p(xb, ctypes.c_float), _p(oo, ctypes.c_uint64), len(oo) - 1, ctypes.byref(o), ctypes.byref(r))
        return LogmelResult.take(r)[1]

    def last_logmel_ms(self):
        """(product kernel, clamp kernel) GPU milliseconds of the context's last log-mel call."""
        ms = (ctypes.c_float * 2)()
        _need("tk_last_logmel_ms")(self._h, ctypes.byref(ms))
        return tuple(float(v) for v in ms)

    def audio_splice_device(self, d_ids_ptr, d_id_offs_ptr, n_parts, n_ids, d_part_tokens_ptr, fill_id, stream=0):
        """tk_audio_splice_device: per part its own ids, then part_tokens[p] copies of fill_id -> a RaggedResult (context-owned)."""
        r = _Ragged()
        self._call("tk_audio_splice_device", ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr or None), n_parts, n_ids,
                   ctypes.c_void_p(d_part_tokens_ptr or None), int(fill_id), ctypes.c_void_p(stream), ctypes.byref(r))
        return RaggedResult(r)

    def audio_splice_calls(self):
        return int(_need("tk_audio_splice_calls")(self._h))

    def encode_batch(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False):
        """Host buffers in, host buffers out: (ids uint32[T], out_offsets uint64[D+1])."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res = _Result()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = lib().tk_encode_batch(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1,
                                   int(add_bos), int(add_eos), int(validate_utf8), ctypes.byref(res))
        if rc != TK_OK:
            raise self._err(rc)
        return _take_result(res)

    def encode_batch_pipelined(self, data, offs, add_bos=True, add_eos=True, slice_bytes=0, ids_out=None, offsets_out=None):
        """tk_encode_batch_pipelined: the batch streams through the GPU in slices (copy up / kernels / copy down overlapped).
        data / offs / ids_out / offsets_out may be pinned arrays from `host_empty` (then every copy is an asynchronous
        DMA); ids_out (uint32) must hold offs[-1] + 2 * n_docs ids at most.  Returns (ids view, offsets)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n_docs = len(offs) - 1
        if ids_out is None:
            ids_out = np.empty(int(offs[-1]) + 2 * n_docs + 1, np.uint32)
        if offsets_out is None:
            offsets_out = np.empty(n_docs + 1, np.uint64)
        n = ctypes.c_uint64(0)
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = lib().tk_encode_batch_pipelined(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), n_docs, int(add_bos),
                                             int(add_eos), int(slice_bytes), _p(ids_out, ctypes.c_uint32), len(ids_out),
                                             _p(offsets_out, ctypes.c_uint64), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        return ids_out[:int(n.value)], offsets_out

    def encode_one(self, text, add_bos=False, add_eos=False, out=None):
        """tk_encode_one: one document, caller-owned output (numpy uint32 array of >= len + 2 entries; made if None)."""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        if out is None:
            out = np.empty(len(raw) + 2, np.uint32)
        n = ctypes.c_uint64(0)
        rc = lib().tk_encode_one(self._h, raw, len(raw), int(add_bos), int(add_eos), _p(out, ctypes.c_uint32), len(out), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        return out[:n.value]

    def round_path_docs(self):
        """Documents so far whose long piece was merged in rounds by a workgroup (csrc/tk_long.hip)."""
        return int(lib().tk_round_path_docs(self._h))

    def long_piece_records(self):
        """Pieces of 65..256 bytes of the last batch that stayed on the flat path as records."""
        return int(lib().tk_long_piece_records(self._h))

    def set_memo(self, log2_entries, policy=0):
        """Memo of merged pieces (tk_ctx_set_memo): 0 = off, 10..26 = 2^n entries; policy 0 adaptive, 1 always on."""
        rc = lib().tk_ctx_set_memo(self._h, int(log2_entries), int(policy))
        if rc != TK_OK:
            raise self._err(rc)

    def memo_clear(self):
        rc = lib().tk_ctx_memo_clear(self._h)
        if rc != TK_OK:
            raise self._err(rc)

    def memo_stats(self):
        """{lookups_last, hits_last, lookups_total, hits_total, active_last} (tk_memo_stats)."""
        if not hasattr(lib(), "tk_memo_stats"):
            return {"lookups_last": 0, "hits_last": 0, "lookups_total": 0, "hits_total": 0, "active_last": False}
        v = [ctypes.c_uint64(0) for _ in range(4)]
        act = ctypes.c_int(0)
        lib().tk_memo_stats(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(act))
        return {"lookups_last": v[0].value, "hits_last": v[1].value, "lookups_total": v[2].value, "hits_total": v[3].value,
                "active_last": bool(act.value)}

    def cut_chunks(self):
        """Regions of the last batch whose long pieces were cut into independently merged fragments."""
        return int(lib().tk_cut_chunks(self._h)) if hasattr(lib(), "tk_cut_chunks") else 0

    def last_host_syncs(self):
        """Host waits of the last batch on the flat pipeline."""
        return int(lib().tk_last_host_syncs(self._h)) if hasattr(lib(), "tk_last_host_syncs") else 0

    def small_path_calls(self):
        """Calls served by the one-launch small-batch path so far."""
        return int(lib().tk_small_path_calls(self._h))

    def encode_docs(self, docs, add_bos=True, add_eos=True, validate_utf8=False):
        data, offs = pack_docs(docs)
        ids, oo = self.encode_batch(data, offs, add_bos, add_eos, validate_utf8)
        return [ids[int(oo[d]):int(oo[d + 1])].tolist() for d in range(len(docs))]

    def encode_batch_device(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, stream=0, checks=0):
        """Inputs resident in HBM (raw device pointers).  Returns (d_ids_ptr, d_out_offs_ptr, n_ids);
        the output buffers belong to the context and stay valid until the next call.  checks: CHECK_OFFSETS | CHECK_UTF8
        (tk_encode_batch_device_ex: the offsets / the documents are checked on the device first)."""
        d_ids, d_oo, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        if checks:
            rc = lib().tk_encode_batch_device_ex(self._h, ctypes.c_void_p(d_bytes_ptr), ctypes.c_void_p(d_offs_ptr), n_docs,
                                                 n_bytes, int(add_bos), int(add_eos), int(checks), ctypes.c_void_p(stream),
                                                 ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n))
        else:
            rc = lib().tk_encode_batch_device(self._h, ctypes.c_void_p(d_bytes_ptr), ctypes.c_void_p(d_offs_ptr), n_docs,
                                              n_bytes, int(add_bos), int(add_eos), ctypes.c_void_p(stream),
                                              ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        return d_ids.value, d_oo.value, int(n.value)

    def encode_batch_spans(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, checks=0):
        """tk_encode_batch_spans: (ids uint32[T], out_offsets uint64[D+1], spans uint32[T, 2]) -- spans[i] = (start, end) of id i in
        BYTES relative to the start of its document (include/tekken_hip.h).  checks: SPANS_CHECK_COVER | SPANS_CHECK_BYTES; a failed
        check raises TokenizerError with .bad_doc set."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res = _Result()
        sp = ctypes.POINTER(ctypes.c_uint32)()
        bad = ctypes.c_uint64(0)
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = _need("tk_encode_batch_spans")(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                                            int(add_eos), int(validate_utf8), int(checks), ctypes.byref(res), ctypes.byref(sp), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_doc = int(bad.value)
            raise e
        n = int(res.n_ids)
        spans = np.ctypeslib.as_array(sp, shape=(max(2 * n, 1),))[:2 * n].copy().reshape(n, 2)
        lib().tk_free_spans(sp)
        ids, oo = _take_result(res)
        return ids, oo, spans

    def token_spans_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_doc_offs_ptr=0, d_bytes_ptr=0, checks=0, stream=0):
        """tk_token_spans_device: spans of ids resident in HBM (raw device pointers; the document offsets / the text only for
        the checks).  Returns the context-owned d_spans pointer (uint32[2 * n_ids]); raises with .bad_doc on a failed check."""
        d_sp, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
        rc = _need("tk_token_spans_device")(self._h, ctypes.c_void_p(d_ids_ptr), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                                            ctypes.c_void_p(d_doc_offs_ptr or None), ctypes.c_void_p(d_bytes_ptr or None), int(checks),
                                            ctypes.c_void_p(stream), ctypes.byref(d_sp), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_doc = int(bad.value)
            raise e
        return d_sp.value

    def encode_batch_device_spans(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, checks=0, stream=0):
        """tk_encode_batch_device_spans: encode_batch_device + the spans pass.  checks may mix CHECK_OFFSETS / CHECK_UTF8 with
        SPANS_CHECK_COVER / SPANS_CHECK_BYTES.  Returns (d_ids_ptr, d_out_offs_ptr, d_spans_ptr, n_ids), context-owned."""
        d_ids, d_oo, d_sp, n, bad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = _need("tk_encode_batch_device_spans")(self._h, ctypes.c_void_p(d_bytes_ptr), ctypes.c_void_p(d_offs_ptr), n_docs, n_bytes,
                                                   int(add_bos), int(add_eos), int(checks), ctypes.c_void_p(stream), ctypes.byref(d_ids),
                                                   ctypes.byref(d_oo), ctypes.byref(d_sp), ctypes.byref(n), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_doc = int(bad.value)
            raise e
        return d_ids.value, d_oo.value, d_sp.value, int(n.value)

    def token_spans_units_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, unit=UNIT_CHAR, stream=0):
        """tk_token_spans_units_device: spans of ids resident in HBM in `unit` (UNIT_BYTE | UNIT_CHAR | UNIT_UTF16; the definition is
        in include/tekken_hip.h).  Returns the context-owned d_spans pointer (uint32[2 * n_ids]), a buffer apart from the byte
        spans and every encode output."""
        d_sp = ctypes.c_void_p()
        self._call("tk_token_spans_units_device", ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                   int(unit), ctypes.c_void_p(stream), ctypes.byref(d_sp))
        return d_sp.value

    def encode_batch_device_spans_units(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, unit=UNIT_CHAR,
                                        checks=0, stream=0):
        """tk_encode_batch_device_spans_units: encode_batch_device + the units pass.  checks: CHECK_OFFSETS | CHECK_UTF8 only.
        Returns (d_ids_ptr, d_out_offs_ptr, d_spans_ptr, n_ids), context-owned."""
        d_ids, d_oo, d_sp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        self._call("tk_encode_batch_device_spans_units", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_docs, n_bytes,
                   int(add_bos), int(add_eos), int(checks), int(unit), ctypes.c_void_p(stream), ctypes.byref(d_ids), ctypes.byref(d_oo),
                   ctypes.byref(d_sp), ctypes.byref(n))
        return d_ids.value, d_oo.value, d_sp.value, int(n.value)

    def encode_batch_spans_units(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, unit=UNIT_CHAR):
        """tk_encode_batch_spans_units: (ids uint32[T], out_offsets uint64[D+1], spans uint32[T, 2]) -- spans[i] = (start, end) of
        id i in `unit`, relative to the start of its document (include/tekken_hip.h)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res = _Result()
        sp = ctypes.POINTER(ctypes.c_uint32)()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        self._call("tk_encode_batch_spans_units", _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                   int(add_eos), int(validate_utf8), int(unit), ctypes.byref(res), ctypes.byref(sp))
        n = int(res.n_ids)
        spans = np.ctypeslib.as_array(sp, shape=(max(2 * n, 1),))[:2 * n].copy().reshape(n, 2)
        lib().tk_free_spans(sp)
        ids, oo = _take_result(res)
        return ids, oo, spans

    def spans_locate_device(self, d_spans_ptr, d_id_offs_ptr, n_docs, n_ids, d_ann_doc_ptr, d_ann_ptr, n_ann, stream=0):
        """tk_spans_locate_device: for every annotation (as, ae) of document ann_doc, in the unit of the spans, the
        document-relative id range (lo, hi) whose spans overlap it.  Returns the context-owned d_tok_range pointer (uint32[n_ann, 2]);
        a bad annotation raises TokenizerError with .bad_ann set."""
        d_out, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
        rc = _need("tk_spans_locate_device")(self._h, ctypes.c_void_p(d_spans_ptr or None), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                                             ctypes.c_void_p(d_ann_doc_ptr or None), ctypes.c_void_p(d_ann_ptr or None), n_ann,
                                             ctypes.c_void_p(stream), ctypes.byref(d_out), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_ann = int(bad.value)
            raise e
        return d_out.value

    # ---- the three entries around a layout pass (dense, seqpack, window, rowfit): R the result class, o the pass's options
    def _from_ids_device(self, R, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, extra, stream):
        """tk_<pass>_from_ids_device; extra: the pass's second input stream on the device, if its entry takes one."""
        st = R.STRUCT()
        self._call("tk_%s_from_ids_device" % R.PASS, ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                   *[ctypes.c_void_p(x or None) for x in extra], ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st))
        return R(st, int(flags), n_docs)

    def _encode_device(self, R, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream):
        """tk_encode_batch_device_<pass> -> (d_ids_ptr, d_out_offs_ptr, n_ids, R)."""
        st, d_ids, d_oo, n = R.STRUCT(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        self._call("tk_encode_batch_device_" + R.PASS, ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_docs, n_bytes,
                   int(add_bos), int(add_eos), int(checks), ctypes.byref(o), ctypes.c_void_p(stream),
                   ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n), ctypes.byref(st))
        return d_ids.value, d_oo.value, int(n.value), R(st, int(flags), n_docs)

    def _encode_host(self, R, o, flags, data, offs, add_bos, add_eos, validate_utf8):
        """tk_encode_batch_<pass>, host in / host out -> (R with the counts, its numpy arrays and counts by name)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        st = R.STRUCT()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        self._call("tk_encode_batch_" + R.PASS, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                   int(add_eos), int(validate_utf8), ctypes.byref(o), ctypes.byref(st))
        return R.take(st, int(flags), len(offs) - 1)

    def dense_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, max_length=0, multiple_of=0, pad_id=0, keep_head=0,
                              keep_tail=0, flags=0, stream=0):
        """tk_dense_from_ids_device: ragged ids resident in HBM -> dense[n_docs, row_len] (+ mask with DENSE_MASK, lengths, the
        truncated count); the definition is in include/tekken_hip.h.  Returns a DenseResult (context-owned device buffers,
        apart from the encode and spans outputs)."""
        o = _dense_opts(max_length, multiple_of, pad_id, keep_head, keep_tail, flags)
        return self._from_ids_device(DenseResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (), stream)

    def encode_batch_device_dense(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, max_length=0, multiple_of=0,
                                  pad_id=0, flags=0, checks=0, stream=0):
        """tk_encode_batch_device_dense: encode_batch_device + the dense pass on the same stream; BOS / EOS survive truncation.
        Returns (d_ids_ptr, d_out_offs_ptr, n_ids, DenseResult), all context-owned."""
        o = _dense_opts(max_length, multiple_of, pad_id, 0, 0, flags)
        return self._encode_device(DenseResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_dense(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, max_length=0, multiple_of=0, pad_id=0,
                           flags=0):
        """tk_encode_batch_dense, host in / host out: (dense int32 or int64 [D, L], mask uint8 [D, L] or None, lengths uint32 [D]);
        .n_truncated of the call is kept in self.last_n_truncated."""
        o = _dense_opts(max_length, multiple_of, pad_id, 0, 0, flags)
        r, out = self._encode_host(DenseResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)
        self.last_n_truncated = r.n_truncated
        return out["ids"], out["mask"], out["lengths"]

    def seqpack_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, seq_len, pad_id=0, flags=0, stream=0):
        """tk_seqpack_from_ids_device: ragged ids resident in HBM -> the id stream cut into rows of seq_len (+ position_ids,
        segment_ids, cu_seqlens as flags select); the definition is in include/tekken_hip.h.  Returns a SeqpackResult
        (context-owned device buffers, apart from the encode, spans and dense outputs)."""
        o = _SeqpackOpts(int(seq_len), int(pad_id), int(flags))
        return self._from_ids_device(SeqpackResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (), stream)

    def encode_batch_device_seqpack(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, seq_len, add_bos=True, add_eos=True, pad_id=0, flags=0,
                                    checks=0, stream=0):
        """tk_encode_batch_device_seqpack: encode_batch_device + the packed pass on the same stream.
        Returns (d_ids_ptr, d_out_offs_ptr, n_ids, SeqpackResult), all context-owned."""
        o = _SeqpackOpts(int(seq_len), int(pad_id), int(flags))
        return self._encode_device(SeqpackResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_seqpack(self, data, offs, seq_len, add_bos=True, add_eos=True, validate_utf8=False, pad_id=0, flags=0):
        """tk_encode_batch_seqpack, host in / host out: a dict of numpy arrays (input_ids, position_ids, segment_ids [n_rows, seq_len]
        int32 or int64, cu_seqlens int32 [n_segments + 1]; an unselected one: None) and the counts n_rows, n_used, n_left,
        n_segments, max_seqlen."""
        o = _SeqpackOpts(int(seq_len), int(pad_id), int(flags))
        return self._encode_host(SeqpackResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)[1]

    def rowfit_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, seq_len, pad_id=0, keep_tail=0, flags=0, d_labels_ptr=0,
                               ignore_index=-100, stream=0):
        """tk_rowfit_from_ids_device: ragged ids resident in HBM -> whole documents placed next-fit into rows of seq_len, never cut
        (+ labels from d_labels_ptr, position_ids, segment_ids, cu_seqlens, doc_start as flags select); the definition is in
        include/tekken_hip.h.  Returns a RowfitResult (context-owned device buffers, apart from every other output)."""
        o = _RowfitOpts(int(seq_len), int(pad_id), int(keep_tail), int(flags), int(ignore_index))
        return self._from_ids_device(RowfitResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (d_labels_ptr,), stream)

    def encode_batch_device_rowfit(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, seq_len, add_bos=True, add_eos=True, pad_id=0, keep_tail=0,
                                   flags=0, checks=0, stream=0):
        """tk_encode_batch_device_rowfit: encode_batch_device + the rowfit pass on the same stream.
        Returns (d_ids_ptr, d_out_offs_ptr, n_ids, RowfitResult), all context-owned."""
        o = _RowfitOpts(int(seq_len), int(pad_id), int(keep_tail), int(flags), -100)
        return self._encode_device(RowfitResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_rowfit(self, data, offs, seq_len, add_bos=True, add_eos=True, validate_utf8=False, pad_id=0, keep_tail=0, flags=0):
        """tk_encode_batch_rowfit, host in / host out: a dict of numpy arrays (input_ids, position_ids, segment_ids [n_rows, seq_len]
        int32 or int64, cu_seqlens int32 [n_segments + 1], doc_start uint64 [n_docs]; an unselected one: None; labels: None, text
        has none) and the counts n_rows, n_segments, max_seqlen, n_truncated, n_pad."""
        o = _RowfitOpts(int(seq_len), int(pad_id), int(keep_tail), int(flags), -100)
        return self._encode_host(RowfitResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)[1]

    def regroup_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, order=REGROUP_ORDER_KEEP, min_length=0, max_length=0, seed=0,
                                window=0, max_tokens=0, max_docs=0, flags=0, d_labels_ptr=0, d_keep_ptr=0, stream=0):
        """tk_regroup_from_ids_device: ragged ids resident in HBM -> the kept documents in another order, ragged again (ids, offsets,
        labels with REGROUP_LABELS and d_labels_ptr, perm) and the batches a padded-token budget cuts them into; the definition is in
        include/tekken_hip.h.  d_keep_ptr: uint8 [n_docs] or 0.  Returns a RegroupResult (context-owned device buffers, apart from
        every other output: its ids_ptr / offsets_ptr go into the other passes as they are)."""
        o = _regroup_opts(order, min_length, max_length, seed, window, max_tokens, max_docs, flags)
        return self._from_ids_device(RegroupResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (d_labels_ptr, d_keep_ptr), stream)

    def encode_batch_device_regroup(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, order=REGROUP_ORDER_KEEP,
                                    min_length=0, max_length=0, seed=0, window=0, max_tokens=0, max_docs=0, flags=0, checks=0, stream=0):
        """tk_encode_batch_device_regroup: encode_batch_device + the regroup pass on the same stream (no labels, no keep mask).
        Returns (d_ids_ptr, d_out_offs_ptr, n_ids, RegroupResult), all context-owned."""
        o = _regroup_opts(order, min_length, max_length, seed, window, max_tokens, max_docs, flags)
        return self._encode_device(RegroupResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_regroup(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, order=REGROUP_ORDER_KEEP, min_length=0,
                             max_length=0, seed=0, window=0, max_tokens=0, max_docs=0, flags=0):
        """tk_encode_batch_regroup, host in / host out: a dict of numpy arrays (ids uint32, offsets uint64, perm uint32,
        batch_offsets uint64, batch_rowlen uint32; an unselected one None) and the counts."""
        o = _regroup_opts(order, min_length, max_length, seed, window, max_tokens, max_docs, flags)
        return self._encode_host(RegroupResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)[1]

    def dense_from_regroup_batch(self, res, first_doc, end_doc, pad_id=0, flags=0, max_length=0, multiple_of=0, stream=0):
        """The dense pass over documents first_doc .. end_doc of a RegroupResult (one of its batches()): the same ids pointer and
        offsets + first_doc -- the dense kernel indexes ids[offsets[d] + j], so nothing is rebased or copied.  Returns a DenseResult
        [end_doc - first_doc, the longest document of the range]."""
        if not 0 <= first_doc <= end_doc <= res.n_docs:
            raise TokenizerError(TK_ERR_INVALID_ARG, "dense_from_regroup_batch: documents %d .. %d of %d" % (first_doc, end_doc, res.n_docs))
        return self.dense_from_ids_device(res.ids_ptr, res.offsets_ptr + 8 * first_doc, end_doc - first_doc, res.n_ids, max_length, multiple_of,
                                          pad_id, 0, 0, flags, stream)

    # ---- word ids (tk_words): the three entries take the text, so they are the pass's own
    def _words_raise(self, rc, bad):
        e = self._err(rc)
        e.bad_doc = int(bad.value)
        raise e

    def words_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_bytes_ptr, d_doc_offs_ptr, n_bytes, flags=0, checks=0, stream=0):
        """tk_words_from_ids_device: ids and their text resident in HBM -> the word of every id (HF's word_ids(); the definition is
        in include/tekken_hip.h).  flags: WORDS_FIRST; checks: WORDS_CHECK_ALIGNED (a failed check raises with .bad_doc set).
        Returns a WordsResult (context-owned device buffers, apart from every other output)."""
        st, bad, o = _Words(), ctypes.c_uint64(0), _WordsOpts(int(flags))
        rc = _need("tk_words_from_ids_device")(self._h, ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                                               ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_doc_offs_ptr), n_bytes, int(checks),
                                               ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st), ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        return WordsResult(st)

    def encode_batch_device_words(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, flags=0, checks=0, stream=0):
        """tk_encode_batch_device_words: encode_batch_device + the words pass on the same stream.  checks may mix CHECK_OFFSETS /
        CHECK_UTF8 with WORDS_CHECK_ALIGNED.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids, WordsResult), all context-owned."""
        st, bad, o = _Words(), ctypes.c_uint64(0), _WordsOpts(int(flags))
        d_ids, d_oo, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        rc = _need("tk_encode_batch_device_words")(self._h, ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_docs, n_bytes,
                                                   int(add_bos), int(add_eos), int(checks), ctypes.byref(o), ctypes.c_void_p(stream),
                                                   ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n), ctypes.byref(st), ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        return d_ids.value, d_oo.value, int(n.value), WordsResult(st)

    def encode_batch_words(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, flags=0, checks=0):
        """tk_encode_batch_words, host in / host out: (ids uint32[T], out_offsets uint64[D+1], {"word_ids": uint32[T] (WORD_NONE
        for a special id), "doc_words": uint64[D+1], "word_first": uint32[n_words] or None, "n_words"})."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res, st, bad, o = _Result(), _Words(), ctypes.c_uint64(0), _WordsOpts(int(flags))
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = _need("tk_encode_batch_words")(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                                            int(add_eos), int(validate_utf8), int(checks), ctypes.byref(o), ctypes.byref(res), ctypes.byref(st),
                                            ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        _, out = WordsResult.take(st)
        ids, oo = _take_result(res)
        return ids, oo, out

    # ---- special-token strings parsed out of text (tk_specials): the entries take the text, so they are the pass's own
    def split_specials_device(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, modes=None, flags=0, checks=0, stream=0):
        """tk_specials_split_device: text resident in HBM -> the text without the special-token strings found in it, cut into the
        parts that encode_parts_device_join takes (the definition is in include/tekken_hip.h).  modes: None (every string is
        parsed) or one SPECIAL_TEXT / SPECIAL_PARSE / SPECIAL_RAISE per special id; flags: SPECIALS_BOS | SPECIALS_EOS |
        SPECIALS_PART_SRC; checks: CHECK_OFFSETS | CHECK_UTF8.  A SPECIAL_RAISE match raises with .bad_doc set.  Returns a
        SpecialsResult (context-owned device buffers, apart from every other output)."""
        (o, keep), st, bad = _specials_opts(modes, flags), _Specials(), ctypes.c_uint64(0)
        rc = _need("tk_specials_split_device")(self._h, ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_docs, n_bytes,
                                               int(checks), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st), ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        return SpecialsResult(st)

    def encode_batch_device_parsed(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, modes=None, flags=0,
                                   ignore_index=-100, join_flags=0, checks=0, stream=0):
        """tk_encode_batch_device_parsed: the split + encode_parts_device_join over its parts on the same stream.  add_bos / add_eos
        are SPECIALS_BOS / SPECIALS_EOS of flags.  Returns (SpecialsResult, JoinResult), both context-owned."""
        f = int(flags) | (SPECIALS_BOS if add_bos else 0) | (SPECIALS_EOS if add_eos else 0)
        (o, keep), st, j, bad = _specials_opts(modes, f), _Specials(), _Join(), ctypes.c_uint64(0)
        jo = _JoinOpts(int(ignore_index), int(join_flags))
        rc = _need("tk_encode_batch_device_parsed")(self._h, ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_docs,
                                                    n_bytes, int(checks), ctypes.byref(o), ctypes.byref(jo), ctypes.c_void_p(stream),
                                                    ctypes.byref(st), ctypes.byref(j), ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        return SpecialsResult(st), JoinResult(j)

    def encode_batch_parsed(self, data, offs, add_bos=True, add_eos=True, modes=None, flags=0, ignore_index=-100, join_flags=0,
                            validate_utf8=False, return_parts=False):
        """tk_encode_batch_parsed, host in / host out: the join's dict (ids uint32 [N], offsets uint64 [D + 1], labels, part_index,
        the counts) and, with return_parts, the split's (bytes, part_offsets, part_ctrl, conv_offsets, part_src, the counts) as a
        second dict."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        f = int(flags) | (SPECIALS_BOS if add_bos else 0) | (SPECIALS_EOS if add_eos else 0)
        (o, keep), st, j, bad = _specials_opts(modes, f), _Specials(), _Join(), ctypes.c_uint64(0)
        jo = _JoinOpts(int(ignore_index), int(join_flags))
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = _need("tk_encode_batch_parsed")(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(validate_utf8),
                                             ctypes.byref(o), ctypes.byref(jo), ctypes.byref(st) if return_parts else None, ctypes.byref(j),
                                             ctypes.byref(bad))
        if rc != TK_OK:
            self._words_raise(rc, bad)
        out = JoinResult.take(j)[1]
        return (out, SpecialsResult.take(st)[1]) if return_parts else out

    def last_specials_ms(self):
        """tk_last_specials_ms: GPU time of the stages of the last specials pass on this context: (candidates, chain, part tables,
        text compaction)."""
        ms = (ctypes.c_float * 4)()
        _need("tk_last_specials_ms")(self._h, ctypes.byref(ms))
        return tuple(ms)

    # ---- fill-in-the-middle rows (tk_fim): a pass in front of encode (text) or of the join (ids), so the entries are its own.
    # opts: the keywords of _fim_opts (rate_q32, spm_q32, seed, prefix_id, suffix_id, middle_id, head, tail, min_units, flags)
    def fim_split_device(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, d_cuts_ptr=0, checks=0, stream=0, **opts):
        """tk_fim_split_device: text resident in HBM -> every chosen document cut in two places and reordered inside its own range,
        with the part tables that encode_parts_device_join takes (the definition is in include/tekken_hip.h).  d_cuts_ptr: uint64
        [n_docs, 2] on the device or 0 (drawn from seed); checks: CHECK_OFFSETS | CHECK_UTF8.  Returns a FimResult (context-owned
        device buffers, apart from every other output)."""
        o, st = _fim_opts(**opts), _Fim()
        self._call("tk_fim_split_device", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_docs, n_bytes,
                   ctypes.c_void_p(d_cuts_ptr or None), int(checks), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st))
        return FimResult(st, unit_bytes=1)

    def fim_split_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_cuts_ptr=0, stream=0, **opts):
        """tk_fim_split_ids_device: the same over ids resident in HBM (head / tail ids stay in place).  Returns a FimResult whose
        units are uint32 and whose part_offsets are the id offsets join_from_ids_device takes."""
        o, st = _fim_opts(**opts), _Fim()
        self._call("tk_fim_split_ids_device", ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr or None), n_docs, n_ids,
                   ctypes.c_void_p(d_cuts_ptr or None), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st))
        return FimResult(st, unit_bytes=4)

    def encode_batch_device_fim(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, d_cuts_ptr=0, ignore_index=-100, join_flags=0, checks=0,
                                stream=0, **opts):
        """tk_encode_batch_device_fim: the text split + encode_parts_device_join over its parts (part_flags included) on the same
        stream.  Returns (FimResult, JoinResult), both context-owned."""
        o, st, j, jo = _fim_opts(**opts), _Fim(), _Join(), _JoinOpts(int(ignore_index), int(join_flags))
        self._call("tk_encode_batch_device_fim", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_docs, n_bytes,
                   ctypes.c_void_p(d_cuts_ptr or None), int(checks), ctypes.byref(o), ctypes.byref(jo), ctypes.c_void_p(stream),
                   ctypes.byref(st), ctypes.byref(j))
        return FimResult(st, unit_bytes=1), JoinResult(j)

    def fim_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_cuts_ptr=0, ignore_index=-100, join_flags=0, stream=0, **opts):
        """tk_fim_from_ids_device: the ids split + join_from_ids_device (documents tokenised once, a new draw every epoch).
        Returns (FimResult, JoinResult), both context-owned."""
        o, st, j, jo = _fim_opts(**opts), _Fim(), _Join(), _JoinOpts(int(ignore_index), int(join_flags))
        self._call("tk_fim_from_ids_device", ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr or None), n_docs, n_ids,
                   ctypes.c_void_p(d_cuts_ptr or None), ctypes.byref(o), ctypes.byref(jo), ctypes.c_void_p(stream), ctypes.byref(st),
                   ctypes.byref(j))
        return FimResult(st, unit_bytes=4), JoinResult(j)

    def encode_batch_fim(self, data, offs, cuts=None, ignore_index=-100, join_flags=0, validate_utf8=False, return_parts=False, **opts):
        """tk_encode_batch_fim, host in / host out: the join's dict (ids uint32 [N], offsets uint64 [D + 1], labels, part_index, the
        counts) and, with return_parts, the split's (FimResult.OUTPUTS and the counts) as a second dict.  cuts: None or uint64
        [D, 2]."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        D = len(offs) - 1
        cbuf = None
        if cuts is not None:
            cbuf = np.ascontiguousarray(cuts, dtype=np.uint64).reshape(-1)
            if len(cbuf) != 2 * D:
                raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_fim: cuts must be [n_docs, 2]")
            cbuf = cbuf if D else np.zeros(2, np.uint64)
        o, st, j, jo = _fim_opts(**opts), _Fim(), _Join(), _JoinOpts(int(ignore_index), int(join_flags))
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        self._call("tk_encode_batch_fim", _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), D, None if cbuf is None else _p(cbuf, ctypes.c_uint64),
                   int(validate_utf8), ctypes.byref(o), ctypes.byref(jo), ctypes.byref(st) if return_parts else None, ctypes.byref(j))
        out = JoinResult.take(j)[1]
        return (out, FimResult.take(st)[1]) if return_parts else out

    def last_fim_ms(self):
        """tk_last_fim_ms: GPU milliseconds of the last FIM pass on this context -- (cut kernel, permute kernel)."""
        ms = (ctypes.c_float * 2)()
        _need("tk_last_fim_ms")(self._h, ctypes.byref(ms))
        return tuple(float(x) for x in ms)

    # ---- masked-LM and span-corruption rows (tk_noise_replace / tk_noise_spans): a pass over ids with two optional second inputs,
    # so the entries are its own.  opts: the keywords of _noise_opts (start_q32, mask_q32, random_q32, seed, unit, span_min, span_max,
    # mask_id, n_sentinels, sentinel_first, final_id, flags, ignore_index)
    def _noise_device(self, mode, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_word_ids_ptr, d_sel_ptr, stream, opts):
        S, R = _NOISE[mode]
        o, st = _noise_opts(**opts), S()
        self._call("tk_noise_%s_device" % mode, ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr or None), n_docs, n_ids,
                   ctypes.c_void_p(d_word_ids_ptr or None), ctypes.c_void_p(d_sel_ptr or None), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(st))
        return R(st)

    def noise_replace_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_word_ids_ptr=0, d_sel_ptr=0, stream=0, **opts):
        """tk_noise_replace_device: ids resident in HBM -> the ids with a hash-drawn (or, d_sel_ptr: uint8 [n_ids], given) choice of
        them masked / replaced, and the labels (masked LM; the definition is in include/tekken_hip.h).  d_word_ids_ptr: uint32
        [n_ids] of the words pass (NOISE_UNIT_WORD).  Returns a NoiseReplaceResult (context-owned device buffers)."""
        return self._noise_device("replace", d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_word_ids_ptr, d_sel_ptr, stream, opts)

    def noise_spans_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_word_ids_ptr=0, d_sel_ptr=0, stream=0, **opts):
        """tk_noise_spans_device: the same choice, every chosen run replaced by a sentinel in the inputs and spelt out behind it in
        the targets (T5 / UL2 span corruption).  flags: NOISE_SPLIT | NOISE_JOINED (| NOISE_DESC).  Returns a NoiseSpansResult."""
        return self._noise_device("spans", d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_word_ids_ptr, d_sel_ptr, stream, opts)

    def _encode_device_noise(self, mode, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream, opts):
        S, R = _NOISE[mode]
        o, st = _noise_opts(**opts), S()
        d_ids, d_oo, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        self._call("tk_encode_batch_device_noise_" + mode, ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_docs, n_bytes,
                   int(add_bos), int(add_eos), int(checks), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(d_ids), ctypes.byref(d_oo),
                   ctypes.byref(n), ctypes.byref(st))
        return d_ids.value, d_oo.value, int(n.value), R(st)

    def encode_batch_device_noise_replace(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, checks=0, stream=0, **opts):
        """tk_encode_batch_device_noise_replace: encode_batch_device, the words pass where unit is NOISE_UNIT_WORD, and the noise pass
        on the same stream.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids, NoiseReplaceResult), all context-owned."""
        return self._encode_device_noise("replace", d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream, opts)

    def encode_batch_device_noise_spans(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, checks=0, stream=0, **opts):
        """tk_encode_batch_device_noise_spans: the same in front of spans mode.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids,
        NoiseSpansResult)."""
        return self._encode_device_noise("spans", d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream, opts)

    def _encode_host_noise(self, mode, data, offs, add_bos, add_eos, validate_utf8, opts):
        S, R = _NOISE[mode]
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        o, st, res = _noise_opts(**opts), S(), _Result()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        self._call("tk_encode_batch_noise_" + mode, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos), int(add_eos),
                   int(validate_utf8), ctypes.byref(o), ctypes.byref(res), ctypes.byref(st))
        _, out = R.take(st)
        ids, oo = _take_result(res)
        return ids, oo, out

    def encode_batch_noise_replace(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, **opts):
        """tk_encode_batch_noise_replace, host in / host out: (ids uint32 [T] in front of the noise, out_offsets uint64 [D + 1],
        {"input_ids": uint32 [T], "labels": int32 [T], "selected": uint8 [T] or None, the counts})."""
        return self._encode_host_noise("replace", data, offs, add_bos, add_eos, validate_utf8, opts)

    def encode_batch_noise_spans(self, data, offs, add_bos=True, add_eos=True, validate_utf8=False, **opts):
        """tk_encode_batch_noise_spans, host in / host out: (ids, out_offsets, {NoiseSpansResult.OUTPUTS and the counts})."""
        return self._encode_host_noise("spans", data, offs, add_bos, add_eos, validate_utf8, opts)

    def last_noise_ms(self):
        """tk_last_noise_ms: GPU milliseconds of the last noise pass on this context -- (selection, counts and scans, fill kernel)."""
        ms = (ctypes.c_float * 3)()
        _need("tk_last_noise_ms")(self._h, ctypes.byref(ms))
        return tuple(float(x) for x in ms)

    def last_words_ms(self):
        """tk_last_words_ms: GPU milliseconds of the last words pass -- (split launch, words kernel, scan, word_first)."""
        ms = (ctypes.c_float * 4)()
        _need("tk_last_words_ms")(self._h, ctypes.byref(ms))
        return tuple(float(x) for x in ms)

    def last_regroup_ms(self):
        """tk_last_regroup_ms: GPU time of the stages of the last regroup pass on this context: (select, sort, gather, batches)."""
        ms = (ctypes.c_float * 4)()
        _need("tk_last_regroup_ms")(self._h, ctypes.byref(ms))
        return tuple(ms)

    def last_rowfit_ms(self):
        """tk_last_rowfit_ms: GPU time of the stages of the last rowfit pass on this context."""
        a, b, c = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
        _need("tk_last_rowfit_ms")(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"placement_ms": a.value, "fill_ms": b.value, "cu_ms": c.value}

    def encode_parts_device_rowfit(self, d_bytes_ptr, d_offs_ptr, n_parts, n_bytes, d_part_ctrl_ptr, d_part_flags_ptr, d_conv_offs_ptr, n_convs,
                                   seq_len, pad_id=0, keep_tail=0, flags=0, ignore_index=-100, join_flags=JOIN_LABELS, checks=0, stream=0):
        """tk_encode_parts_device_rowfit: encode_parts_device_join + the rowfit pass over the conversations' ids, labels and offsets
        on the same stream.  Returns (JoinResult, RowfitResult), both context-owned."""
        jo, j = _JoinOpts(int(ignore_index), int(join_flags)), _Join()
        o, p = _RowfitOpts(int(seq_len), int(pad_id), int(keep_tail), int(flags), int(ignore_index)), _Rowfit()
        self._call("tk_encode_parts_device_rowfit", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_parts, n_bytes,
                   ctypes.c_void_p(d_part_ctrl_ptr or None), ctypes.c_void_p(d_part_flags_ptr or None), ctypes.c_void_p(d_conv_offs_ptr or None),
                   n_convs, int(checks), ctypes.byref(jo), ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(j), ctypes.byref(p))
        return JoinResult(j), RowfitResult(p, int(flags), n_convs)

    def window_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, max_length, stride=0, multiple_of=0, pad_id=0, keep_head=0,
                               keep_tail=0, flags=0, d_spans_ptr=0, stream=0):
        """tk_window_from_ids_device: ragged ids resident in HBM -> overlapping windows [n_windows, row_len] (+ mask with
        WINDOW_MASK, spans with WINDOW_SPANS from d_spans_ptr, lengths, window_doc, window_start, doc_windows); the definition is
        in include/tekken_hip.h.  Returns a WindowResult (context-owned device buffers, apart from every other output)."""
        o = _window_opts(max_length, stride, multiple_of, pad_id, keep_head, keep_tail, flags)
        return self._from_ids_device(WindowResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (d_spans_ptr,), stream)

    def encode_batch_device_window(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, max_length, stride=0, add_bos=True, add_eos=True,
                                   multiple_of=0, pad_id=0, flags=0, checks=0, stream=0):
        """tk_encode_batch_device_window: encode_batch_device (+ the spans pass with WINDOW_SPANS) + the window pass on the same
        stream; every window repeats BOS / EOS.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids, WindowResult), all context-owned."""
        o = _window_opts(max_length, stride, multiple_of, pad_id, 0, 0, flags)
        return self._encode_device(WindowResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_window(self, data, offs, max_length, stride=0, add_bos=True, add_eos=True, validate_utf8=False, multiple_of=0,
                            pad_id=0, flags=0):
        """tk_encode_batch_window, host in / host out: a dict of numpy arrays (input_ids int32 or int64 [n_windows, row_len], mask
        uint8 or None, lengths / window_doc / window_start uint32 [n_windows], doc_windows uint64 [n_docs + 1], spans uint32
        [n_windows, row_len, 2] or None) and the counts n_windows, n_split."""
        o = _window_opts(max_length, stride, multiple_of, pad_id, 0, 0, flags)
        return self._encode_host(WindowResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)[1]

    def chunk_levels_device(self, d_spans_ptr, d_id_offs_ptr, n_docs, n_ids, d_bytes_ptr, d_offs_ptr, n_bytes, levels=CHUNK_LEVELS_ALL, stream=0):
        """tk_chunk_levels_device: the level byte of every id (the strength of the break of the text in front of it, CHUNK_LEVEL_*)
        from its span and the text, under the mask `levels`; the rules are in include/tekken_hip.h.  Returns the device pointer of
        n_ids uint8 (context-owned, valid until the next call that makes levels)."""
        d_lev = ctypes.c_void_p()
        self._call("tk_chunk_levels_device", ctypes.c_void_p(d_spans_ptr or None), ctypes.c_void_p(d_id_offs_ptr), n_docs, n_ids,
                   ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_bytes, int(levels), ctypes.c_void_p(stream), ctypes.byref(d_lev))
        return d_lev.value

    def chunk_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, d_levels_ptr, max_length, min_length, overlap=0, multiple_of=0,
                              pad_id=0, keep_head=0, keep_tail=0, flags=0, d_spans_ptr=0, stream=0):
        """tk_chunk_from_ids_device: ragged ids and their level bytes resident in HBM -> chunks [n_windows, row_len] cut at the
        strongest break a chunk of min_length .. max_length - keep_head - keep_tail body ids can end at (+ mask with CHUNK_MASK,
        spans with CHUNK_SPANS and chunk_bytes with CHUNK_BYTES from d_spans_ptr, lengths, window_doc, window_start, doc_windows,
        cut_level, level_counts); the definition is in include/tekken_hip.h.  Returns a ChunkResult (context-owned device buffers,
        apart from every other output)."""
        o = _chunk_opts(max_length, min_length, overlap, multiple_of, pad_id, keep_head, keep_tail, CHUNK_LEVELS_ALL, flags)
        return self._from_ids_device(ChunkResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_docs, n_ids, (d_levels_ptr, d_spans_ptr), stream)

    def encode_batch_device_chunk(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, max_length, min_length, overlap=0, add_bos=True, add_eos=True,
                                  multiple_of=0, pad_id=0, levels=CHUNK_LEVELS_ALL, flags=0, checks=0, stream=0):
        """tk_encode_batch_device_chunk: encode_batch_device + the spans pass (into a buffer of the chunk pass) + the levels + the
        chunk pass on the same stream; every chunk repeats BOS / EOS.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids, ChunkResult), all
        context-owned."""
        o = _chunk_opts(max_length, min_length, overlap, multiple_of, pad_id, 0, 0, levels, flags)
        return self._encode_device(ChunkResult, o, flags, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, checks, stream)

    def encode_batch_chunk(self, data, offs, max_length, min_length, overlap=0, add_bos=True, add_eos=True, validate_utf8=False, multiple_of=0,
                           pad_id=0, levels=CHUNK_LEVELS_ALL, flags=0):
        """tk_encode_batch_chunk, host in / host out: a dict of numpy arrays (encode_batch_window's, cut_level uint8 [n_windows],
        chunk_bytes uint32 [n_windows, 2] or None, level_counts uint64 [6]) and the counts n_windows, n_split."""
        o = _chunk_opts(max_length, min_length, overlap, multiple_of, pad_id, 0, 0, levels, flags)
        return self._encode_host(ChunkResult, o, flags, data, offs, add_bos, add_eos, validate_utf8)[1]

    def last_chunk_ms(self):
        """tk_last_chunk_ms: GPU milliseconds of the last chunk pass -- (levels kernel, the two walks and the scan, fill kernel)."""
        ms = (ctypes.c_float * 3)()
        _need("tk_last_chunk_ms")(self._h, ctypes.byref(ms))
        return tuple(float(x) for x in ms)

    def pair_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_parts, n_ids, max_length, strategy=PAIR_LONGEST_FIRST, stride=0, max_fixed=0,
                             multiple_of=0, pad_id=0, head=(), sep=(), tail=(), flags=0, d_spans_ptr=0, stream=0):
        """tk_pair_from_ids_device: the ragged ids of 2P parts resident in HBM (part 2p the first text, part 2p + 1 the second) ->
        rows head + A + sep + B + tail [n_windows, row_len] (+ mask, type_ids, sequence_ids, spans from d_spans_ptr by flag, lengths,
        window_pair, window_start, second_start, pair_windows); the definition is in include/tekken_hip.h.  Returns a PairResult
        (context-owned device buffers, apart from every other output)."""
        o = _pair_opts(max_length, strategy, stride, max_fixed, multiple_of, pad_id, head, sep, tail, flags)
        return self._from_ids_device(PairResult, o, flags, d_ids_ptr, d_id_offs_ptr, n_parts, n_ids, (d_spans_ptr,), stream)

    def encode_pairs_device(self, d_bytes_ptr, d_offs_ptr, n_parts, n_bytes, max_length, strategy=PAIR_LONGEST_FIRST, stride=0, max_fixed=0,
                            multiple_of=0, pad_id=0, head=(), sep=(), tail=(), flags=0, checks=0, stream=0):
        """tk_encode_pairs_device: the 2P part texts encoded one by one without BOS / EOS (+ the spans pass with PAIR_SPANS) + the
        pair pass on the same stream.  Returns (d_ids_ptr, d_out_offs_ptr, n_ids, PairResult), all context-owned."""
        o = _pair_opts(max_length, strategy, stride, max_fixed, multiple_of, pad_id, head, sep, tail, flags)
        st, d_ids, d_oo, n = _Pair(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        self._call("tk_encode_pairs_device", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr), n_parts, n_bytes, int(checks),
                   ctypes.byref(o), ctypes.c_void_p(stream), ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n), ctypes.byref(st))
        return d_ids.value, d_oo.value, int(n.value), PairResult(st, int(flags))

    def encode_pairs(self, data, offs, max_length, strategy=PAIR_LONGEST_FIRST, stride=0, max_fixed=0, multiple_of=0, pad_id=0, head=(),
                     sep=(), tail=(), flags=0, validate_utf8=False):
        """tk_encode_pairs, host in / host out: a dict of numpy arrays by output name (PairResult.OUTPUTS; an unselected one: None)
        and the counts n_windows, n_truncated, n_split, n_fixed_cut."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        o, st = _pair_opts(max_length, strategy, stride, max_fixed, multiple_of, pad_id, head, sep, tail, flags), _Pair()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        self._call("tk_encode_pairs", _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(validate_utf8), ctypes.byref(o),
                   ctypes.byref(st))
        return PairResult.take(st, int(flags))[1]

    def join_from_ids_device(self, d_ids_ptr, d_id_offs_ptr, n_parts, n_ids, d_part_ctrl_ptr, d_part_flags_ptr, d_conv_offs_ptr, n_convs,
                             ignore_index=-100, flags=0, checks=0, stream=0):
        """tk_join_from_ids_device: ragged ids of parts resident in HBM (+ part_ctrl uint32[n_parts], part_flags uint32[n_parts] or
        0, conv_offsets uint64[n_convs + 1], all raw device pointers) -> the joined stream; the definition is in
        include/tekken_hip.h.  checks: 0 | CHECK_PARTS.  Returns a JoinResult (context-owned device buffers, apart from every
        other output)."""
        o, j = _JoinOpts(int(ignore_index), int(flags)), _Join()
        self._call("tk_join_from_ids_device", ctypes.c_void_p(d_ids_ptr or None), ctypes.c_void_p(d_id_offs_ptr or None), n_parts, n_ids,
                   ctypes.c_void_p(d_part_ctrl_ptr or None), ctypes.c_void_p(d_part_flags_ptr or None),
                   ctypes.c_void_p(d_conv_offs_ptr or None), n_convs, int(checks), ctypes.byref(o),
                   ctypes.c_void_p(stream), ctypes.byref(j))
        return JoinResult(j)

    def encode_parts_device_join(self, d_bytes_ptr, d_offs_ptr, n_parts, n_bytes, d_part_ctrl_ptr, d_part_flags_ptr, d_conv_offs_ptr, n_convs,
                                 ignore_index=-100, flags=0, checks=0, stream=0):
        """tk_encode_parts_device_join: the part texts encoded one by one without BOS / EOS + the join on the same stream.
        checks may mix CHECK_OFFSETS / CHECK_UTF8 with CHECK_PARTS.  Returns a JoinResult."""
        o, j = _JoinOpts(int(ignore_index), int(flags)), _Join()
        self._call("tk_encode_parts_device_join", ctypes.c_void_p(d_bytes_ptr or None), ctypes.c_void_p(d_offs_ptr or None), n_parts, n_bytes,
                   ctypes.c_void_p(d_part_ctrl_ptr or None), ctypes.c_void_p(d_part_flags_ptr or None),
                   ctypes.c_void_p(d_conv_offs_ptr or None), n_convs, int(checks), ctypes.byref(o),
                   ctypes.c_void_p(stream), ctypes.byref(j))
        return JoinResult(j)

    def encode_parts_join(self, data, offs, part_ctrl, part_flags, conv_offs, ignore_index=-100, flags=0, validate_utf8=False):
        """tk_encode_parts_join, host in / host out: a dict of numpy arrays (ids uint32 [N], offsets uint64 [n_convs + 1], labels
        int32 [N], part_index uint32 [N]; an unselected one: None) and the counts n_ids, n_ctrl, n_labelled.  part_flags may be
        None (all zero)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ctrl = np.ascontiguousarray(part_ctrl, dtype=np.uint32)
        pf = None if part_flags is None else np.ascontiguousarray(part_flags, dtype=np.uint32)
        conv = np.ascontiguousarray(conv_offs, dtype=np.uint64)
        n_parts = len(offs) - 1
        if len(ctrl) != n_parts or (pf is not None and len(pf) != n_parts) or len(conv) < 1:
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_parts_join: one part_ctrl / part_flags entry per part, n_convs + 1 conv_offsets")
        o, j = _JoinOpts(int(ignore_index), int(flags)), _Join()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        cbuf = ctrl if n_parts else np.zeros(1, np.uint32)
        fbuf = None if pf is None else pf if n_parts else np.zeros(1, np.uint32)
        self._call("tk_encode_parts_join", _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), n_parts, _p(cbuf, ctypes.c_uint32),
                   None if fbuf is None else _p(fbuf, ctypes.c_uint32), _p(conv, ctypes.c_uint64), len(conv) - 1,
                   int(validate_utf8), ctypes.byref(o), ctypes.byref(j))
        return JoinResult.take(j)[1]

    def ragged_from_dense_device(self, d_dense_ptr, n_docs, row_len, flags=0, d_lengths_ptr=0, pad_id=0, stream=0):
        """tk_ragged_from_dense_device: dense rows in HBM (int32, or int64 with DENSE_I64; DENSE_PAD_LEFT) -> (d_ids_ptr,
        d_id_offs_ptr, n_ids), context-owned and valid through a following decode_batch_device.  d_lengths_ptr (uint32[n_docs]) 0:
        the run of pad_id at the padded end of every row is trimmed."""
        d_ids, d_oo, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        self._call("tk_ragged_from_dense_device", ctypes.c_void_p(d_dense_ptr or None), n_docs, row_len, int(flags),
                   ctypes.c_void_p(d_lengths_ptr or None), int(pad_id), ctypes.c_void_p(stream),
                   ctypes.byref(d_ids), ctypes.byref(d_oo), ctypes.byref(n))
        return d_ids.value, d_oo.value, int(n.value)

    def encode_batch_device_views(self, d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos=True, add_eos=True, stream=0):
        """Same, returning (ids view as int32[n_ids], offsets view as int64[n_docs+1])."""
        p_ids, p_oo, n = self.encode_batch_device(d_bytes_ptr, d_offs_ptr, n_docs, n_bytes, add_bos, add_eos, stream)
        return DeviceView(p_ids, n, "<i4"), DeviceView(p_oo, n_docs + 1, "<i8")

    def pack_ids18_device(self, d_ids_ptr, n_ids, d_packed_ptr, stream=0):
        """ids (uint32, device) -> 18-bit wire format (ids18_bytes(n_ids) bytes, device); raises if an id needs more bits."""
        rc = lib().tk_pack_ids18_device(self._h, ctypes.c_void_p(d_ids_ptr), n_ids, ctypes.c_void_p(d_packed_ptr), ctypes.c_void_p(stream))
        if rc != TK_OK:
            raise self._err(rc)

    def unpack_ids18_device(self, d_packed_ptr, n_ids, d_ids_ptr, stream=0):
        """18-bit wire format -> ids (uint32, device); enqueued on `stream`, not waited for."""
        rc = lib().tk_unpack_ids18_device(self._h, ctypes.c_void_p(d_packed_ptr), n_ids, ctypes.c_void_p(d_ids_ptr), ctypes.c_void_p(stream))
        if rc != TK_OK:
            raise self._err(rc)

    def set_pattern(self, mode):
        """0 = the reference's hard-coded pattern (default), 1 = the JSON pattern of Mistral's tekken.json (opt-in, row f-3)."""
        rc = lib().tk_ctx_set_pattern(self._h, int(mode))
        if rc != TK_OK:
            raise self._err(rc)

    def set_special_tokens(self, strings):
        """Special-token strings by position (needed by decode with SpecialTokenPolicy.Keep)."""
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in strings]
        offs = np.zeros(len(raw) + 1, np.uint32)
        offs[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64).astype(np.uint32)
        blob = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy()
        rc = lib().tk_ctx_set_special_tokens(self._h, _p(blob, ctypes.c_uint8), _p(offs, ctypes.c_uint32), len(raw))
        if rc != TK_OK:
            raise self._err(rc)

    @staticmethod
    def _lossy(errors):
        if errors not in ("strict", "replace"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "errors must be 'strict' or 'replace', not %r" % (errors,))
        return errors == "replace"

    def decode_batch(self, ids, offs, policy=SpecialTokenPolicy.Ignore, errors="strict"):
        """Batch Tekkenizer::decode on the GPU: (uint32 ids, uint64 offsets[D+1]) -> (uint8 bytes, uint64 offsets[D+1]).
        errors="replace": a run that is not valid UTF-8 is decoded as python's errors="replace" does it (U+FFFD; tk_decode_batch_lossy)
        instead of failing the call; self.n_replaced then holds the U+FFFD written, self.first_bad_doc the first document with one
        (None: none)."""
        lossy = self._lossy(errors)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res = _TextResult()
        bad = ctypes.c_uint64(0)
        ibuf = ids if len(ids) else np.zeros(1, np.uint32)
        if lossy:
            nrep, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rc = _need("tk_decode_batch_lossy")(self._h, _p(ibuf, ctypes.c_uint32), _p(offs, ctypes.c_uint64), len(offs) - 1, int(policy),
                                                ctypes.byref(res), ctypes.byref(bad), ctypes.byref(nrep), ctypes.byref(first))
        else:
            rc = lib().tk_decode_batch(self._h, _p(ibuf, ctypes.c_uint32), _p(offs, ctypes.c_uint64), len(offs) - 1, int(policy),
                                       ctypes.byref(res), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_doc = int(bad.value)
            raise e
        if lossy:
            self._set_lossy(nrep, first)
        n, D = int(res.n_bytes), int(res.n_docs)
        data = np.ctypeslib.as_array(res.bytes, shape=(max(n, 1),))[:n].copy()
        oo = np.ctypeslib.as_array(res.offsets, shape=(D + 1,)).copy()
        lib().tk_free_text_result(ctypes.byref(res))
        return data, oo

    n_replaced = 0           # of the last decode with errors="replace" on this engine: U+FFFD written ...
    first_bad_doc = None     # ... and the first document with one

    def _set_lossy(self, nrep, first):
        self.n_replaced = int(nrep.value)
        self.first_bad_doc = None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value)

    def decode_docs(self, id_lists, policy=SpecialTokenPolicy.Ignore, errors="strict"):
        offs = np.zeros(len(id_lists) + 1, np.uint64)
        if id_lists:
            offs[1:] = np.cumsum([len(x) for x in id_lists], dtype=np.uint64)
        ids = np.array([i for x in id_lists for i in x], dtype=np.uint32)
        data, oo = self.decode_batch(ids, offs, policy, errors)
        raw = data.tobytes()
        return [raw[int(oo[d]):int(oo[d + 1])] for d in range(len(id_lists))]

    def decode_batch_device(self, d_ids_ptr, d_offs_ptr, n_docs, n_ids, policy=SpecialTokenPolicy.Ignore, stream=0, errors="strict"):
        """ids resident in HBM -> (bytes view uint8[n_bytes], offsets view int64[n_docs+1]) context-owned.  errors="replace" as in
        decode_batch (tk_decode_batch_device_lossy): where every run is valid the views are the strict entry's own buffers."""
        lossy = self._lossy(errors)
        d_b, d_o, n, bad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        if lossy:
            nrep, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rc = _need("tk_decode_batch_device_lossy")(self._h, ctypes.c_void_p(d_ids_ptr), ctypes.c_void_p(d_offs_ptr), n_docs, n_ids,
                                                       int(policy), ctypes.c_void_p(stream), ctypes.byref(d_b), ctypes.byref(d_o),
                                                       ctypes.byref(n), ctypes.byref(bad), ctypes.byref(nrep), ctypes.byref(first))
        else:
            rc = lib().tk_decode_batch_device(self._h, ctypes.c_void_p(d_ids_ptr), ctypes.c_void_p(d_offs_ptr), n_docs, n_ids,
                                              int(policy), ctypes.c_void_p(stream), ctypes.byref(d_b), ctypes.byref(d_o),
                                              ctypes.byref(n), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_doc = int(bad.value)
            raise e
        if lossy:
            self._set_lossy(nrep, first)
        return DeviceView(d_b.value, int(n.value), "|u1"), DeviceView(d_o.value, n_docs + 1, "<i8")

    def last_decode_lossy(self):
        """tk_last_decode_lossy_ms / _stats: GPU time of the strict pipeline and of the repair pass of the last lossy batch decode
        on this context, its counters, and the kernels launched behind the strict pipeline (0: the fast path)."""
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        x, y, z = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _need("tk_last_decode_lossy_ms")(self._h, ctypes.byref(a), ctypes.byref(b))
        _need("tk_last_decode_lossy_stats")(self._h, ctypes.byref(x), ctypes.byref(y), ctypes.byref(z))
        return {"strict_ms": a.value, "repair_ms": b.value, "n_replaced": int(x.value), "n_bad_docs": int(y.value),
                "repair_launches": int(z.value)}

    def decode_stream_step_device(self, d_state_ptr, d_ids_ptr, d_offs_ptr, n_seqs, n_ids, policy=SpecialTokenPolicy.Ignore, flags=0,
                                  stream=0):
        """tk_decode_stream_step_device: one step of streaming decode over states, ids and offsets in HBM -> (bytes view, offsets
        view int64[n_seqs + 1]), context-owned.  An error carries .bad_seq and leaves the states untouched."""
        d_b, d_o, n, bad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = _need("tk_decode_stream_step_device")(self._h, ctypes.c_void_p(d_state_ptr), ctypes.c_void_p(d_ids_ptr),
                                                   ctypes.c_void_p(d_offs_ptr), n_seqs, n_ids, int(policy), int(flags),
                                                   ctypes.c_void_p(stream), ctypes.byref(d_b), ctypes.byref(d_o), ctypes.byref(n),
                                                   ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_seq = e.bad_doc = int(bad.value)
            raise e
        return DeviceView(d_b.value, int(n.value), "|u1"), DeviceView(d_o.value, n_seqs + 1, "<i8")

    def decode_stream_step(self, state, id_lists, policy=SpecialTokenPolicy.Ignore, flags=0):
        """tk_decode_stream_step: state (uint32[n_seqs] numpy, rewritten in place) and the new ids of every sequence in host
        memory -> list of bytes."""
        if state.dtype != np.uint32 or not state.flags["C_CONTIGUOUS"] or len(state) != len(id_lists):
            raise TokenizerError(TK_ERR_INVALID_ARG, "decode_stream_step: state must be a contiguous uint32 array, one word per sequence")
        offs = np.zeros(len(id_lists) + 1, np.uint64)
        if id_lists:
            offs[1:] = np.cumsum([len(x) for x in id_lists], dtype=np.uint64)
        ids = np.array([i for x in id_lists for i in x] or [0], dtype=np.uint32)
        sbuf = state if len(state) else np.zeros(1, np.uint32)
        res = _TextResult()
        bad = ctypes.c_uint64(0)
        rc = _need("tk_decode_stream_step")(self._h, _p(sbuf, ctypes.c_uint32), _p(ids, ctypes.c_uint32), _p(offs, ctypes.c_uint64),
                                            len(id_lists), int(policy), int(flags), ctypes.byref(res), ctypes.byref(bad))
        if rc != TK_OK:
            e = self._err(rc)
            e.bad_seq = e.bad_doc = int(bad.value)
            raise e
        n = int(res.n_bytes)
        raw = np.ctypeslib.as_array(res.bytes, shape=(max(n, 1),))[:n].tobytes()
        oo = np.ctypeslib.as_array(res.offsets, shape=(len(id_lists) + 1,)).copy()
        lib().tk_free_text_result(ctypes.byref(res))
        return [raw[int(oo[d]):int(oo[d + 1])] for d in range(len(id_lists))]

    def decode_stream(self, n_seqs, policy=SpecialTokenPolicy.Ignore, text=False):
        """A DecodeStream over n_seqs running sequences (text: its steps return str, not bytes)."""
        return DecodeStream(self, n_seqs, policy, text)

    def last_timing(self):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        lib().tk_last_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        return {"pipeline_ms": a.value, "encode_kernel_ms": b.value, "merge_ms": float(lib().tk_last_merge_ms(self._h)) if hasattr(lib(), "tk_last_merge_ms") else 0.0}

    def last_stats(self):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        lib().tk_last_stats(self._h, ctypes.byref(a), ctypes.byref(b))
        return {"long_docs": int(a.value), "handed_back": int(b.value)}

    def split_docs(self, docs):
        """Piece-start offsets per document (vocab-free split, debug / parity entry)."""
        data, offs = pack_docs(docs)
        n = int(offs[-1])
        out = np.zeros(max(n, 1), np.uint8)
        dbuf = data if n else np.zeros(1, np.uint8)
        rc = lib().tk_split_batch(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(docs),
                                  _p(out, ctypes.c_uint8))
        if rc != TK_OK:
            raise self._err(rc)
        res = []
        for d in range(len(docs)):
            a, b = int(offs[d]), int(offs[d + 1])
            res.append(np.nonzero(out[a:b])[0].tolist())
        return res


class Node:
    """tk_node_*: every listed GPU behind one call -- documents sharded whole by bytes, one RCCL gather of the id buffers to
    devices[0] (include/tekken_hip.h, csrc/tk_node.cpp).  One process; the path a Rust / C host calls."""

    def __init__(self, token_bytes, num_special, bos_id, eos_id, devices=(0,)):
        toks = list(token_bytes)
        offs = np.zeros(len(toks) + 1, np.uint32)
        offs[1:] = np.cumsum([len(t) for t in toks], dtype=np.uint64).astype(np.uint32)
        blob = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8)
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = lib().tk_node_create(_p(blob, ctypes.c_uint8), _p(offs, ctypes.c_uint32), len(toks), num_special, bos_id, eos_id,
                                  devs, len(devices), ctypes.byref(h))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_node_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().tk_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def n_devices(self):
        return lib().tk_node_n_devices(self._h)

    def encode_batch(self, data, offs, add_bos=True, add_eos=True):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        res = _Result()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = lib().tk_node_encode_batch(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                                        int(add_eos), ctypes.byref(res))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_node_last_error(self._h).decode())
        return _take_result(res)

    def encode_batch_into(self, data, offs, ids_out, offs_out, add_bos=True, add_eos=True):
        """tk_node_encode_batch_pinned: caller-owned buffers (host_empty: pinned -- nothing allocated or pinned per call).  Returns the
        number of ids written into ids_out; offs_out[: n_docs + 1] holds the id offsets."""
        assert data.dtype == np.uint8 and offs.dtype == np.uint64 and ids_out.dtype == np.uint32 and offs_out.dtype == np.uint64
        # (the C side writes n_docs + 1 offsets and takes no capacity for them; every buffer is handed over as one flat block)
        assert len(offs_out) >= len(offs), "offs_out holds %d offsets, the call writes %d" % (len(offs_out), len(offs))
        for a in (data, offs, ids_out, offs_out):
            assert a.flags["C_CONTIGUOUS"], "tk_node_encode_batch_pinned wants contiguous buffers"
        n = ctypes.c_uint64(0)
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = lib().tk_node_encode_batch_pinned(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(offs) - 1, int(add_bos),
                                               int(add_eos), _p(ids_out, ctypes.c_uint32), len(ids_out), _p(offs_out, ctypes.c_uint64), ctypes.byref(n))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_node_last_error(self._h).decode())
        return int(n.value)

    def last_timing(self):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        lib().tk_node_last_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        return {"kernels_ms_max": a.value, "gather_ms": b.value}

    def last_shards(self):
        """(text bytes, ids) of every device's run in the last batch (tk_node_last_shards)."""
        n = self.n_devices()
        b, i = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        lib().tk_node_last_shards(self._h, b, i, n)
        return list(b), list(i)


class _Pinned:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            lib().tk_host_free(ctypes.c_void_p(self.ptr))
        except Exception:
            pass


def ids18_bytes(n_ids):
    return int(lib().tk_ids18_bytes(int(n_ids)))


def host_empty(n, dtype):
    """numpy array of n elements in PINNED host memory (tk_host_alloc): the buffers tk_encode_batch_pipelined wants."""
    dt = np.dtype(dtype)
    nbytes = max(int(n) * dt.itemsize, 1)
    ptr = lib().tk_host_alloc(nbytes)
    if not ptr:
        raise MemoryError("tk_host_alloc(%d) failed" % nbytes)
    owner = _Pinned(ptr)
    raw = (ctypes.c_uint8 * nbytes).from_address(ptr)
    raw._tk_owner = owner                  # the array keeps `raw` alive (its base), `raw` keeps the allocation alive
    return np.frombuffer(raw, dtype=dt, count=int(n))


class Tekkenizer:
    """Mirror of tekken::tekkenizer::Tekkenizer for the text path (reference src/tekkenizer.rs)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_file(cls, path, device=0):
        """Tekkenizer::from_file (src/tekkenizer.rs:222-248).  device=-1: host-only (no encode)."""
        h = ctypes.c_void_p()
        rc = lib().tk_tokenizer_from_file(os.fsencode(path), device, ctypes.byref(h))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_tokenizer_last_error(None).decode())
        return cls(h)

    @classmethod
    def from_json(cls, text, device=0):
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        h = ctypes.c_void_p()
        rc = lib().tk_tokenizer_from_json(raw, len(raw), device, ctypes.byref(h))
        if rc != TK_OK:
            raise TokenizerError(rc, lib().tk_tokenizer_last_error(None).decode())
        return cls(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().tk_tokenizer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc):
        return TokenizerError(rc, lib().tk_tokenizer_last_error(self._h).decode())

    # ---- audio (reference src/tekkenizer.rs:697-760) ----
    @property
    def has_audio_support(self):
        return bool(_need("tk_tokenizer_has_audio")(self._h))

    @property
    def audio_config(self):
        """The AudioConfig of the loaded tekken.json as a dict (chunk_length_s None where it has none); None without audio."""
        if not self.has_audio_support:
            return None
        st = _AudioConfig()
        rc = _need("tk_tokenizer_audio_config")(self._h, ctypes.byref(st))
        if rc != TK_OK:
            raise self._err(rc)
        return {"sampling_rate": int(st.sampling_rate), "frame_rate": float(st.frame_rate), "num_mel_bins": int(st.num_mel_bins),
                "hop_length": int(st.hop_length), "window_size": int(st.window_size),
                "chunk_length_s": float(st.chunk_length_s) if st.has_chunk_length else None}

    def _audio_ids(self):
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = _need("tk_tokenizer_audio_ids")(self._h, ctypes.byref(a), ctypes.byref(b))
        if rc != TK_OK:
            raise self._err(rc)
        return a.value, b.value

    @property
    def audio_token_id(self):
        return self._audio_ids()[0]

    @property
    def begin_audio_token_id(self):
        return self._audio_ids()[1]

    def _audio_count(self, audio):
        """(ids, padded samples) of one clip: tk_tokenizer_encode_audio."""
        ids = ctypes.POINTER(ctypes.c_uint32)()
        n, padded = ctypes.c_size_t(0), ctypes.c_uint64(0)
        rc = _need("tk_tokenizer_encode_audio")(self._h, len(audio.audio_array), int(audio.sampling_rate), ctypes.byref(ids), ctypes.byref(n),
                                                ctypes.byref(padded))
        if rc != TK_OK:
            raise self._err(rc)
        out = np.ctypeslib.as_array(ids, shape=(n.value,)).copy()
        lib().tk_free_ids(ids)
        return out, int(padded.value)

    def encode_audio(self, audio):
        """Tekkenizer::encode_audio (src/tekkenizer.rs:728-735): (ids, the padded clip) -- [BEGIN_AUDIO] + [AUDIO] * N."""
        ids, padded = self._audio_count(audio)
        x = np.zeros(padded, np.float32)
        x[:len(audio.audio_array)] = audio.audio_array
        return ids.tolist(), Audio(x, audio.sampling_rate)

    def _audio_features(self, eng, audios):
        """The clips go up once; -> (LogmelResult, the device samples, kept alive with it)."""
        import torch
        lens = [len(a.audio_array) for a in audios]
        offs = np.zeros(len(audios) + 1, np.int64)
        if audios:
            offs[1:] = np.cumsum(lens)
        flat = np.concatenate([a.audio_array for a in audios]) if int(offs[-1]) else np.zeros(1, np.float32)
        d_x, d_o = torch.from_numpy(flat).cuda(), torch.from_numpy(offs).cuda()
        r = eng.audio_logmel_device(d_x.data_ptr(), d_o.data_ptr(), len(audios), int(offs[-1]), checks=CHECK_OFFSETS,
                                    stream=torch.cuda.current_stream().cuda_stream)
        return r

    def _feature_tensors(self, r, copy=True):
        """features of a LogmelResult: [S, M, T] under a chunked config, else a list of [M, T_s] views of one tensor."""
        import torch
        v = r.views()
        flat = _torch_wrap(v[0], copy)
        fo = _torch_wrap(v[1], True).cpu().numpy().astype(np.uint64)
        cs = _torch_wrap(v[2], True).cpu().numpy().astype(np.uint64)
        M = r.n_mel
        if self.audio_config["chunk_length_s"] is not None:
            T = int(fo[1] - fo[0]) if r.n_segments else 0
            feats = flat.reshape(r.n_segments, M, T) if r.n_segments else torch.empty((0, M, 0), dtype=torch.float32, device="cuda")
        else:
            feats = [flat[M * int(fo[k]):M * int(fo[k + 1])].reshape(M, int(fo[k + 1] - fo[k])) for k in range(r.n_segments)]
        return feats, fo, cs

    def encode_audio_batch(self, audios, return_features=True, copy=True):
        """encode_audio over a batch of clips -> {"ids": uint32 [N] the clips' ids back to back, "offsets": uint64 [n + 1],
        "tokens_per_clip": the [AUDIO] count of each, "features": the log-mel features on the tokenizer's GPU ([S, M, T] float32
        under a chunked config, else a list of [M, T_i] views; None without return_features), "frame_off": uint64 [S + 1],
        "clip_seg": uint64 [n + 1]}.  The definition of the features is in include/tekken_hip.h."""
        per = [self._audio_count(a)[0] for a in audios]
        offs = np.zeros(len(audios) + 1, np.uint64)
        if audios:
            offs[1:] = np.cumsum([len(x) for x in per], dtype=np.uint64)
        out = {"ids": np.concatenate(per).astype(np.uint32) if per else np.zeros(0, np.uint32), "offsets": offs,
               "tokens_per_clip": np.array([len(x) - 1 for x in per], np.uint64), "features": None, "frame_off": None, "clip_seg": None}
        if return_features:
            r = self._audio_features(self._device_engine(), audios)
            out["features"], out["frame_off"], out["clip_seg"] = self._feature_tensors(r, copy)
        return out

    def set_honour_pattern(self, honour=True):
        """Opt-in (row f-3): use the `pattern` of the loaded tekken.json instead of ignoring it like the reference does."""
        rc = lib().tk_tokenizer_set_honour_pattern(self._h, int(bool(honour)))
        if rc != TK_OK:
            raise self._err(rc)

    def encode(self, text, add_bos=False, add_eos=False):
        """Tekkenizer::encode (src/tekkenizer.rs:378-405)."""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        ids = ctypes.POINTER(ctypes.c_uint32)()
        n = ctypes.c_size_t(0)
        rc = lib().tk_tokenizer_encode(self._h, raw, len(raw), int(add_bos), int(add_eos), ctypes.byref(ids),
                                       ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        out = [ids[i] for i in range(n.value)]
        lib().tk_free_ids(ids)
        return out

    def _unit(self, offsets_unit):
        if offsets_unit not in _UNITS:
            raise TokenizerError(TK_ERR_INVALID_ARG, "offsets_unit %r is none of 'byte', 'char', 'utf16'" % (offsets_unit,))
        return _UNITS[offsets_unit]

    def encode_with_offsets(self, text, add_bos=False, add_eos=False, offsets_unit="byte"):
        """Tekkenizer::encode + the span of every id: (ids, [(start, end), ...]).  offsets_unit "byte": offsets in BYTES of the
        UTF-8 text (a byte-fallback token can end inside a character; BOS / EOS get zero-length spans at 0 / len); "char": code
        points, the indices of a Python str; "utf16": UTF-16 units.  In the last two a token that begins or ends inside a
        character covers that whole character (the definition is in include/tekken_hip.h), and the spans come from the units pass
        on the tokenizer's GPU."""
        if self._unit(offsets_unit) != UNIT_BYTE:
            return self.encode_batch_with_offsets([text], add_bos, add_eos, offsets_unit=offsets_unit)[0]
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        ids = ctypes.POINTER(ctypes.c_uint32)()
        sp = ctypes.POINTER(ctypes.c_uint32)()
        n = ctypes.c_size_t(0)
        rc = _need("tk_tokenizer_encode_with_spans")(self._h, raw, len(raw), int(add_bos), int(add_eos), ctypes.byref(ids),
                                                     ctypes.byref(sp), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        out = [ids[i] for i in range(n.value)]
        spans = [(sp[2 * i], sp[2 * i + 1]) for i in range(n.value)]
        lib().tk_free_ids(ids)
        lib().tk_free_ids(sp)
        return out, spans

    def encode_batch_with_offsets(self, docs, add_bos=False, add_eos=False, checks=0, offsets_unit="byte"):
        """Batch form on the tokenizer's engine context (tk_encode_batch_spans; with offsets_unit "char" / "utf16"
        tk_encode_batch_spans_units, which takes no SPANS_CHECK_*): [(ids, [(start, end), ...]) per document]."""
        eng = self.engine()
        if eng is None:
            raise TokenizerError(TK_ERR_NO_DEVICE, "tokenizer was created without a device (host-only object)")
        unit = self._unit(offsets_unit)
        if unit != UNIT_BYTE and checks:
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_with_offsets: the spans checks belong to the byte pass (offsets_unit='byte')")
        if add_bos:
            self.bos_id()      # (TokenNotFound when the vocabulary has no such control token, as encode)
        if add_eos:
            self.eos_id()
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        if unit != UNIT_BYTE:
            ids, oo, spans = eng.encode_batch_spans_units(data, offs, add_bos, add_eos, unit=unit)
        else:
            ids, oo, spans = eng.encode_batch_spans(data, offs, add_bos, add_eos, checks=checks)
        return [(ids[int(oo[d]):int(oo[d + 1])].tolist(), [tuple(x) for x in spans[int(oo[d]):int(oo[d + 1])].tolist()])
                for d in range(len(docs))]

    def _device_engine(self):
        eng = self.engine()
        if eng is None:
            raise TokenizerError(TK_ERR_NO_DEVICE, "tokenizer was created without a device (host-only object)")
        return eng

    def _batch_prelude(self, method, docs, add_bos, add_eos, pad_id, values_ok, values, ranges=None, upload=True):
        """What the batch methods do behind _device_engine(), in the order their errors are raised in: values_ok, the method's check
        of its keyword values (values: how its message names them); the BOS / EOS probe; the pad id (None: self.pad_id());
        ranges, {name: number} that go into uint32 options; the documents packed and -- upload -- on the GPU.
        -> (pad, data, offs, uint8 tensor, int64 tensor, stream), the last three None without upload."""
        if not values_ok:
            raise TokenizerError(TK_ERR_INVALID_ARG, "%s: unknown %s value" % (method, values))
        if add_bos:
            self.bos_id()      # (TokenNotFound when the vocabulary has no such control token, as encode)
        if add_eos:
            self.eos_id()
        pad = self.pad_id() if pad_id is None else int(pad_id)
        if not all(0 <= int(x) < 2 ** 32 for x in (ranges or {}).values()):
            raise TokenizerError(TK_ERR_INVALID_ARG, "%s: %s" % (method, ", ".join("%s %r" % kv for kv in ranges.items())))
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        return (pad, data, offs) + (_upload(data, offs) if upload else (None, None, None))

    def encode_batch_padded(self, docs, add_bos=False, add_eos=False, max_length=None, padding="longest", truncation_side="right",
                            padding_side="right", pad_to_multiple_of=None, pad_id=None, dtype="int64", return_mask=True,
                            return_tensors="pt", copy=True):
        """Model-ready batch (tk_encode_batch_device_dense / tk_encode_batch_dense; the definition is in include/tekken_hip.h):
        {"input_ids": [B, L] of `dtype` ("int64" | "int32"), "attention_mask": uint8 [B, L] (None without return_mask),
        "lengths": int32 [B] kept ids per row, "n_truncated": int}.  Rows longer than max_length are cut on truncation_side with
        BOS / EOS kept; padding "longest": L = the longest kept row, "max_length": L = max_length; then rounded up to
        pad_to_multiple_of.  pad_id None: self.pad_id().  return_tensors "pt": torch tensors on the tokenizer's GPU (the text goes
        up once; copy=False returns views of context-owned buffers, valid until the next call on this tokenizer); "np": numpy."""
        eng = self._device_engine()
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_padded", docs, add_bos, add_eos, pad_id,
            padding in ("longest", "max_length") and truncation_side in ("left", "right") and padding_side in ("left", "right")
            and dtype in ("int64", "int32") and return_tensors in ("pt", "np"), "padding / side / dtype / return_tensors",
            upload=return_tensors != "np")
        flags = (DENSE_FIXED if padding == "max_length" else 0) | (DENSE_TRUNC_LEFT if truncation_side == "left" else 0) \
            | (DENSE_PAD_LEFT if padding_side == "left" else 0) | (DENSE_I64 if dtype == "int64" else 0) | (DENSE_MASK if return_mask else 0)
        if return_tensors == "np":
            dense, mask, lengths = eng.encode_batch_dense(data, offs, add_bos, add_eos, False, max_length, pad_to_multiple_of, pad, flags)
            return {"input_ids": dense, "attention_mask": mask, "lengths": lengths.astype(np.int32), "n_truncated": eng.last_n_truncated}
        _, _, _, res = eng.encode_batch_device_dense(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos, add_eos,
                                                     max_length, pad_to_multiple_of, pad, flags, CHECK_OFFSETS, stream)
        t = res.tensors(copy)
        return {"input_ids": t["ids"], "attention_mask": t["mask"], "lengths": t["lengths"], "n_truncated": t["n_truncated"]}

    def encode_with_words(self, text, add_bos=False, add_eos=False):
        """Tekkenizer::encode + the word of every id, HF's word_ids(): (ids, word_ids) with None for a special id.  A word is a
        piece of the pre-tokenization split (the definition is in include/tekken_hip.h); a batch of one document."""
        got = self.encode_batch_with_words([text], add_bos, add_eos, return_word_first=False)
        return got["ids"].tolist(), [None if w < 0 else w for w in got["word_ids"].tolist()]

    def encode_batch_with_words(self, docs, add_bos=False, add_eos=False, return_word_first=True, checks=0, return_tensors="np", copy=True):
        """Batch form on the tokenizer's engine context (tk_encode_batch_words / tk_encode_batch_device_words): {"ids", "id_offsets"
        (int64 [D + 1]), "word_ids" (int32, -1 for a special id), "doc_words" (int64 [D + 1]), "word_first" (the
        document-relative first id of every word, None without return_word_first), "n_words"}.  checks: WORDS_CHECK_ALIGNED.
        return_tensors "np": numpy; "pt": torch tensors on the tokenizer's GPU (copy=False: views of context-owned buffers, valid
        until the next call on this tokenizer)."""
        eng = self._device_engine()
        _, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_with_words", docs, add_bos, add_eos, 0, return_tensors in ("pt", "np"), "return_tensors", upload=return_tensors != "np")
        flags = WORDS_FIRST if return_word_first else 0
        if return_tensors == "np":
            ids, oo, w = eng.encode_batch_words(data, offs, add_bos, add_eos, False, flags, checks)
            return {"ids": ids, "id_offsets": oo.astype(np.int64), "word_ids": w["word_ids"].view(np.int32), "doc_words": w["doc_words"].astype(np.int64),
                    "word_first": w["word_first"], "n_words": w["n_words"]}
        d_ids, d_oo, n, res = eng.encode_batch_device_words(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos, add_eos, flags,
                                                           CHECK_OFFSETS | checks, stream)
        out = res.tensors(copy)
        out["ids"] = _torch_wrap(DeviceView(d_ids, n, "<i4"), copy)
        out["id_offsets"] = _torch_wrap(DeviceView(d_oo, len(docs) + 1, "<i8"), copy)
        return out

    def encode_batch_padded_words(self, docs, add_bos=False, add_eos=False, max_length=None, padding="longest", truncation_side="right",
                                  padding_side="right", pad_to_multiple_of=None, pad_id=None, dtype="int64", return_mask=True,
                                  return_tensors="pt", copy=True):
        """encode_batch_padded plus "word_ids" [B, L] of `dtype`: the word of every kept id, -1 for a special id and under the
        padding.  One encode and one words pass; then the dense pass over the ids and over word_ids, one after the other with the
        same options (word_ids as int32 elements padded with WORD_NONE, widened here -- which sign-extends; BOS / EOS survive
        truncation in both).  return_tensors "pt": torch tensors on the tokenizer's GPU; "np": numpy copies of them."""
        eng = self._device_engine()
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_padded_words", docs, add_bos, add_eos, pad_id,
            padding in ("longest", "max_length") and truncation_side in ("left", "right") and padding_side in ("left", "right")
            and dtype in ("int64", "int32") and return_tensors in ("pt", "np"), "padding / side / dtype / return_tensors")
        import torch
        flags = (DENSE_FIXED if padding == "max_length" else 0) | (DENSE_TRUNC_LEFT if truncation_side == "left" else 0) \
            | (DENSE_PAD_LEFT if padding_side == "left" else 0)
        i64 = dtype == "int64"
        D = len(docs)
        d_ids, d_oo, N, w = eng.encode_batch_device_words(d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), add_bos, add_eos, 0, CHECK_OFFSETS, stream)

        def dense(ptr, pad_value, fl):
            return eng.dense_from_ids_device(ptr if N else 0, d_oo, D, N, max_length, pad_to_multiple_of, pad_value, int(bool(add_bos)),
                                             int(bool(add_eos)), fl, stream).tensors(True)

        # (the first dense result is copied before the second call: both live in the dense pass's buffers)
        d = dense(d_ids, pad, flags | (DENSE_I64 if i64 else 0) | (DENSE_MASK if return_mask else 0))
        words = dense(w.word_ids_ptr, WORD_NONE, flags)["ids"]
        out = {"input_ids": d["ids"], "attention_mask": d["mask"], "lengths": d["lengths"], "n_truncated": d["n_truncated"],
               "word_ids": words.to(torch.int64) if i64 else words}
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}
        return out

    def _dense_pair(self, eng, ids_ptr, labels_ptr, offs_ptr, D, N, stream, max_length, padding, truncation_side, padding_side,
                    pad_to_multiple_of, pad, dtype, ignore_index, return_mask, keep_head=0, keep_tail=0):
        """The dense pass over ragged ids and over their labels, one after the other with the same options (the labels as int32
        elements padded with ignore_index, widened here -- which sign-extends), as encode_chat_padded runs it."""
        import torch
        flags = (DENSE_FIXED if padding == "max_length" else 0) | (DENSE_TRUNC_LEFT if truncation_side == "left" else 0) \
            | (DENSE_PAD_LEFT if padding_side == "left" else 0)
        i64 = dtype == "int64"

        def dense(ptr, pad_value, fl):
            return eng.dense_from_ids_device(ptr if N else 0, offs_ptr, D, N, max_length, pad_to_multiple_of, pad_value, keep_head, keep_tail,
                                             fl, stream).tensors(True)

        d = dense(ids_ptr, pad, flags | (DENSE_I64 if i64 else 0) | (DENSE_MASK if return_mask else 0))
        labels = dense(labels_ptr, int(ignore_index) & 0xFFFFFFFF, flags)["ids"]
        return {"input_ids": d["ids"], "attention_mask": d["mask"], "labels": labels.to(torch.int64) if i64 else labels, "lengths": d["lengths"],
                "n_truncated": d["n_truncated"]}

    def _token_id(self, token, default_name):
        if token is None:
            return self.get_control_token(default_name)
        return self.get_control_token(token) if isinstance(token, str) else int(token)

    def encode_batch_mlm(self, docs, mlm_probability=0.15, unit="token", span=(1, 1), mask_token=None, mask_rate=0.8, random_rate=0.1, seed=0,
                         add_bos=False, add_eos=False, padding=None, max_length=None, truncation_side="right", padding_side="right",
                         pad_to_multiple_of=None, pad_id=None, dtype="int64", ignore_index=-100, return_mask=True, return_selected=False,
                         return_tensors="pt"):
        """Masked-LM rows (tk_encode_batch_device_noise_replace; the definition is in include/tekken_hip.h): HF's
        DataCollatorForLanguageModeling(mlm=True) (unit "token"), DataCollatorForWholeWordMask (unit "word": the words of
        encode_batch_with_words) and SpanBERT's contiguous spans (span=(min, max) units), drawn on the device from `seed` -- the
        epoch.  mlm_probability is the expected fraction of units covered (noise_start_q32); of the chosen ids mask_rate become
        mask_token (an id, or a control token's name; None: "<unk>" -- Tekken has no [MASK]), random_rate a random ordinary token,
        the rest stay.  padding None: ragged {"input_ids" int32 [N], "offsets" int64 [D + 1], "labels" int32 [N] (ignore_index where
        not chosen), "selected" uint8 [N] or None, "n_selected", "n_masked", "n_random"}.  padding "longest" | "max_length": the
        dense pass over the ids and over the labels as encode_chat_padded runs it -- {"input_ids", "attention_mask", "labels",
        "lengths", "n_truncated"} and the counts (of the rows before truncation).  torch tensors on the tokenizer's GPU;
        return_tensors "np": numpy copies."""
        eng = self._device_engine()
        ok = unit in _NOISE_UNITS and padding in (None, "longest", "max_length") and truncation_side in ("left", "right") \
            and padding_side in ("left", "right") and dtype in ("int64", "int32") and return_tensors in ("pt", "np")
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude("encode_batch_mlm", docs, add_bos, add_eos, pad_id if padding else 0, ok,
                                                                       "unit / padding / side / dtype / return_tensors")
        import torch
        D = len(docs)
        d_ids, d_oo, N, res = eng.encode_batch_device_noise_replace(
            d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), add_bos, add_eos, CHECK_OFFSETS, stream,
            start_q32=noise_start_q32(mlm_probability, span[0], span[1]), mask_q32=fim_q32(mask_rate), random_q32=fim_q32(random_rate), seed=seed,
            unit=_NOISE_UNITS[unit], span_min=span[0], span_max=span[1], mask_id=self._token_id(mask_token, "<unk>"),
            flags=NOISE_SELECTED if return_selected else 0, ignore_index=ignore_index)
        if padding is None:
            t = res.tensors(True)
            out = {"input_ids": t["input_ids"], "offsets": _torch_wrap(DeviceView(d_oo, D + 1, "<i8"), True), "labels": t["labels"],
                   "selected": t["selected"]}
        else:
            out = self._dense_pair(eng, res.input_ids_ptr, res.labels_ptr, d_oo, D, N, stream, max_length, padding, truncation_side, padding_side,
                                   pad_to_multiple_of, pad, dtype, ignore_index, return_mask, int(bool(add_bos)), int(bool(add_eos)))
        out.update(res._counts())
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}
        return out

    def encode_batch_span_corruption(self, docs, noise_density=0.15, span=(1, 5), sentinels=None, final=None, unit="token", seed=0,
                                     form="seq2seq", add_bos=False, add_eos=False, padding=None, max_length=None, truncation_side="right",
                                     padding_side="right", pad_to_multiple_of=None, pad_id=None, dtype="int64", ignore_index=-100,
                                     return_mask=True, return_tensors="pt"):
        """Span-corruption rows (tk_encode_batch_device_noise_spans): T5 / UL2 denoising drawn on the device from `seed`.  Spans of
        span=(min, max) units (tokens, or words) cover noise_density of each document in expectation; every run of chosen ids is
        replaced by one sentinel in the inputs, and the targets are the sentinels followed by what they hide, then `final` (an id
        or a control token's name; None: nothing).  sentinels = (first, count, descending): control ids first, first +- 1, ...;
        runs beyond `count` in a document stay as they are.  form "seq2seq": {"input_ids", "input_offsets", "labels",
        "label_offsets"} -- two ragged batches --, or with padding each through the dense pass: {"input_ids", "attention_mask",
        "labels" (padded with ignore_index), "lengths", "label_lengths"}.  form "joined" (decoder-only): {"input_ids", "offsets",
        "labels"} with ignore_index on the inputs' part, padded as encode_batch_mlm pads.  The counts n_selected, n_runs,
        n_runs_dropped, n_inputs, n_targets come with every form.  torch tensors on the tokenizer's GPU; "np": numpy copies."""
        eng = self._device_engine()
        ok = unit in _NOISE_UNITS and form in ("seq2seq", "joined") and padding in (None, "longest", "max_length") \
            and truncation_side in ("left", "right") and padding_side in ("left", "right") and dtype in ("int64", "int32") \
            and return_tensors in ("pt", "np") and sentinels is not None and len(sentinels) == 3
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude("encode_batch_span_corruption", docs, add_bos, add_eos,
                                                                       pad_id if padding else 0, ok,
                                                                       "unit / form / padding / side / dtype / return_tensors / sentinels")
        import torch
        D = len(docs)
        joined = form == "joined"
        _, _, _, res = eng.encode_batch_device_noise_spans(
            d_bytes.data_ptr(), d_offs.data_ptr(), D, len(data), add_bos, add_eos, CHECK_OFFSETS, stream,
            start_q32=noise_start_q32(noise_density, span[0], span[1]), seed=seed, unit=_NOISE_UNITS[unit], span_min=span[0], span_max=span[1],
            n_sentinels=sentinels[1], sentinel_first=sentinels[0], final_id=JOIN_NONE if final is None else self._token_id(final, "</s>"),
            flags=(NOISE_JOINED if joined else NOISE_SPLIT) | (NOISE_DESC if sentinels[2] else 0), ignore_index=ignore_index)
        n_all = res.n_inputs + res.n_targets
        if padding is None:
            t = res.tensors(True)
            out = {"input_ids": t["joined"], "offsets": t["joined_offsets"], "labels": t["joined_labels"]} if joined else \
                {"input_ids": t["inputs"], "input_offsets": t["input_offsets"], "labels": t["targets"], "label_offsets": t["target_offsets"]}
        elif joined:
            out = self._dense_pair(eng, res.joined_ptr, res.joined_labels_ptr, res.joined_offsets_ptr, D, n_all, stream, max_length, padding,
                                   truncation_side, padding_side, pad_to_multiple_of, pad, dtype, ignore_index, return_mask)
        else:
            fl = (DENSE_FIXED if padding == "max_length" else 0) | (DENSE_TRUNC_LEFT if truncation_side == "left" else 0) \
                | (DENSE_PAD_LEFT if padding_side == "left" else 0)
            i64 = DENSE_I64 if dtype == "int64" else 0
            x = eng.dense_from_ids_device(res.inputs_ptr if res.n_inputs else 0, res.input_offsets_ptr, D, res.n_inputs, max_length, pad_to_multiple_of,
                                          pad, 0, 0, fl | i64 | (DENSE_MASK if return_mask else 0), stream).tensors(True)
            y = eng.dense_from_ids_device(res.targets_ptr if res.n_targets else 0, res.target_offsets_ptr, D, res.n_targets, max_length,
                                          pad_to_multiple_of, int(ignore_index) & 0xFFFFFFFF, 0, 0, fl, stream).tensors(True)
            out = {"input_ids": x["ids"], "attention_mask": x["mask"], "labels": y["ids"].to(torch.int64) if i64 else y["ids"],
                   "lengths": x["lengths"], "label_lengths": y["lengths"], "n_truncated": x["n_truncated"] + y["n_truncated"]}
        out.update(res._counts())
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}
        return out

    def encode_batch_packed(self, docs, seq_len, add_bos=True, add_eos=True, drop_last=False, pad_id=None, dtype="int64",
                            return_position_ids=True, return_segment_ids=True, return_cu_seqlens=True, return_tensors="pt", copy=True):
        """Packed pre-training rows (tk_encode_batch_device_seqpack / tk_encode_batch_seqpack; the definition is in
        include/tekken_hip.h): the documents' ids, BOS / EOS included, are one stream that is cut into rows of seq_len.
        {"input_ids", "position_ids", "segment_ids": [n_rows, seq_len] of `dtype` ("int64" | "int32"), "cu_seqlens": int32
        [n_segments + 1] (offsets into the flattened tensor, for variable-length attention), "max_seqlen", "n_rows", "n_used",
        "n_left", "n_segments": int}; an unselected tensor is None.  Positions restart and segment numbers advance at every document
        start and row start.  drop_last: no padded last row; the last n_left ids of the stream are not in the tensor (carry them
        into the next batch).  pad_id None: self.pad_id().  return_tensors "pt": torch tensors on the tokenizer's GPU (copy=False:
        views of context-owned buffers, valid until the next call on this tokenizer); "np": numpy."""
        eng = self._device_engine()
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_packed", docs, add_bos, add_eos, pad_id, dtype in ("int64", "int32") and return_tensors in ("pt", "np"),
            "dtype / return_tensors", {"seq_len": seq_len}, upload=return_tensors != "np")
        flags = (SEQPACK_I64 if dtype == "int64" else 0) | (SEQPACK_POSITIONS if return_position_ids else 0) \
            | (SEQPACK_SEGMENTS if return_segment_ids else 0) | (SEQPACK_CU_SEQLENS if return_cu_seqlens else 0) \
            | (SEQPACK_DROP_LAST if drop_last else 0)
        if return_tensors == "np":
            return eng.encode_batch_seqpack(data, offs, seq_len, add_bos, add_eos, False, pad, flags)
        _, _, _, res = eng.encode_batch_device_seqpack(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), seq_len, add_bos, add_eos,
                                                       pad, flags, CHECK_OFFSETS, stream)
        return res.tensors(copy)

    @staticmethod
    def _rowfit_flags(dtype, return_position_ids, return_segment_ids, return_cu_seqlens, return_doc_start):
        return (ROWFIT_I64 if dtype == "int64" else 0) | (ROWFIT_POSITIONS if return_position_ids else 0) \
            | (ROWFIT_SEGMENTS if return_segment_ids else 0) | (ROWFIT_CU_SEQLENS if return_cu_seqlens else 0) \
            | (ROWFIT_DOC_START if return_doc_start else 0)

    def encode_batch_packed_whole(self, docs, seq_len, add_bos=True, add_eos=True, pad_id=None, dtype="int64", return_position_ids=True,
                                  return_segment_ids=True, return_cu_seqlens=True, return_doc_start=True, return_tensors="pt", copy=True):
        """Whole documents packed into rows of seq_len without cutting one (tk_encode_batch_device_rowfit / tk_encode_batch_rowfit;
        the definition is in include/tekken_hip.h): next-fit in the given order, a document that does not fit the current row
        opens the next one, one of more than seq_len ids is truncated on the right (its EOS survives with add_eos).
        {"input_ids", "position_ids", "segment_ids": [n_rows, seq_len] of `dtype` ("int64" | "int32"), "cu_seqlens": int32
        [n_segments + 1] (offsets into the flattened tensor that tile it, every pad run a segment of its own), "doc_start": [D]
        where every document went (row * seq_len + column), "labels": None, "max_seqlen", "n_rows", "n_segments", "n_truncated",
        "n_pad": int}; an unselected tensor is None.  Next-fit keeps the order and pays for it in padding (n_pad): the regroup pass
        (encode_batch_regrouped, Engine.regroup_from_ids_device) puts the documents into length order on the device first.  pad_id None: self.pad_id().  return_tensors "pt": torch tensors on
        the tokenizer's GPU (copy=False: views of context-owned buffers, valid until the next call on this tokenizer); "np": numpy."""
        eng = self._device_engine()
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_packed_whole", docs, add_bos, add_eos, pad_id, dtype in ("int64", "int32") and return_tensors in ("pt", "np"),
            "dtype / return_tensors", {"seq_len": seq_len}, upload=return_tensors != "np")
        flags = self._rowfit_flags(dtype, return_position_ids, return_segment_ids, return_cu_seqlens, return_doc_start)
        keep_tail = min(1, int(seq_len)) if add_eos else 0
        if return_tensors == "np":
            return eng.encode_batch_rowfit(data, offs, seq_len, add_bos, add_eos, False, pad, keep_tail, flags)
        _, _, _, res = eng.encode_batch_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), seq_len, add_bos, add_eos,
                                                      pad, keep_tail, flags, CHECK_OFFSETS, stream)
        return res.tensors(copy)

    def encode_batch_regrouped(self, docs, order="keep", add_bos=False, add_eos=False, min_length=0, max_length=0, seed=0, window=0,
                               max_tokens=0, max_docs=0, descending=False, keep=None, return_perm=True, return_tensors="pt", copy=True):
        """The documents encoded, selected, reordered and cut into batches on the device (tk_encode_batch_device_regroup /
        tk_regroup_from_ids_device / tk_encode_batch_regroup; the definition is in include/tekken_hip.h).  order: "keep" |
        "length" (stable; descending=True: longest first) | "shuffle" (by a hash of seed and the document index) | "grouped"
        (shuffled, then sorted by length inside consecutive groups of `window`).  Documents of fewer than min_length or more than
        max_length (0: no limit) ids are dropped, as are those where keep (a sequence of D truth values) is false.  max_tokens >
        0: the order is cut into batches whose padded size, documents * longest document, stays within max_tokens (and max_docs).
        {"ids": int32 [n_ids], "offsets": int64 [n_docs + 1] (n_docs: the kept documents), "perm": int32 [n_docs], the source
        document of every output document, "batch_offsets": int64 [n_batches + 1], "batch_rowlen": int32 [n_batches], "labels":
        None, and the counts n_docs, n_ids, n_masked, n_short, n_long, n_batches, n_oversize, n_batch_pad}; an unselected array is
        None.  return_tensors "pt": torch tensors on the tokenizer's GPU (copy=False: views of context-owned buffers, valid until
        the next call on this tokenizer); "np": numpy (no keep mask: the host entry has none)."""
        eng = self._device_engine()
        _, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_regrouped", docs, add_bos, add_eos, 0, order in _ORDERS and return_tensors in ("pt", "np")
            and not (keep is not None and return_tensors == "np"), "order / return_tensors / keep",
            {"min_length": min_length, "max_length": max_length, "seed": seed, "window": window, "max_docs": max_docs},
            upload=return_tensors != "np")
        flags = (REGROUP_DESC if descending else 0) | (REGROUP_PERM if return_perm else 0) \
            | (REGROUP_BATCHES | REGROUP_BATCH_OFFSETS | REGROUP_BATCH_ROWLEN if max_tokens else 0)
        opts = (_ORDERS[order], min_length, max_length, seed, window, max_tokens, max_docs, flags)
        if return_tensors == "np":
            return eng.encode_batch_regroup(data, offs, add_bos, add_eos, False, *opts)
        if keep is None:
            _, _, _, res = eng.encode_batch_device_regroup(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos, add_eos, *opts,
                                                           CHECK_OFFSETS, stream)
        else:
            import torch
            if len(keep) != len(docs):
                raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_regrouped: keep has %d entries for %d documents" % (len(keep), len(docs)))
            d_keep = torch.as_tensor(np.asarray(keep, bool).astype(np.uint8)).cuda() if len(docs) else None
            d_ids, d_oo, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos, add_eos, stream,
                                                         CHECK_OFFSETS)[:3]
            res = eng.regroup_from_ids_device(d_ids, d_oo, len(docs), n_ids, *opts, 0, d_keep.data_ptr() if d_keep is not None else 0, stream)
        return res.tensors(copy)

    def encode_batch_windows(self, docs, max_length, stride=0, add_bos=False, add_eos=False, padding="max_length", pad_to_multiple_of=None,
                             pad_id=None, dtype="int64", return_attention_mask=True, return_offsets_mapping=False, return_tensors="pt",
                             copy=True, offsets_unit="byte"):
        """Overlapping windows for documents longer than the context (tk_encode_batch_device_window / tk_encode_batch_window; the
        definition is in include/tekken_hip.h): a document of more than max_length ids is split into windows whose text parts
        overlap by `stride` ids, each with its own BOS / EOS; a shorter one is one window.
        {"input_ids": [W, L] of `dtype` ("int64" | "int32"), "attention_mask": uint8 [W, L] or None, "lengths": int32 [W],
        "overflow_to_sample_mapping": int32 [W] the document of every window, "window_start": int32 [W] the index in the document's
        ids of the window's first text id, "doc_windows": int64 [D + 1] the first window of every document, "offset_mapping":
        int32 [W, L, 2] the (start, end) span under every element ((0, 0) under a pad) or None -- in bytes, or with offsets_unit
        "char" / "utf16" in code points / UTF-16 units (encode, the units pass and the window pass over its spans) --, "n_windows",
        "n_split": int}.
        padding "max_length": L = max_length, "longest": L = min(the longest document, max_length); then rounded up to
        pad_to_multiple_of.  pad_id None: self.pad_id().  return_tensors "pt": torch tensors on the tokenizer's GPU (copy=False:
        views of context-owned buffers, valid until the next call on this tokenizer); "np": numpy."""
        eng = self._device_engine()
        unit = self._unit(offsets_unit)
        in_units = unit != UNIT_BYTE and return_offsets_mapping
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_windows", docs, add_bos, add_eos, pad_id,
            padding in ("longest", "max_length") and dtype in ("int64", "int32") and return_tensors in ("pt", "np"),
            "padding / dtype / return_tensors", {"max_length": max_length, "stride": stride}, upload=return_tensors != "np" or in_units)
        flags = (WINDOW_FIXED if padding == "max_length" else 0) | (WINDOW_I64 if dtype == "int64" else 0) \
            | (WINDOW_MASK if return_attention_mask else 0) | (WINDOW_SPANS if return_offsets_mapping else 0)
        if return_tensors == "np" and not in_units:
            r = eng.encode_batch_window(data, offs, max_length, stride, add_bos, add_eos, False, pad_to_multiple_of, pad, flags)
            return _window_dict(r)
        import torch
        if in_units:
            # three calls on the stream: encode, the units pass, the window pass over the unit spans (every window repeats BOS / EOS)
            p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans_units(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos,
                                                                       add_eos, unit, CHECK_OFFSETS, stream)
            res = eng.window_from_ids_device(p_ids, p_oo, len(docs), n, max_length, stride, pad_to_multiple_of or 0, pad, int(bool(add_bos)),
                                             int(bool(add_eos)), flags, p_sp, stream)
        else:
            _, _, _, res = eng.encode_batch_device_window(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), max_length, stride,
                                                          add_bos, add_eos, pad_to_multiple_of, pad, flags, CHECK_OFFSETS, stream)
        out = _window_dict(res.tensors(copy))
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}
        return out

    def encode_batch_chunks(self, docs, max_length, overlap=0, min_length=None, levels=("word", "sentence", "line", "paragraph"),
                            add_bos=False, add_eos=False, padding="max_length", pad_to_multiple_of=None, pad_id=None, dtype="int64",
                            return_attention_mask=True, return_offsets_mapping=False, return_tensors="pt", copy=True, return_text=False):
        """Token-budget chunks that respect the text's structure (tk_encode_batch_device_chunk / tk_encode_batch_chunk; the
        definition is in include/tekken_hip.h): a document of more than max_length ids is cut into chunks of at most max_length
        ids, each with its own BOS / EOS, and every cut is made at the strongest break -- paragraph, line, sentence, word, token --
        that a chunk of at least min_length text ids can end at; the next chunk starts up to `overlap` ids earlier, at a word.  A
        shorter document is one chunk.  min_length None: max(c // 2, overlap + 1) with c = max_length - BOS - EOS.  levels: the
        kinds of break that count (one left out is demoted to the next one below, at last to a token break).
        The keys of encode_batch_windows, and "cut_level": uint8 [W] the CHUNK_LEVEL_* of the cut behind every chunk
        (CHUNK_CUT_LAST for a document's last), "chunk_bytes": int32 [W, 2] the byte range of the document that the chunk's text
        ids cover, "level_counts": int64 [6] the cuts made at every level (many at NONE or TOKEN: min_length is too close to
        max_length); with return_text, "texts": the document's bytes under chunk_bytes, decoded with errors="replace".
        padding, pad_to_multiple_of, pad_id, dtype, return_tensors and copy as in encode_batch_windows."""
        eng = self._device_engine()
        body = int(max_length or 0) - int(bool(add_bos)) - int(bool(add_eos))
        m = max(body // 2, int(overlap or 0) + 1) if min_length is None else min_length
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_batch_chunks", docs, add_bos, add_eos, pad_id,
            padding in ("longest", "max_length") and dtype in ("int64", "int32") and return_tensors in ("pt", "np")
            and all(x in _LEVELS for x in levels), "padding / dtype / return_tensors / levels",
            {"max_length": max_length, "min_length": m, "overlap": overlap}, upload=return_tensors != "np")
        mask = sum(1 << _LEVELS[x] for x in set(levels))
        flags = (CHUNK_FIXED if padding == "max_length" else 0) | (CHUNK_I64 if dtype == "int64" else 0) | CHUNK_BYTES \
            | (CHUNK_MASK if return_attention_mask else 0) | (CHUNK_SPANS if return_offsets_mapping else 0)
        if return_tensors == "np":
            r = eng.encode_batch_chunk(data, offs, max_length, m, overlap, add_bos, add_eos, False, pad_to_multiple_of, pad, mask, flags)
            out = _window_dict(r, cut_level=r["cut_level"], chunk_bytes=r["chunk_bytes"].astype(np.int32),
                               level_counts=r["level_counts"].astype(np.int64))
            where, wdoc = out["chunk_bytes"], out["overflow_to_sample_mapping"]
        else:
            _, _, _, res = eng.encode_batch_device_chunk(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), max_length, m, overlap,
                                                         add_bos, add_eos, pad_to_multiple_of or 0, pad, mask, flags, CHECK_OFFSETS, stream)
            t = res.tensors(copy)
            out = _window_dict(t, cut_level=t["cut_level"], chunk_bytes=t["chunk_bytes"], level_counts=t["level_counts"])
            if return_text:
                where, wdoc = out["chunk_bytes"].cpu().numpy(), out["overflow_to_sample_mapping"].cpu().numpy()
        if return_text:
            raw = data.tobytes()
            out["texts"] = [raw[int(offs[d]) + int(s):int(offs[d]) + int(e)].decode("utf-8", errors="replace")
                            for d, (s, e) in zip(wdoc.tolist(), where.tolist())]
        return out

    def _fixed_ids(self, ids, default):
        """The head / sep / tail keyword of encode_pairs as a list of ids: None is the default, a name goes through get_control_token."""
        if ids is None:
            return default()
        if isinstance(ids, (str, int)):
            ids = [ids]
        return [self.get_control_token(x) if isinstance(x, str) else int(x) for x in ids]

    def encode_pairs(self, first, second, max_length, truncation="longest_first", stride=0, return_overflowing_tokens=False, max_fixed=None,
                     head=None, sep=(), tail=None, padding="max_length", pad_to_multiple_of=None, pad_id=None, dtype="int64",
                     return_attention_mask=True, return_token_type_ids=True, return_sequence_ids=False, return_offsets_mapping=False,
                     offsets_unit="byte", return_tensors="pt", copy=True):
        """Sentence-pair rows, HF's tokenizer(text, text_pair, ...) (tk_encode_pairs_device / tk_encode_pairs; the definition is in
        include/tekken_hip.h): row p is head + first[p] + sep + second[p] + tail, the two texts encoded on their own (no token
        spans the seam).  head / sep / tail: at most 4 ids or control-token names each (defaults [bos], (), [eos]).  truncation
        "longest_first" cuts both sides on the right to share max_length; "only_second" / "only_first" keep (at most max_fixed
        ids of) the other side and cut the named one -- or, with return_overflowing_tokens, split it into windows that overlap by
        `stride` ids and all repeat the other side (extractive QA: the question in front of every slice of the context).
        {"input_ids": [W, L] of `dtype`, "attention_mask" / "token_type_ids" / "sequence_ids": uint8 [W, L] or None (sequence_ids:
        0 under first, 1 under second, PAIR_SEQ_NONE = 255 under a fixed id or a pad), "lengths", "overflow_to_sample_mapping",
        "window_start" (the index in the windowed side's ids of the row's first id of it), "second_start" (the column of the row's
        first id of second): int32 [W], "pair_windows": int64 [P + 1] the first row of every pair, "offset_mapping": int32
        [W, L, 2] the (start, end) span under every element relative to its own text ((0, 0) under a fixed id or a pad) or None --
        in bytes, or with offsets_unit "char" / "utf16" in code points / UTF-16 units --, "n_windows", "n_truncated", "n_split",
        "n_fixed_cut": int}.  A QA answer's token range in its context (spans_locate) lies in a row at columns
        second_start + (token - window_start).
        padding "max_length": L = max_length, "longest": L = the longest row; then rounded up to pad_to_multiple_of.  pad_id None:
        self.pad_id().  return_tensors "pt": torch tensors on the tokenizer's GPU (copy=False: views of context-owned buffers,
        valid until the next call on this tokenizer); "np": numpy."""
        eng = self._device_engine()
        unit = self._unit(offsets_unit)
        if len(first) != len(second):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_pairs: %d first texts, %d second texts" % (len(first), len(second)))
        in_units = unit != UNIT_BYTE and return_offsets_mapping
        parts = [t for pair in zip(first, second) for t in pair]
        pad, data, offs, d_bytes, d_offs, stream = self._batch_prelude(
            "encode_pairs", parts, False, False, pad_id,
            truncation in _STRATEGIES and padding in ("longest", "max_length") and dtype in ("int64", "int32") and return_tensors in ("pt", "np"),
            "truncation / padding / dtype / return_tensors", {"max_length": max_length, "stride": stride, "max_fixed": max_fixed or 0},
            upload=return_tensors != "np" or in_units)
        lists = (self._fixed_ids(head, lambda: [self.bos_id()]), self._fixed_ids(sep, list), self._fixed_ids(tail, lambda: [self.eos_id()]))
        if not all(0 <= x < 2 ** 32 for l in lists for x in l):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_pairs: a head / sep / tail id is outside 0 .. 2^32 - 1")
        flags = (PAIR_FIXED if padding == "max_length" else 0) | (PAIR_I64 if dtype == "int64" else 0) \
            | (PAIR_MASK if return_attention_mask else 0) | (PAIR_TYPE_IDS if return_token_type_ids else 0) \
            | (PAIR_SEQUENCE_IDS if return_sequence_ids else 0) | (PAIR_SPANS if return_offsets_mapping else 0) \
            | (PAIR_OVERFLOW if return_overflowing_tokens else 0)
        args = (max_length, _STRATEGIES[truncation], stride, max_fixed or 0, pad_to_multiple_of or 0, pad) + lists + (flags,)
        names = (("input_ids", "input_ids"), ("attention_mask", "mask"), ("token_type_ids", "type_ids"), ("sequence_ids", "sequence_ids"),
                 ("lengths", "lengths"), ("overflow_to_sample_mapping", "window_pair"), ("window_start", "window_start"),
                 ("second_start", "second_start"), ("pair_windows", "pair_windows"), ("offset_mapping", "spans"))
        if return_tensors == "np" and not in_units:
            r = eng.encode_pairs(data, offs, *args)
            signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
            out = {k: None if r[n] is None else r[n].astype(signed.get(r[n].dtype, r[n].dtype)) for k, n in names}
            out.update({k: r[k] for k in PairResult.DICT_COUNTS})
            return out
        import torch
        if in_units:
            # three calls on the stream: encode, the units pass, the pair pass over the unit spans
            p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans_units(d_bytes.data_ptr(), d_offs.data_ptr(), len(parts), len(data), False, False,
                                                                       unit, CHECK_OFFSETS, stream)
            res = eng.pair_from_ids_device(p_ids, p_oo, len(parts), n, *args, d_spans_ptr=p_sp, stream=stream)
        else:
            _, _, _, res = eng.encode_pairs_device(d_bytes.data_ptr(), d_offs.data_ptr(), len(parts), len(data), *args, checks=CHECK_OFFSETS,
                                                   stream=stream)
        t = res.tensors(copy)
        out = {k: t[n] for k, n in names}
        out.update({k: t[k] for k in PairResult.DICT_COUNTS})
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}
        return out

    def encode_batch_with_alignment(self, docs, annotations, offsets_unit="char", add_bos=False, add_eos=False, return_tensors="np"):
        """Encode + the spans in offsets_unit + which ids every annotated range covers (tk_encode_batch_device_spans_units,
        tk_spans_locate_device; the definitions are in include/tekken_hip.h).  annotations: per document a list of (start, end) in
        offsets_unit ("char": indices of the str, as a QA answer_start / a NER range).
        {"ids": int32 [T], "id_offsets": int64 [D + 1], "offset_mapping": int32 [T, 2], "ann_offsets": int64 [D + 1] the first
        annotation of every document in the flattened list, "token_ranges": int32 [A, 2] per annotation the document-relative id
        indices (lo, hi): ids id_offsets[d] + lo .. id_offsets[d] + hi - 1 overlap the range; hi == lo: none does}.
        return_tensors "np": numpy; "pt": torch tensors on the tokenizer's GPU (copies)."""
        eng = self._device_engine()
        unit = self._unit(offsets_unit)
        if return_tensors not in ("pt", "np"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_with_alignment: unknown return_tensors value")
        if len(annotations) != len(docs):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_with_alignment: %d documents, %d annotation lists" % (len(docs), len(annotations)))
        if add_bos:
            self.bos_id()      # (TokenNotFound when the vocabulary has no such control token, as encode)
        if add_eos:
            self.eos_id()
        ann_offs = np.zeros(len(docs) + 1, np.int64)
        ann_offs[1:] = np.cumsum([len(a) for a in annotations])
        flat = [(int(s), int(e)) for a in annotations for s, e in a]
        if any(not (0 <= s < 2 ** 32 and 0 <= e < 2 ** 32) for s, e in flat):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_with_alignment: an annotation is outside 0 .. 2^32 - 1")
        ann = np.array(flat, np.uint32).reshape(len(flat), 2)
        ann_doc = np.repeat(np.arange(len(docs), dtype=np.uint32), np.diff(ann_offs))
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        import torch
        d_bytes, d_offs, stream = _upload(data, offs)
        p_ids, p_oo, p_sp, n = eng.encode_batch_device_spans_units(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), add_bos,
                                                                   add_eos, unit, CHECK_OFFSETS, stream)
        A = len(flat)
        d_ann = torch.from_numpy(ann.view(np.int32) if A else np.zeros((1, 2), np.int32)).cuda()
        d_ann_doc = torch.from_numpy(ann_doc.view(np.int32) if A else np.zeros(1, np.int32)).cuda()
        p_rng = eng.spans_locate_device(p_sp, p_oo, len(docs), n, d_ann_doc.data_ptr(), d_ann.data_ptr(), A, stream)
        out = {"ids": _torch_wrap(DeviceView(p_ids, n, "<i4"), True), "id_offsets": _torch_wrap(DeviceView(p_oo, len(docs) + 1, "<i8"), True),
               "offset_mapping": _torch_wrap(DeviceView(p_sp, (n, 2), "<i4"), True), "ann_offsets": torch.from_numpy(ann_offs).cuda(),
               "token_ranges": _torch_wrap(DeviceView(p_rng, (A, 2), "<i4"), True)}
        if return_tensors == "np":
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out

    CHAT_ROLES = {"user": ("[INST]", "[/INST]", False), "system": ("[SYSTEM_PROMPT]", "[/SYSTEM_PROMPT]", False),
                  "assistant": (None, "</s>", True)}

    def _parts_of(self, convs, audio=None):
        """Conversations of (ctrl, text, label) parts -> (data, offs, part_ctrl, part_flags, conv_offs) as the join entries take them.
        audio: a list that receives (part index, clip) of every part whose text is an Audio -- such a part gets the control id
        [BEGIN_AUDIO], no text and no label --; None: the caller takes no audio parts."""
        names, texts, ctrl, pf, conv = {}, [], [], [], [0]
        for parts in convs:
            for part in parts:
                if len(part) != 3:
                    raise TokenizerError(TK_ERR_INVALID_ARG, "encode_conversations: a part is (ctrl, text, label)")
                c, text, label = part
                if isinstance(text, Audio):
                    if audio is None:
                        raise TokenizerError(TK_ERR_INVALID_ARG, "audio parts are taken by encode_conversations and encode_chat only")
                    audio.append((len(texts), text))
                    ctrl.append(self.begin_audio_token_id)
                    pf.append(0)
                    texts.append(b"")
                    continue
                if isinstance(c, str):
                    if c not in names:
                        names[c] = self.get_control_token(c)      # (TokenNotFound for an unknown name)
                    c = names[c]
                ctrl.append(JOIN_NONE if c is None else int(c))
                lc, lt = label if isinstance(label, (tuple, list)) else (label, label)
                pf.append((PART_LABEL_CTRL if lc else 0) | (PART_LABEL_TEXT if lt else 0))
                texts.append(text.encode("utf-8") if isinstance(text, str) else bytes(text or b""))
            conv.append(len(texts))
        data, offs = pack_docs(texts)
        return data, offs, np.array(ctrl, np.uint32), np.array(pf, np.uint32), np.array(conv, np.uint64)

    def _join_device(self, eng, parts, ignore_index, flags):
        """The parts (from _parts_of) go up once; -> (JoinResult, stream).  The result's buffers are the context's."""
        import torch
        data, offs, ctrl, pf, conv = parts
        d_bytes, d_offs, stream = _upload(data, offs)
        up = [torch.from_numpy(x).cuda() for x in ((ctrl if len(ctrl) else np.zeros(1, np.uint32)).view(np.int32),
                                                    (pf if len(pf) else np.zeros(1, np.uint32)).view(np.int32), conv.astype(np.int64))]
        res = eng.encode_parts_device_join(d_bytes.data_ptr(), d_offs.data_ptr(), len(ctrl), len(data), up[0].data_ptr(), up[1].data_ptr(),
                                           up[2].data_ptr(), len(conv) - 1, ignore_index, flags, CHECK_OFFSETS | CHECK_PARTS, stream)
        return res, stream

    def encode_conversations(self, convs, return_labels=True, return_part_index=False, ignore_index=-100, return_tensors="pt", copy=True):
        """Chat batches from explicit parts (tk_encode_parts_device_join / tk_encode_parts_join; the definition is in
        include/tekken_hip.h).  convs: a list of conversations, each a list of parts (ctrl, text, label) -- ctrl: None, an id, or a
        control-token name (get_control_token: an unknown one raises TokenNotFound); text: encoded on its own, without BOS / EOS,
        so no token spans a part boundary and control strings inside it stay plain text; label: a bool, or a pair (ctrl, text).
        -> {"input_ids": [N] all conversations back to back, "offsets": [C + 1], "labels": [N] int32 (the id, or ignore_index
        where the part is not labelled), "part_index": [N], "n_labelled": int}; an unselected tensor is None.  return_tensors
        "pt": torch tensors on the tokenizer's GPU (input_ids / labels / part_index int32, offsets int64; copy=False: views of
        context-owned buffers, valid until the next call on this tokenizer); "np": numpy (uint32 / uint64 / int32 / uint32)."""
        eng = self._device_engine()
        if return_tensors not in ("pt", "np"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_conversations: unknown return_tensors value")
        flags = (JOIN_LABELS if return_labels else 0) | (JOIN_PART_INDEX if return_part_index else 0)
        audio = []
        parts = self._parts_of(convs, audio)
        if audio:
            return self._conversations_audio(eng, parts, audio, ignore_index, flags, return_tensors, copy)
        if return_tensors == "np":
            r = eng.encode_parts_join(*parts, ignore_index=ignore_index, flags=flags)
            return {"input_ids": r["ids"], "offsets": r["offsets"], "labels": r["labels"], "part_index": r["part_index"],
                    "n_labelled": r["n_labelled"]}
        t = self._join_device(eng, parts, ignore_index, flags)[0].tensors(copy)
        return {"input_ids": t["ids"], "offsets": t["offsets"], "labels": t["labels"], "part_index": t["part_index"], "n_labelled": t["n_labelled"]}

    def _conversations_audio(self, eng, parts, audio, ignore_index, flags, return_tensors, copy):
        """encode_conversations with audio parts: encode the part texts, splice N times [AUDIO] behind every audio part
        (tk_audio_splice_device), join; the clips' log-mel features beside it.  The result gains "audio_features" (as
        encode_audio_batch's features), "audio_frame_off", "audio_clip_seg" and "audio_positions": the (start, N) of each [AUDIO]
        run in input_ids, in clip order."""
        import torch
        data, offs, ctrl, pf, conv = parts
        n_parts = len(ctrl)
        tokens = np.zeros(max(n_parts, 1), np.uint32)
        for p, clip in audio:
            tokens[p] = len(self._audio_count(clip)[0]) - 1
        d_bytes, d_offs, stream = _upload(data, offs)
        up = [torch.from_numpy(x).cuda() for x in (ctrl.view(np.int32), pf.view(np.int32), conv.astype(np.int64), tokens.view(np.int32))]
        ids_ptr, oo_ptr, n_ids = eng.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_parts, len(data), False, False, stream,
                                                         checks=CHECK_OFFSETS)
        sp = eng.audio_splice_device(ids_ptr, oo_ptr, n_parts, n_ids, up[3].data_ptr(), self.audio_token_id, stream)
        soffs = _torch_wrap(sp.views()[1], True).cpu().numpy().astype(np.int64)
        res = eng.join_from_ids_device(sp.ids_ptr, sp.offsets_ptr, n_parts, sp.n_ids, up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(),
                                       len(conv) - 1, ignore_index, flags, CHECK_PARTS, stream)
        t = res.tensors(copy)
        out = {"input_ids": t["ids"], "offsets": t["offsets"], "labels": t["labels"], "part_index": t["part_index"], "n_labelled": t["n_labelled"]}
        # a part's place in the joined stream: its spliced ids start behind the control ids of the parts up to and including it
        has_ctrl = np.cumsum(ctrl != JOIN_NONE)
        out["audio_positions"] = [(int(soffs[p]) + int(has_ctrl[p]), int(tokens[p])) for p, _ in audio]
        r = self._audio_features(eng, [clip for _, clip in audio])
        out["audio_features"], out["audio_frame_off"], out["audio_clip_seg"] = self._feature_tensors(r, copy)
        if return_tensors == "np":
            for k in ("input_ids", "offsets", "labels", "part_index"):
                if out[k] is not None:
                    out[k] = out[k].cpu().numpy()
            out["input_ids"] = out["input_ids"].view(np.uint32)
            out["offsets"] = out["offsets"].view(np.uint64)
            if out["part_index"] is not None:
                out["part_index"] = out["part_index"].view(np.uint32)
        return out

    def _chat_parts(self, conversations, roles, add_bos):
        table = dict(self.CHAT_ROLES)
        table.update(roles or {})
        convs = []
        for msgs in conversations:
            parts = [("<s>", "", False)] if add_bos else []
            for m in msgs:
                if m["role"] not in table:
                    raise TokenizerError(TK_ERR_INVALID_ARG, "encode_chat: no entry in roles for %r" % (m["role"],))
                opn, close, train = table[m["role"]]
                content = m["content"]
                if isinstance(content, (Audio, list, tuple)):
                    # content items: text and clips in order.  The open control id stays in front (a part of its own where a
                    # clip comes first); a clip is a part of its own and never labelled
                    items = [content] if isinstance(content, Audio) else list(content)
                    for k, it in enumerate(items):
                        if isinstance(it, Audio):
                            if k == 0 and opn is not None:
                                parts.append((opn, "", False))
                            parts.append((None, it, False))
                        else:
                            parts.append((opn if k == 0 else None, it, (False, bool(train))))
                    if not items:
                        parts.append((opn, "", (False, bool(train))))
                else:
                    parts.append((opn, content, (False, bool(train))))
                if close is not None:
                    parts.append((close, "", bool(train)))
            convs.append(parts)
        return convs

    def encode_chat(self, conversations, roles=None, add_bos=True, **kw):
        """encode_conversations over messages: a conversation is a list of {"role", "content"}.  roles maps a role to (open control
        name or None, close control name or None, train); given entries replace the defaults
            user: ("[INST]", "[/INST]", False), system: ("[SYSTEM_PROMPT]", "[/SYSTEM_PROMPT]", False), assistant: (None, "</s>", True).
        Layout of one conversation: "<s>" as one leading part (add_bos); then per message one part (open control id, the content)
        and, if the role has a close token, one part (close control id, no text).  With train the content and the close token are
        labelled; the open token never is, nor is "<s>".  The content is encoded on its own, so "[INST]" typed by a user stays
        text.  This is the plain Mistral instruct layout as far as the vocabulary's control tokens describe it; parity with
        mistral-common's templates (spacing, tool calls, where the system prompt goes in each version) is NOT claimed: that
        package was not at hand to compare against.  **kw: as encode_conversations."""
        return self.encode_conversations(self._chat_parts(conversations, roles, add_bos), **kw)

    def encode_chat_padded(self, conversations, roles=None, add_bos=True, max_length=None, padding="longest", truncation_side="right",
                           padding_side="right", pad_to_multiple_of=None, pad_id=None, dtype="int64", ignore_index=-100, return_mask=True):
        """encode_chat as a model-ready batch: {"input_ids": [B, L], "attention_mask": uint8 [B, L] (None without return_mask),
        "labels": [B, L] (ignore_index under the padding and under everything that is not trained), "lengths": int32 [B],
        "n_truncated", "n_labelled" (before truncation)}, torch tensors on the tokenizer's GPU.  The joined ids and the labels
        stream go through the dense pass of encode_batch_padded one after the other (the same options; "<s>" survives
        truncation), the labels padded with ignore_index; dtype "int64" | "int32" is the type of input_ids and labels."""
        eng = self._device_engine()
        if padding not in ("longest", "max_length") or truncation_side not in ("left", "right") or padding_side not in ("left", "right") \
                or dtype not in ("int64", "int32"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_chat_padded: unknown padding / side / dtype value")
        import torch
        pad = self.pad_id() if pad_id is None else int(pad_id)
        res, stream = self._join_device(eng, self._parts_of(self._chat_parts(conversations, roles, add_bos)), ignore_index, JOIN_LABELS)
        C, N = res.n_convs, res.n_ids
        flags = (DENSE_FIXED if padding == "max_length" else 0) | (DENSE_TRUNC_LEFT if truncation_side == "left" else 0) \
            | (DENSE_PAD_LEFT if padding_side == "left" else 0)

        def dense(ptr, pad_value, fl):
            return eng.dense_from_ids_device(ptr if N else 0, res.offsets_ptr, C, N, max_length, pad_to_multiple_of, pad_value, int(bool(add_bos)), 0,
                                             fl, stream).tensors(True)

        i64 = dtype == "int64"
        d = dense(res.ids_ptr, pad, flags | (DENSE_I64 if i64 else 0) | (DENSE_MASK if return_mask else 0))
        # (the labels are int32 with negative values: int32 elements through the pass, widened here -- which sign-extends)
        labels = dense(res.labels_ptr, int(ignore_index) & 0xFFFFFFFF, flags)["ids"]
        return {"input_ids": d["ids"], "attention_mask": d["mask"], "labels": labels.to(torch.int64) if i64 else labels, "lengths": d["lengths"],
                "n_truncated": d["n_truncated"], "n_labelled": res.n_labelled}

    def encode_chat_packed(self, conversations, seq_len, roles=None, add_bos=True, ignore_index=-100, pad_id=None, dtype="int64",
                           return_position_ids=True, return_segment_ids=True, return_cu_seqlens=True, return_doc_start=True,
                           return_tensors="pt", copy=True):
        """encode_chat packed for fine-tuning: whole conversations placed next-fit into rows of seq_len, never cut (a conversation of
        more than seq_len ids simply ends there).  One upload, the join pass and the rowfit pass over its ids, labels and offsets,
        nothing through the host in between.  -> what encode_batch_packed_whole returns, with "labels": [n_rows, seq_len]
        (ignore_index under the padding and under everything that is not trained; widened for dtype "int64") and "n_labelled"
        (before truncation)."""
        eng = self._device_engine()
        if dtype not in ("int64", "int32") or return_tensors not in ("pt", "np"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_chat_packed: unknown dtype / return_tensors value")
        if not 0 <= int(seq_len) < 2 ** 32:
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_chat_packed: seq_len %r" % (seq_len,))
        import torch
        pad = self.pad_id() if pad_id is None else int(pad_id)
        flags = self._rowfit_flags(dtype, return_position_ids, return_segment_ids, return_cu_seqlens, return_doc_start) | ROWFIT_LABELS
        data, offs, ctrl, pf, conv = self._parts_of(self._chat_parts(conversations, roles, add_bos))
        d_bytes, d_offs, stream = _upload(data, offs)
        up = [torch.from_numpy(x).cuda() for x in ((ctrl if len(ctrl) else np.zeros(1, np.uint32)).view(np.int32),
                                                    (pf if len(pf) else np.zeros(1, np.uint32)).view(np.int32), conv.astype(np.int64))]
        res, fit = eng.encode_parts_device_rowfit(d_bytes.data_ptr(), d_offs.data_ptr(), len(ctrl), len(data), up[0].data_ptr(), up[1].data_ptr(),
                                                  up[2].data_ptr(), len(conv) - 1, seq_len, pad, 0, flags, ignore_index, JOIN_LABELS,
                                                  CHECK_OFFSETS | CHECK_PARTS, stream)
        out = fit.tensors(copy)
        # (the labels are int32 with negative values: int32 elements through the pass, widened here -- which sign-extends)
        if dtype == "int64":
            out["labels"] = out["labels"].to(torch.int64)
        out["n_labelled"] = res.n_labelled
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}
        return out

    def decode_batch_padded(self, input_ids, lengths=None, policy=SpecialTokenPolicy.Ignore, pad_id=None, padding_side="right",
                            errors="strict"):
        """Batch decode of dense rows (tk_ragged_from_dense_device + tk_decode_batch_device): input_ids [B, L], int32 or int64, a
        torch tensor on the tokenizer's GPU or a numpy array -> list of str.  lengths (per row, optional): without them the run of
        pad_id (None: self.pad_id()) at the padded end of every row is dropped.  Errors as decode_batch (.bad_doc); errors="replace"
        as in decode_batch (self.n_replaced)."""
        eng = self._device_engine()
        import torch
        pad = self.pad_id() if pad_id is None else int(pad_id)
        t = torch.from_numpy(np.ascontiguousarray(input_ids)) if isinstance(input_ids, np.ndarray) else input_ids
        if t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise TokenizerError(TK_ERR_INVALID_ARG, "decode_batch_padded: input_ids must be [B, L] of int32 or int64")
        t = t.cuda().contiguous()
        D, L = int(t.shape[0]), int(t.shape[1])
        d_len = None
        if lengths is not None:
            d_len = torch.as_tensor(np.asarray(lengths) if not torch.is_tensor(lengths) else lengths).to(device="cuda", dtype=torch.int32).contiguous()
            if d_len.numel() != D:
                raise TokenizerError(TK_ERR_INVALID_ARG, "decode_batch_padded: one length per row")
        flags = (DENSE_I64 if t.dtype == torch.int64 else 0) | (DENSE_PAD_LEFT if padding_side == "left" else 0)
        stream = torch.cuda.current_stream().cuda_stream
        p_ids, p_oo, n = eng.ragged_from_dense_device(t.data_ptr() if D * L else 0, D, L, flags, d_len.data_ptr() if d_len is not None and D else 0,
                                                      pad, stream)
        v_bytes, v_offs = eng.decode_batch_device(p_ids, p_oo, D, n, policy, stream, errors)
        if errors == "replace":
            self.n_replaced = eng.n_replaced
        oo = torch.as_tensor(v_offs, device="cuda").cpu().numpy()
        total = int(oo[-1])
        raw = torch.as_tensor(v_bytes, device="cuda").cpu().numpy().tobytes() if total else b""
        return [raw[int(oo[d]):int(oo[d + 1])].decode("utf-8") for d in range(D)]

    def encode_batch(self, docs, add_bos=False, add_eos=False):
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        res = _Result()
        dbuf = data if len(data) else np.zeros(1, np.uint8)
        rc = lib().tk_tokenizer_encode_batch(self._h, _p(dbuf, ctypes.c_uint8), _p(offs, ctypes.c_uint64), len(docs),
                                             int(add_bos), int(add_eos), ctypes.byref(res))
        if rc != TK_OK:
            raise self._err(rc)
        ids, oo = _take_result(res)
        return [ids[int(oo[d]):int(oo[d + 1])].tolist() for d in range(len(docs))]

    def _special_modes(self, allowed, disallowed):
        """One SPECIAL_* per special id from tiktoken's two keywords ("all" or an iterable of special-token names); None: every
        string is parsed.  A name in neither is SPECIAL_TEXT."""
        if isinstance(allowed, str) and allowed != "all" or isinstance(disallowed, str) and disallowed != "all":
            raise ValueError("allowed / disallowed: 'all' or an iterable of special-token names")
        if allowed == "all" and disallowed == "all":
            raise ValueError("allowed and disallowed cannot both be 'all'")
        a = None if allowed == "all" else {self.get_control_token(x) for x in allowed}      # (an unknown name: TokenNotFound)
        d = None if disallowed == "all" else {self.get_control_token(x) for x in disallowed}
        if a is not None and d is not None and a & d:
            raise ValueError("special token ids %s are both allowed and disallowed" % sorted(a & d))
        if a is None and not d:
            return None
        modes = np.full(self.num_special_tokens(), SPECIAL_PARSE if a is None else SPECIAL_RAISE if d is None else SPECIAL_TEXT, np.uint8)
        for ids, m in ((a, SPECIAL_PARSE), (d, SPECIAL_RAISE)):
            if ids:
                modes[sorted(ids)] = m
        return modes

    def encode_with_specials(self, text, add_bos=False, add_eos=False, allowed="all", disallowed=()):
        """encode, with the special-token strings found in the text turned into their ids (tiktoken's allowed_special /
        disallowed_special; tk_tokenizer_encode_parsed, the definition is in include/tekken_hip.h): allowed / disallowed are "all" or
        an iterable of special-token names; a string of a disallowed token in the text raises; a name in neither stays text."""
        modes = self._special_modes(allowed, disallowed)
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        if add_bos:
            self.bos_id()      # (TokenNotFound when the vocabulary has no such control token, as encode)
        if add_eos:
            self.eos_id()
        ids = ctypes.POINTER(ctypes.c_uint32)()
        n = ctypes.c_size_t(0)
        rc = _need("tk_tokenizer_encode_parsed")(self._h, raw, len(raw), int(add_bos), int(add_eos),
                                                 None if modes is None else _p(modes, ctypes.c_uint8), 0 if modes is None else len(modes),
                                                 ctypes.byref(ids), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        out = [ids[i] for i in range(n.value)]
        lib().tk_free_ids(ids)
        return out

    def encode_batch_with_specials(self, docs, add_bos=False, add_eos=False, allowed="all", disallowed=()):
        """The batch form on the tokenizer's engine context (tk_encode_batch_parsed): {"ids": uint32 [N], "id_offsets": uint64
        [D + 1], "n_matches"}."""
        eng = self._device_engine()
        modes = self._special_modes(allowed, disallowed)
        if add_bos:
            self.bos_id()
        if add_eos:
            self.eos_id()
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        j = eng.encode_batch_parsed(data, offs, add_bos, add_eos, modes=modes)
        # (every match, BOS and EOS is one part with a control id: the text itself does not come back for the count)
        return {"ids": j["ids"], "id_offsets": j["offsets"], "n_matches": j["n_ctrl"] - len(docs) * (bool(add_bos) + bool(add_eos))}

    # ---- fill-in-the-middle rows (tk_fim; the definition is in include/tekken_hip.h)
    def _fim_opts_of(self, method, fim_rate, spm_rate, seed, format, train_on, add_bos, add_eos, min_length, return_tensors):
        """The keywords of the engine's FIM entries from those of the Tekkenizer methods.  "mistral": always suffix first and no
        middle token, "[SUFFIX] S [PREFIX] P M"; "psm_spm": "[PREFIX] P [SUFFIX] S [MIDDLE] M", or suffix first with probability
        spm_rate.  The ids come from get_control_token (TokenNotFound where the vocabulary lacks one)."""
        if format not in ("mistral", "psm_spm") or train_on not in ("all", "middle") or return_tensors not in ("pt", "np"):
            raise TokenizerError(TK_ERR_INVALID_ARG, "%s: unknown format / train_on / return_tensors value" % method)
        if not 0 <= int(min_length) < 2 ** 32:
            raise TokenizerError(TK_ERR_INVALID_ARG, "%s: min_length %r" % (method, min_length))
        if add_bos:
            self.bos_id()
        if add_eos:
            self.eos_id()
        mistral = format == "mistral"
        return dict(rate_q32=fim_q32(fim_rate), spm_q32=(1 << 32) if mistral else fim_q32(spm_rate), seed=seed,
                    prefix_id=self.get_control_token("[PREFIX]"), suffix_id=self.get_control_token("[SUFFIX]"),
                    middle_id=JOIN_NONE if mistral else self.get_control_token("[MIDDLE]"), min_units=min_length,
                    flags=FIM_SNAP | (FIM_BOS if add_bos else 0) | (FIM_EOS if add_eos else 0) | (FIM_LABEL_MIDDLE if train_on == "middle" else 0))

    @staticmethod
    def _fim_cuts(cuts, n_docs):
        """cuts of the Tekkenizer methods -- None, or per document None or a pair of byte positions -- as uint64 [D, 2]."""
        if cuts is None:
            return None
        if len(cuts) != n_docs:
            raise TokenizerError(TK_ERR_INVALID_ARG, "fim: one cuts entry per document (None, or a pair of byte positions)")
        out = np.full((n_docs, 2), FIM_NO_CUT, np.uint64)
        for d, c in enumerate(cuts):
            if c is not None:
                out[d] = (int(c[0]), int(c[1]))
        return out

    def encode_batch_fim(self, docs, fim_rate=0.5, spm_rate=0.5, seed=0, format="mistral", train_on="all", add_bos=True, add_eos=True,
                         cuts=None, min_length=0, ignore_index=-100, return_tensors="np", copy=True):
        """Fill-in-the-middle rows for a code / infill model (tk_encode_batch_device_fim / tk_encode_batch_fim): with probability
        fim_rate a document is cut at two byte positions drawn from (seed, its index), snapped back to character starts, and
        encoded as "[SUFFIX] S [PREFIX] P M" (format "mistral") or "[PREFIX] P [SUFFIX] S [MIDDLE] M" / suffix first with probability
        spm_rate ("psm_spm"); every piece is encoded on its own, so no token spans a cut -- the seam inference sees (encode_fim).
        Another seed is another draw: pass the epoch.  cuts: None, or per document None (leave it alone) or (a, b) byte positions,
        which replace the draws (fim_rate and min_length then play no part).  min_length: shorter documents (in bytes) are left
        alone.  train_on "middle": only the middle and what closes the row are labelled in transformed documents.
        -> {"input_ids": [N] all rows back to back, "offsets": [D + 1], "labels": [N] int32, "cuts": [D, 2] the cuts made (FIM_NO_CUT:
        none), "mode": uint8 [D] (FIM_NONE / FIM_PSM / FIM_SPM), "n_transformed", "n_spm", "n_skipped", "n_labelled"}.  return_tensors
        "np": numpy; "pt": torch tensors on the tokenizer's GPU (copy=False: views of context-owned buffers)."""
        eng = self._device_engine()
        opts = self._fim_opts_of("encode_batch_fim", fim_rate, spm_rate, seed, format, train_on, add_bos, add_eos, min_length, return_tensors)
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        c = self._fim_cuts(cuts, len(docs))
        if return_tensors == "np":
            j, f = eng.encode_batch_fim(data, offs, c, ignore_index, JOIN_LABELS, return_parts=True, **opts)
        else:
            import torch
            d_bytes, d_offs, stream = _upload(data, offs)
            d_cuts = None if c is None else torch.from_numpy((c if len(c) else np.zeros((1, 2), np.uint64)).view(np.int64)).cuda()
            fr, jr = eng.encode_batch_device_fim(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), 0 if d_cuts is None else d_cuts.data_ptr(),
                                                 ignore_index, JOIN_LABELS, CHECK_OFFSETS, stream, **opts)
            j, f = jr.tensors(copy), fr.tensors(copy)
        return {"input_ids": j["ids"], "offsets": j["offsets"], "labels": j["labels"], "cuts": f["cuts"], "mode": f["mode"],
                "n_transformed": f["n_transformed"], "n_spm": f["n_spm"], "n_skipped": f["n_skipped"], "n_labelled": j["n_labelled"]}

    def encode_batch_fim_packed(self, docs, seq_len, fim_rate=0.5, spm_rate=0.5, seed=0, format="mistral", train_on="all", add_bos=True,
                                add_eos=True, cuts=None, min_length=0, ignore_index=-100, pad_id=None, dtype="int64", return_position_ids=True,
                                return_segment_ids=True, return_cu_seqlens=True, return_doc_start=True, return_tensors="pt", copy=True):
        """encode_batch_fim packed for training: the split, then encode_parts_device_rowfit over its parts -- whole rows placed
        next-fit into rows of seq_len, never cut, with labels; one upload and nothing through the host in between.  -> what
        encode_chat_packed returns, and "n_transformed", "n_spm", "n_skipped"."""
        eng = self._device_engine()
        opts = self._fim_opts_of("encode_batch_fim_packed", fim_rate, spm_rate, seed, format, train_on, add_bos, add_eos, min_length, return_tensors)
        if dtype not in ("int64", "int32") or not 0 <= int(seq_len) < 2 ** 32:
            raise TokenizerError(TK_ERR_INVALID_ARG, "encode_batch_fim_packed: dtype %r, seq_len %r" % (dtype, seq_len))
        import torch
        pad = self.pad_id() if pad_id is None else int(pad_id)
        flags = self._rowfit_flags(dtype, return_position_ids, return_segment_ids, return_cu_seqlens, return_doc_start) | ROWFIT_LABELS
        data, offs = pack_docs([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
        c = self._fim_cuts(cuts, len(docs))
        d_bytes, d_offs, stream = _upload(data, offs)
        d_cuts = None if c is None else torch.from_numpy((c if len(c) else np.zeros((1, 2), np.uint64)).view(np.int64)).cuda()
        f = eng.fim_split_device(d_bytes.data_ptr(), d_offs.data_ptr(), len(docs), len(data), 0 if d_cuts is None else d_cuts.data_ptr(),
                                 CHECK_OFFSETS, stream, **opts)
        res, fit = eng.encode_parts_device_rowfit(f.units_ptr, f.part_offsets_ptr, f.n_parts, f.n_units, f.part_ctrl_ptr, f.part_flags_ptr,
                                                  f.conv_offsets_ptr, len(docs), seq_len, pad, 0, flags, ignore_index, JOIN_LABELS, 0, stream)
        out = fit.tensors(copy)
        # (the labels are int32 with negative values: int32 elements through the pass, widened here -- which sign-extends)
        if dtype == "int64":
            out["labels"] = out["labels"].to(torch.int64)
        out.update(n_labelled=res.n_labelled, n_transformed=f.n_transformed, n_spm=f.n_spm, n_skipped=f.n_skipped)
        if return_tensors == "np":
            out = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}
        return out

    def encode_fim(self, prefix, suffix, add_bos=True):
        """The inference prompt of a Mistral / Codestral infill model: [BOS, SUFFIX, enc(suffix), PREFIX, enc(prefix)], each text
        encoded on its own (encode_parts_join) -- what encode_batch_fim(format="mistral") gives for prefix + middle + suffix cut at
        the two seams, without the middle and EOS.  The model continues with the middle."""
        eng = self._device_engine()
        parts = ([(self.bos_id(), "", False)] if add_bos else []) + [(self.get_control_token("[SUFFIX]"), suffix, False),
                                                                     (self.get_control_token("[PREFIX]"), prefix, False)]
        return [int(x) for x in eng.encode_parts_join(*self._parts_of([parts]))["ids"]]

    def decode(self, ids, policy=SpecialTokenPolicy.Ignore):
        """Tekkenizer::decode (src/tekkenizer.rs:436-443)."""
        arr = np.ascontiguousarray(ids, dtype=np.uint32)
        buf = arr if len(arr) else np.zeros(1, np.uint32)
        text = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        rc = lib().tk_tokenizer_decode(self._h, _p(buf, ctypes.c_uint32), len(arr), int(policy), ctypes.byref(text),
                                       ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        out = ctypes.string_at(text, n.value).decode("utf-8")
        lib().tk_free_text(text)
        return out

    def _strs(self, fn, *args):
        text = ctypes.c_void_p()
        ends = ctypes.POINTER(ctypes.c_uint64)()
        n = ctypes.c_size_t(0)
        rc = fn(self._h, *args, ctypes.byref(text), ctypes.byref(ends), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        e = [int(ends[i]) for i in range(n.value)]
        raw = ctypes.string_at(text, e[-1] if e else 0)
        lib().tk_free_text(text)
        lib().tk_free_offsets(ends)
        return [raw[a:b].decode("utf-8") for a, b in zip([0] + e[:-1], e)]

    def decode_all(self, ids, policy=SpecialTokenPolicy.Ignore):
        """Tekkenizer::decode_all (src/tekkenizer.rs:463-560): one string per run of special / non-special ids."""
        arr = np.ascontiguousarray(ids, dtype=np.uint32)
        buf = arr if len(arr) else np.zeros(1, np.uint32)
        return self._strs(lib().tk_tokenizer_decode_all, _p(buf, ctypes.c_uint32), len(arr), int(policy))

    def vocab(self):
        """Tekkenizer::vocab (src/tekkenizer.rs:348-350): the piece string of every id."""
        return self._strs(lib().tk_tokenizer_vocab)

    def decode_batch(self, id_lists, policy=SpecialTokenPolicy.Ignore, errors="strict"):
        """Batch decode on the GPU: list of id lists -> list of str (an addition; the reference decodes one at a time).
        errors="replace": invalid UTF-8 becomes U+FFFD as in python's bytes.decode (a run of non-special ids at a time: a character
        never spans a special id); self.n_replaced then holds the U+FFFD written by the last such call."""
        eng = self.engine()
        if eng is None:
            raise TokenizerError(TK_ERR_NO_DEVICE, "tokenizer was created without a device (host-only object)")
        out = [b.decode("utf-8") for b in eng.decode_docs(id_lists, policy, errors)]
        if errors == "replace":
            self.n_replaced = eng.n_replaced
        return out

    n_replaced = 0           # U+FFFD written by the last decode_batch / decode_batch_padded with errors="replace"

    def decode_stream(self, n_seqs, policy=SpecialTokenPolicy.Ignore):
        """A DecodeStream over n_seqs running sequences for generation: .step(id_lists) -> list of str with only complete
        characters (the open tail of a character waits for the next step), .step_device(ids_ptr, offs_ptr, n_ids) -> device
        views, .finish() flushes, .reset(rows) zeroes slots, .state is the device state buffer."""
        return self._device_engine().decode_stream(n_seqs, policy, text=True)

    def _piece(self, fn, *args):
        text = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        rc = fn(self._h, *args, ctypes.byref(text), ctypes.byref(n))
        if rc != TK_OK:
            raise self._err(rc)
        out = ctypes.string_at(text, n.value)
        lib().tk_free_text(text)
        return out

    def id_to_piece(self, token_id):
        return self._piece(lib().tk_tokenizer_id_to_piece, token_id).decode("utf-8")

    def id_to_byte_piece(self, token_id, policy=SpecialTokenPolicy.Raise):
        return self._piece(lib().tk_tokenizer_id_to_byte_piece, token_id, int(policy))

    def vocab_size(self):
        return lib().tk_tokenizer_vocab_size(self._h)

    def num_special_tokens(self):
        return lib().tk_tokenizer_num_special_tokens(self._h)

    def version(self):
        return lib().tk_tokenizer_version(self._h).decode()

    def get_control_token(self, name):
        v = ctypes.c_uint32(0)
        rc = lib().tk_tokenizer_control_token(self._h, name.encode("utf-8"), ctypes.byref(v))
        if rc != TK_OK:
            raise self._err(rc)
        return v.value

    def bos_id(self):
        return self.get_control_token("<s>")

    def eos_id(self):
        return self.get_control_token("</s>")

    def pad_id(self):
        return self.get_control_token("<pad>")

    def unk_id(self):
        return self.get_control_token("<unk>")

    def is_special_token(self, token_id):
        return bool(lib().tk_tokenizer_is_special(self._h, token_id))

    def is_byte(self, token_id):
        return bool(lib().tk_tokenizer_is_byte(self._h, token_id))

    def json_pattern(self):
        """config.pattern of the loaded tekken.json (parsed and ignored by the reference, src/tekkenizer.rs:74)."""
        return lib().tk_tokenizer_json_pattern(self._h).decode("utf-8")

    def from_cache(self):
        """True when the object was loaded from a TK_TABLE_CACHE_DIR side file instead of the JSON (row f-2)."""
        return bool(lib().tk_tokenizer_from_cache(self._h))

    def engine(self):
        """The engine context behind this tokenizer (None for host-only objects)."""
        h = lib().tk_tokenizer_ctx(self._h)
        return Engine(None, 0, 0, 0, _borrowed=ctypes.c_void_p(h)) if h else None

    def rank_table(self):
        """list[bytes]: token bytes by rank (what reload_mergeable_ranks produced)."""
        blob = ctypes.POINTER(ctypes.c_uint8)()
        offs = ctypes.POINTER(ctypes.c_uint32)()
        n = ctypes.c_uint32(0)
        lib().tk_tokenizer_rank_table(self._h, ctypes.byref(blob), ctypes.byref(offs), ctypes.byref(n))
        o = np.ctypeslib.as_array(offs, shape=(n.value + 1,))
        total = int(o[-1])
        b = ctypes.string_at(blob, total)
        return [b[int(o[i]):int(o[i + 1])] for i in range(n.value)]
