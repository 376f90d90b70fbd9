//! Safe wrappers over ffi.rs.  `HipEngine` = one GPU (one `tk_ctx`), `HipNode` = several GPUs of one node.
use crate::ffi::*;
use std::os::raw::c_int;

/// What the shim hands back; tekken-rs maps it onto its `TokenizerError` (src/errors.rs:23-59):
/// InvalidConfig -> `TokenizerError::InvalidConfig` (:45-46), TokenNotFound -> `TokenNotFound` (:49-50),
/// SpecialTokenPolicy -> `SpecialTokenPolicy` (:53-54), everything else -> `Tokenizers(msg)` (:37-38).
#[derive(Debug)]
pub enum HipError {
    InvalidConfig(String),
    TokenNotFound(String),
    SpecialTokenPolicy(String),
    Audio(String),
    Tokenizers(String),
}

impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        match self {
            HipError::InvalidConfig(m) | HipError::TokenNotFound(m) | HipError::SpecialTokenPolicy(m) | HipError::Audio(m) | HipError::Tokenizers(m) => f.write_str(m),
        }
    }
}
impl std::error::Error for HipError {}

fn map_err(rc: c_int, msg: *const std::os::raw::c_char) -> HipError {
    let msg = if msg.is_null() { String::new() } else { unsafe { std::ffi::CStr::from_ptr(msg) }.to_string_lossy().into_owned() };
    match rc {
        TK_ERR_INVALID_CONFIG | TK_ERR_INVALID_ARG => HipError::InvalidConfig(msg),
        TK_ERR_TOKEN_NOT_FOUND => HipError::TokenNotFound(msg),
        TK_ERR_SPECIAL_POLICY => HipError::SpecialTokenPolicy(msg),
        TK_ERR_AUDIO => HipError::Audio(msg),
        _ => HipError::Tokenizers(msg), // runtime / no device / invalid UTF-8
    }
}

fn pack_ranks(ranks: &[Vec<u8>]) -> (Vec<u8>, Vec<u32>) {
    let mut blob = Vec::with_capacity(ranks.iter().map(|t| t.len()).sum());
    let mut offs = Vec::with_capacity(ranks.len() + 1);
    offs.push(0u32);
    for t in ranks {
        blob.extend_from_slice(t);
        offs.push(blob.len() as u32);
    }
    (blob, offs)
}

fn pack_docs(docs: &[&str]) -> (Vec<u8>, Vec<u64>) {
    let mut bytes = Vec::with_capacity(docs.iter().map(|d| d.len()).sum());
    let mut offs = Vec::with_capacity(docs.len() + 1);
    offs.push(0u64);
    for d in docs {
        bytes.extend_from_slice(d.as_bytes());
        offs.push(bytes.len() as u64);
    }
    (bytes, offs)
}

unsafe fn take(res: &mut TkResult, n_docs: usize) -> Vec<Vec<u32>> {
    let ids = std::slice::from_raw_parts(res.ids, res.n_ids as usize);
    let o = std::slice::from_raw_parts(res.offsets, n_docs + 1);
    let out = (0..n_docs).map(|d| ids[o[d] as usize..o[d + 1] as usize].to_vec()).collect();
    tk_free_result(res);
    out
}

pub struct HipEngine {
    ctx: *mut TkCtx,
}
unsafe impl Send for HipEngine {}
unsafe impl Sync for HipEngine {} // the context serialises its calls internally (one stream + mutex)

impl HipEngine {
    /// `ranks[i]` = token bytes of rank i, i.e. the inverse of the map `reload_mergeable_ranks` builds (src/tekkenizer.rs:776-816).
    pub fn new(ranks: &[Vec<u8>], num_special: u32, bos: u32, eos: u32, device: i32) -> Result<Self, HipError> {
        let (blob, offs) = pack_ranks(ranks);
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe { tk_ctx_create(blob.as_ptr(), offs.as_ptr(), ranks.len() as u32, num_special, bos, eos, device, &mut ctx) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(std::ptr::null()) }));
        }
        Ok(Self { ctx })
    }

    /// Memo of merged pieces: `log2_entries` 0 switches it off, 10..26 sizes the table (32-byte entries); `always` = no adaptive pause.
    /// The table can change how long a call takes, never an id (an entry is the exact key and the exact merge result).
    pub fn set_memo(&self, log2_entries: i32, always: bool) -> Result<(), HipError> {
        let rc = unsafe { tk_ctx_set_memo(self.ctx, log2_entries as c_int, always as c_int) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        Ok(())
    }

    /// `Tekkenizer::encode` for ONE `&str` (the reference's own signature): no allocation inside the library, the ids land in
    /// a Vec sized for the worst case (one id per byte + BOS + EOS).
    pub fn encode(&self, text: &str, add_bos: bool, add_eos: bool) -> Result<Vec<u32>, HipError> {
        let mut ids: Vec<u32> = Vec::with_capacity(text.len() + 2);
        let mut n = 0u64;
        let rc = unsafe {
            tk_encode_one(self.ctx, text.as_ptr(), text.len() as u64, add_bos as c_int, add_eos as c_int, ids.as_mut_ptr(),
                          ids.capacity() as u64, &mut n)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        unsafe { ids.set_len(n as usize) };
        Ok(ids)
    }

    pub fn encode_batch(&self, docs: &[&str], add_bos: bool, add_eos: bool) -> Result<Vec<Vec<u32>>, HipError> {
        let (bytes, offs) = pack_docs(docs);
        let mut res = TkResult { ids: std::ptr::null_mut(), offsets: std::ptr::null_mut(), n_ids: 0, n_docs: 0 };
        // &str is valid UTF-8 by construction => validate_utf8 = 0
        let rc = unsafe { tk_encode_batch(self.ctx, bytes.as_ptr(), offs.as_ptr(), docs.len() as u64, add_bos as c_int, add_eos as c_int, 0, &mut res) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        Ok(unsafe { take(&mut res, docs.len()) })
    }

    /// `encode` + where every id came from: `(start, end)` byte offsets into `text` (HF tokenizers' `offset_mapping`, in bytes of
    /// the UTF-8 text -- a byte-fallback token can end inside a char; BOS is `(0, 0)`, EOS `(len, len)`).
    pub fn encode_with_offsets(&self, text: &str, add_bos: bool, add_eos: bool) -> Result<(Vec<u32>, Vec<(u32, u32)>), HipError> {
        Ok(self.encode_batch_with_offsets(&[text], add_bos, add_eos)?.pop().unwrap_or_default())
    }

    /// The batch form: per document `(ids, spans)`, spans relative to the start of the document (tk_encode_batch_spans).
    pub fn encode_batch_with_offsets(&self, docs: &[&str], add_bos: bool, add_eos: bool)
                                     -> Result<Vec<(Vec<u32>, Vec<(u32, u32)>)>, HipError> {
        let (bytes, offs) = pack_docs(docs);
        let mut res = TkResult { ids: std::ptr::null_mut(), offsets: std::ptr::null_mut(), n_ids: 0, n_docs: 0 };
        let mut spans: *mut u32 = std::ptr::null_mut();
        let mut bad_doc = 0u64;
        let rc = unsafe {
            tk_encode_batch_spans(self.ctx, bytes.as_ptr(), offs.as_ptr(), docs.len() as u64, add_bos as c_int, add_eos as c_int, 0, 0,
                                  &mut res, &mut spans, &mut bad_doc)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        let out = unsafe {
            let sp = std::slice::from_raw_parts(spans, 2 * res.n_ids as usize);
            let o = std::slice::from_raw_parts(res.offsets, docs.len() + 1);
            let per_doc: Vec<Vec<(u32, u32)>> =
                (0..docs.len()).map(|d| (o[d] as usize..o[d + 1] as usize).map(|i| (sp[2 * i], sp[2 * i + 1])).collect()).collect();
            tk_free_spans(spans);
            take(&mut res, docs.len()).into_iter().zip(per_doc).collect()
        };
        Ok(out)
    }

    /// Model-ready batch (tk_encode_batch_dense): `(input_ids [B * L] row-major, attention_mask [B * L], lengths [B], L)`.  Rows longer
    /// than `max_length` (0 = no limit) are cut on the right with BOS / EOS kept; `fixed`: L = `max_length`, else the longest kept
    /// row; rows are filled with `pad_id` on the right.  Ids are < 2^31, so `i32` holds them.
    pub fn encode_batch_padded(&self, docs: &[&str], add_bos: bool, add_eos: bool, max_length: u32, fixed: bool, pad_id: u32)
                               -> Result<(Vec<i32>, Vec<u8>, Vec<u32>, usize), HipError> {
        let (bytes, offs) = pack_docs(docs);
        let opts = TkDenseOpts { max_length, multiple_of: 0, pad_id, keep_head: 0, keep_tail: 0,
                                 flags: TK_DENSE_MASK | if fixed { TK_DENSE_FIXED } else { 0 } };
        let mut d = TkDense { ids: std::ptr::null_mut(), mask: std::ptr::null_mut(), lengths: std::ptr::null_mut(), n_docs: 0, row_len: 0,
                              n_truncated: 0 };
        let rc = unsafe {
            tk_encode_batch_dense(self.ctx, bytes.as_ptr(), offs.as_ptr(), docs.len() as u64, add_bos as c_int, add_eos as c_int, 0, &opts, &mut d)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        let n = (d.n_docs * d.row_len) as usize;
        let out = unsafe {
            let ids = std::slice::from_raw_parts(d.ids as *const i32, n).to_vec();
            let mask = std::slice::from_raw_parts(d.mask as *const u8, n).to_vec();
            let lengths = std::slice::from_raw_parts(d.lengths as *const u32, d.n_docs as usize).to_vec();
            let row_len = d.row_len as usize;
            tk_free_dense(&mut d);
            (ids, mask, lengths, row_len)
        };
        Ok(out)
    }

    /// Overlapping windows for documents longer than the context (tk_encode_batch_window): `(input_ids [W * max_length] row-major,
    /// attention_mask [W * max_length], lengths [W], window_doc [W], window_start [W])`.  A document of more than `max_length` ids is
    /// split into windows whose text parts share `stride` ids, each with its own BOS / EOS; `window_doc[w]` is the document window w
    /// came from (HF tokenizers' `overflow_to_sample_mapping`), `window_start[w]` the index of its first text id in that document.
    pub fn encode_batch_windows(&self, docs: &[&str], add_bos: bool, add_eos: bool, max_length: u32, stride: u32, pad_id: u32)
                                -> Result<(Vec<i32>, Vec<u8>, Vec<u32>, Vec<u32>, Vec<u32>), HipError> {
        let (bytes, offs) = pack_docs(docs);
        let opts = TkWindowOpts { max_length, stride, multiple_of: 0, pad_id, keep_head: 0, keep_tail: 0, flags: TK_WINDOW_FIXED | TK_WINDOW_MASK };
        let mut w = TkWindow { input_ids: std::ptr::null_mut(), mask: std::ptr::null_mut(), lengths: std::ptr::null_mut(),
                               window_doc: std::ptr::null_mut(), window_start: std::ptr::null_mut(), doc_windows: std::ptr::null_mut(),
                               spans: std::ptr::null_mut(), n_docs: 0, n_windows: 0, row_len: 0, n_split: 0 };
        let rc = unsafe {
            tk_encode_batch_window(self.ctx, bytes.as_ptr(), offs.as_ptr(), docs.len() as u64, add_bos as c_int, add_eos as c_int, 0, &opts, &mut w)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        let (rows, n) = (w.n_windows as usize, (w.n_windows * w.row_len) as usize);
        let out = unsafe {
            let ids = std::slice::from_raw_parts(w.input_ids as *const i32, n).to_vec();
            let mask = std::slice::from_raw_parts(w.mask as *const u8, n).to_vec();
            let lengths = std::slice::from_raw_parts(w.lengths as *const u32, rows).to_vec();
            let window_doc = std::slice::from_raw_parts(w.window_doc as *const u32, rows).to_vec();
            let window_start = std::slice::from_raw_parts(w.window_start as *const u32, rows).to_vec();
            tk_free_window(&mut w);
            (ids, mask, lengths, window_doc, window_start)
        };
        Ok(out)
    }

    /// Chat batch (tk_encode_parts_join): every part is `(control id or None, text, label the control id, label the text)`, a
    /// conversation is a slice of parts.  Returns `(ids, offsets [C + 1], labels)`: all conversations back to back, every text
    /// encoded on its own without BOS / EOS, its control id in front; `labels[i]` is the id or `ignore_index`.
    pub fn encode_conversations(&self, convs: &[&[(Option<u32>, &str, bool, bool)]], ignore_index: i32)
                                -> Result<(Vec<u32>, Vec<u64>, Vec<i32>), HipError> {
        let parts: Vec<&(Option<u32>, &str, bool, bool)> = convs.iter().flat_map(|c| c.iter()).collect();
        let texts: Vec<&str> = parts.iter().map(|p| p.1).collect();
        let (bytes, offs) = pack_docs(&texts);
        let ctrl: Vec<u32> = parts.iter().map(|p| p.0.unwrap_or(TK_JOIN_NONE)).collect();
        let flags: Vec<u32> = parts.iter().map(|p| (if p.2 { TK_PART_LABEL_CTRL } else { 0 }) | (if p.3 { TK_PART_LABEL_TEXT } else { 0 })).collect();
        let mut conv_offs: Vec<u64> = vec![0];
        for c in convs {
            conv_offs.push(conv_offs[conv_offs.len() - 1] + c.len() as u64);
        }
        let opts = TkJoinOpts { ignore_index, flags: TK_JOIN_LABELS };
        let mut j = TkJoin { ids: std::ptr::null_mut(), offsets: std::ptr::null_mut(), labels: std::ptr::null_mut(),
                             part_index: std::ptr::null_mut(), n_convs: 0, n_parts: 0, n_ids: 0, n_ctrl: 0, n_labelled: 0 };
        let rc = unsafe {
            tk_encode_parts_join(self.ctx, bytes.as_ptr(), offs.as_ptr(), parts.len() as u64, ctrl.as_ptr(), flags.as_ptr(), conv_offs.as_ptr(),
                                 convs.len() as u64, 0, &opts, &mut j)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(self.ctx) }));
        }
        let n = j.n_ids as usize;
        let out = unsafe {
            let ids = std::slice::from_raw_parts(j.ids as *const u32, n).to_vec();
            let offsets = std::slice::from_raw_parts(j.offsets as *const u64, convs.len() + 1).to_vec();
            let labels = std::slice::from_raw_parts(j.labels as *const i32, n).to_vec();
            tk_free_join(&mut j);
            (ids, offsets, labels)
        };
        Ok(out)
    }
}
impl Drop for HipEngine {
    fn drop(&mut self) {
        unsafe { tk_ctx_destroy(self.ctx) }
    }
}

/// The host mirror of `Tekkenizer` for the audio surface (src/tekkenizer.rs:697-760): `has_audio_support`, `audio_config`,
/// `encode_audio`, and the log-mel features of a batch of clips on the tokenizer's GPU.
pub struct HipTekkenizer {
    t: *mut TkTokenizer,
}
unsafe impl Send for HipTekkenizer {}

/// `AudioEncoding` (src/audio.rs:476-479): the ids and the clip padded as the reference pads it.
pub struct HipAudioEncoding {
    pub tokens: Vec<u32>,
    pub audio: Vec<f32>,
    pub sampling_rate: usize,
}

impl HipTekkenizer {
    pub fn from_file(path: &str, device: i32) -> Result<Self, HipError> {
        let c = std::ffi::CString::new(path).map_err(|e| HipError::InvalidConfig(e.to_string()))?;
        let mut t: *mut TkTokenizer = std::ptr::null_mut();
        let rc = unsafe { tk_tokenizer_from_file(c.as_ptr(), device, &mut t) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_tokenizer_last_error(std::ptr::null()) }));
        }
        Ok(Self { t })
    }
    fn err(&self, rc: c_int) -> HipError {
        map_err(rc, unsafe { tk_tokenizer_last_error(self.t) })
    }
    pub fn has_audio_support(&self) -> bool {
        unsafe { tk_tokenizer_has_audio(self.t) != 0 }
    }
    pub fn audio_config(&self) -> Option<TkAudioConfig> {
        let mut a = TkAudioConfig::default();
        if unsafe { tk_tokenizer_audio_config(self.t, &mut a) } == TK_OK { Some(a) } else { None }
    }
    /// `Tekkenizer::encode_audio`: `[BEGIN_AUDIO] + [AUDIO] * N` and the padded clip; a clip at another rate is
    /// `Audio("Resampling not yet implemented")`, a tokenizer without audio `Audio("Audio encoder not configured")`.
    pub fn encode_audio(&self, samples: &[f32], sampling_rate: usize) -> Result<HipAudioEncoding, HipError> {
        let (mut ids, mut n, mut padded) = (std::ptr::null_mut::<u32>(), 0usize, 0u64);
        let rc = unsafe { tk_tokenizer_encode_audio(self.t, samples.len() as u64, sampling_rate as u64, &mut ids, &mut n, &mut padded) };
        if rc != TK_OK {
            return Err(self.err(rc));
        }
        let tokens = unsafe { std::slice::from_raw_parts(ids, n).to_vec() };
        unsafe { tk_free_ids(ids) };
        let mut audio = samples.to_vec();
        audio.resize(padded as usize, 0.0);
        Ok(HipAudioEncoding { tokens, audio, sampling_rate })
    }
    /// The log-mel features of a batch of clips (tk_audio_logmel): `(features, frame_off [S + 1], clip_seg [n + 1], n_mel)`;
    /// segment s is `[n_mel][T_s]` row-major at element `n_mel * frame_off[s]`.
    pub fn audio_features(&self, clips: &[&[f32]]) -> Result<(Vec<f32>, Vec<u64>, Vec<u64>, u64), HipError> {
        let ctx = unsafe { tk_tokenizer_ctx(self.t) };
        let mut offs: Vec<u64> = vec![0];
        let mut flat: Vec<f32> = Vec::new();
        for c in clips {
            flat.extend_from_slice(c);
            offs.push(flat.len() as u64);
        }
        let opts = TkLogmelOpts { log_mel_max: f32::NAN, flags: 0 };
        let mut r = TkLogmel { features: std::ptr::null_mut(), frame_off: std::ptr::null_mut(), clip_seg: std::ptr::null_mut(),
                               n_clips: 0, n_segments: 0, n_frames: 0, n_mel: 0 };
        let rc = unsafe { tk_audio_logmel(ctx, flat.as_ptr(), offs.as_ptr(), clips.len() as u64, &opts, &mut r) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_last_error(ctx) }));
        }
        let out = unsafe {
            let f = std::slice::from_raw_parts(r.features as *const f32, (r.n_mel * r.n_frames) as usize).to_vec();
            let fo = std::slice::from_raw_parts(r.frame_off as *const u64, r.n_segments as usize + 1).to_vec();
            let cs = std::slice::from_raw_parts(r.clip_seg as *const u64, r.n_clips as usize + 1).to_vec();
            let m = r.n_mel;
            tk_free_logmel(&mut r);
            (f, fo, cs, m)
        };
        Ok(out)
    }
}
impl Drop for HipTekkenizer {
    fn drop(&mut self) {
        unsafe { tk_tokenizer_destroy(self.t) }
    }
}

/// All GPUs of one node behind one call: the batch is cut into contiguous runs of whole documents balanced by BYTES, every GPU
/// tokenizes its run, the id buffers are gathered on the first device with direct peer -> root RCCL transfers (18 bits per id
/// on the wire) and come back in document order.
pub struct HipNode {
    node: *mut TkNode,
}
unsafe impl Send for HipNode {}
unsafe impl Sync for HipNode {}

impl HipNode {
    pub fn new(ranks: &[Vec<u8>], num_special: u32, bos: u32, eos: u32, devices: &[i32]) -> Result<Self, HipError> {
        let (blob, offs) = pack_ranks(ranks);
        let mut node = std::ptr::null_mut();
        let rc = unsafe {
            tk_node_create(blob.as_ptr(), offs.as_ptr(), ranks.len() as u32, num_special, bos, eos, devices.as_ptr(), devices.len() as c_int, &mut node)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_node_last_error(std::ptr::null()) }));
        }
        Ok(Self { node })
    }

    pub fn encode_batch(&self, docs: &[&str], add_bos: bool, add_eos: bool) -> Result<Vec<Vec<u32>>, HipError> {
        let (bytes, offs) = pack_docs(docs);
        let mut res = TkResult { ids: std::ptr::null_mut(), offsets: std::ptr::null_mut(), n_ids: 0, n_docs: 0 };
        let rc = unsafe { tk_node_encode_batch(self.node, bytes.as_ptr(), offs.as_ptr(), docs.len() as u64, add_bos as c_int, add_eos as c_int, &mut res) };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_node_last_error(self.node) }));
        }
        Ok(unsafe { take(&mut res, docs.len()) })
    }

    /// The batch form for a host that encodes batch after batch: packed text + offsets in, ids + id offsets out, all four in
    /// buffers the caller keeps (pinned: `tk_host_alloc`) -- returns the number of ids written.
    pub fn encode_batch_into(&self, bytes: &[u8], doc_offsets: &[u64], add_bos: bool, add_eos: bool, ids_out: &mut [u32],
                             offsets_out: &mut [u64]) -> Result<usize, HipError> {
        assert!(!doc_offsets.is_empty() && offsets_out.len() >= doc_offsets.len());
        let mut n: u64 = 0;
        let rc = unsafe {
            tk_node_encode_batch_pinned(self.node, bytes.as_ptr(), doc_offsets.as_ptr(), (doc_offsets.len() - 1) as u64, add_bos as c_int,
                                        add_eos as c_int, ids_out.as_mut_ptr(), ids_out.len() as u64, offsets_out.as_mut_ptr(), &mut n)
        };
        if rc != TK_OK {
            return Err(map_err(rc, unsafe { tk_node_last_error(self.node) }));
        }
        Ok(n as usize)
    }
}
impl Drop for HipNode {
    fn drop(&mut self) {
        unsafe { tk_node_destroy(self.node) }
    }
}
