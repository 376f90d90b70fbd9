// tk_flat_impl.h -- the FLAT tokenization path: one wave per CHUNK of the packed byte stream.
//
// Same computation as tk_encode_impl.h (CoreBPE::encode behind reference src/tekkenizer.rs:384-386, pattern
// literal :123) but laid out for the machine instead of for the document:
//
//   * the packed text of ALL documents is cut into regions of 64 x TKF_W bytes (TKF_W = 32: 2048); a wave owns one
//     region at a time, lane l owns bytes [W l, W l + W) and holds every class / rule mask as W bits of a VGPR
//     ("lane layout": one VALU instruction = one mask operation over the whole region; shifts borrow from
//     the neighbour lane with DPP, ripple carries cross lanes through a 64-bit carry look-ahead);
//   * document boundaries are a mask (DS): look-behind shifts are cut at a document start, look-ahead
//     shifts at a document end, runs are broken there -- documents never cost a branch;
//   * piece starts are enumerated into LDS and probed ONE LANE PER PIECE (64 probes per instruction
//     instead of ~13 with one lane per byte); the piece bytes come from an LDS copy of the region, the
//     probe is one scattered load for most pieces (KEY8: 16-byte entries; spill flags, tk_hash.h);
//   * a piece that misses the vocabulary reserves `len` id slots and is queued; tk_merge_wave merges the
//     queue ONE LANE PER PIECE (tiktoken's order) -- 64 independent chains of dependent
//     PAIR probes per wave at high occupancy -- and marks the slots it does not need as holes;
//   * ids are written chunk-dense (chunk c at tmp[c*TKF_STRIDE ..]), K[c] slots per chunk; the slot of
//     every document start inside its chunk (lstart) and the holes per document let tk_flat_assemble
//     cut the stream into documents and squeeze the holes out.
//
// Regions overlap: 32 bytes of left halo (look-behind context), 64 of right halo (look-ahead, piece
// ends), the rest committed (1952 bytes of 2048).  ASCII is classified from the bit planes alone; a region with multi-byte code
// points additionally looks the class of every lead byte up in the trie (the char-level rules use the
// char-start mask).  A document with a digit / CR-LF run that covers the whole left halo, a white-space
// run that reaches the end of the region or a piece of more than TKF_LONGCAP (256) bytes is flagged and redone by the
// per-document kernel (tk_encode_impl.h), which handles everything.  A piece of 65..256 bytes becomes a RECORD
// (step 6: slots reserved, the merge left to tk_flat_long_wave / tk_merge_long_wave) and its document stays here.
//
// The rules are modelled in tools/flat_split_model.py (Python ints as masks, checked against the
// oracle); tk_flat_lane.h is that model in lane layout.  Runs on the CPU wave emulator (tests/emu).
//
// The source (all against the wv_* primitives alone; the tail is tk_flat_tail_impl.h): tk_flat_lane.h -- LDS words of a wave (TKF_L_*), mask
// algebra (tkf_shl .. tkf_scan_excl), tkf_classify, tkf_rules, tkf_rules_json; tk_flat_chunk_impl.h -- tk_flat_chunk, steps 1 to 7 (tkf_walk_chars,
// tkf_long_pieces, tkf_doc_outputs and the shared helpers above it); tk_merge_impl.h -- the long-piece records (tk_flat_long_wave,
// tk_flat_long_coop_wave, tk_merge_long_wave), the merge of the queued misses (tk_merge_find / _wave / _lds), holes, the memo's log and commit
#ifndef TK_FLAT_IMPL_H
#define TK_FLAT_IMPL_H
#include "tk_flat_lane.h"
#include "tk_flat_chunk_impl.h"
#include "tk_merge_impl.h"
#endif
