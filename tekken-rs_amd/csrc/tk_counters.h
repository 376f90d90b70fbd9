// tk_counters.h -- the words (u32) of the context's device counter block (tk_ctx::counters) and of its pinned host mirror
// (tk_ctx::h_pin): the one map host and device code share.  Plain C++: the *_impl.h headers include it, the CPU wave emulator too.
#ifndef TK_COUNTERS_H
#define TK_COUNTERS_H

enum TkCounter {
    TKC_WORK = 0,            // work-queue head of the per-document kernels, ticket counter of the long-job queue
    TKC_DEFERRED = 1,        // documents pass 1 deferred to pass 2
    TKC_INVALID = 2,         // invalid documents (offsets check, UTF-8 validation)
    TKC_DEFER_MAXLEN = 3,    // the longest deferred document
    TKC_HANDED_BACK = 4,     // documents the flat path handed back (counted by the counts kernel)
    TKC_PASS2_SPARE = 5,     // pass 2's defer count (it defers nothing); tk_long_walk_kernel leaves TKC_OVERFLOW here
    TKC_TOTAL = 6,           // 6..7: total ids (u64, left by the assembly)
    TKC_PACK_BAD = 8,        // ids that do not fit the 18-bit wire format
    TKC_LONG_LIST = 9,       // documents pass 2 handed on to the round-based kernels
    TKC_LONG_JOBS = 10,      // long pieces the walk queued for them
    TKC_LONG_RECS = 11,      // long-piece records of the flat kernel
    TKC_CUT_CHUNKS = 12,     // chunks left to the CUT instantiation
    TKC_TODO = 13,           // handed-back documents as listed (tk_flat_todo_kernel)
    TKC_TODO_MAXLEN = 14,    // the longest of them
    TKC_LATE = 15,           // documents flagged late by a long-piece record
    TKC_LONG_CTL = 16,       // control words of the flat kernel (TkFlatArgs::long_ctl): long_recs lo, hi, long_cap
    TKC_LONG_CTL_HI = 17,
    TKC_LONG_CTL_CAP = 18,
    TKC_CUT_CTL = 19,        // cut_list lo, hi
    TKC_CUT_CTL_HI = 20,
    TKC_MEMO_HITS = 24,      // memo hits of the call (also cleared by the pre-pass)
    TKC_NARROW_LEFT = 25,    // pieces of 2..16 bytes the narrow merge kernel still had to merge

    TKC_CLEARED = 16,        // words 0..15: what the flat pre-pass (and the per-document pipeline's memset) clears
    TKC_EARLY_WORDS = 16,    // words of the early copy (stream B: the list of handed-back documents is made)
    TKC_FINAL_WORDS = 28,    // words of the final copy
    TKC_DEVICE_WORDS = 32,   // the device block
    TKC_EARLY_MIRROR = 32,   // word of h_pin at which the early copy lands (the final copy lands at 0)
    TKC_PIN_WORDS = 64       // h_pin
};
#define TKC_CTL(word) ((int)(word) - (int)TKC_LONG_CTL)   /* a word of the block as the flat kernel reaches it from its long_ctl pointer */
#define TKC_OVERFLOW 0xDEADu   /* in TKC_PASS2_SPARE: the long-piece job list overflowed */

static_assert(TKC_LONG_CTL >= TKC_CLEARED && TKC_CUT_CTL_HI < TKC_MEMO_HITS, "the control words lie outside what the pre-pass clears");
static_assert(TKC_TODO_MAXLEN < TKC_EARLY_WORDS && TKC_NARROW_LEFT < TKC_FINAL_WORDS && TKC_FINAL_WORDS <= TKC_DEVICE_WORDS, "copies hold what the host reads");
static_assert(TKC_FINAL_WORDS <= TKC_EARLY_MIRROR && TKC_EARLY_MIRROR + TKC_EARLY_WORDS <= TKC_PIN_WORDS, "both copies fit h_pin, apart");
static_assert(TKC_LONG_CTL_CAP == TKC_LONG_CTL + 2 && TKC_CUT_CTL == TKC_LONG_CTL + 3 && TKC_CUT_CTL_HI == TKC_CUT_CTL + 1, "one block of control words");

#endif
