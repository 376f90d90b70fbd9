// tk_test_hooks.h -- TEST INFRASTRUCTURE ONLY: entries of the development build (`make ablate`, -DTK_TEST_HOOKS) that run single
// stages of the pipeline on inputs a test made up, through the product's own launch functions.  They are not part of
// include/tekken_hip.h and the shipped libtekken_hip.so does not export them (tests/test_host_tokenizer.py checks that).
// The CPU wave emulator (tests/emu/emu_driver.cpp: emu_flat_tail) takes the same case record.
#ifndef TK_TEST_HOOKS_H
#define TK_TEST_HOOKS_H
#include <stdint.h>

// One layout for the bookkeeping tail of the flat path (tk_flat_tail_impl.h): what the flat / merge / per-document kernels
// would have left behind, and room for everything the tail makes of it.  The arrays marked in/out are pre-filled by the
// caller and come back as the tail left them; every array is exactly as long as stated.
struct TkTestTailCase {
    uint64_t n_docs, n_bytes, n_chunks;
    uint64_t p_base;              // added to the chunk prefix sums (the pipeline passes them offset by the miss total)
    const uint64_t* doc_offs;     // [n_docs + 1]
    const uint32_t* kcount;       // [n_chunks]
    const uint32_t* miss_count;   // [4 * n_chunks]
    const uint32_t* lstart;       // [n_docs]
    const uint32_t* flags;        // [n_docs]
    const uint32_t* holes;        // [n_docs]
    const uint32_t* tmp;          // [n_chunks * TKF_STRIDE]
    const uint32_t* staging;      // [n_staging]
    uint64_t n_staging;
    const uint32_t* counters_in;  // [TKC_DEVICE_WORDS] the counter block before the pre-pass
    uint32_t long_recs;           // TKC_LONG_RECS as the flat kernel left it
    uint32_t bos_id, eos_id;
    int32_t add_bos, add_eos;
    int32_t final_pass;           // 0: the optimistic pass (skip_if set), 1: the final pass
    uint64_t out_cap;             // words of out_ids
    uint64_t n_wave_first, n_wave_first_wide;
    uint32_t* counts;             // in/out [n_docs]
    uint32_t* out_ids;            // in/out [out_cap]
    uint32_t* first_doc;          // in/out [n_chunks]
    uint32_t* flags_cleared;      // in/out [n_docs + 1] the flags as the pre-pass left them (the layout's are set afterwards)
    uint32_t* holes_cleared;      // in/out [n_docs + 1]
    uint32_t* wave_first;         // in/out [n_wave_first]
    uint32_t* wave_first_wide;    // in/out [n_wave_first_wide]
    uint32_t* todo;               // in/out [n_docs]
    uint64_t* out_offs;           // in/out [n_docs + 1]
    uint32_t* counters_out;       // out [TKC_DEVICE_WORDS] the counter block at the end (TKC_TODO, TKC_TODO_MAXLEN,
                                  // TKC_HANDED_BACK, TKC_TOTAL, TKC_NARROW_LEFT)
    char* err;                    // out: what went wrong (a changed guard word, a failed call)
    uint32_t err_cap;
};

#define TK_TEST_GUARD_WORDS 64u          /* guard band on either side of every array the tail writes */
#define TK_TEST_GUARD_FILL 0xDEADBEEFu

#ifdef __cplusplus
extern "C" {
#endif
// 0, or an error code with the reason in c->err.  The development build only.
int tk_test_flat_tail(int device, struct TkTestTailCase* c);
// the same with the folded forms of the two scans (tk_flat_tail_impl.h) where tk_pipeline.cpp would take them: fold = 0 never,
// 1 wherever they can run, -1 while the miss side has at most miss_max block sums / the documents at most doc_max blocks of 4096
// miss_prefix_out: NULL, or [4 n_chunks + 1] words for the prefix sums of the sub-queue counts as the merge kernels would read them
int tk_test_flat_tail_fold(int device, struct TkTestTailCase* c, int fold, uint32_t miss_max, uint32_t doc_max, uint64_t* miss_prefix_out);
// offs[0 .. n] = exclusive prefix sums of counts[0 .. n) through tk_launch_scan; offs must hold n + 2 words: the last one comes
// back as it went in
int tk_test_scan(int device, const uint32_t* counts, uint64_t n, uint64_t* offs_out);
#ifdef __cplusplus
}
#endif

#endif
