// emu_fold_driver.cpp -- the FOLDED bookkeeping tail of the flat path (tk_flat_tail_impl.h: tkf_fold_apply_wave,
// tkf_counts_sums_wave, tkf_assemble_fold_waves) on the CPU wave emulator, next to emu_driver.cpp's run_flat_tail, which runs
// the pinned bodies (firstdoc, wavefirst, todo, counts, assemble_waves) with the scans done by the host.
// TEST INFRASTRUCTURE ONLY; see tk_wave_emu.h.  Built into a library of its own by tests/test_flat_tail_fold_emu.py.
//
// emu_fold_tail(t, fold_miss, fold_doc) takes the same case record as emu_flat_tail and tk_test_flat_tail_fold.  With both
// flags 0 it is the pinned flow; with a flag set that side runs the folded bodies with the thread / wave indices the launch
// functions of tk_flat.hip give the kernels (what tk_scan_block_sums and the counts kernel's LDS reduction do is done by the
// host here: neither is written against wv_*).  The folded miss side's prefix sums are compared here with the host's scan of
// the same counts (the case record has no room for them); everything else comes back in the record.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "tk_wave_emu.h"
#include "../../include/tekken_hip.h"
#include "../../tekken-rs_amd/csrc/tk_flat_tail_impl.h"
#include "../../tekken-rs_amd/csrc/tk_counters.h"
#include "../../tekken-rs_amd/csrc/tk_test_hooks.h"

namespace tkemu {
Wave* g_wave = nullptr;
Block* g_block = nullptr;
}

static std::string g_err;

namespace {
struct GBuf {   // n words between two guard zones
    std::vector<uint32_t> raw;
    size_t n;
    const char* name;
    GBuf(const char* nm, size_t words, const uint32_t* init) : raw(words + 2 * TK_TEST_GUARD_WORDS, TK_TEST_GUARD_FILL), n(words), name(nm) {
        if (init && words) memcpy(p(), init, words * 4);
    }
    uint32_t* p() { return raw.data() + TK_TEST_GUARD_WORDS; }
    bool intact() const {
        for (size_t i = 0; i < TK_TEST_GUARD_WORDS; ++i)
            if (raw[i] != TK_TEST_GUARD_FILL || raw[TK_TEST_GUARD_WORDS + n + i] != TK_TEST_GUARD_FILL) return false;
        return true;
    }
    void out(void* dst) { if (dst && n) memcpy(dst, p(), n * 4); }
};
template <class T> std::vector<T> exact(const T* p, size_t n) { return n ? std::vector<T>(p, p + n) : std::vector<T>(); }
}

static int run_fold_tail(TkTestTailCase& t, bool fold_miss, bool fold_doc) {
    const uint64_t D = t.n_docs, C = t.n_chunks;
    if (C == 0) fold_miss = false;      // (the pipeline folds only where there is something to scan)
    if (D == 0) fold_doc = false;
    const std::vector<uint64_t> doc_offs = exact(t.doc_offs, D + 1);
    const std::vector<uint32_t> kcount = exact(t.kcount, C), lstart = exact(t.lstart, D), tmp = exact(t.tmp, C * TKF_STRIDE),
                                staging = exact(t.staging, t.n_staging);
    // the pipeline scans the 4 C sub-queue counts and the C slot counts behind them as one array
    std::vector<uint32_t> mk(5 * C);
    for (uint64_t e = 0; e < 4 * C; ++e) mk[e] = t.miss_count[e];
    for (uint64_t c = 0; c < C; ++c) mk[4 * C + c] = kcount[c];
    std::vector<uint64_t> mpfx(5 * C + 1, 0);
    for (uint64_t e = 0; e < 5 * C; ++e) mpfx[e + 1] = mpfx[e] + mk[e];
    GBuf first_doc("first_doc", C, t.first_doc), flags("flags", D + 1, t.flags_cleared), holes("holes", D + 1, t.holes_cleared);
    GBuf ctr("the counters", TKC_DEVICE_WORDS, t.counters_in), wf("wave_first", t.n_wave_first, t.wave_first);
    GBuf wfw("wave_first_wide", t.n_wave_first_wide, t.wave_first_wide), todo("todo", D, t.todo), counts("counts", D, t.counts);
    GBuf info("the info records", 4 * D, nullptr), out_offs("out_offs", 2 * (D + 1), (const uint32_t*)t.out_offs), out_ids("out_ids", t.out_cap, t.out_ids);
    GBuf prefix("the folded prefix sums", fold_miss ? 2 * (5 * C + 1) : 0, nullptr);
    GBuf gsum("the group sums", fold_doc ? 2 * ((D + 63) / 64) : 0, nullptr), bsum("the document block sums", fold_doc ? 2 * ((D + 4095) / 4096) : 0, nullptr);
    GBuf* all[] = {&first_doc, &flags, &holes, &ctr, &wf, &wfw, &todo, &counts, &info, &out_offs, &out_ids, &prefix, &gsum, &bsum};
    for (uint64_t d = 0; d < D + 32; ++d) tkf_firstdoc_body(d, doc_offs.data(), D, C, first_doc.p(), flags.p(), holes.p(), ctr.p());
    first_doc.out(t.first_doc); flags.out(t.flags_cleared); holes.out(t.holes_cleared);
    if (D) { memcpy(flags.p(), t.flags, D * 4); memcpy(holes.p(), t.holes, D * 4); }
    ctr.p()[TKC_LONG_RECS] = t.long_recs;
    // ---- miss side ----
    std::vector<uint64_t> P(C + 1);
    if (fold_miss) {
        const uint64_t n = 5 * C;
        const std::vector<uint64_t> raw_sums = [&] {   // tk_scan_block_sums
            std::vector<uint64_t> s((n + TKF_FOLD_TILE - 1) / TKF_FOLD_TILE, 0);
            for (uint64_t e = 0; e < n; ++e) s[e / TKF_FOLD_TILE] += mk[e];
            return s;
        }();
        uint64_t* pf = reinterpret_cast<uint64_t*>(prefix.p());
        const uint64_t waves = ((n + TKF_FOLD_WAVE - 1) / TKF_FOLD_WAVE + 3) / 4 * 4;   // blocks of 256 threads
        for (uint64_t w = 0; w < waves; ++w)
            tkemu::run_wave([&](int lane) {
                tkf_fold_apply_wave(w, lane, mk.data(), n, C, raw_sums.data(), pf, wf.p(), wfw.p(), ctr.p() + TKC_NARROW_LEFT);
            });
        for (uint64_t e = 0; e <= n; ++e)
            if (pf[e] != mpfx[e]) {
                g_err = "the folded prefix sum of entry " + std::to_string(e) + " is " + std::to_string(pf[e]) + ", the scan's " + std::to_string(mpfx[e]);
                return TK_ERR_RUNTIME;
            }
        // (offset like tk_test_flat_tail_fold's: p_base stands in for the miss total)
        for (uint64_t c = 0; c <= C; ++c) P[c] = pf[4 * C + c] + (t.p_base - mpfx[4 * C]);
    } else {
        if (C)
            for (uint64_t e = 0; e < 4 * C + 32; ++e) tkf_wavefirst_body(e, mpfx.data(), C, wf.p(), wfw.p(), ctr.p() + TKC_NARROW_LEFT);
        for (uint64_t c = 0; c <= C; ++c) P[c] = mpfx[4 * C + c] - mpfx[4 * C] + t.p_base;
    }
    const uint64_t n_waves = (D + 255) / 256 * 4;
    for (uint64_t w = 0; w < n_waves; ++w)
        tkemu::run_wave([&](int lane) { tkf_todo_body(w * 64 + (uint64_t)lane, lane, flags.p(), doc_offs.data(), D, todo.p(), ctr.p() + TKC_TODO, ctr.p() + TKC_TODO_MAXLEN); });
    // ---- document side ----
    const uint32_t extra = (uint32_t)((t.add_bos ? 1 : 0) + (t.add_eos ? 1 : 0));
    TkFlatDocInfo* inf = reinterpret_cast<TkFlatDocInfo*>(info.p());
    uint64_t* oo = reinterpret_cast<uint64_t*>(out_offs.p());
    TkFlatAssembleArgs a;
    a.n_docs = D; a.info = inf; a.kcount = kcount.data(); a.out_offs = oo; a.tmp = tmp.data(); a.staging = staging.data();
    a.out_ids = out_ids.p(); a.bos_id = t.bos_id; a.eos_id = t.eos_id; a.add_bos = t.add_bos; a.add_eos = t.add_eos;
    a.total_out = reinterpret_cast<uint64_t*>(ctr.p() + TKC_TOTAL);
    a.skip_if = t.final_pass ? nullptr : ctr.p() + TKC_HANDED_BACK;
    const uint64_t aw = D > 64 ? 3 : 2;   // the waves stride over the documents
    if (fold_doc) {
        uint64_t* gs = reinterpret_cast<uint64_t*>(gsum.p());
        uint64_t* bs = reinterpret_cast<uint64_t*>(bsum.p());
        const uint64_t waves_per_block = TKF_FOLD_DOC_BLOCK / (64 * TKF_FOLD_GROUPS);
        for (uint64_t b = 0; b < (D + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK; ++b) {
            uint64_t block_sum = 0;                      // (the kernel: 16 wave sums through LDS, one barrier)
            for (uint64_t v = 0; v < waves_per_block; ++v) {
                uint64_t s[64];
                tkemu::run_wave([&](int lane) {
                    s[lane] = tkf_counts_sums_wave(b * waves_per_block + v, lane, doc_offs.data(), D, t.n_bytes, C, P.data(), lstart.data(), flags.p(),
                                                   holes.p(), extra, counts.p(), inf, t.final_pass, ctr.p() + TKC_HANDED_BACK, gs);
                });
                for (int l = 1; l < 64; ++l)
                    if (s[l] != s[0]) { g_err = "the wave sum differs between the lanes"; return TK_ERR_RUNTIME; }
                block_sum += s[0];
            }
            bs[b] = block_sum;
        }
        a.out_offs = nullptr;                            // (not read by the folded assembly)
        for (uint64_t w = 0; w < aw; ++w) tkemu::run_wave([&](int lane) { tkf_assemble_fold_waves(a, counts.p(), gs, bs, oo, w, aw, lane); });
    } else {
        for (uint64_t w = 0; w < n_waves; ++w)
            tkemu::run_wave([&](int lane) {
                tkf_counts_body(w * 64 + (uint64_t)lane, lane, doc_offs.data(), D, t.n_bytes, C, P.data(), lstart.data(), flags.p(), holes.p(), extra,
                                counts.p(), inf, t.final_pass, ctr.p() + TKC_HANDED_BACK);
            });
        uint64_t run = 0;
        for (uint64_t d = 0; d < D; ++d) { oo[d] = run; run += counts.p()[d]; }
        oo[D] = run;
        if (D)
            for (uint64_t w = 0; w < aw; ++w) tkemu::run_wave([&](int lane) { tkf_assemble_waves(a, w, aw, lane); });
    }
    for (GBuf* g : all)
        if (!g->intact()) { g_err = std::string("the tail wrote outside ") + g->name; return TK_ERR_RUNTIME; }
    wf.out(t.wave_first); wfw.out(t.wave_first_wide); todo.out(t.todo); counts.out(t.counts); out_offs.out(t.out_offs);
    out_ids.out(t.out_ids); ctr.out(t.counters_out);
    return TK_OK;
}

// fold = 0 never, 1 wherever the folded forms can run, -1 by the bounds (as TkKnobs::tail_fold and tk_test_flat_tail_fold)
extern "C" int emu_fold_tail(TkTestTailCase* t, int fold, uint32_t miss_max, uint32_t doc_max) {
    const uint64_t miss_sums = (5 * t->n_chunks + 2047) / 2048, doc_blocks = (t->n_docs + 4095) / 4096;
    const int rc = run_fold_tail(*t, fold != 0 && (fold == 1 || miss_sums <= miss_max), fold != 0 && (fold == 1 || doc_blocks <= doc_max));
    if (rc != TK_OK && t->err && t->err_cap) snprintf(t->err, t->err_cap, "%s", g_err.c_str());
    return rc;
}

// the slices of tkf_wave_sum_u64 / tkf_wave_scan_excl_u36 on values a test chose: out[0 .. 63] the exclusive scan of the low
// 36 bits, out[64] the sum of all 64 bits
extern "C" void emu_fold_wave_sums(const uint64_t* v, uint64_t* out) {
    tkemu::run_wave([&](int lane) {
        const uint64_t s = tkf_wave_sum_u64(v[lane]);
        const uint64_t x = tkf_wave_scan_excl_u36(v[lane] & 0xFFFFFFFFFull);
        out[lane] = x;
        if (lane == 17) out[64] = s;
    });
}
