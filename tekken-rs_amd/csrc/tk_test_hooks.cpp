// tk_test_hooks.cpp -- TEST INFRASTRUCTURE ONLY (tk_test_hooks.h): compiled to nothing unless TK_TEST_HOOKS is defined, which only
// the development build (`make ablate`) does.  The bookkeeping tail of the flat path and the exclusive scan on inputs a test made
// up, through the launch functions the pipeline uses (tk_pipeline.cpp: run_pipeline_flat, flat_fork_todo, flat_finish), every
// array in an allocation of its own between two guard bands.
#ifdef TK_TEST_HOOKS
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "tk_kernels.h"
#include "tk_test_hooks.h"

namespace {
const size_t G = TK_TEST_GUARD_WORDS;

struct GDev {   // n words on the device between two guard bands
    uint32_t* base = nullptr;
    size_t n = 0;
    const char* name = "";
    hipError_t init(const char* nm, size_t words, const void* src) {
        name = nm; n = words;
        std::vector<uint32_t> h(words + 2 * G, TK_TEST_GUARD_FILL);
        if (src && words) memcpy(h.data() + G, src, words * 4);
        hipError_t e = hipMalloc((void**)&base, h.size() * 4);
        if (e != hipSuccess) return e;
        return hipMemcpy(base, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    }
    uint32_t* p() const { return base + G; }
    // the payload back into dst (may be NULL); *intact = 0 if a guard word changed
    hipError_t back(void* dst, int* intact) const {
        std::vector<uint32_t> h(n + 2 * G);
        hipError_t e = hipMemcpy(h.data(), base, h.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (size_t i = 0; i < G; ++i)
            if (h[i] != TK_TEST_GUARD_FILL || h[G + n + i] != TK_TEST_GUARD_FILL) *intact = 0;
        if (dst && n) memcpy(dst, h.data() + G, n * 4);
        return hipSuccess;
    }
    ~GDev() { if (base) (void)hipFree(base); }
    GDev() {}
    GDev(const GDev&) = delete;
    GDev& operator=(const GDev&) = delete;
};

int fail(TkTestTailCase* c, const std::string& what) {
    if (c && c->err && c->err_cap) snprintf(c->err, c->err_cap, "%s", what.c_str());
    return TK_ERR_RUNTIME;
}
}  // namespace

#define TT_HIP(call)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) return fail(c, std::string(#call) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// fold_miss / fold_doc: the folded forms of the two scans (tk_flat_tail_impl.h), chosen like tk_pipeline.cpp's flat_fold_choice does
static int run_tail(int device, TkTestTailCase* c, bool fold_miss, bool fold_doc, uint64_t* miss_prefix_out) {
    if (!c) return TK_ERR_INVALID_ARG;
    const uint64_t D = c->n_docs, C = c->n_chunks;
    TT_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    GDev doc_offs, kcount, miss_count, lstart, flags, holes, tmp, staging, ctr, counts, out_ids, first_doc, wf, wfw, todo, out_offs, info,
        mpfx, P, block_sums, mk_count, gsum, bsum;
    TT_HIP(doc_offs.init("doc_offs", 2 * (D + 1), c->doc_offs));
    TT_HIP(kcount.init("kcount", C, c->kcount));
    TT_HIP(miss_count.init("miss_count", 4 * C, c->miss_count));
    TT_HIP(lstart.init("lstart", D, c->lstart));
    TT_HIP(flags.init("flags", D + 1, c->flags_cleared));
    TT_HIP(holes.init("holes", D + 1, c->holes_cleared));
    TT_HIP(tmp.init("tmp", C * TKF_STRIDE, c->tmp));
    TT_HIP(staging.init("staging", c->n_staging, c->staging));
    TT_HIP(ctr.init("the counters", TKC_DEVICE_WORDS, c->counters_in));
    TT_HIP(counts.init("counts", D, c->counts));
    TT_HIP(out_ids.init("out_ids", c->out_cap, c->out_ids));
    TT_HIP(first_doc.init("first_doc", C, c->first_doc));
    TT_HIP(wf.init("wave_first", c->n_wave_first, c->wave_first));
    TT_HIP(wfw.init("wave_first_wide", c->n_wave_first_wide, c->wave_first_wide));
    TT_HIP(todo.init("todo", D, c->todo));
    TT_HIP(out_offs.init("out_offs", 2 * (D + 1), c->out_offs));
    TT_HIP(info.init("the info records", 4 * D, nullptr));
    TT_HIP(mpfx.init("the miss prefix sums", 2 * (4 * C + 1), nullptr));
    TT_HIP(P.init("the chunk prefix sums", 2 * (C + 1), nullptr));
    const uint64_t scanned = fold_miss ? 5 * C : 4 * C, longest = scanned > D ? scanned : D;
    TT_HIP(block_sums.init("the scan's block sums", 2 * (longest / 2048 + 2), nullptr));
    // the folded miss side scans what the pipeline scans: the sub-queue counts and the slot counts behind them, in one array
    std::vector<uint32_t> mk(5 * C);
    uint64_t miss_total = 0;
    for (uint64_t e = 0; e < 4 * C; ++e) { mk[e] = c->miss_count[e]; miss_total += mk[e]; }
    for (uint64_t k = 0; k < C; ++k) mk[4 * C + k] = c->kcount[k];
    TT_HIP(mk_count.init("the miss and slot counts", fold_miss ? 5 * C : 0, mk.data()));
    GDev mpfx5;
    TT_HIP(mpfx5.init("the miss and slot prefix sums", fold_miss ? 2 * (5 * C + 1) : 0, nullptr));
    TT_HIP(gsum.init("the group sums", fold_doc ? 2 * ((D + 63) / 64) : 0, nullptr));
    TT_HIP(bsum.init("the document block sums", fold_doc ? 2 * ((D + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK) : 0, nullptr));
    GDev* all[] = {&doc_offs, &kcount, &miss_count, &lstart, &flags, &holes, &tmp, &staging, &ctr, &counts, &out_ids, &first_doc, &wf, &wfw,
                   &todo, &out_offs, &info, &mpfx, &P, &block_sums, &mk_count, &mpfx5, &gsum, &bsum};
    int intact = 1;
    const uint64_t* d_offs = (const uint64_t*)doc_offs.p();
    // the pre-pass
    TT_HIP(tk_launch_flat_firstdoc(d_offs, D, C, first_doc.p(), flags.p(), holes.p(), ctr.p(), s));
    TT_HIP(hipStreamSynchronize(s));
    TT_HIP(first_doc.back(c->first_doc, &intact));
    TT_HIP(flags.back(c->flags_cleared, &intact));
    TT_HIP(holes.back(c->holes_cleared, &intact));
    // what the flat / merge kernels would have left
    if (D) {
        TT_HIP(hipMemcpy(flags.p(), c->flags, D * 4, hipMemcpyHostToDevice));
        TT_HIP(hipMemcpy(holes.p(), c->holes, D * 4, hipMemcpyHostToDevice));
    }
    TT_HIP(hipMemcpy(ctr.p() + TKC_LONG_RECS, &c->long_recs, 4, hipMemcpyHostToDevice));
    // the merge kernels' bookkeeping
    const uint64_t* d_P = (const uint64_t*)P.p();
    if (fold_miss) {
        // one scan like the pipeline's: the chunk prefix sums stand behind those of the miss counts, offset by the miss total
        TT_HIP(tk_launch_fold_apply(mk_count.p(), 5 * C, C, (uint64_t*)mpfx5.p(), (uint64_t*)block_sums.p(), wf.p(), wfw.p(),
                                    ctr.p() + TKC_NARROW_LEFT, s));
        if (miss_prefix_out) TT_HIP(hipMemcpy(miss_prefix_out, mpfx5.p(), (4 * C + 1) * 8, hipMemcpyDeviceToHost));   // (before the offset below)
        TT_HIP(tk_launch_add_u64((uint64_t*)mpfx5.p() + 4 * C, C + 1, c->p_base - miss_total, s));
        d_P = (const uint64_t*)mpfx5.p() + 4 * C;
    } else {
        TT_HIP(tk_launch_scan(miss_count.p(), 4 * C, (uint64_t*)mpfx.p(), (uint64_t*)block_sums.p(), s));
        if (miss_prefix_out) TT_HIP(hipMemcpy(miss_prefix_out, mpfx.p(), (4 * C + 1) * 8, hipMemcpyDeviceToHost));
        TT_HIP(tk_launch_merge_wavefirst((const uint64_t*)mpfx.p(), C, wf.p(), wfw.p(), ctr.p() + TKC_NARROW_LEFT, s));
        // the chunk prefix sums, offset like the pipeline's (they stand behind those of the miss counts)
        TT_HIP(tk_launch_scan(kcount.p(), C, (uint64_t*)P.p(), (uint64_t*)block_sums.p(), s));
        TT_HIP(tk_launch_add_u64((uint64_t*)P.p(), C + 1, c->p_base, s));
    }
    TT_HIP(tk_launch_flat_todo(flags.p(), d_offs, D, todo.p(), ctr.p() + TKC_TODO, ctr.p() + TKC_TODO_MAXLEN, s));
    const uint32_t extra = (uint32_t)((c->add_bos ? 1 : 0) + (c->add_eos ? 1 : 0));
    if (fold_doc) {
        TT_HIP(tk_launch_flat_counts_sums(d_offs, D, c->n_bytes, C, d_P, lstart.p(), flags.p(), holes.p(), extra, counts.p(), info.p(),
                                          c->final_pass, ctr.p() + TKC_HANDED_BACK, (uint64_t*)gsum.p(), (uint64_t*)bsum.p(), s));
        TT_HIP(tk_launch_flat_assemble_fold(D, info.p(), kcount.p(), counts.p(), (const uint64_t*)gsum.p(), (const uint64_t*)bsum.p(),
                                            (uint64_t*)out_offs.p(), tmp.p(), staging.p(), out_ids.p(), c->bos_id, c->eos_id, c->add_bos,
                                            c->add_eos, (uint64_t*)(ctr.p() + TKC_TOTAL), c->final_pass ? nullptr : ctr.p() + TKC_HANDED_BACK, s));
    } else {
        TT_HIP(tk_launch_flat_counts(d_offs, D, c->n_bytes, C, d_P, lstart.p(), flags.p(), holes.p(), extra, counts.p(),
                                     info.p(), c->final_pass, ctr.p() + TKC_HANDED_BACK, s));
        TT_HIP(tk_launch_scan(counts.p(), D, (uint64_t*)out_offs.p(), (uint64_t*)block_sums.p(), s));
        TT_HIP(tk_launch_flat_assemble(D, info.p(), kcount.p(), (const uint64_t*)out_offs.p(), tmp.p(), staging.p(), out_ids.p(), c->bos_id,
                                       c->eos_id, c->add_bos, c->add_eos, (uint64_t*)(ctr.p() + TKC_TOTAL),
                                       c->final_pass ? nullptr : ctr.p() + TKC_HANDED_BACK, s));
    }
    TT_HIP(hipStreamSynchronize(s));
    TT_HIP(wf.back(c->wave_first, &intact));
    TT_HIP(wfw.back(c->wave_first_wide, &intact));
    TT_HIP(todo.back(c->todo, &intact));
    TT_HIP(counts.back(c->counts, &intact));
    TT_HIP(out_offs.back(c->out_offs, &intact));
    TT_HIP(out_ids.back(c->out_ids, &intact));
    TT_HIP(ctr.back(c->counters_out, &intact));
    for (GDev* g : all) {
        int ok = 1;
        TT_HIP(g->back(nullptr, &ok));
        if (!ok) return fail(c, std::string("a guard word of ") + g->name + " changed");
    }
    if (!intact) return fail(c, "a guard word changed");
    return TK_OK;
}

extern "C" int tk_test_flat_tail(int device, TkTestTailCase* c) { return run_tail(device, c, false, false, nullptr); }

extern "C" int tk_test_flat_tail_fold(int device, TkTestTailCase* c, int fold, uint32_t miss_max, uint32_t doc_max, uint64_t* miss_prefix_out) {
    if (!c) return TK_ERR_INVALID_ARG;
    const uint64_t miss_sums = (5 * c->n_chunks + TKF_FOLD_TILE - 1) / TKF_FOLD_TILE, doc_blocks = (c->n_docs + TKF_FOLD_DOC_BLOCK - 1) / TKF_FOLD_DOC_BLOCK;
    return run_tail(device, c, c->n_chunks != 0 && fold != 0 && (fold == 1 || miss_sums <= miss_max),
                    c->n_docs != 0 && fold != 0 && (fold == 1 || doc_blocks <= doc_max), miss_prefix_out);
}

extern "C" int tk_test_scan(int device, const uint32_t* counts_h, uint64_t n, uint64_t* offs_out) {
    TkTestTailCase* c = nullptr;
    TT_HIP(hipSetDevice(device));
    GDev counts, offs, block_sums;
    TT_HIP(counts.init("counts", n, counts_h));
    TT_HIP(offs.init("offs", 2 * (n + 2), offs_out));
    TT_HIP(block_sums.init("block sums", 2 * (n / 2048 + 2), nullptr));
    TT_HIP(tk_launch_scan(counts.p(), n, (uint64_t*)offs.p(), (uint64_t*)block_sums.p(), nullptr));
    TT_HIP(hipStreamSynchronize(nullptr));
    int intact = 1;
    TT_HIP(counts.back(nullptr, &intact));
    TT_HIP(block_sums.back(nullptr, &intact));
    TT_HIP(offs.back(offs_out, &intact));
    return intact ? TK_OK : TK_ERR_RUNTIME;
}
#endif
