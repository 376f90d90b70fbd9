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

extern "C" int tk_test_flat_tail(int device, TkTestTailCase* c) {
    if (!c) return TK_ERR_INVALID_ARG;
    const uint64_t D = c->n_docs, C = c->n_chunks;
    TT_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    GDev doc_offs, kcount, miss_count, lstart, flags, holes, tmp, staging, ctr, counts, out_ids, first_doc, wf, wfw, todo, out_offs, info,
        mpfx, P, block_sums;
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
    const uint64_t longest = 4 * C > D ? 4 * C : D;
    TT_HIP(block_sums.init("the scan's block sums", 2 * (longest / 2048 + 2), nullptr));
    GDev* all[] = {&doc_offs, &kcount, &miss_count, &lstart, &flags, &holes, &tmp, &staging, &ctr, &counts, &out_ids, &first_doc, &wf, &wfw,
                   &todo, &out_offs, &info, &mpfx, &P, &block_sums};
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
    TT_HIP(tk_launch_scan(miss_count.p(), 4 * C, (uint64_t*)mpfx.p(), (uint64_t*)block_sums.p(), s));
    TT_HIP(tk_launch_merge_wavefirst((const uint64_t*)mpfx.p(), C, wf.p(), wfw.p(), ctr.p() + TKC_NARROW_LEFT, s));
    // the chunk prefix sums, offset like the pipeline's (they stand behind those of the miss counts)
    TT_HIP(tk_launch_scan(kcount.p(), C, (uint64_t*)P.p(), (uint64_t*)block_sums.p(), s));
    TT_HIP(tk_launch_add_u64((uint64_t*)P.p(), C + 1, c->p_base, s));
    TT_HIP(tk_launch_flat_todo(flags.p(), d_offs, D, todo.p(), ctr.p() + TKC_TODO, ctr.p() + TKC_TODO_MAXLEN, s));
    const uint32_t extra = (uint32_t)((c->add_bos ? 1 : 0) + (c->add_eos ? 1 : 0));
    TT_HIP(tk_launch_flat_counts(d_offs, D, c->n_bytes, C, (const uint64_t*)P.p(), lstart.p(), flags.p(), holes.p(), extra, counts.p(),
                                 info.p(), c->final_pass, ctr.p() + TKC_HANDED_BACK, s));
    TT_HIP(tk_launch_scan(counts.p(), D, (uint64_t*)out_offs.p(), (uint64_t*)block_sums.p(), s));
    TT_HIP(tk_launch_flat_assemble(D, info.p(), kcount.p(), (const uint64_t*)out_offs.p(), tmp.p(), staging.p(), out_ids.p(), c->bos_id,
                                   c->eos_id, c->add_bos, c->add_eos, (uint64_t*)(ctr.p() + TKC_TOTAL),
                                   c->final_pass ? nullptr : ctr.p() + TKC_HANDED_BACK, s));
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
