// tk_audio.hip -- the audio pass (include/tekken_hip.h "audio"): the log-mel features of a batch of clips, and the splice that
// puts the [AUDIO] runs of audio parts into the ragged input of the join pass.
//
// Log-mel.  A block takes a tile of TKA_FRAMES frames of one segment (TkaTile; the host lays the segments out).  It stages the
// (TKA_FRAMES - 1) H + W samples the tile's frames read in LDS, reflection about the segment's ends and the zero padding resolved
// while staging (a read past the clip's end is 0: the padding is never materialised).  The windowed DFT is an exact-f32 MFMA
// product against the [W][2F] table (tk_audio_tables.h), which stays L2-resident: a wave takes 32 bins of a round of
// TKA_ROUND_BINS and all 64 frames, so a pair of table values (real, imaginary part) feeds four 32x32x2 MFMAs on four independent
// accumulators, and the operands of the next eight steps are loaded while the MFMAs of these eight run.  The result tile has
// the frame on the lane and the bin in the registers: re^2 + im^2 goes to LDS as power[bin][frame], and behind a barrier every thread adds the round's bins to the mel sums it owns -- thread (frame, wave) owns
// the filters wave, wave + 4, ... of its frame, each filter a short contiguous run of bins, added in ascending bin order: the
// sums do not depend on anything outside the segment.  Behind the last round log10(max(mel, 1e-10)) is written with the frame
// on the lane (coalesced along t), and the segment's maximum is one wave reduction and one atomicMax on the bit pattern of the
// positive float max(mel, 1e-10) -- a maximum, so the order of the blocks does not matter.  The clamp kernel then rewrites the
// features in 16-byte accesses; with a fixed log_mel_max the product kernel writes the feature itself and nothing follows.
#include <hip/hip_runtime.h>
#include <math.h>

#include "tk_kernels.h"
#include "tk_layout.h"

typedef float __attribute__((ext_vector_type(16))) tka_f32x16;
typedef float __attribute__((ext_vector_type(4))) tka_f32x4;

#define TKA_PW_STRIDE (TKA_FRAMES + 1u)     /* power[bin][frame]: an odd row */
#define TKA_LDS_LIMIT (159u * 1024u)        /* of the CU's 160 KiB */
#define TKA_BATCH 8u                        /* steps whose operands are loaded together: 32 MFMAs */

// where sample j of the tile's staged run lies in LDS: one pad word per 32, so that the 32 frames of an MFMA operand, H apart,
// fall into different banks for the hops in use (H = 160: a stride of 165 words)
__device__ __forceinline__ uint32_t tka_slot(uint32_t j) { return j + (j >> 5); }

// p[j] of the definition for the tile whose first frame starts at sample `base` of the padded signal (base = t0 H - W / 2, which
// is negative in front of the segment): reflection about 0 and L - 1, zeros for the padding and for whatever a frame beyond the
// segment's last one would read
__device__ __forceinline__ float tka_sample(const float* x, int64_t base, uint32_t j, int64_t L, int64_t valid) {
    int64_t q = base + (int64_t)j;
    if (q < 0) q = -q;
    else if (q >= L) q = 2 * (L - 1) - q;
    return q >= 0 && q < valid ? x[q] : 0.f;
}

// log10 of a value that is at least the floor 1e-10f; the floor itself gives -10 exactly (its correctly rounded logarithm), so
// that silence is -1.5 whatever the library's last bit
__device__ __forceinline__ float tka_log10(float v) { return v == 1e-10f ? -10.f : log10f(v); }

template <int STAGED>
__global__ __launch_bounds__(TKA_BLOCK) void tk_logmel_kernel(const TkLogmelArgs a) {
    extern __shared__ float tka_lds[];
    float* s_samp = tka_lds;                                        // [lds_samples]
    float* s_pw = tka_lds + a.lds_samples;                          // [TKA_ROUND_BINS][TKA_PW_STRIDE]
    float* s_mel = s_pw + TKA_ROUND_BINS * TKA_PW_STRIDE;           // [M][TKA_FRAMES]
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const TkaTile tile = a.tiles[blockIdx.x];
    const TkaSegment seg = a.segs[tile.seg];
    const float* x = a.samples + seg.start;
    const uint32_t W = a.W, H = a.H, F = a.F, M = a.M;
    const int64_t L = (int64_t)seg.len, valid = (int64_t)seg.valid;
    const int64_t base = (int64_t)tile.t0 * H - (int64_t)(W / 2u);
    if (STAGED) {
        const uint32_t n_j = (TKA_FRAMES - 1u) * H + W;
        for (uint32_t j = tid; j < n_j; j += TKA_BLOCK) s_samp[tka_slot(j)] = tka_sample(x, base, j, L, valid);
    }
    for (uint32_t e = tid; e < M * TKA_FRAMES; e += TKA_BLOCK) s_mel[e] = 0.f;
    __syncthreads();

    const uint32_t j0 = col * H, j1 = (col + 32u) * H;              // where the lane's two frames start in the staged run
    for (uint32_t r0 = 0; r0 < F; r0 += TKA_ROUND_BINS) {
        const uint32_t b0 = r0 + wave * 32u;                        // (wave-uniform)
        if (b0 < F) {
            // A[i = bin][k = sample] = the table, B[k = sample][j = frame] = the samples: lane l holds A[l & 31][l >> 5] and
            // B[l >> 5][l & 31].  A bin beyond F - 1 repeats the last one; nothing reads its power
            const uint32_t bin = b0 + col < F ? b0 + col : F - 1u;
            const float* tre = a.dft + bin;
            const float* tim = tre + F;
            tka_f32x16 re0 = {0.f}, im0 = {0.f}, re1 = {0.f}, im1 = {0.f};
            // W is even: both lane halves make W / 2 steps of two samples.  The operands of a batch of TKA_BATCH steps are loaded
            // while the MFMAs of the batch before run: the table comes from L2, and one wave a SIMD has nothing else to hide
            // that latency behind.  A step beyond the last multiplies zeros
            const uint32_t steps = W / 2u, row2 = 2u * F;
            float are[2][TKA_BATCH], aim[2][TKA_BATCH], x0[2][TKA_BATCH], x1[2][TKA_BATCH];
            auto load = [&](uint32_t first, float* pre, float* pim, float* p0, float* p1) {
#pragma unroll
                for (uint32_t u = 0; u < TKA_BATCH; ++u) {
                    const bool ok = first + u < steps;              // (wave-uniform)
                    const uint32_t k = ok ? 2u * (first + u) + half : half;
                    const float vre = tre[(size_t)k * row2], vim = tim[(size_t)k * row2];
                    const float v0 = STAGED ? s_samp[tka_slot(j0 + k)] : tka_sample(x, base, j0 + k, L, valid);
                    const float v1 = STAGED ? s_samp[tka_slot(j1 + k)] : tka_sample(x, base, j1 + k, L, valid);
                    pre[u] = ok ? vre : 0.f; pim[u] = ok ? vim : 0.f; p0[u] = ok ? v0 : 0.f; p1[u] = ok ? v1 : 0.f;
                }
            };
            auto product = [&](const float* pre, const float* pim, const float* p0, const float* p1) {
#pragma unroll
                for (uint32_t u = 0; u < TKA_BATCH; ++u) {
                    re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pre[u], p0[u], re0, 0, 0, 0);
                    im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pim[u], p0[u], im0, 0, 0, 0);
                    re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pre[u], p1[u], re1, 0, 0, 0);
                    im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pim[u], p1[u], im1, 0, 0, 0);
                }
            };
            load(0u, are[0], aim[0], x0[0], x1[0]);
            for (uint32_t kk = 0; kk < steps; kk += 2u * TKA_BATCH) {
                load(kk + TKA_BATCH, are[1], aim[1], x0[1], x1[1]);
                product(are[0], aim[0], x0[0], x1[0]);
                load(kk + 2u * TKA_BATCH, are[0], aim[0], x0[0], x1[0]);
                if (kk + TKA_BATCH < steps) product(are[1], aim[1], x0[1], x1[1]);
            }
            // C: column (frame) = l & 31, row (bin) = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
#pragma unroll
            for (uint32_t r = 0; r < 16u; ++r) {
                const uint32_t row = (r & 3u) + 8u * (r >> 2) + 4u * half;
                float* p = s_pw + (wave * 32u + row) * TKA_PW_STRIDE + col;
                p[0] = fmaf(re0[r], re0[r], im0[r] * im0[r]);
                p[32] = fmaf(re1[r], re1[r], im1[r] * im1[r]);
            }
        }
        __syncthreads();
        // the round's bins into the mel sums: thread (frame = lane, wave) owns the filters wave, wave + 4, ... of its frame
        for (uint32_t m = wave; m < M; m += TKA_BLOCK / 64u) {
            const uint32_t first = a.fb_first[m], end = first + a.fb_count[m];
            const uint32_t lo = first > r0 ? first : r0, hi = end < r0 + TKA_ROUND_BINS ? end : r0 + TKA_ROUND_BINS;
            if (lo >= hi) continue;
            const float* w = a.fb_weights + a.fb_start[m];
            float acc = s_mel[m * TKA_FRAMES + lane];
            for (uint32_t b = lo; b < hi; ++b) acc = fmaf(w[b - first], s_pw[(b - r0) * TKA_PW_STRIDE + lane], acc);
            s_mel[m * TKA_FRAMES + lane] = acc;
        }
        __syncthreads();
    }

    // L = log10(max(mel, 1e-10)) with the frame on the lane; a NaN stays one
    const uint32_t frame = tile.t0 + lane;
    const bool live = frame < seg.frames;
    float* out = a.out + seg.out + frame;
    const float floor_fixed = a.fixed_max - 8.f;
    float vmax = 0.f;
    for (uint32_t m = wave; m < M; m += TKA_BLOCK / 64u) {
        if (!live) continue;
        const float mel = s_mel[m * TKA_FRAMES + lane];
        const float v = mel < 1e-10f ? 1e-10f : mel;
        float lg = tka_log10(v);
        if (a.seg_max) vmax = fmaxf(vmax, v);
        else lg = ((lg < floor_fixed ? floor_fixed : lg) + 4.f) * 0.25f;
        out[(size_t)m * seg.frames] = lg;
    }
    if (a.seg_max) {
        for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
        if (lane == 0u && vmax > 0.f) atomicMax(a.seg_max + tile.seg, __float_as_uint(vmax));
    }
}

// (max(L, Lmax - 8) + 4) / 4 in place, four elements a thread: the segment of the first comes from a search over frame_off, the
// others step on from it (a segment may have no frame)
__global__ __launch_bounds__(TKA_BLOCK) void tk_logmel_clamp_kernel(const TkLogmelArgs a) {
    const uint64_t n4 = (a.n_elems + 3u) / 4u;
    for (uint64_t i = (uint64_t)blockIdx.x * TKA_BLOCK + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * TKA_BLOCK) {
        const uint64_t e0 = 4u * i;
        uint64_t s = tky_count_le(a.frame_off, (uint64_t)a.n_segs + 1u, e0 / a.M) - 1u;   // the last segment that starts at or before e0
        uint64_t end = a.M * a.frame_off[s + 1u];
        float floor_s = tka_log10(__uint_as_float(a.seg_max[s])) - 8.f;
        const uint32_t n = a.n_elems - e0 < 4u ? (uint32_t)(a.n_elems - e0) : 4u;
        float v[4];
        if (n == 4u) {
            const tka_f32x4 q = *reinterpret_cast<const tka_f32x4*>(a.out + e0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (uint32_t k = 0; k < n; ++k) v[k] = a.out[e0 + k];
        }
        for (uint32_t k = 0; k < n; ++k) {
            while (e0 + k >= end) {                                 // (e0 + k < n_elems: a later segment holds it)
                ++s;
                end = a.M * a.frame_off[s + 1u];
                floor_s = tka_log10(__uint_as_float(a.seg_max[s])) - 8.f;
            }
            v[k] = ((v[k] < floor_s ? floor_s : v[k]) + 4.f) * 0.25f;
        }
        if (n == 4u) {
            const tka_f32x4 q = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<tka_f32x4*>(a.out + e0) = q;
        } else {
            for (uint32_t k = 0; k < n; ++k) a.out[e0 + k] = v[k];
        }
    }
}

hipError_t tk_launch_logmel(const TkLogmelArgs& args, hipStream_t s) {
    if (args.n_tiles == 0u) return hipSuccess;
    TkLogmelArgs a = args;
    const uint32_t last = (TKA_FRAMES - 1u) * a.H + a.W - 1u;      // the last staged sample
    const uint32_t want = last + (last >> 5) + 1u;
    const size_t rest = ((size_t)TKA_ROUND_BINS * TKA_PW_STRIDE + (size_t)a.M * TKA_FRAMES) * sizeof(float);
    a.staged = rest + (size_t)want * sizeof(float) <= TKA_LDS_LIMIT ? 1u : 0u;
    a.lds_samples = a.staged ? want : 0u;
    const size_t lds = rest + (size_t)a.lds_samples * sizeof(float);
    hipError_t e;
    if (a.staged) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tk_logmel_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TKA_LDS_LIMIT);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tk_logmel_kernel<1>, dim3(a.n_tiles), dim3(TKA_BLOCK), lds, s, a);
    } else {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tk_logmel_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TKA_LDS_LIMIT);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tk_logmel_kernel<0>, dim3(a.n_tiles), dim3(TKA_BLOCK), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t tk_launch_logmel_clamp(const TkLogmelArgs& a, hipStream_t s) {
    if (a.n_elems == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_logmel_clamp_kernel, dim3(tky_blocks((a.n_elems + 3u) / 4u, 1u << 16)), dim3(TKA_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- the splice: per part its own ids, then part_tokens[p] copies of fill_id ----
// the ids of part p: the offsets are the caller's and not checked, so a decreasing pair is an empty part and nothing at or beyond
// n_ids is read
__device__ __forceinline__ uint64_t tks_own(const TkSpliceArgs& a, uint64_t p) {
    const uint64_t lo = a.id_offs[p], hi = a.id_offs[p + 1u] < a.n_ids ? a.id_offs[p + 1u] : a.n_ids;
    return hi > lo ? hi - lo : 0u;
}
__global__ __launch_bounds__(TKY_BLOCK) void tk_splice_counts_kernel(const TkSpliceArgs a) {
    for (uint64_t p = (uint64_t)blockIdx.x * TKY_BLOCK + threadIdx.x; p < a.n_parts; p += (uint64_t)gridDim.x * TKY_BLOCK)
        a.counts[p] = tky_len32(tks_own(a, p) + a.part_tokens[p]);
}

// a block takes tile after tile of TKY_TILE output positions (the join kernel's launch shape), a thread four consecutive ones a
// step: the part of the first comes from a search over the new offsets, the others step on from it; one 16-byte store
__global__ __launch_bounds__(TKY_BLOCK) void tk_splice_fill_kernel(const TkSpliceArgs a) {
    const uint64_t n_tiles = (a.n_out + TKY_TILE - 1u) / TKY_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        for (uint32_t u = threadIdx.x; u < TKY_TILE / 4u; u += TKY_BLOCK) {
            const uint64_t g = tile * TKY_TILE + 4u * u;
            if (g >= a.n_out) break;
            const uint32_t n = a.n_out - g < 4u ? (uint32_t)(a.n_out - g) : 4u;
            uint64_t p = tky_count_le(a.out_offs, a.n_parts + 1u, g) - 1u;      // the last part that starts at or before g
            uint64_t start = a.out_offs[p], end = a.out_offs[p + 1u], src = a.id_offs[p], own = tks_own(a, p);
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            for (uint32_t k = 0; k < n; ++k) {
                while (g + k >= end) {                              // (g + k < n_out: a later part holds it)
                    ++p;
                    start = end; end = a.out_offs[p + 1u]; src = a.id_offs[p]; own = tks_own(a, p);
                }
                const uint64_t local = g + k - start;
                v[k] = local < own ? a.ids[src + local] : a.fill_id;
            }
            if (n == 4u) tky_store<0, 1>(a.out_ids, g, v);
            else for (uint32_t k = 0; k < n; ++k) a.out_ids[g + k] = v[k];
        }
    }
}

hipError_t tk_launch_splice_counts(const TkSpliceArgs& a, hipStream_t s) {
    if (a.n_parts == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_splice_counts_kernel, dim3(tky_blocks(a.n_parts, 4096u)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t tk_launch_splice_fill(const TkSpliceArgs& a, hipStream_t s) {
    if (a.n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(tk_splice_fill_kernel, dim3(tky_blocks(a.n_out, 1u << 16, TKY_TILE)), dim3(TKY_BLOCK), 0, s, a);
    return hipGetLastError();
}
