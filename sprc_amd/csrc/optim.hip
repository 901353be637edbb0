// optim.hip -- the optimiser step of the fine-tuning loops (sprc.h "Optimiser step"): AdamW with decoupled weight decay over every
// tensor of a parameter group in one launch, GradScaler's unscale and inf-skip folded in (blip_fine_tune_2.py:257-259, :90-93, :302).
// Memory-bound: 28 bytes per element (read p, g, m, v; write p, m, v), no reuse -- the mapping is a chunk table over the tensors,
// 16-byte accesses, a grid of at most 2048 workgroups striding over the chunks.
#include "common.hpp"

#include <math.h>

namespace sprc {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_GRID = 2048;               // 256 CUs x 8 workgroups: every wave slot of the chip once

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// what the prologue leaves in sprc_adamw_args.scratch (40 of the 64 bytes)
struct OptScalars {
    float inv_scale, c_wd, w1, w2, beta2, bc2s, eps, nss;
    int32_t skip, pad;
};

// One wave, one working lane: the scalars of this step, formed in fp64 and rounded once (torch forms them in Python floats), from the
// DEVICE step counter -- a skipped step (found_inf != 0) leaves the counter alone.
__global__ __launch_bounds__(64) void adamw_prologue_kernel(double lr, double beta1, double beta2, double eps, double wd,
                                                            const float* grad_scale, const float* found_inf, float* step, OptScalars* out) {
    if (threadIdx.x != 0) return;
    OptScalars sc;
    sc.skip = (found_inf != nullptr && found_inf[0] != 0.0f) ? 1 : 0;
    sc.pad = 0;
    const float t = step[0] + (sc.skip ? 0.0f : 1.0f);
    if (!sc.skip) step[0] = t;
    sc.inv_scale = grad_scale ? (float)(1.0 / (double)grad_scale[0]) : 1.0f;       // GradScaler: _scale.double().reciprocal().float()
    sc.c_wd = (float)(1.0 - lr * wd);
    sc.w1 = (float)(1.0 - beta1);
    sc.w2 = (float)(1.0 - beta2);
    sc.beta2 = (float)beta2;
    sc.eps = (float)eps;
    const double td = (double)t;
    sc.bc2s = (float)sqrt(1.0 - pow(beta2, td));
    sc.nss = (float)(-(lr / (1.0 - pow(beta1, td))));
    *out = sc;
}

// The numerical contract (sprc.h): every operation rounds on its own, in this order.  hipcc contracts a * b + c into an fma by default;
// torch's scalar path does not.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const OptScalars& sc) {
#pragma clang fp contract(off)
    const float gs = g * sc.inv_scale;
    p = p * sc.c_wd;
    m = m + sc.w1 * (gs - m);
    v = v * sc.beta2 + (sc.w2 * gs) * gs;
    const float d = sqrtf(v) / sc.bc2s + sc.eps;
    p = p + sc.nss * (m / d);
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(const sprc_opt_tensor* __restrict__ tensors, int n_tensors,
                                                            const int32_t* __restrict__ chunk_first, int n_chunks,
                                                            const OptScalars* __restrict__ scalars) {
    const OptScalars sc = *scalars;
    if (sc.skip) return;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        int lo = 0, hi = n_tensors;                       // the LAST tensor with chunk_first[t] <= chunk (uniform over the workgroup)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_first[mid] <= chunk) lo = mid; else hi = mid;
        }
        const sprc_opt_tensor t = tensors[lo];
        const int64_t off = (int64_t)(chunk - chunk_first[lo]) * SPRC_OPT_CHUNK;
        const int64_t left = t.n - off;
        if (left <= 0) continue;                          // (a table that over-counts a tensor's chunks: nothing to do, never out of bounds)
        const int cnt = left < SPRC_OPT_CHUNK ? (int)left : SPRC_OPT_CHUNK;
        // pointers read from the table are generic to the compiler: say that they are global memory (global_load, not flat_load)
        gfloat* p = (gfloat*)t.p + off;
        const gfloat* g = (const gfloat*)t.g + off;
        gfloat* m = (gfloat*)t.m + off;
        gfloat* v = (gfloat*)t.v + off;
        const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
        int done = 0;
        if (aligned) {
            const int nvec = cnt >> 2;
#pragma unroll 4
            for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {
                f32x4 pp = ((const gf32x4*)p)[i];
                const f32x4 gg = ((const gf32x4*)g)[i];
                f32x4 mm = ((const gf32x4*)m)[i];
                f32x4 vv = ((const gf32x4*)v)[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pp[e], me = mm[e], ve = vv[e];
                    adamw_element(pe, gg[e], me, ve, sc);
                    pp[e] = pe; mm[e] = me; vv[e] = ve;
                }
                ((gf32x4*)p)[i] = pp;
                ((gf32x4*)m)[i] = mm;
                ((gf32x4*)v)[i] = vv;
            }
            done = nvec << 2;
        }
        for (int i = done + threadIdx.x; i < cnt; i += OPT_THREADS) {      // a base that is only 4-byte aligned, and the last n % 4 elements
            float pe = p[i], me = m[i], ve = v[i];
            adamw_element(pe, g[i], me, ve, sc);
            p[i] = pe; m[i] = me; v[i] = ve;
        }
    }
}

}  // namespace sprc

using namespace sprc;

extern "C" int sprc_adamw_step(const sprc_opt_tensor* tensors, int32_t n_tensors, const int32_t* chunk_first, int32_t n_chunks,
                               const sprc_adamw_args* a, sprc_stream s) {
    SPRC_REQUIRE(tensors && chunk_first && a, "sprc_adamw_step: null pointer (tensors, chunk_first or args)");
    SPRC_REQUIRE(a->step && a->scratch, "sprc_adamw_step: null pointer (step or scratch)");
    SPRC_REQUIRE(((uintptr_t)a->scratch & 7u) == 0, "sprc_adamw_step: scratch must be 8-byte aligned");
    SPRC_REQUIRE(n_tensors >= 1, "sprc_adamw_step: n_tensors = %d < 1", n_tensors);
    // every tensor has n >= 1, so its chunk count is >= 1 and the prefix ends at >= n_tensors; the table itself is on the device
    SPRC_REQUIRE(n_chunks >= n_tensors, "sprc_adamw_step: n_chunks = %d disagrees with the prefix of %d tensors (its last entry is >= %d)",
                 n_chunks, n_tensors, n_tensors);
    SPRC_REQUIRE(a->lr >= 0.0 && a->weight_decay >= 0.0, "sprc_adamw_step: lr = %g, weight_decay = %g must be >= 0", a->lr, a->weight_decay);
    SPRC_REQUIRE(a->beta1 >= 0.0 && a->beta1 < 1.0 && a->beta2 >= 0.0 && a->beta2 < 1.0, "sprc_adamw_step: betas (%g, %g) outside [0, 1)",
                 a->beta1, a->beta2);
    SPRC_REQUIRE(a->eps > 0.0, "sprc_adamw_step: eps = %g must be > 0", a->eps);
    hipStream_t st = (hipStream_t)s;
    OptScalars* sc = reinterpret_cast<OptScalars*>(a->scratch);
    hipLaunchKernelGGL(adamw_prologue_kernel, dim3(1), dim3(64), 0, st, a->lr, a->beta1, a->beta2, a->eps, a->weight_decay, a->grad_scale,
                       a->found_inf, a->step, sc);
    SPRC_CHECK_LAUNCH("sprc_adamw_step (prologue)");
    const int grid = n_chunks < OPT_MAX_GRID ? n_chunks : OPT_MAX_GRID;
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(OPT_THREADS), 0, st, tensors, (int)n_tensors, chunk_first, (int)n_chunks, sc);
    SPRC_CHECK_LAUNCH("sprc_adamw_step");
    return SPRC_OK;
}
