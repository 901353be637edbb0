// search.hip -- index search: streaming small-batch scoring (sprc_sim_max_stream), its row-list form (sprc_sim_max_stream_rows)
// and the row-list form with a per-query admit mask (sprc_sim_max_stream_admit).
//
// sim[q, n] = max_j <fusion[q,:], feats[n,j,:]> for 1 <= nq <= 32 queries against a gallery that is read from HBM exactly once:
// 16 KiB per image (16-bit), 2 * 32 * 256 * nq flops per image -- at nq = 1 almost no arithmetic per byte.  sprc_sim_max runs this
// as a GEMM with M = nq on 256-row tiles and stages both operands through LDS; here the gallery goes global -> VGPR -> MFMA.
//
// One image per wave per 16 v_mfma_f32_32x32x16_{f16,bf16}:
//   A = the image's 32 feature rows: lane (r = l & 31, h = l >> 5) holds feats[n, r, 16 t + 8 h .. + 7] for k-step t -- one 16-B load
//       per k-step, 16 loads (64 VGPRs) per image;
//   B = the queries, zero-padded to 32 columns: lane (r, h) holds fusion[q = r, 16 t + 8 h .. + 7]; loaded once, 64 VGPRs for the
//       whole launch;
//   D = [feature row j][query q]: q on the lane (col = l & 31), j in the 16 registers x 2 lane halves, so max_j is 15 in-lane
//       v_max_f32 and one exchange between the halves.
// A wave holds two images' operands: the loads of images i + 2, i + 3 are issued behind the MFMAs of images i, i + 1 (hipcc
// interleaves the two chains) and every MFMA waits for its own fragment only (counted vmcnt, 5 .. 31 in the listing; 0 only in the
// peeled last trip, which fetches nothing).  No LDS, no barrier.  A workgroup (4 waves)
// takes STREAM_P = 8 consecutive images per loop trip and a contiguous range of trips; the grid is 2 workgroups per CU (256
// VGPRs each), so a CU has 16 images = 256 KiB in flight.  After a pair of images the lanes of half 0 store the first image's
// scores and the lanes of half 1 the second's: one store instruction per pair, 8 contiguous bytes per query.
// Products of 16-bit operands are exact in fp32; the sum runs in the MFMA's order over k (not the GEMM's K-tile order).
#include "common.hpp"

namespace sprc {

constexpr int STREAM_P = 8;              // images per workgroup per loop trip (sprc_amd/engine.py: STREAM_P)
constexpr int STREAM_WG_PER_CU = 2;
constexpr int STREAM_E = 256;
constexpr int STREAM_IMG_BYTES = 32 * STREAM_E * 2;

template <bool F16>
__device__ __forceinline__ f32x16 stream_mfma(const u32x4& a, const u32x4& b, f32x16 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the 16 operand loads of image n (clamped to the last image: a load is never predicated, so the compiler's waits stay counted)
__device__ __forceinline__ void stream_load(u32x4 (&a)[16], const char* lane_base, int n, int N) {
    const u32x4* p = reinterpret_cast<const u32x4*>(lane_base + (int64_t)min(n, N - 1) * STREAM_IMG_BYTES);
#pragma unroll
    for (int t = 0; t < 16; ++t) a[t] = p[2 * t];
}

template <bool F16>
__device__ __forceinline__ f32x16 stream_dot(const u32x4 (&a)[16], const u32x4 (&q)[16]) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; ++t) acc = stream_mfma<F16>(a[t], q[t], acc);
    return acc;
}

// max over the 32 feature rows of the lane's query: 16 registers, then the other lane half
__device__ __forceinline__ float stream_rowmax(const f32x16& acc) {
    float m = acc[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, acc[i]);
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

template <bool F16>
__global__ __launch_bounds__(256, 2) void sim_max_stream_kernel(const char* __restrict__ fusion, const char* __restrict__ feats,
                                                                float* __restrict__ sim, int64_t ld, int nq, int N, int trips) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    u32x4 q[16];
    {
        const u32x4* p = reinterpret_cast<const u32x4*>(fusion + (int64_t)min(r, nq - 1) * (STREAM_E * 2) + h * 16);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const u32x4 v = p[2 * t];
            q[t] = r < nq ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    const int t0 = (int)((int64_t)blockIdx.x * trips / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * trips / gridDim.x);
    if (t0 >= t1) return;
    const char* lane_base = feats + r * (STREAM_E * 2) + h * 16;
    float* out = sim + (int64_t)r * ld + h;          // lane (r, h) stores image n + h of its pair
    int n = t0 * STREAM_P + 2 * wave;                // first image of this wave's pair in the current trip
    u32x4 a0[16], a1[16];
    stream_load(a0, lane_base, n, N);
    stream_load(a1, lane_base, n + 1, N);
    for (int trip = t0; trip + 1 < t1; ++trip, n += STREAM_P) {
        const f32x16 c0 = stream_dot<F16>(a0, q);
        stream_load(a0, lane_base, n + STREAM_P, N);
        const f32x16 c1 = stream_dot<F16>(a1, q);
        stream_load(a1, lane_base, n + STREAM_P + 1, N);
        const float m0 = stream_rowmax(c0), m1 = stream_rowmax(c1);
        if (r < nq && n + h < N) out[n] = h ? m1 : m0;
    }
    const float m0 = stream_rowmax(stream_dot<F16>(a0, q)), m1 = stream_rowmax(stream_dot<F16>(a1, q));
    if (r < nq && n + h < N) out[n] = h ? m1 : m0;
}

// ---- the same walk through a row list (sprc_sim_max_stream_rows): position m of the list takes image rows[m] ------------------------
// The loop is sim_max_stream_kernel's (one image per wave per 16 MFMAs, two images held, the next pair's loads behind the current
// pair's MFMAs, peeled last trip, no LDS, no barrier) and the per-image chain is the same stream_dot, so sim[q, m] has the bits of
// the plain kernel's sim[q, rows[m]].  What is new is that a load's address depends on a value from memory.  The wave's two row
// indices of trip t + 2 are fetched while trip t computes and are first looked at in trip t + 1, whose loads they address: the fetch
// never sits between an MFMA chain and the loads behind it.  They are two 4-byte vector loads in the same in-order vmcnt queue as
// the operand loads, so their wait is one of the counted waits the MFMAs need anyway.  (Written as relaxed wave-scope atomic loads,
// which compile to plain global_load_dword: an ordinary load of a value that is only used a trip later is sunk by hipcc behind the
// trip's conditional store, to the loop's end, and waited for at once.)  The position is clamped to M - 1 and the row VALUE to
// [0, N - 1]: no list content addresses outside feats, and no load is predicated.
__device__ __forceinline__ int stream_row_ahead(const int32_t* rows, int m, int M) {
    return __hip_atomic_load(rows + min(m, M - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ int stream_row_clamp(int row, int N) { return min(max(row, 0), N - 1); }

__device__ __forceinline__ void stream_load_row(u32x4 (&a)[16], const char* feats, int lane_off, int row) {
    const u32x4* p = reinterpret_cast<const u32x4*>(feats + (int64_t)row * STREAM_IMG_BYTES + lane_off);
#pragma unroll
    for (int t = 0; t < 16; ++t) a[t] = p[2 * t];
}

template <bool F16>
__global__ __launch_bounds__(256, 2) void sim_max_stream_rows_kernel(const char* __restrict__ fusion, const char* __restrict__ feats,
                                                                     const int32_t* __restrict__ rows, float* __restrict__ sim, int64_t ld,
                                                                     int nq, int M, int N, int trips) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    u32x4 q[16];
    {
        const u32x4* p = reinterpret_cast<const u32x4*>(fusion + (int64_t)min(r, nq - 1) * (STREAM_E * 2) + h * 16);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const u32x4 v = p[2 * t];
            q[t] = r < nq ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    const int t0 = (int)((int64_t)blockIdx.x * trips / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * trips / gridDim.x);
    if (t0 >= t1) return;
    const int lane_off = r * (STREAM_E * 2) + h * 16;
    float* out = sim + (int64_t)r * ld + h;          // lane (r, h) stores position m + h of its pair
    int m = t0 * STREAM_P + 2 * wave;                // first list position of this wave's pair in the current trip
    u32x4 a0[16], a1[16];
    stream_load_row(a0, feats, lane_off, stream_row_clamp(rows[min(m, M - 1)], N));
    stream_load_row(a1, feats, lane_off, stream_row_clamp(rows[min(m + 1, M - 1)], N));
    int n0 = rows[min(m + STREAM_P, M - 1)], n1 = rows[min(m + STREAM_P + 1, M - 1)];      // the next trip's rows, as fetched
    for (int trip = t0; trip + 1 < t1; ++trip, m += STREAM_P) {
        const int j0 = stream_row_clamp(n0, N), j1 = stream_row_clamp(n1, N);                // fetched a trip ago
        n0 = stream_row_ahead(rows, m + 2 * STREAM_P, M), n1 = stream_row_ahead(rows, m + 2 * STREAM_P + 1, M);
        const f32x16 c0 = stream_dot<F16>(a0, q);
        stream_load_row(a0, feats, lane_off, j0);
        const f32x16 c1 = stream_dot<F16>(a1, q);
        stream_load_row(a1, feats, lane_off, j1);
        const float m0 = stream_rowmax(c0), m1 = stream_rowmax(c1);
        if (r < nq && m + h < M) out[m] = h ? m1 : m0;
    }
    const float m0 = stream_rowmax(stream_dot<F16>(a0, q)), m1 = stream_rowmax(stream_dot<F16>(a1, q));
    if (r < nq && m + h < M) out[m] = h ? m1 : m0;
}

// ---- the row-list walk with a per-query filter (sprc_sim_max_stream_admit): bit q of admit[m] admits image rows[m] for query q ---------
// Query q sits on lane column r = q and lane (r, h) stores position m + h of its pair, so the filter is one word per lane, admit[m + h],
// and one bit test at the store: an admitted score is the rows kernel's value (the same stream_dot chain on the same operands), any
// other element of sim[q < nq, 0..M) is -inf.  The store stays unconditional for r < nq && m + h < M and there is still one store
// instruction per pair.  The word of trip t + 1 is fetched at the top of trip t, next to the row indices and ahead of the trip's operand
// loads in the same in-order vmcnt queue: by the time trip t + 1 stores, its MFMAs have already waited for younger loads, so the word
// costs no wait of its own and never sits between an MFMA chain and the loads behind it.  Like the row indices it is a relaxed
// wave-scope atomic load with the position clamped to M - 1 (see stream_row_ahead: a plain load is sunk to the loop's end and waited
// for at once).  Bits at or above nq belong to lanes that store nothing.
__device__ __forceinline__ uint32_t stream_admit_ahead(const uint32_t* admit, int m, int M) {
    return __hip_atomic_load(admit + min(m, M - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

template <bool F16>
__global__ __launch_bounds__(256, 2) void sim_max_stream_admit_kernel(const char* __restrict__ fusion, const char* __restrict__ feats,
                                                                      const int32_t* __restrict__ rows, const uint32_t* __restrict__ admit,
                                                                      float* __restrict__ sim, int64_t ld, int nq, int M, int N, int trips) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    u32x4 q[16];
    {
        const u32x4* p = reinterpret_cast<const u32x4*>(fusion + (int64_t)min(r, nq - 1) * (STREAM_E * 2) + h * 16);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const u32x4 v = p[2 * t];
            q[t] = r < nq ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    const int t0 = (int)((int64_t)blockIdx.x * trips / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * trips / gridDim.x);
    if (t0 >= t1) return;
    const int lane_off = r * (STREAM_E * 2) + h * 16;
    float* out = sim + (int64_t)r * ld + h;          // lane (r, h) stores position m + h of its pair
    int m = t0 * STREAM_P + 2 * wave;                // first list position of this wave's pair in the current trip
    u32x4 a0[16], a1[16];
    stream_load_row(a0, feats, lane_off, stream_row_clamp(rows[min(m, M - 1)], N));
    stream_load_row(a1, feats, lane_off, stream_row_clamp(rows[min(m + 1, M - 1)], N));
    int n0 = rows[min(m + STREAM_P, M - 1)], n1 = rows[min(m + STREAM_P + 1, M - 1)];      // the next trip's rows, as fetched
    uint32_t w = admit[min(m + h, M - 1)];                                                  // this trip's admit word of the lane
    const float none = -__builtin_inff();
    for (int trip = t0; trip + 1 < t1; ++trip, m += STREAM_P) {
        const int j0 = stream_row_clamp(n0, N), j1 = stream_row_clamp(n1, N);                // fetched a trip ago
        n0 = stream_row_ahead(rows, m + 2 * STREAM_P, M), n1 = stream_row_ahead(rows, m + 2 * STREAM_P + 1, M);
        const uint32_t wn = stream_admit_ahead(admit, m + STREAM_P + h, M);                  // used by the next trip's store
        const f32x16 c0 = stream_dot<F16>(a0, q);
        stream_load_row(a0, feats, lane_off, j0);
        const f32x16 c1 = stream_dot<F16>(a1, q);
        stream_load_row(a1, feats, lane_off, j1);
        const float m0 = stream_rowmax(c0), m1 = stream_rowmax(c1);
        if (r < nq && m + h < M) out[m] = (w >> r) & 1u ? (h ? m1 : m0) : none;
        w = wn;
    }
    const float m0 = stream_rowmax(stream_dot<F16>(a0, q)), m1 = stream_rowmax(stream_dot<F16>(a1, q));
    if (r < nq && m + h < M) out[m] = (w >> r) & 1u ? (h ? m1 : m0) : none;
}

}  // namespace sprc

using namespace sprc;

extern "C" int sprc_sim_max_stream(const void* fusion, const void* feats, float* sim, int64_t ld_sim, int32_t nq, int32_t N, int32_t E,
                                   int32_t dtype, sprc_stream s) {
    SPRC_REQUIRE(fusion && feats && sim, "sprc_sim_max_stream: null pointer");
    SPRC_REQUIRE(nq >= 1 && nq <= 32, "sprc_sim_max_stream: nq=%d must be in [1,32] (walk more queries in blocks of 32)", nq);
    SPRC_REQUIRE(E == STREAM_E, "sprc_sim_max_stream: E=%d must be %d", E, STREAM_E);
    SPRC_REQUIRE(dtype == SPRC_F16 || dtype == SPRC_BF16, "sprc_sim_max_stream: dtype %d must be SPRC_F16 or SPRC_BF16", dtype);
    SPRC_REQUIRE(N >= 1 && ld_sim >= N, "sprc_sim_max_stream: bad shape N=%d ld_sim=%lld", N, (long long)ld_sim);
    SPRC_REQUIRE(((uintptr_t)fusion & 15) == 0 && ((uintptr_t)feats & 15) == 0, "sprc_sim_max_stream: fusion and feats must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const int trips = (int)(((int64_t)N + STREAM_P - 1) / STREAM_P);
    const int grid = min(trips, STREAM_WG_PER_CU * stream_cus(st));
    ProfScope prof(SPRC_K_RANK, st, 2.0 * nq * (double)N * 32.0 * E, (double)N * STREAM_IMG_BYTES + (double)nq * E * 2.0 + (double)nq * N * 4.0);
    const char* f = (const char*)fusion;
    const char* g = (const char*)feats;
    if (dtype == SPRC_F16)
        hipLaunchKernelGGL(sim_max_stream_kernel<true>, dim3(grid), dim3(256), 0, st, f, g, sim, ld_sim, nq, N, trips);
    else
        hipLaunchKernelGGL(sim_max_stream_kernel<false>, dim3(grid), dim3(256), 0, st, f, g, sim, ld_sim, nq, N, trips);
    SPRC_CHECK_LAUNCH("sprc_sim_max_stream");
    return SPRC_OK;
}

extern "C" int sprc_sim_max_stream_rows(const void* fusion, const void* feats, const int32_t* rows, float* sim, int64_t ld_sim, int32_t nq,
                                        int32_t M, int32_t N, int32_t E, int32_t dtype, sprc_stream s) {
    SPRC_REQUIRE(fusion && feats && rows && sim, "sprc_sim_max_stream_rows: null pointer");
    SPRC_REQUIRE(nq >= 1 && nq <= 32, "sprc_sim_max_stream_rows: nq=%d must be in [1,32] (walk more queries in blocks of 32)", nq);
    SPRC_REQUIRE(E == STREAM_E, "sprc_sim_max_stream_rows: E=%d must be %d", E, STREAM_E);
    SPRC_REQUIRE(dtype == SPRC_F16 || dtype == SPRC_BF16, "sprc_sim_max_stream_rows: dtype %d must be SPRC_F16 or SPRC_BF16", dtype);
    SPRC_REQUIRE(N >= 1 && M >= 1 && M <= INT32_MAX - 4 * STREAM_P && ld_sim >= M, "sprc_sim_max_stream_rows: bad shape M=%d N=%d ld_sim=%lld", M, N,
                 (long long)ld_sim);
    SPRC_REQUIRE(((uintptr_t)fusion & 15) == 0 && ((uintptr_t)feats & 15) == 0 && ((uintptr_t)rows & 3) == 0,
                 "sprc_sim_max_stream_rows: fusion and feats must be 16-byte aligned, rows 4-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const int trips = (int)(((int64_t)M + STREAM_P - 1) / STREAM_P);
    const int grid = min(trips, STREAM_WG_PER_CU * stream_cus(st));
    ProfScope prof(SPRC_K_RANK, st, 2.0 * nq * (double)M * 32.0 * E,
                   (double)M * (STREAM_IMG_BYTES + 4) + (double)nq * E * 2.0 + (double)nq * M * 4.0);
    const char* f = (const char*)fusion;
    const char* g = (const char*)feats;
    if (dtype == SPRC_F16)
        hipLaunchKernelGGL(sim_max_stream_rows_kernel<true>, dim3(grid), dim3(256), 0, st, f, g, rows, sim, ld_sim, nq, M, N, trips);
    else
        hipLaunchKernelGGL(sim_max_stream_rows_kernel<false>, dim3(grid), dim3(256), 0, st, f, g, rows, sim, ld_sim, nq, M, N, trips);
    SPRC_CHECK_LAUNCH("sprc_sim_max_stream_rows");
    return SPRC_OK;
}

extern "C" int sprc_sim_max_stream_admit(const void* fusion, const void* feats, const int32_t* rows, const uint32_t* admit, float* sim,
                                         int64_t ld_sim, int32_t nq, int32_t M, int32_t N, int32_t E, int32_t dtype, sprc_stream s) {
    SPRC_REQUIRE(fusion && feats && rows && admit && sim, "sprc_sim_max_stream_admit: null pointer");
    SPRC_REQUIRE(nq >= 1 && nq <= 32, "sprc_sim_max_stream_admit: nq=%d must be in [1,32] (walk more queries in blocks of 32)", nq);
    SPRC_REQUIRE(E == STREAM_E, "sprc_sim_max_stream_admit: E=%d must be %d", E, STREAM_E);
    SPRC_REQUIRE(dtype == SPRC_F16 || dtype == SPRC_BF16, "sprc_sim_max_stream_admit: dtype %d must be SPRC_F16 or SPRC_BF16", dtype);
    SPRC_REQUIRE(N >= 1 && M >= 1 && M <= INT32_MAX - 4 * STREAM_P && ld_sim >= M, "sprc_sim_max_stream_admit: bad shape M=%d N=%d ld_sim=%lld", M, N,
                 (long long)ld_sim);
    SPRC_REQUIRE(((uintptr_t)fusion & 15) == 0 && ((uintptr_t)feats & 15) == 0 && ((uintptr_t)rows & 3) == 0 && ((uintptr_t)admit & 3) == 0,
                 "sprc_sim_max_stream_admit: fusion and feats must be 16-byte aligned, rows and admit 4-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const int trips = (int)(((int64_t)M + STREAM_P - 1) / STREAM_P);
    const int grid = min(trips, STREAM_WG_PER_CU * stream_cus(st));
    ProfScope prof(SPRC_K_RANK, st, 2.0 * nq * (double)M * 32.0 * E,
                   (double)M * (STREAM_IMG_BYTES + 8) + (double)nq * E * 2.0 + (double)nq * M * 4.0);
    const char* f = (const char*)fusion;
    const char* g = (const char*)feats;
    if (dtype == SPRC_F16)
        hipLaunchKernelGGL(sim_max_stream_admit_kernel<true>, dim3(grid), dim3(256), 0, st, f, g, rows, admit, sim, ld_sim, nq, M, N, trips);
    else
        hipLaunchKernelGGL(sim_max_stream_admit_kernel<false>, dim3(grid), dim3(256), 0, st, f, g, rows, admit, sim, ld_sim, nq, M, N, trips);
    SPRC_CHECK_LAUNCH("sprc_sim_max_stream_admit");
    return SPRC_OK;
}
