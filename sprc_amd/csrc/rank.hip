// rank.hip -- ranking stage (R7): wavefront bitonic top-k and exact rank counting.
//
// The ranking contract (oracle.rank_stable): order gallery items by the key
//   ( fl32(1 - sim) , index )  ascending
// i.e. a STABLE argsort of the fp32 distance the reference computes (validate_blip.py:253-254).
// Keys are built as 64-bit integers (order-preserving image of the fp32 distance in the high word,
// the index in the low word), so every comparison is an integer comparison and the result is
// bit-exact and independent of how the row is split across waves, workgroups or GPUs.
//
// sprc_topk: one 256-thread workgroup per query row.  Each of the 4 waves streams 64-element
// chunks of the row (coalesced 256-B reads), skips a chunk when none of its keys beats the wave's
// current 64th-best (one ballot), otherwise bitonic-sorts the chunk across lanes (21 compare-
// exchange stages on shuffles) and bitonic-merges it into its sorted running top-64 held one key
// per lane.  The 4 per-wave lists are merged through LDS.  HBM traffic = the sim row once.
// sprc_rank_of: position of listed gallery items in that order by counting smaller keys (no sort).
// sprc_ap_at_k: average precision at K over up to 32 ground truths per query (the CIRCO protocol): the ranks of all ground
// truths from ONE counting pass over the row, then AP@K in fp64 from those ranks, summed in ascending-rank order.
#include "common.hpp"

namespace sprc {

__device__ __forceinline__ uint32_t dist_bits(float sim) {
    const float d = 1.0f - sim;                      // the reference's `1 - pred_sim`, fp32
    if (d != d) return 0xffffffffu;                  // NaN sorts last (torch.argsort convention)
    uint32_t u = __float_as_uint(d + 0.0f);          // -0.0 -> +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Item {
    uint64_t key;      // (dist_bits << 32) | index
    uint32_t pos;      // position inside the row (to fetch the original sim at the end)
};

__device__ __forceinline__ Item shfl_item(const Item& a, int src) {
    Item r;
    const uint32_t lo = __shfl((uint32_t)a.key, src, 64);
    const uint32_t hi = __shfl((uint32_t)(a.key >> 32), src, 64);
    r.key = ((uint64_t)hi << 32) | lo;
    r.pos = __shfl(a.pos, src, 64);
    return r;
}

// compare-exchange with lane^j; keep_min: this lane keeps the smaller key
__device__ __forceinline__ void cmpxchg(Item& a, int lane, int j, bool keep_min) {
    const Item o = shfl_item(a, lane ^ j);
    const bool take = keep_min ? (o.key < a.key) : (o.key > a.key);
    if (take) a = o;
}

__device__ __forceinline__ void bitonic_sort64(Item& a, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool asc = (lane & k) == 0;                // k == 64 -> all ascending
            const bool lower = (lane & j) == 0;
            cmpxchg(a, lane, j, asc == lower);
        }
    }
}

// `a` holds a bitonic sequence across lanes -> ascending
__device__ __forceinline__ void bitonic_merge64(Item& a, int lane) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) cmpxchg(a, lane, j, (lane & j) == 0);
}

// top (sorted asc) <- 64 smallest of top U other (other sorted asc)
__device__ __forceinline__ void merge_keep_low(Item& top, const Item& other, int lane) {
    const Item rev = shfl_item(other, 63 - lane);
    if (rev.key < top.key) top = rev;
    bitonic_merge64(top, lane);
}

__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ sim, int64_t ld, const int32_t* __restrict__ gidx,
                                                   int idx_base, int N, int k, float* __restrict__ out_sim,
                                                   int32_t* __restrict__ out_idx) {
    __shared__ uint64_t s_key[4][64];
    __shared__ uint32_t s_pos[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const float* row = sim + q * ld;
    const int32_t* grow = gidx ? gidx + q * (int64_t)N : nullptr;

    Item top;
    top.key = ~0ull;
    top.pos = 0xffffffffu;
    const int nchunks = (N + 63) >> 6;
    for (int c = wave; c < nchunks; c += 4) {
        const int n = c * 64 + lane;
        Item it;
        it.key = ~0ull;
        it.pos = 0xffffffffu;
        if (n < N) {
            const uint32_t id = grow ? (uint32_t)grow[n] : (uint32_t)(n + idx_base);
            it.key = ((uint64_t)dist_bits(row[n]) << 32) | id;
            it.pos = (uint32_t)n;
        }
        const uint64_t worst = shfl_item(top, 63).key;
        if (!__any(it.key < worst)) continue;                // nothing in this chunk enters the top-64
        bitonic_sort64(it, lane);
        merge_keep_low(top, it, lane);
    }
    s_key[wave][lane] = top.key;
    s_pos[wave][lane] = top.pos;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            Item o;
            o.key = s_key[w][lane];
            o.pos = s_pos[w][lane];
            merge_keep_low(top, o, lane);
        }
        if (lane < k) {
            const bool ok = top.pos != 0xffffffffu;
            out_idx[q * k + lane] = ok ? (int32_t)(uint32_t)top.key : -1;
            out_sim[q * k + lane] = ok ? row[top.pos] : -INFINITY;
        }
    }
}

constexpr int RANK_L = 16;
__global__ __launch_bounds__(256) void rank_of_kernel(const float* __restrict__ sim, int64_t ld, const int32_t* __restrict__ listed,
                                                      int N, int L, int32_t* __restrict__ rank) {
    __shared__ uint64_t s_t[RANK_L];
    __shared__ int s_cnt[RANK_L];
    const int64_t q = blockIdx.x;
    const float* row = sim + q * ld;
    for (int l0 = 0; l0 < L; l0 += RANK_L) {
        const int nl = min(RANK_L, L - l0);
        if ((int)threadIdx.x < nl) {
            const int t = listed[q * L + l0 + threadIdx.x];
            s_t[threadIdx.x] = (t >= 0 && t < N) ? (((uint64_t)dist_bits(row[t]) << 32) | (uint32_t)t) : 0ull;
            s_cnt[threadIdx.x] = 0;
        }
        __syncthreads();
        int cnt[RANK_L];
#pragma unroll
        for (int l = 0; l < RANK_L; ++l) cnt[l] = 0;
        for (int n = threadIdx.x; n < N; n += 256) {
            const uint64_t key = ((uint64_t)dist_bits(row[n]) << 32) | (uint32_t)n;
#pragma unroll
            for (int l = 0; l < RANK_L; ++l)
                if (l < nl) cnt[l] += (key < s_t[l]) ? 1 : 0;
        }
#pragma unroll
        for (int l = 0; l < RANK_L; ++l) {
            if (l < nl) {
                int v = cnt[l];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if ((threadIdx.x & 63) == 0) atomicAdd(&s_cnt[l], v);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < nl) {
            const int t = listed[q * L + l0 + threadIdx.x];
            rank[q * L + l0 + threadIdx.x] = (t >= 0 && t < N) ? s_cnt[threadIdx.x] : -1;
        }
        __syncthreads();
    }
}

constexpr int AP_MAX_G = 32, AP_MAX_K = 8;
struct ApKs {
    int32_t k[AP_MAX_K];           // the K values, by value: the ABI takes them from HOST memory
};

// One workgroup per query.  The keys of the query's ground truths sit in LDS; every thread walks the row with stride 256
// (coalesced) and counts, for each of the GP ground-truth slots at once, the keys smaller than that slot's -- GP counters in
// registers, the row read once.  Wave sums by shuffle, the four waves meet in LDS (integer adds: order-free).  Wave 0 then
// places the ranks in ascending order (a ground truth's place among the ground truths is its own count of smaller ranks)
// and lane k sums the fp64 terms of ks.k[k] in that order.
template <int GP>
__global__ __launch_bounds__(256) void ap_at_k_kernel(const float* __restrict__ sim, int64_t ld, const int32_t* __restrict__ gt, int N,
                                                      int G, ApKs ks, int nk, double* __restrict__ ap, int32_t* __restrict__ rank) {
    __shared__ uint64_t s_t[GP];
    __shared__ int s_cnt[GP];
    __shared__ int s_sorted[AP_MAX_G];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float* row = sim + q * ld;
    if (tid < GP) {
        const int t = tid < G ? gt[q * G + tid] : -1;
        // padding gets key 0: no key of the row is smaller (a valid key has a non-zero high word), its count stays 0
        s_t[tid] = (t >= 0 && t < N) ? (((uint64_t)dist_bits(row[t]) << 32) | (uint32_t)t) : 0ull;
        s_cnt[tid] = 0;
    }
    if (tid < AP_MAX_G) s_sorted[tid] = 0x7fffffff;
    __syncthreads();
    int cnt[GP];
#pragma unroll
    for (int l = 0; l < GP; ++l) cnt[l] = 0;
    for (int n = tid; n < N; n += 256) {
        const uint64_t key = ((uint64_t)dist_bits(row[n]) << 32) | (uint32_t)n;
#pragma unroll
        for (int l = 0; l < GP; ++l) cnt[l] += (key < s_t[l]) ? 1 : 0;
    }
#pragma unroll
    for (int l = 0; l < GP; ++l) {
        int v = cnt[l];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((tid & 63) == 0) atomicAdd(&s_cnt[l], v);
    }
    __syncthreads();
    int n_gt = 0;                                  // ground truths of this query that are not padding
    if (tid < GP) {
        const bool valid = s_t[tid] != 0ull;
        const int r = valid ? s_cnt[tid] : -1;
        if (rank && tid < G) rank[q * G + tid] = r;
        int before = 0;                            // ground truths ranked before this one
        for (int j = 0; j < GP; ++j) {
            const bool vj = s_t[j] != 0ull;
            n_gt += vj ? 1 : 0;
            before += (vj && valid && s_cnt[j] < r) ? 1 : 0;
        }
        if (valid) s_sorted[before] = r;           // ranks are distinct (the index is part of the key): a permutation
    }
    __syncthreads();
    if (tid < nk) {
        const int K = ks.k[tid];
        double acc = 0.0;
        for (int i = 0; i < n_gt; ++i) {
            const int ri = s_sorted[i];
            if (ri < K) acc += (double)(i + 1) / (double)(ri + 1);
        }
        const int denom = n_gt < K ? n_gt : K;
        ap[q * nk + tid] = denom > 0 ? acc / (double)denom : 0.0;
    }
}

}  // namespace sprc

using namespace sprc;

extern "C" int sprc_topk(const float* sim, int64_t ld, const int32_t* gidx, int32_t idx_base, int32_t nq, int32_t N,
                         int32_t k, float* out_sim, int32_t* out_idx, sprc_stream s) {
    SPRC_REQUIRE(sim && out_sim && out_idx, "sprc_topk: null pointer");
    SPRC_REQUIRE(nq > 0 && N > 0 && ld >= N, "sprc_topk: bad shape nq=%d N=%d ld=%lld", nq, N, (long long)ld);
    SPRC_REQUIRE(k >= 1 && k <= 64, "sprc_topk: k=%d must be in [1,64]", k);
    ProfScope prof(SPRC_K_RANK, (hipStream_t)s, 0.0, (double)nq * N * (gidx ? 8.0 : 4.0) + (double)nq * k * 8.0);
    hipLaunchKernelGGL(topk_kernel, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gidx, idx_base, N, k, out_sim, out_idx);
    SPRC_CHECK_LAUNCH("sprc_topk");
    return SPRC_OK;
}

extern "C" int sprc_rank_of(const float* sim, int64_t ld, const int32_t* listed, int32_t nq, int32_t N, int32_t L,
                            int32_t* rank, sprc_stream s) {
    SPRC_REQUIRE(sim && listed && rank, "sprc_rank_of: null pointer");
    SPRC_REQUIRE(nq > 0 && N > 0 && L > 0 && ld >= N, "sprc_rank_of: bad shape");
    ProfScope prof(SPRC_K_RANK, (hipStream_t)s, 0.0, (double)nq * N * 4.0);
    hipLaunchKernelGGL(rank_of_kernel, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, listed, N, L, rank);
    SPRC_CHECK_LAUNCH("sprc_rank_of");
    return SPRC_OK;
}

extern "C" int sprc_ap_at_k(const float* sim, int64_t ld, const int32_t* gt, int32_t nq, int32_t N, int32_t G, const int32_t* ks,
                            int32_t nk, double* ap, int32_t* rank, sprc_stream s) {
    SPRC_REQUIRE(sim && gt && ks && ap, "sprc_ap_at_k: null pointer");
    SPRC_REQUIRE(nq > 0 && N > 0 && ld >= N, "sprc_ap_at_k: bad shape nq=%d N=%d ld=%lld", nq, N, (long long)ld);
    SPRC_REQUIRE(G >= 1 && G <= AP_MAX_G, "sprc_ap_at_k: G=%d must be in [1,%d]", G, AP_MAX_G);
    SPRC_REQUIRE(nk >= 1 && nk <= AP_MAX_K, "sprc_ap_at_k: nk=%d must be in [1,%d]", nk, AP_MAX_K);
    ApKs kk = {};
    for (int i = 0; i < nk; ++i) {
        SPRC_REQUIRE(ks[i] >= 1, "sprc_ap_at_k: ks[%d]=%d must be >= 1", i, ks[i]);
        kk.k[i] = ks[i];
    }
    ProfScope prof(SPRC_K_RANK, (hipStream_t)s, 0.0, (double)nq * N * 4.0);
    if (G <= 8)
        hipLaunchKernelGGL(ap_at_k_kernel<8>, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gt, N, G, kk, nk, ap, rank);
    else if (G <= 16)
        hipLaunchKernelGGL(ap_at_k_kernel<16>, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gt, N, G, kk, nk, ap, rank);
    else if (G <= 24)
        hipLaunchKernelGGL(ap_at_k_kernel<24>, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gt, N, G, kk, nk, ap, rank);
    else
        hipLaunchKernelGGL(ap_at_k_kernel<32>, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gt, N, G, kk, nk, ap, rank);
    SPRC_CHECK_LAUNCH("sprc_ap_at_k");
    return SPRC_OK;
}
