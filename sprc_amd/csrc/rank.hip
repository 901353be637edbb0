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
// sprc_topk_wide: top-k for k up to 256 with an optional left-out column (the stage-2 validation takes the first 200 of the
// reference-less order): a running top-256 one key per THREAD, a 256-entry staging buffer in LDS fed by ballots, and a 512-key
// bitonic sort (shuffles inside a wave, LDS between waves) whenever staging fills.
// sprc_rerank_order: the stage-2 re-ordering of up to 256 candidates per query by (dist_bits(P), stage-1 position), and the new
// places of up to 16 listed items, with the same sorting network.
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

// Bitonic sort, ascending, of 256*E keys held E per thread by one 256-thread workgroup: item e of thread t is element t + 256*e.
// A compare-exchange distance below 64 stays inside a wave (cmpxchg: shuffles), 64 and 128 go through the LDS exchange arrays
// xk / xp (256*E entries each, two barriers per exchange), 256 is between a thread's own two items.  Every branch below is
// decided by k, j and E alone, so the whole workgroup reaches the same barriers.
template <int E>
__device__ __forceinline__ void block_bitonic_sort(Item (&it)[E], int tid, uint64_t* xk, uint32_t* xp) {
    const int lane = tid & 63;
#pragma unroll
    for (int k = 2; k <= 256 * E; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j == 256) {                                  // E == 2, k == 512: ascending over the whole sequence
                if (it[E - 1].key < it[0].key) {
                    const Item t = it[0];
                    it[0] = it[E - 1];
                    it[E - 1] = t;
                }
            } else if (j >= 64) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    xk[tid + 256 * e] = it[e].key;
                    xp[tid + 256 * e] = it[e].pos;
                }
                __syncthreads();
                Item o[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    o[e].key = xk[(tid ^ j) + 256 * e];
                    o[e].pos = xp[(tid ^ j) + 256 * e];
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool keep_min = (((tid + 256 * e) & k) == 0) == ((tid & j) == 0);
                    const bool take = keep_min ? (o[e].key < it[e].key) : (o[e].key > it[e].key);
                    if (take) it[e] = o[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) cmpxchg(it[e], lane, j, (((tid + 256 * e) & k) == 0) == ((tid & j) == 0));
            }
        }
    }
}

// One 256-thread workgroup per row; the row is read from HBM once, 256 elements per step (the next step's element is loaded
// before this step's barrier).  Thread t keeps key t of the running top-256 (sorted ascending across the workgroup); `thr` is
// its k-th key, ~0 until k keys have been seen.  A step ballots the keys below thr, the four wave counts meet in LDS (one
// barrier per step, the count slots alternate), and the passing keys are appended to the 256-entry staging buffer.  When they
// would not fit, and at the end of the row, top and staging are sorted as one 512-key sequence and the low half is the new
// top.  A key at or above thr can never be among the k smallest, whatever arrives later, and everything else reaches the
// sort: the result is the k smallest 64-bit keys of the row, however the row is cut into steps.  After the first steps
// almost nothing passes and a step costs its load, one ballot and one barrier.
__global__ __launch_bounds__(256) void topk_wide_kernel(const float* __restrict__ sim, int64_t ld, const int32_t* __restrict__ gidx,
                                                        int idx_base, const int32_t* __restrict__ skip, int N, int k,
                                                        float* __restrict__ out_sim, int32_t* __restrict__ out_idx) {
    __shared__ uint64_t s_xk[512];
    __shared__ uint32_t s_xp[512];
    __shared__ uint64_t s_sk[256];         // staging
    __shared__ uint32_t s_sp[256];
    __shared__ uint64_t s_thr;
    __shared__ int s_wcnt[3][4];           // [0], [1]: the steps' counts, alternating; [2]: the recount after a sort
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const float* row = sim + q * ld;
    const int32_t* grow = gidx ? gidx + q * (int64_t)N : nullptr;
    const int skipc = skip ? skip[q] : -1;

    Item top[2];                           // [0]: this thread's key of the running top-256; [1]: its staging key during a sort
    top[0].key = ~0ull;
    top[0].pos = 0xffffffffu;
    uint64_t thr = ~0ull;
    int nstage = 0;                        // the same in every thread

    auto flush = [&]() {                   // reached by the whole workgroup, after a barrier that follows the last staging write
        top[1].key = tid < nstage ? s_sk[tid] : ~0ull;
        top[1].pos = tid < nstage ? s_sp[tid] : 0xffffffffu;
        block_bitonic_sort<2>(top, tid, s_xk, s_xp);     // (its barriers also separate the staging reads above from later appends)
        if (tid == k - 1) s_thr = top[0].key;
        __syncthreads();
        thr = s_thr;
        nstage = 0;
    };

    const int nsteps = (N + 255) >> 8;
    float v = tid < N ? row[tid] : 0.0f;
    for (int c = 0; c < nsteps; ++c) {
        const int n = c * 256 + tid;
        const float vn = n + 256 < N ? row[n + 256] : 0.0f;
        uint64_t key = ~0ull;
        if (n < N && n != skipc) {
            const uint32_t id = grow ? (uint32_t)grow[n] : (uint32_t)(n + idx_base);
            key = ((uint64_t)dist_bits(v) << 32) | id;
        }
        v = vn;
        bool pass = key < thr;
        uint64_t bal = __ballot(pass);
        if (lane == 0) s_wcnt[c & 1][wave] = __popcll(bal);
        __syncthreads();
        int w0 = s_wcnt[c & 1][0], w1 = s_wcnt[c & 1][1], w2 = s_wcnt[c & 1][2], w3 = s_wcnt[c & 1][3];
        if (w0 + w1 + w2 + w3 == 0) continue;
        if (nstage + w0 + w1 + w2 + w3 > 256) {
            flush();
            pass = key < thr;              // a subset of what passed before: at most 256 keys, and staging is empty
            bal = __ballot(pass);
            if (lane == 0) s_wcnt[2][wave] = __popcll(bal);
            __syncthreads();
            w0 = s_wcnt[2][0], w1 = s_wcnt[2][1], w2 = s_wcnt[2][2], w3 = s_wcnt[2][3];
        }
        if (pass) {
            const int before = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
            const int at = nstage + before + __popcll(bal & ((1ull << lane) - 1ull));      // < 256 by the test above
            s_sk[at] = key;
            s_sp[at] = (uint32_t)n;
        }
        nstage += w0 + w1 + w2 + w3;
    }
    __syncthreads();
    if (nstage > 0) flush();
    if (tid < k) {
        const bool ok = top[0].pos != 0xffffffffu;
        out_idx[q * k + tid] = ok ? (int32_t)(uint32_t)top[0].key : -1;
        out_sim[q * k + tid] = ok ? row[top[0].pos] : -INFINITY;
    }
}

// One 256-thread workgroup per query, one candidate per thread: T <= 256 is exactly one item per thread of the sorting network
// above, so the sort is the 256-key case of the code sprc_topk_wide runs (a single wave would hold four items per lane and
// need a second network for them).  Key = (dist_bits(prob) << 32) | stage-1 position: integer comparisons only, ties keep the
// stage-1 order.  Padding candidates (id < 0) get the largest distance word and a low word above every position, so they
// follow every real candidate, a NaN one included, whatever their prob.  The sorted ids then sit in LDS and every thread
// compares its id with the up to 16 listed ones of the query.
constexpr int RERANK_L = 16;
__global__ __launch_bounds__(256) void rerank_order_kernel(const int32_t* __restrict__ cand, const float* __restrict__ prob, int T,
                                                           const int32_t* __restrict__ listed, const int32_t* __restrict__ listed_rank,
                                                           int L, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_rank) {
    __shared__ uint64_t s_xk[256];
    __shared__ uint32_t s_xp[256];
    __shared__ int32_t s_listed[RERANK_L];
    __shared__ int32_t s_rank[RERANK_L];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    Item it[1];
    it[0].key = ~0ull;
    it[0].pos = 0xffffffffu;
    int32_t id = -1;
    if (tid < T) {
        id = cand[q * T + tid];
        const uint32_t hi = id >= 0 ? dist_bits(prob[q * T + tid]) : 0xffffffffu;
        it[0].key = ((uint64_t)hi << 32) | (uint32_t)(id >= 0 ? tid : (0x80000000u | tid));
        it[0].pos = (uint32_t)(id >= 0 ? id : -1);          // the candidate's id travels with the key
    }
    if (tid < L) {
        const int32_t g = listed[q * L + tid];
        s_listed[tid] = g;
        s_rank[tid] = g >= 0 ? listed_rank[q * L + tid] : -1;
    }
    block_bitonic_sort<1>(it, tid, s_xk, s_xp);             // (has barriers: s_listed / s_rank are visible after it)
    const int32_t mine = tid < T ? (int32_t)it[0].pos : -1;
    if (tid < T) out_idx[q * T + tid] = mine;
    if (mine >= 0)
        for (int l = 0; l < L; ++l)
            if (s_listed[l] == mine) s_rank[l] = tid;
    __syncthreads();
    if (tid < L) out_rank[q * L + tid] = s_rank[tid];
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

extern "C" int sprc_topk_wide(const float* sim, int64_t ld, const int32_t* gidx, int32_t idx_base, const int32_t* skip, int32_t nq,
                              int32_t N, int32_t k, float* out_sim, int32_t* out_idx, sprc_stream s) {
    SPRC_REQUIRE(sim && out_sim && out_idx, "sprc_topk_wide: null pointer");
    SPRC_REQUIRE(nq > 0 && N >= 1 && ld >= N, "sprc_topk_wide: bad shape nq=%d N=%d ld=%lld", nq, N, (long long)ld);
    SPRC_REQUIRE(k >= 1 && k <= 256, "sprc_topk_wide: k=%d must be in [1,256]", k);
    ProfScope prof(SPRC_K_RANK, (hipStream_t)s, 0.0, (double)nq * N * (gidx ? 8.0 : 4.0) + (double)nq * k * 8.0);
    hipLaunchKernelGGL(topk_wide_kernel, dim3(nq), dim3(256), 0, (hipStream_t)s, sim, ld, gidx, idx_base, skip, N, k, out_sim, out_idx);
    SPRC_CHECK_LAUNCH("sprc_topk_wide");
    return SPRC_OK;
}

extern "C" int sprc_rerank_order(const int32_t* cand, const float* prob, int32_t nq, int32_t T, const int32_t* listed,
                                 const int32_t* listed_rank, int32_t L, int32_t* out_idx, int32_t* out_rank, sprc_stream s) {
    SPRC_REQUIRE(cand && prob && out_idx, "sprc_rerank_order: null pointer");
    SPRC_REQUIRE(nq > 0 && T >= 1 && T <= 256, "sprc_rerank_order: bad shape nq=%d T=%d (T must be in [1,256])", nq, T);
    SPRC_REQUIRE(L >= 0 && L <= RERANK_L, "sprc_rerank_order: L=%d must be in [0,%d]", L, RERANK_L);
    SPRC_REQUIRE(L == 0 || (listed && listed_rank && out_rank), "sprc_rerank_order: L=%d needs listed, listed_rank and out_rank", L);
    ProfScope prof(SPRC_K_RANK, (hipStream_t)s, 0.0, (double)nq * T * 12.0 + (double)nq * L * 12.0);
    hipLaunchKernelGGL(rerank_order_kernel, dim3(nq), dim3(256), 0, (hipStream_t)s, cand, prob, T, listed, listed_rank, L, out_idx, out_rank);
    SPRC_CHECK_LAUNCH("sprc_rerank_order");
    return SPRC_OK;
}
