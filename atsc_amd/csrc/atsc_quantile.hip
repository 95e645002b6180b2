// atsc_quantile.hip -- gfx950 kernels of the windowed quantiles (atsc_quantile_windows_dev): exact order statistics of
// sample windows, selected from decoded samples in the call's scratch.
//
// The contract (include/atsc_hip.h, DESIGN.md "Windowed quantiles"): a window's non-NaN samples x[0..n) sorted by the
// total-order key below (-0.0 before +0.0); for level q, v = (double)(n - 1) * q, the ranks and the interpolation of
// q_pick / q_interp (atsc_quantile_rule.h).  Every tier reads its ranks and values through those two functions.
//   short  (n <= QNT_SHORT_MAX)   one wavefront per window: up to 4 keys per lane, bitonic sort across the wave
//                                 with __shfl_xor, every level's samples fetched by lane shuffle
//   medium (n <= QNT_MEDIUM_MAX)  one workgroup per window: the keys bitonic-sorted in LDS
//   long                          MSD radix select over 8-bit digits: per pass, k_qnt_hist counts the digits of the
//                                 samples that match a live prefix (many workgroups per window, LDS counts flushed with
//                                 integer atomics) and k_qnt_pick, one workgroup per window, walks the counts to the
//                                 digit holding each needed rank.  After QNT_PASSES passes every rank's key is known.
// Selection is exact: no float atomics, no order of addition to keep.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"
#include "atsc_quantile_rule.h"

namespace atsc {

namespace {

constexpr uint32_t QNT_LDS_ROWS = 32; // k_qnt_hist counts in LDS up to this many live prefixes, in global memory beyond

// ---- short tier ---------------------------------------------------------------------------------------------------
// K keys per lane; element e = lane * K + r lives in v[r]
template <int K>
__device__ __forceinline__ void wave_sort(uint64_t (&v)[4], uint32_t lane)
{
#pragma unroll
    for (uint32_t k = 2; k <= 64u * K; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j < (uint32_t)K) {
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    if (r & j) continue;
                    const bool up = ((lane * K + r) & k) == 0;
                    const uint64_t a = v[r], b = v[r + j];
                    const bool sw = up ? a > b : a < b;
                    v[r] = sw ? b : a;
                    v[r + j] = sw ? a : b;
                }
            } else {
                const uint32_t lj = j / K;
                const bool lower = (lane & lj) == 0;
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const uint64_t o = __shfl_xor(v[r], (int)lj, 64);
                    const bool up = ((lane * K + r) & k) == 0;
                    v[r] = (lower == up) ? (o < v[r] ? o : v[r]) : (o > v[r] ? o : v[r]);
                }
            }
        }
    }
}

template <int K>
__device__ __forceinline__ uint64_t wave_at(const uint64_t (&v)[4], uint64_t e)
{
    uint64_t o = 0;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const uint64_t w = __shfl(v[r], (int)(e / K), 64);
        o = (e % K == (uint64_t)r) ? w : o;
    }
    return o;
}

// lane j (< n_q) writes level j; every lane takes part in the shuffles
template <int K>
__device__ __forceinline__ void short_finish(uint64_t (&v)[4], uint32_t lane, uint32_t nv, const double *q, uint32_t n_q,
                                             int method, double *out)
{
    wave_sort<K>(v, lane);
    const uint32_t j = lane < n_q ? lane : n_q - 1;
    const QPick p = nv ? q_pick(nv, q[j], method) : QPick{0, 0, 0.0};
    const double a = q_unkey(wave_at<K>(v, p.lo)), b = q_unkey(wave_at<K>(v, p.hi));
    if (lane < n_q) out[j] = nv ? q_interp(p, a, b) : __builtin_nan("");
}

}  // namespace

// One wavefront per window of at most QNT_SHORT_MAX samples (an empty window included: NaN for every level).
__global__ __launch_bounds__(256) void k_qnt_short(const DevQTask *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, const double *__restrict__ q,
                                                   uint32_t n_q, int method, double *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n) return;
    const DevQTask t = tasks[i];
    const double *x = scratch + t.src;
    uint64_t v[4];
    uint32_t nv = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t e = 64u * r + lane;
        uint64_t k = KEY_NAN;
        if (e < t.n) {
            const double d = x[e];
            if (!__builtin_isnan(d)) k = q_key(d);
        }
        v[r] = k;
        nv += (uint32_t)__popcll(__ballot(k != KEY_NAN));
    }
    double *o = out + (uint64_t)t.win * n_q;
    if (t.n <= 64) short_finish<1>(v, lane, nv, q, n_q, method, o);
    else if (t.n <= 128) short_finish<2>(v, lane, nv, q, n_q, method, o);
    else short_finish<4>(v, lane, nv, q, n_q, method, o);
}

// One workgroup per window of at most QNT_MEDIUM_MAX samples: P keys (a power of two >= the window, NaN and padding
// as KEY_NAN) bitonic-sorted in LDS.
__global__ __launch_bounds__(1024) void k_qnt_medium(const DevQTask *__restrict__ tasks, uint32_t P,
                                                     const double *__restrict__ scratch, const double *__restrict__ q,
                                                     uint32_t n_q, int method, double *__restrict__ out)
{
    extern __shared__ uint64_t sk[];  // the whole 64 KiB at QNT_MEDIUM_MAX: no static LDS beside it
    const uint32_t tid = threadIdx.x, bd = blockDim.x;
    const DevQTask t = tasks[blockIdx.x];
    const double *x = scratch + t.src;
    for (uint32_t i = tid; i < P; i += bd) {
        uint64_t k = KEY_NAN;
        if (i < t.n) {
            const double d = x[i];
            if (!__builtin_isnan(d)) k = q_key(d);
        }
        sk[i] = k;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t h = tid; h < P / 2; h += bd) {
                const uint32_t a = ((h & ~(j - 1)) << 1) | (h & (j - 1)), b = a + j;
                const uint64_t ka = sk[a], kb = sk[b];
                if (((a & k) == 0) ? ka > kb : ka < kb) { sk[a] = kb; sk[b] = ka; }
            }
            __syncthreads();
        }
    }
    // n: the first KEY_NAN of the sorted keys (every key of a sample is below it)
    uint32_t lo = 0, hi = P;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (sk[m] != KEY_NAN) lo = m + 1;
        else hi = m;
    }
    const uint32_t nv = lo;
    for (uint32_t j = tid; j < n_q; j += bd) {
        double r = __builtin_nan("");
        if (nv) {
            const QPick p = q_pick(nv, q[j], method);
            r = q_interp(p, q_unkey(sk[p.lo]), q_unkey(sk[p.hi]));
        }
        out[(uint64_t)t.win * n_q + j] = r;
    }
}

// Long tier, pass `pass` (digit bits [56 - 8 pass, 64 - 8 pass) of the key): one workgroup per chunk counts, per live
// prefix of its window, the digits of the chunk's non-NaN samples that start with that prefix.  hist: per state slot,
// `rows` rows of 256 counts (zero on entry; k_qnt_pick clears what it reads).
__global__ __launch_bounds__(256) void k_qnt_hist(const DevQChunk *__restrict__ chunks, const double *__restrict__ scratch,
                                                  const DevQState *__restrict__ st, uint32_t *__restrict__ hist,
                                                  uint32_t rows, uint32_t pass)
{
    extern __shared__ uint32_t lh[];
    __shared__ uint64_t s_pre[QNT_SLOTS];
    const uint32_t tid = threadIdx.x;
    const DevQChunk c = chunks[blockIdx.x];
    const uint32_t nu = pass ? st[c.slot].nu : 1u;
    if (nu == 0) return;  // an all-NaN window: done in pass 0
    const bool in_lds = nu <= QNT_LDS_ROWS;
    uint32_t *g = hist + (uint64_t)c.slot * rows * 256u;
    for (uint32_t i = tid; i < nu; i += 256u) s_pre[i] = pass ? st[c.slot].upre[i] : 0ull;
    if (in_lds)
        for (uint32_t i = tid; i < nu * 256u; i += 256u) lh[i] = 0;
    __syncthreads();
    uint32_t *cnt = in_lds ? lh : g;
    const uint64_t mask = pass ? ~0ull << (64u - 8u * pass) : 0ull;
    const uint32_t shift = 56u - 8u * pass;
    const double *x = scratch + c.src;
    for (uint32_t base = 0; base < c.len; base += 1024u) {
        double d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + 256u * u + tid;
            d[u] = i < c.len ? x[i] : __builtin_nan("");
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t bin = ~0u;
            if (!__builtin_isnan(d[u])) {
                const uint64_t k = q_key(d[u]), p = k & mask;
                uint32_t lo = 0, hi = nu;
                while (hi - lo > 1) {
                    const uint32_t m = (lo + hi) >> 1;
                    if (s_pre[m] <= p) lo = m;
                    else hi = m;
                }
                if (s_pre[lo] == p) bin = lo * 256u + (uint32_t)((k >> shift) & 255u);
            }
            // a wavefront whose samples all fall in one bin (runs of equal values) adds once
            if (__all(bin == __shfl(bin, 0, 64))) {
                if ((tid & 63u) == 0 && bin != ~0u) atomicAdd(&cnt[bin], 64u);
            } else if (bin != ~0u) {
                atomicAdd(&cnt[bin], 1u);
            }
        }
    }
    if (!in_lds) return;
    __syncthreads();
    for (uint32_t i = tid; i < nu * 256u; i += 256u)
        if (lh[i]) atomicAdd(&g[i], lh[i]);
}

// Long tier, pass `pass`: one workgroup per window.  Pass 0 takes n from the counts and sets each level's two ranks
// (an all-NaN window gets NaN here and is done); every pass moves each rank to the digit that holds it, narrowing its
// prefix by 8 bits, and merges equal prefixes; the last pass writes the levels.
__global__ __launch_bounds__(256) void k_qnt_pick(const DevQTask *__restrict__ tasks, DevQState *__restrict__ st,
                                                  uint32_t *__restrict__ hist, uint32_t rows, uint32_t pass,
                                                  const double *__restrict__ q, uint32_t n_q, int method,
                                                  double *__restrict__ out)
{
    __shared__ uint64_t s_rank[QNT_SLOTS], s_upre[QNT_SLOTS], n_pre[QNT_SLOTS], n_rank[QNT_SLOTS];
    __shared__ uint32_t s_ridx[QNT_SLOTS], s_first[QNT_SLOTS];
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const DevQTask t = tasks[blockIdx.x];
    DevQState &S = st[t.slot];
    uint32_t *g = hist + (uint64_t)t.slot * rows * 256u;
    double *o = out + (uint64_t)t.win * n_q;
    uint64_t n;
    uint32_t nr, nu;
    if (pass == 0) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const uint32_t c = g[tid];
        if (c) atomicAdd(&s_cnt, c);
        __syncthreads();
        n = s_cnt;
        if (n == 0) {
            if (tid < n_q) o[tid] = __builtin_nan("");
            if (tid == 0) { S.n = 0; S.nr = 0; S.nu = 0; }
            g[tid] = 0;
            return;
        }
        nr = 2 * n_q;
        nu = 1;
        if (tid < n_q) {
            const QPick p = q_pick(n, q[tid], method);
            s_rank[2 * tid] = p.lo;
            s_rank[2 * tid + 1] = p.hi;
            s_ridx[2 * tid] = s_ridx[2 * tid + 1] = 0;
        }
        if (tid == 0) s_upre[0] = 0;
    } else {
        nr = S.nr;
        if (nr == 0) return;
        n = S.n;
        nu = S.nu;
        if (tid < nr) { s_rank[tid] = S.rank[tid]; s_ridx[tid] = S.ridx[tid]; }
        if (tid < nu) s_upre[tid] = S.upre[tid];
    }
    __syncthreads();
    const uint32_t shift = 56u - 8u * pass;
    for (uint32_t u = w; u < nu; u += 4u) {
        uint32_t *row = g + u * 256u;
        const uint32_t h0 = row[4 * lane], h1 = row[4 * lane + 1], h2 = row[4 * lane + 2], h3 = row[4 * lane + 3];
        const uint32_t c1 = h0, c2 = c1 + h1, c3 = c2 + h2, c4 = c3 + h3;
        uint32_t incl = c4;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        const uint64_t base = incl - c4;
        for (uint32_t r = 0; r < nr; ++r) {
            if (s_ridx[r] != u) continue;
            const uint64_t rr = s_rank[r];
            if (rr >= base && rr < base + c4) {
                const uint32_t b = rr < base + c1 ? 0u : rr < base + c2 ? 1u : rr < base + c3 ? 2u : 3u;
                const uint64_t before = base + (b == 0 ? 0u : b == 1 ? c1 : b == 2 ? c2 : c3);
                n_pre[r] = s_upre[u] | ((uint64_t)(4 * lane + b) << shift);
                n_rank[r] = rr - before;
            }
        }
        row[4 * lane] = row[4 * lane + 1] = row[4 * lane + 2] = row[4 * lane + 3] = 0;
    }
    __syncthreads();
    // merge equal prefixes: the distinct ones, ascending, become the next pass's rows
    if (tid < nr) {
        const uint64_t p = n_pre[tid];
        uint32_t first = 1;
        for (uint32_t r = 0; r < tid; ++r) first &= n_pre[r] != p;
        s_first[tid] = first;
    }
    __syncthreads();
    if (tid < nr) {
        const uint64_t p = n_pre[tid];
        uint32_t idx = 0;
        for (uint32_t r = 0; r < nr; ++r) idx += (s_first[r] && n_pre[r] < p) ? 1u : 0u;
        s_ridx[tid] = idx;
        if (s_first[tid]) s_upre[idx] = p;
    }
    __syncthreads();
    if (pass + 1 < QNT_PASSES) {
        if (tid < nr) { S.rank[tid] = n_rank[tid]; S.ridx[tid] = s_ridx[tid]; }
        uint32_t nu2 = 0;
        for (uint32_t r = 0; r < nr; ++r) nu2 += s_first[r];
        if (tid < nu2) S.upre[tid] = s_upre[tid];
        if (tid == 0) { S.n = n; S.nr = nr; S.nu = nu2; }
        return;
    }
    // every prefix is a whole key now
    if (tid < n_q) {
        const QPick p = q_pick(n, q[tid], method);
        o[tid] = q_interp(p, q_unkey(n_pre[2 * tid]), q_unkey(n_pre[2 * tid + 1]));
    }
}

hipError_t launch_qnt_short(const DevQTask *tasks, uint32_t n, const double *scratch, const double *q, uint32_t n_q,
                            int method, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_qnt_short, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n, scratch, q, n_q, method, out);
    return hipGetLastError();
}

// P: the power of two (QNT_SHORT_MAX < P <= QNT_MEDIUM_MAX) that holds each of the n windows
hipError_t launch_qnt_medium(const DevQTask *tasks, uint32_t n, uint32_t P, const double *scratch, const double *q,
                             uint32_t n_q, int method, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t threads = P / 2 < 256u ? 256u : P / 2 > 1024u ? 1024u : P / 2;
    hipLaunchKernelGGL(k_qnt_medium, dim3(n), dim3(threads), (size_t)P * sizeof(uint64_t), s, tasks, P, scratch, q, n_q,
                       method, out);
    return hipGetLastError();
}

hipError_t launch_qnt_hist(const DevQChunk *chunks, uint32_t n, const double *scratch, const DevQState *st, uint32_t *hist,
                           uint32_t rows, uint32_t pass, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t lds_rows = pass == 0 ? 1u : rows < QNT_LDS_ROWS ? rows : QNT_LDS_ROWS;
    hipLaunchKernelGGL(k_qnt_hist, dim3(n), dim3(256), (size_t)lds_rows * 256u * sizeof(uint32_t), s, chunks, scratch,
                       st, hist, rows, pass);
    return hipGetLastError();
}

hipError_t launch_qnt_pick(const DevQTask *tasks, uint32_t n, DevQState *st, uint32_t *hist, uint32_t rows,
                           uint32_t pass, const double *q, uint32_t n_q, int method, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_qnt_pick, dim3(n), dim3(256), 0, s, tasks, st, hist, rows, pass, q, n_q, method, out);
    return hipGetLastError();
}

}  // namespace atsc
