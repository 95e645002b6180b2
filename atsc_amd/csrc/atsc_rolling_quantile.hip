// atsc_rolling_quantile.hip -- gfx950 kernel of the windowed rolling quantiles (atsc_rolling_quantile_windows_dev): the
// levels of the window [lo, lo + w) at every position of a range, from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling quantiles"): a position's row is the row
// atsc_quantile_windows gives for the listed window (lo, w) -- the window's non-NaN samples in the total order of q_key,
// ranks and interpolation through q_pick / q_interp (atsc_quantile_rule.h) and nothing else.
//
// A quantile is not a sum: it does not ride the rolling's pyramid.  Neighbouring windows share all but `stride` of their
// samples, so a span of samples is sorted once and every window inside it reads its levels off the sorted span.  A task
// (DevRollTask) is a run of B consecutive positions of one range inside one piece; its windows cover a span of
// (B - 1) stride + w <= P samples, P a power of two (rq_span_keys, the host's rule).  One workgroup per task:
//   load   the span into LDS as (key, index in the span): a 64-bit key and a 16-bit index a slot, NaN and the padding up
//          to P as KEY_NAN;
//   sort   the pairs by key, k_qnt_medium's compare-exchange network with the index moved with its key (equal keys are
//          equal bits: their order decides nothing); nv, the real keys, ends at the first KEY_NAN;
//   walk   one wavefront per position, round robin: the sorted indices 64 at a time, an entry a member of the window
//          when (uint32_t)(index - lo_rel) < w; a ballot and a popcount carry the number of members so far, lane t < n_q
//          holds level t's ranks and, when one of them falls among the current 64 entries, takes the key at that set
//          bit of the ballot; the walk ends once the count has passed every rank.
// A task of one position has no walk: its span is its window, and a rank is the key's place.  Where every task of a
// call is one (B = 1: w = 8192, or a stride beyond P - w) the keys are sorted without their indices (IDX = false), which
// is k_qnt_medium's work and its 8 bytes a slot.
// The window's n is w when the span holds no NaN (nv equals the span's length); else the wavefront counts the NaN of
// its own window from the scratch.  Selection is exact; no atomics; every output double has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"
#include "atsc_quantile_rule.h"

namespace atsc {

namespace {

// the position (0 .. 63) of the set bit of m that has r set bits below it (r < popcount(m))
DEVI uint32_t rq_nth_bit(uint64_t m, uint32_t r)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t c = (uint32_t)__popcll(m & ((1ull << s) - 1ull));
        const bool up = r >= c;
        r -= up ? c : 0u;
        m >>= up ? s : 0u;
        pos += up ? s : 0u;
    }
    return pos;
}

}  // namespace

// One workgroup per task: sk[P] keys and, with IDX, behind them si[P] indices in dynamic LDS (10 P bytes; 8 P without).
// a0: the stream index of scratch[0].  The task's span, (t.n - 1) stride + w samples from t.lo on, is at most P (the host
// cuts tasks so).  IDX = false: every task holds one position.
template <bool IDX>
__global__ __launch_bounds__(1024) void k_rq_span(const DevRollTask *__restrict__ tasks, uint32_t P,
                                                  const double *__restrict__ scratch, uint64_t a0, uint32_t w,
                                                  uint64_t stride, const double *__restrict__ q, uint32_t n_q, int method,
                                                  double *__restrict__ out)
{
    extern __shared__ uint64_t sk[];
    uint16_t *si = (uint16_t *)(sk + P);
    const uint32_t tid = threadIdx.x, bd = blockDim.x, lane = tid & 63u;
    const DevRollTask t = tasks[blockIdx.x];
    const double *x = scratch + (t.lo - a0);
    const uint32_t span = (uint32_t)((uint64_t)(t.n - 1u) * stride) + w;
    for (uint32_t i = tid; i < P; i += bd) {
        uint64_t k = KEY_NAN;
        if (i < span) {
            const double d = x[i];
            if (!__builtin_isnan(d)) k = q_key(d);
        }
        sk[i] = k;
        if constexpr (IDX) si[i] = (uint16_t)i;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t h = tid; h < P / 2; h += bd) {
                const uint32_t a = ((h & ~(j - 1)) << 1) | (h & (j - 1)), b = a + j;
                const uint64_t ka = sk[a], kb = sk[b];
                if (((a & k) == 0) ? ka > kb : ka < kb) {
                    sk[a] = kb; sk[b] = ka;
                    if constexpr (IDX) {
                        const uint16_t ia = si[a], ib = si[b];
                        si[a] = ib; si[b] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
    // nv: the first KEY_NAN of the sorted keys (every key of a sample is below it)
    uint32_t nv = 0;
    {
        uint32_t lo = 0, hi = P;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (sk[m] != KEY_NAN) lo = m + 1;
            else hi = m;
        }
        nv = lo;
    }
    const uint32_t lvl = lane < n_q ? lane : n_q - 1u;  // the lanes from n_q on shadow the last level and store nothing
    const double ql = q[lvl];
    const double nan = __builtin_nan("");
    if (!IDX || t.n == 1u) {  // one position: the span is its window, a rank the key's place (the medium tier's read)
        if (tid < n_q) {
            double r = nan;
            if (nv) {
                const QPick pk = q_pick(nv, ql, method);
                r = q_interp(pk, q_unkey(sk[pk.lo]), q_unkey(sk[pk.hi]));
            }
            out[t.rec * (uint64_t)n_q + tid] = r;
        }
        return;
    }
    for (uint32_t p = tid >> 6; p < t.n; p += bd >> 6) {
        const uint32_t lo_rel = (uint32_t)((uint64_t)p * stride);
        double *o = out + (t.rec + p) * (uint64_t)n_q;
        uint32_t n = w;
        if (nv != span) {  // the span holds NaN: the window's own
            uint32_t bad = 0;
            for (uint32_t i = lane; i < w; i += 64u) bad += __builtin_isnan(x[lo_rel + i]) ? 1u : 0u;
            n = w - wave_sum_u32(bad);
        }
        if (n == 0) {
            if (lane < n_q) o[lane] = nan;
            continue;
        }
        const QPick pk = q_pick(n, ql, method);
        const uint32_t r_lo = (uint32_t)pk.lo, r_hi = (uint32_t)pk.hi;
        const uint32_t r_max = wave_max_u32(r_hi);
        uint64_t k_lo = 0, k_hi = 0;
        uint32_t cnt = 0;
        for (uint32_t base = 0; base < nv && cnt <= r_max; base += 64u) {
            const uint32_t e = base + lane;
            const uint32_t idx = e < nv ? si[e] : 0xffffu;
            const uint64_t m = __ballot(e < nv && (uint32_t)(idx - lo_rel) < w);
            const uint32_t c = (uint32_t)__popcll(m);
            if (r_lo - cnt < c) k_lo = sk[base + rq_nth_bit(m, r_lo - cnt)];  // (a rank below cnt wraps: not below c)
            if (r_hi - cnt < c) k_hi = sk[base + rq_nth_bit(m, r_hi - cnt)];
            cnt += c;
        }
        if (lane < n_q) o[lane] = q_interp(pk, q_unkey(k_lo), q_unkey(k_hi));
    }
}

// B: the most positions a task holds (1: none holds more, and the keys go without their indices)
hipError_t launch_rq_span(const DevRollTask *tasks, uint32_t n, uint32_t P, uint64_t B, const double *scratch, uint64_t a0,
                          uint32_t w, uint64_t stride, const double *q, uint32_t n_q, int method, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t threads = P / 2 < 256u ? 256u : P / 2 > 1024u ? 1024u : P / 2;
    const bool idx = B > 1;
    const uint32_t lds = P * (uint32_t)(sizeof(uint64_t) + (idx ? sizeof(uint16_t) : 0));
    const auto kern = idx ? k_rq_span<true> : k_rq_span<false>;
    if (lds > 48u * 1024u) {
        const hipError_t e = ensure_dyn_lds((const void *)kern, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(n), dim3(threads), lds, s, tasks, P, scratch, a0, w, stride, q, n_q, method, out);
    return hipGetLastError();
}

}  // namespace atsc
