// atsc_host_private.h -- what the host sources of libatsc_hip.so share among themselves: atsc_host.cpp (context, plans,
// compress and decompress) and atsc_windows.cpp (the window queries).  Not for the kernels and not for callers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/atsc_hip.h"
#include "atsc_internal.h"

static const int CLASS_LARGE = 6;                // the class of the large frames (atsc_large.hip); 0..5: LDS-resident
static const uint32_t MAX_FRAME = 131072;        // MAX_FRAME_SIZE of the reference chunker (optimizer/mod.rs:27)

struct atsc_ctx {
    int device = 0;
    std::string last_error;
    // diagnostics of the last compress call
    atsc_frame_diag *d_diag = nullptr;
    uint64_t diag_cap = 0;
    uint64_t diag_n = 0;
    hipStream_t diag_stream = nullptr;
    bool want_diag = false;
    // Device memory pool.  The host-pointer entry points build a plan and five buffers per call and
    // drop them at the end; hipMalloc / hipFree of hundreds of megabytes cost milliseconds each, so
    // freed blocks are kept (up to POOL_MAX_BYTES) and handed out again when the size fits.
    std::vector<std::pair<void *, size_t>> pool_free_list;
    std::map<void *, size_t> pool_live;
    size_t pool_held = 0;
    // Streams of the context's own (created on first use; few, because the runtime maps streams onto a handful of
    // hardware queues).  Pipelined calls (atsc_compress_plan_dev_pipelined): consecutive batches go round-robin over the
    // chains of a plan, chain c on chain_streams[c] -- a dependent launch starts 6-10 us after its predecessor ends on this
    // system (tools/gap_probe.hip), and a frame kernel's freed wave slots refill slowly from a single queue; several
    // queues feeding the same CUs hide both (what bench.py --chains did from outside in round 2).
    hipStream_t chain_streams[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t pack_streams[4] = {nullptr, nullptr, nullptr, nullptr};  // a chain's packing: beside its next batch's codecs
    int n_chains = 2;                   // atsc_ctx_set_chains (1..4)
    bool adaptive_order = false;        // pipelined calls start a class's costliest frames first (atsc_ctx_set_adaptive_order)
    int debug_stop = 0;  // ATSC_DEBUG_STOP: phase-timing aid for tools/, never set in production
    // optional timing of the dominant k_compress launch (HIP events on the launch stream)
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    // Host-pointer entry points (atsc_compress_frames ...): plans kept by frame layout (a service compresses
    // the same layout batch after batch; building a plan walks every frame and uploads its tables), and a
    // stream of their own so that the blocking host-to-device copy of one part of a batch does not order
    // itself behind the kernels of the part before it (the legacy default stream would).
    struct CachedPlan {
        uint64_t hash = 0, stamp = 0;
        std::vector<uint32_t> lens;
        atsc_plan *plan = nullptr;
    };
    std::vector<CachedPlan> plan_cache;
    uint64_t plan_stamp = 0;
    hipStream_t work_stream = nullptr;
    hipStream_t copy_stream = nullptr;             // host-to-device copies of the host-pointer entry points
    hipStream_t d2h_stream = nullptr;              // ... and the records' way back, part by part (registered memory)
    std::vector<hipEvent_t> ev_parts;              // "part g's records are packed"
    unsigned char *h_stage = nullptr;              // page-locked staging for tables a kernel copies up (h2d_small)
    size_t h_stage_cap = 0, h_stage_used = 0;
    hipEvent_t ev_copy[2] = {nullptr, nullptr};    // "part g's samples are on the device"
    uint64_t agg_budget = 0;                       // atsc_ctx_set_aggregate_scratch (bytes; 0: the default)
};

namespace atsc {

struct PlanTables {
    std::vector<DevPlan> plans;   // host copy
    std::vector<float2> twpool;   // host copy
    std::map<uint32_t, uint32_t> by_n;
    DevPlan *d_plans = nullptr;
    float2 *d_tw = nullptr;
};

int fail(atsc_ctx *ctx, int rc, const char *what, hipError_t e = hipSuccess);
#define HIPCHK(ctx, call)                                                    \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return fail((ctx), ATSC_E_HIP, #call, e__);   \
    } while (0)
// the same for a kernel launch, whose message names the kernel: "launch k_x"
#define LAUNCHCHK(ctx, what, call)                                           \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return fail((ctx), ATSC_E_HIP, (what), e__);  \
    } while (0)

hipError_t pool_alloc(atsc_ctx *ctx, void **out, size_t bytes);
// The caller guarantees that no kernel still uses the block (plan destruction synchronises the device
// once, as hipFree would for every block; the host-pointer entry points have synchronised already).
void pool_free(atsc_ctx *ctx, void *p);

// What the last window query of one kind on a decode plan owns (atsc_windows.cpp): its task tables -- page-locked
// staging `h` and the device copy `d`, which the call's device-only tables follow -- its scratch of decoded samples, and
// the event that marks the end of its work.  A plan holds one per kind of query, so that a call waits only for the
// previous call of its own kind (atsc_dplan::res, by QueryKind).  A call over several plans (Q_PAIR, Q_ACROSS,
// Q_ACROSS_QUANTILE, Q_PAIR_MATRIX) keeps everything on its first plan's.
enum QueryKind { Q_WINDOW, Q_AGGREGATE, Q_QUANTILE, Q_HISTOGRAM, Q_MOMENTS, Q_DELTA, Q_RUNS, Q_EXTREMES, Q_SELECT, Q_PAIR, Q_ROLLING, Q_ACROSS, Q_ACROSS_QUANTILE, Q_PAIR_MATRIX, Q_KINDS };
struct QueryRes {
    unsigned char *h = nullptr, *d = nullptr;
    size_t h_cap = 0, d_cap = 0;
    double *scratch = nullptr;
    uint64_t scratch_cap = 0;  // samples
    hipEvent_t ev = nullptr;
    bool pending = false;
    // the previous call's tables and scratch may be reused once its work is done
    hipError_t wait()
    {
        if (!pending) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess) pending = false;
        return e;
    }
    // room for an upload of up_bytes, device tables of dev_bytes (the upload in front) and scratch_samples decoded samples
    hipError_t reserve(atsc_ctx *ctx, size_t up_bytes, size_t dev_bytes, uint64_t scratch_samples)
    {
        hipError_t e;
        if (up_bytes > h_cap) {
            if (h) (void)hipHostFree(h);
            h = nullptr;
            h_cap = 0;
            const size_t cap = up_bytes > (64u << 10) ? up_bytes : (64u << 10);
            if ((e = hipHostMalloc((void **)&h, cap, hipHostMallocDefault)) != hipSuccess) return e;
            h_cap = cap;
        }
        if (dev_bytes > d_cap) {
            pool_free(ctx, d);
            d = nullptr;
            d_cap = 0;
            if ((e = pool_alloc(ctx, (void **)&d, dev_bytes)) != hipSuccess) return e;
            d_cap = dev_bytes;
        }
        if (scratch_samples > scratch_cap) {
            pool_free(ctx, scratch);
            scratch = nullptr;
            scratch_cap = 0;
            if ((e = pool_alloc(ctx, (void **)&scratch, scratch_samples * sizeof(double))) != hipSuccess) return e;
            scratch_cap = scratch_samples;
        }
        return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    }
    // the end of this call's work on stream s
    hipError_t record(hipStream_t s)
    {
        const hipError_t e = hipEventRecord(ev, s);
        if (e == hipSuccess) pending = true;
        return e;
    }
    void release(atsc_ctx *ctx)
    {
        if (h) (void)hipHostFree(h);
        pool_free(ctx, d);
        pool_free(ctx, scratch);
        if (ev) (void)hipEventDestroy(ev);
    }
};

}  // namespace atsc

struct atsc_dplan {
    atsc_ctx *ctx = nullptr;
    uint64_t n_frames = 0, n_samples = 0;
    atsc::PlanTables tabs;
    std::vector<uint32_t> class_count, class_lds, class_first;
    atsc::DevDFrame *d_frames = nullptr;
    uint32_t *d_ids = nullptr;
    int *d_status = nullptr;
    unsigned char *d_ws = nullptr;
    uint64_t ws_stride = 0;
    uint32_t ws_slots = 0;
    bool large_tiled = false;
    atsc::LargePre large_pre{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // batched inverse transform of the large FFT frames (tiles1 == 0: off)
    uint32_t large_sp_tiles = 0;        // tiles per frame of the sparse inverse's (tile, frame) grid (0: off)
    uint32_t large_choice_count = 0;    // large frames of the plan the forms above were chosen for
    // host copies for the window decode (atsc_dplan_find_frames, atsc_decompress_windows_dev): frame f holds the
    // samples [h_frames[f].out_off, h_frames[f + 1].out_off or n_samples)
    std::vector<atsc::DevDFrame> h_frames;
    std::vector<int> h_cls;
    // what the last device call of each kind of window query owns
    mutable atsc::QueryRes res[atsc::Q_KINDS];
};

namespace atsc {

hipError_t launch_decompress_large(uint32_t count, const struct DevDFrame *frames, const uint32_t *ids,
                                   const DevPlan *plans, const float2 *twpool, const uint8_t *body,
                                   double *out, int *status, unsigned char *ws, uint64_t ws_stride,
                                   uint32_t ws_slots, int tiled, int sparse, hipStream_t s, const LargePre *pre = nullptr,
                                   uint32_t sp_tiles = 0);

// Inverse transforms of the large tier run from the sparse list of admitted bins (sparse_inverse,
// atsc_large.hip); ATSC_LARGE_DENSE=1 keeps the dense transforms through the workspace (A/B runs).
inline bool large_sparse() { return getenv("ATSC_LARGE_DENSE") == nullptr; }

// Host half of atsc_dplan_create: walks the untrusted record bytes and builds the per-frame table and the
// per-length tables.  No HIP call in here (the sanitizer build of tests/asan drives it without a GPU
// through atsc_internal_dplan_parse).
struct DPlanHost {
    std::vector<DevDFrame> frames;
    std::vector<int> cls;
    PlanTables tabs;
    std::vector<uint32_t> class_count, class_lds;
    uint64_t ws_stride = 0, n_samples = 0;
};
// begin / soft_limit / end_pos: a stream without a count in front can be walked in pieces -- the records from byte
// `begin` up to the first record boundary at or behind `soft_limit` (*end_pos: where that is)
int dplan_parse(const uint8_t *body, uint64_t body_len, int has_count, DPlanHost &H, const char **why, uint64_t begin = 0,
                uint64_t soft_limit = ~0ull, uint64_t *end_pos = nullptr);
// up: the stream a kernel copies the plan's tables up on instead of synchronous copies (h2d_small); the plan may then
// only be used on that stream (or behind it)
int dplan_create_range(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t begin,
                       uint64_t soft_limit, uint64_t *end_pos, atsc_dplan **out, hipStream_t up = nullptr);
// The large tier's launch forms of a plan, from every large frame of it: the transform form, the batched pre-pass and the
// sparse inverse's tile grid.  They depend on the set of large frames, so a window decode takes them from its stream's.
void large_choices(atsc_dplan *p, const std::vector<DevPlan> &plans, const std::vector<DevDFrame> &frames,
                   const std::vector<int> &cls);

}  // namespace atsc
