/*
 * atsc_hip.h -- C ABI of the MI355X-native ATSC compression core (libatsc_hip.so).
 *
 * This is the drop-in boundary for the per-frame compressor path of
 * instaclustr/atsc.  The reference has no FFI of its own (it is a single Rust
 * process); the seam a replacement must honour is the Rust API both CLIs call:
 *     CompressedStream::{compress_chunk_with, compress_chunk_bounded_with,
 *                        to_bytes, from_bytes, decompress}   atsc/src/data.rs:47-109
 *     OptimizerPlan::{plan, get_execution}                   atsc/src/optimizer/mod.rs:47-109
 * The reference compresses one chunk per call; a GPU wants a batch, so the ABI
 * takes the whole chunk list ("frames") of one or many series at once.  Frame
 * semantics (codec choice, payload bytes, error bound) are per frame and equal
 * the reference's.  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add and where it replaces the loop at atsc/src/main.rs:146-163.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative ATSC_E_* code and never aborts/throws across the ABI
 * (the reference panics instead: data.rs:98, header.rs:34-37,72-74).
 * The caller owns every buffer it passes; the library owns device scratch.
 * One atsc_ctx per host thread (mirrors `&mut self`).  `*_dev` entry points
 * take DEVICE pointers and a hipStream_t (as void*), enqueue work and return
 * without synchronising; the others take HOST pointers and are synchronous.
 *
 * All citations are relative to the reference repository root.
 */
#ifndef ATSC_HIP_H
#define ATSC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Compressor wire ids == enum Compressor discriminants, atsc/src/compressor/mod.rs:35-44 */
enum {
    ATSC_NOOP = 0,
    ATSC_FFT = 1,
    ATSC_IDW = 2,
    ATSC_CONSTANT = 3,
    ATSC_POLYNOMIAL = 4,
    ATSC_AUTO = 5,
    ATSC_RLE = 6
};

enum {
    ATSC_OK = 0,
    ATSC_E_INVALID = -1,      /* bad argument (null pointer, empty frame, bad level) */
    ATSC_E_NOMEM = -2,        /* host or device allocation failed */
    ATSC_E_UNSUPPORTED = -3,  /* valid in the reference, not implemented here (see atsc_strerror) */
    ATSC_E_NO_DEVICE = -4,    /* no usable HIP device; the library never falls back to a CPU path */
    ATSC_E_HIP = -5,          /* a HIP runtime call failed; see atsc_ctx_last_error */
    ATSC_E_CAPACITY = -6,     /* caller buffer too small */
    ATSC_E_FORMAT = -7,       /* malformed BRO / WBRO / CSV bytes (reference: panic / Err) */
    ATSC_E_VERSION = -8,      /* BRO version newer than 1 (header.rs:30-42) */
    ATSC_E_IO = -9            /* file could not be read / written */
};

typedef struct atsc_ctx atsc_ctx;
typedef struct atsc_plan atsc_plan;
typedef struct atsc_dplan atsc_dplan;
typedef struct atsc_stream atsc_stream;

const char *atsc_strerror(int rc);
const char *atsc_version(void);

/* ------------------------------------------------------------------------ */
/* context                                                                  */
/* ------------------------------------------------------------------------ */

/* Creates a context on HIP device `device` (0-based).  Fails with
 * ATSC_E_NO_DEVICE when there is no GPU: there is no CPU fallback. */
int atsc_ctx_create(atsc_ctx **out, int device);
/* Plans, decode plans and streams created on a context hold device memory of its pool: destroy them
 * before the context. */
void atsc_ctx_destroy(atsc_ctx *ctx);
const char *atsc_ctx_last_error(const atsc_ctx *ctx);
/* What the library keeps between calls, and how to give it back.  A context keeps freed device blocks in a
 * pool (up to 8 GiB) and, for the host-pointer entry points, up to four plans by frame layout with their
 * scratch sets, workspaces and tables; the process keeps the host block the caller released last through
 * atsc_free (decoded results; up to 2 GiB, ATSC_BIG_KEEP_MAX overrides) and the twiddle tables by
 * transform length (up to 128 MB).  atsc_ctx_trim frees the context's share (it synchronises the
 * device; plans the caller created stay valid), atsc_release_caches the process-wide caches. */
int atsc_ctx_trim(atsc_ctx *ctx);
void atsc_release_caches(void);
/* Page-locks / releases caller memory (hipHostRegister): host-pointer calls on registered buffers copy at
 * the link's rate, asynchronously.  The reference's caller owns its chunk (data.rs:56-76); so does this one. */
int atsc_host_register(void *p, uint64_t bytes);
int atsc_host_unregister(void *p);

/* ------------------------------------------------------------------------ */
/* compress: CompressorFrame::{compress, compress_bounded, compress_best}    */
/*           atsc/src/frame/mod.rs:59-149 over a batch of frames             */
/* ------------------------------------------------------------------------ */

/* Frame layout of one batch.  frame_off[n_frames+1] are prefix offsets (in
 * samples) into the sample array: frame i = samples[frame_off[i] .. frame_off[i+1]).
 * Replaces the chunk list of OptimizerPlan::get_execution (optimizer/mod.rs:101-109). */
int atsc_plan_create(atsc_ctx *ctx, const uint64_t *frame_off, uint64_t n_frames,
                     atsc_plan **out);
void atsc_plan_destroy(atsc_plan *plan);
uint64_t atsc_plan_n_frames(const atsc_plan *plan);
uint64_t atsc_plan_n_samples(const atsc_plan *plan);
/* Worst-case bytes of the encoded frame records of this plan (size d_body with it). */
uint64_t atsc_plan_body_bound(const atsc_plan *plan);
/* Worst-case payload bytes of one frame of n samples (RLE, all values distinct). */
uint64_t atsc_payload_bound_bytes(uint64_t n_samples_in_frame);

/* Compresses every frame of `plan` on the GPU.
 *   compressor   ATSC_* id.  ATSC_AUTO = compress_best (frame/mod.rs:71-149).
 *   bounded      1 = compress_chunk_bounded_with (data.rs:56-76), 0 = compress_chunk_with
 *                (data.rs:47-53).  The atsc CLI uses bounded for fft/polynomial/idw/auto and
 *                unbounded for noop/constant/rle (main.rs:150-162).
 *   max_error    the f32 the reference passes: `e as f32 / 100.0` (main.rs:157)
 *   sample_level 0..6, index into COMPRESSION_SPEED (frame/mod.rs:22); only used by ATSC_AUTO
 * Outputs (device memory):
 *   d_body       encoded frame records in frame order, each exactly the bincode image of
 *                CompressorFrame (frame/mod.rs:25-33): varint(41) varint(sample_count)
 *                varint(compressor) varint(len) payload.  A .bro file is
 *                "BRRO" u32le(1) u8(n_frames) varint(n_frames) followed by these bytes
 *                (header.rs:60-67, data.rs:79-85); see atsc_bro_wrap.
 *   d_rec_off    n_frames+1 byte offsets of the records in d_body; [n_frames] = total bytes
 *   d_chosen     n_frames, compressor id actually used (may be NULL)
 *   d_err        n_frames, CompressorResult.error of the chosen codec (may be NULL)
 * Nothing is synchronised; the work is enqueued on `stream`. */
int atsc_compress_plan_dev(atsc_ctx *ctx, const atsc_plan *plan, const double *d_samples,
                           int compressor, int bounded, float max_error, int sample_level,
                           uint8_t *d_body, uint64_t body_cap, uint64_t *d_rec_off,
                           uint8_t *d_chosen, double *d_err, void *stream);

/* The same call for back-to-back batches (a compression service's steady state; main.rs:146-163
 * run over file after file).  Consecutive calls on a plan go round-robin over up to four *chains*
 * inside the plan: a stream owned by the context plus everything a batch in flight owns (payload
 * slots, results, scan scratch, large-tier workspace).  A call's kernels -- codecs and packing -- run on
 * its chain's stream, ordered after everything enqueued on `stream` before the call by one event (only
 * when `stream` still has work in flight), and every chain has two scratch sets, so up to 2 x chains batches
 * are queued or in flight: the gap a single queue leaves between dependent launches (6-10 us here) and the
 * drain of a launch's last workgroups are covered by the other chains' kernels.  Results are those of
 * atsc_compress_plan_dev, byte for byte.
 *   - A call may block the host until the batch that last used its scratch set (2 x chains calls
 *     earlier) has been packed; nothing else is synchronised.
 *   - The outputs of a call are complete once a stream has passed an atsc_plan_join enqueued
 *     after it (or after hipDeviceSynchronize).  Give the calls in flight their own output buffers:
 *     2 x chains sets (eight always suffice).
 *   - d_samples is read by kernels on the context's streams, NOT in `stream` order: it must not be
 *     overwritten until a stream has passed an atsc_plan_input_release (or atsc_plan_join)
 *     enqueued after the call.  (atsc_compress_plan_dev reads it in `stream` order; the large tier's
 *     frames, which it also deals over the context's streams, are joined back before it returns.)
 *   - atsc_compress_plan_dev may be mixed in; it orders itself after the pending batches. */
int atsc_compress_plan_dev_pipelined(atsc_ctx *ctx, const atsc_plan *plan, const double *d_samples,
                                     int compressor, int bounded, float max_error,
                                     int sample_level, uint8_t *d_body, uint64_t body_cap,
                                     uint64_t *d_rec_off, uint8_t *d_chosen, double *d_err,
                                     void *stream);
/* Chains the pipelined calls of this context rotate over (1..4; default 2, or 4 in a process started with
 * GPU_MAX_HW_QUEUES >= 8 -- four chains plus the caller's streams need more hardware queues than the runtime's default
 * four to pay).  1 keeps every batch on one stream of the context's. */
int atsc_ctx_set_chains(atsc_ctx *ctx, int n);
/* Pipelined calls record how many shader clocks every frame took and start the next batches of the
 * same plan with a class's costliest frames first (frame i of a recurring batch is the same series,
 * one window later); otherwise the frames that run longest start last and the GPU drains half
 * empty.  Only the order of execution changes, never a result.  OFF by default since round 3 (with two chains in
 * flight the next batch's first frames fill the drain the order was there to shorten, and the hint only predicts
 * where the layout recurs -- slot i the same series with the same behaviour, batch after batch); 1 turns it on. */
int atsc_ctx_set_adaptive_order(atsc_ctx *ctx, int on);
/* Makes `stream` wait (device side, no host block) for every batch enqueued so far by
 * atsc_compress_plan_dev_pipelined on `plan`: its records are packed. */
int atsc_plan_join(atsc_ctx *ctx, const atsc_plan *plan, void *stream);
/* Makes `stream` wait (device side) until no kernel of the pipelined calls enqueued so far on `plan`
 * reads their d_samples any more: work enqueued on `stream` afterwards may overwrite the inputs
 * (the reference's caller owns the chunk for the duration of compress_chunk_*, data.rs:47-76). */
int atsc_plan_input_release(atsc_ctx *ctx, const atsc_plan *plan, void *stream);

/* Per-frame diagnostics of the last atsc_compress_plan_dev on this ctx (host copy,
 * synchronises the stream).  One record per frame; used by the parity tests. */
typedef struct {
    uint32_t fft_size, poly_size, rle_size; /* candidate payload bytes; 0xFFFFFFFF = not run */
    uint16_t fft_trips, fft_k;              /* ladder trips (fft.rs:334-353), stored bins */
    uint16_t poly_trips, poly_step;         /* ladder trips (polynomial.rs:231-270), point_step */
    uint32_t poly_points;
    double fft_err, poly_err;
} atsc_frame_diag;
/* Diagnostics cost 40 B/frame of HBM writes, so they are off unless enabled here (or ATSC_DIAG is set). */
int atsc_ctx_enable_diag(atsc_ctx *ctx, int on);
int atsc_ctx_last_diag(atsc_ctx *ctx, atsc_frame_diag *out, uint64_t n_frames);

/* Kernel timing for the roofline report: when on, every compress call hands a HIP event pair to
 * the k_compress dispatch of the frame class holding the most frames (hipExtLaunchKernel start /
 * stop events on the launch stream: the kernel's own timestamps, no marker packets around it; the
 * large-frame tier, several launches, is bracketed by recorded events).  atsc_ctx_profile_read waits
 * for them, returns the summed milliseconds and the number of launches, and resets the counters. */
int atsc_ctx_set_profiling(atsc_ctx *ctx, int on);
int atsc_ctx_profile_read(atsc_ctx *ctx, double *total_ms, uint64_t *launches);

/* Host-pointer convenience: plan + H2D + compress + D2H, synchronous.
 * body_len receives the number of bytes written to `body`.
 *
 * Sample domain (this call and every compress entry point above; tests/test_gpu_extreme_values.py pins it).  Any f64
 * bit pattern is accepted: no sample value is used as an index.  Finite samples of any magnitude, subnormal numbers
 * included, give the reference's codec choice, bytes and reported error, with one exception: a frame whose f32
 * transform can overflow (the sum of its |samples| as f32 reaches FLT_MAX / 2, about 1e36 per sample at 256 samples)
 * has an FFT candidate whose bins and error depend on the order of the f32 additions, here as between two builds of
 * the reference; the record is still well formed, and Polynomial / RLE / Constant / Noop stay exact.  Samples beyond
 * f32 range convert to infinity as the reference's `as f32` does (all of them: the 10-byte FFT payload).  NaN and
 * +-Inf samples are not cleaned here (atsc_compress_data drops them first, as the reference's front end does): the
 * exact codecs and the Polynomial / IDW payloads equal the reference's, the lossy errors are NaN, so AUTO takes RLE;
 * forced FFT returns a well-formed record whose bins are NaN or infinite. */
int atsc_compress_frames(atsc_ctx *ctx, const double *samples, const uint64_t *frame_off,
                         uint64_t n_frames, int compressor, int bounded, float max_error,
                         int sample_level, uint8_t *body, uint64_t body_cap, uint64_t *body_len,
                         uint64_t *rec_off, uint8_t *chosen, double *err);

/* Several GPUs.  Frames are independent (the loop at main.rs:146-163 shares nothing between chunks), so a
 * batch shards by contiguous frame ranges and the encoded stream is the shards' records laid end to
 * end.  atsc_shard_range is the split every layer uses: unit ranges of sizes differing by at most one,
 * rank order = frame order.  A multi-process host (one process and one atsc_ctx per GPU, as bench.py
 * and atsc_amd/parallel.py run it) calls the single-context entry points on its own range and gathers
 * the record bytes to rank 0.  A single-process host hands one context per device to
 * atsc_compress_frames_sharded: each shard runs on its own host thread, and the outputs are byte for
 * byte those of atsc_compress_frames on one context. */
void atsc_shard_range(uint64_t n_units, uint32_t rank, uint32_t world, uint64_t *begin, uint64_t *end);
/* The same split with rank 0 carrying root_weight_milli / 1000 times a peer's share: when the records are
 * gathered to rank 0, every peer's bytes cross one link while the root's stay, so the root can take more
 * frames (1000 = atsc_shard_range up to rounding). */
void atsc_shard_range_weighted(uint64_t n_units, uint32_t rank, uint32_t world, uint32_t root_weight_milli,
                               uint64_t *begin, uint64_t *end);
int atsc_compress_frames_sharded(atsc_ctx *const *ctxs, uint32_t n_ctx, const double *samples,
                                 const uint64_t *frame_off, uint64_t n_frames, int compressor, int bounded,
                                 float max_error, int sample_level, uint8_t *body, uint64_t body_cap,
                                 uint64_t *body_len, uint64_t *rec_off, uint8_t *chosen, double *err);

/* ------------------------------------------------------------------------ */
/* decompress: CompressedStream::decompress (data.rs:104-109) ->             */
/*             CompressorFrame::decompress (frame/mod.rs:152-158)            */
/* ------------------------------------------------------------------------ */

/* Parses frame records (host bytes, as produced above, without the leading
 * varint(n_frames) unless has_count != 0) and builds the per-frame table. */
int atsc_dplan_create(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count,
                      atsc_dplan **out);
void atsc_dplan_destroy(atsc_dplan *dp);
uint64_t atsc_dplan_n_frames(const atsc_dplan *dp);
uint64_t atsc_dplan_n_samples(const atsc_dplan *dp);
/* d_body: the same bytes on the device; d_out: atsc_dplan_n_samples doubles. */
int atsc_decompress_plan_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body,
                             double *d_out, void *stream);
/* Host-pointer convenience (synchronous). out_n receives the sample count.  On an error `out` may hold
 * samples of the frames in front of the failing record (a destination registered with atsc_host_register
 * is filled part by part while the later records are still being parsed; a pageable one is only written
 * once every payload has decoded): *out_n = 0 then, so that nothing in `out` can be mistaken for a result. */
int atsc_decompress_frames(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count,
                           double *out, uint64_t out_cap, uint64_t *out_n);
/* The same with the output allocated by the library at exactly the decoded length (atsc_free):
 * what CompressedStream::decompress returns (data.rs:104-109), without a sizing pass by the caller. */
int atsc_decompress_frames_alloc(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count,
                                 double **out, uint64_t *out_n);

/* Window decode: the samples [begin, begin + count) of the decoded stream (the indices atsc_decompress_frames
 * returns), bit for bit what the full decode gives there, without decoding the frames the window does not touch.
 * Frame records are independent (frame/mod.rs:25-33), so a window needs only the frames that overlap it; every
 * frame keeps its own decode path (an FFT frame that runs an inverse transform in the full decode runs it here too).
 * Validation: the record headers in front of the window's end are walked and checked as atsc_dplan_create checks
 * them; payloads are checked only for the frames the window touches -- a corrupt payload outside the window is not
 * seen.  begin + count beyond the stream: ATSC_E_INVALID, nothing written.  count == 0 is valid and does nothing. */
/* The records a window touches in a .bro image (host only, no GPU): walks the record headers with the checks of
 * atsc_bro_scan up to the first record that ends at or behind the window's end.  Outputs (each may be NULL): the byte
 * range [byte_begin, byte_end) of the touched records in `bro`, their frame range [frame_begin, frame_end) and the
 * stream sample index at which frame_begin starts -- what a storage layer needs to read only those bytes.  count == 0:
 * an empty range at the record holding `begin`. */
int atsc_bro_find_window(const uint8_t *bro, uint64_t len, uint64_t begin, uint64_t count, uint64_t *byte_begin,
                         uint64_t *byte_end, uint64_t *frame_begin, uint64_t *frame_end, uint64_t *sample_begin);
/* The frames [frame_begin, frame_end) of a plan that the window touches (binary search over the plan's host copy of
 * the frame offsets). */
int atsc_dplan_find_frames(const atsc_dplan *dp, uint64_t begin, uint64_t count, uint64_t *frame_begin,
                           uint64_t *frame_end);
/* Decodes n_windows windows of the plan's stream in one call: window i = [begin[i], begin[i] + count[i]) lands at
 * d_out + out_off[i].  begin / count / out_off are HOST arrays, d_body / d_out device memory (d_out 8-byte aligned).
 * Windows may overlap and come in any order; a frame several windows touch is decoded once per call.  Enqueued on
 * `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word, which this call does
 * not read (atsc_decompress_window does).  The plan keeps the call's task tables and scratch: the next window call on
 * the same plan waits (host side) until this one's work is done before it reuses them. */
int atsc_decompress_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                const uint64_t *begin, const uint64_t *count, const uint64_t *out_off, double *d_out,
                                void *stream);
/* Host-pointer window decode (synchronous): walks the record headers only up to the window's last record, plans the
 * touched records and uploads only their bytes.  (A window that touches a frame longer than 4096 samples walks the
 * remaining headers as well: the large tier's launch forms depend on every large frame of the stream, and the window
 * has to decode as the full decode does.)  *out_n = count on success, 0 on any error (ATSC_E_FORMAT for a
 * malformed payload inside the window); ATSC_E_CAPACITY when out_cap < count. */
int atsc_decompress_window(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t begin,
                           uint64_t count, double *out, uint64_t out_cap, uint64_t *out_n);

/* Windowed aggregates: one summary record per window [begin, begin + count) of the decoded stream (the indices of
 * atsc_decompress_frames), from the same decoded samples as the window decode, without handing the samples out.
 *   count       samples of the window that are not NaN
 *   min, max    over those samples (compared as values; a zero extreme comes back with a fixed sign); NaN when count == 0
 *   sum         over those samples in the order below; +0.0 when count == 0
 *   first, last the window's first and last decoded samples as they are (NaN included); NaN for an empty window
 * The order of `sum` depends only on the stream's samples and the window's (begin, count):
 *   1. tiles of 2048 samples at multiples of 2048 in the stream index; a slot outside the window or holding NaN
 *      contributes -0.0, IEEE's exact additive identity;
 *   2. in a tile x[0..2047]: for v = 0..255, p_t = x[512 t + 2 v] + x[512 t + 2 v + 1] (t = 0..3) and
 *      s[v] = (p_0 + p_1) + (p_2 + p_3); then s[v] = s[v] + s[v + h] for v < h, h = 128, 64, 32, 16, 8, 4, 2, 1: s[0];
 *   3. the window's tile partials q[0..P-1] in tile order: q[i] = q[2 i] + q[2 i + 1] level by level (an odd last
 *      entry is added to -0.0) until one is left.
 * |sum - exact| <= (ceil(log2 count) + 2) 2^-53 sum|x| for finite data; with +-Inf the result is IEEE's (+Inf, -Inf, or
 * NaN when both occur).  Validation is the window decode's: a window beyond the stream gives ATSC_E_INVALID with nothing
 * written; payloads are checked only of the frames a window touches.  Windows may overlap and come in any order;
 * count == 0 and n_windows == 0 are valid. */
typedef struct {
    uint64_t count;
    double min, max;
    double sum;
    double first, last;
} atsc_window_stats; /* 48 bytes */
/* d_stats[i] summarises window i.  begin / count are HOST arrays; d_body and d_stats are device memory (d_stats 8-byte
 * aligned).  Enqueued on `stream`, not synchronised.  Decoded samples go through device scratch of at most the
 * context's aggregate budget (raised to one piece's minimum, 65536 samples plus two large frames' room), whatever the
 * windows' total length; a frame cut by a piece boundary is decoded once per piece.  A malformed payload inside a
 * window sets the plan's status word.  The plan keeps the call's tables, partials and scratch: the next aggregate call
 * on the same plan waits (host side) until this one's work is done. */
int atsc_aggregate_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                               const uint64_t *begin, const uint64_t *count, atsc_window_stats *d_stats, void *stream);
/* Host bytes in, host records out, synchronous.  Walks the record headers only up to the last window's end and uploads
 * only the touched records' byte range, as atsc_decompress_window does.  ATSC_E_FORMAT (nothing written) for a
 * malformed payload inside a window. */
int atsc_aggregate_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                           const uint64_t *begin, const uint64_t *count, atsc_window_stats *out);
/* Upper bound in bytes on the decoded-sample scratch the aggregate calls hold; 0 (the default) gives pieces of 16 Mi
 * samples (128 MiB, plus 2 MiB of room for two large frames cut by a piece's ends where a frame longer than 4096 samples
 * is touched).  A budget below what one piece needs is raised to that minimum, never an error.  It bounds the quantile
 * calls below too, whose windows must each fit one piece, and the moments (atsc_moments_windows_dev), delta
 * (atsc_delta_windows_dev), runs (atsc_runs_windows_dev) and histogram calls (atsc_histogram_windows_dev), whose windows may be of any length. */
int atsc_ctx_set_aggregate_scratch(atsc_ctx *ctx, uint64_t bytes);

/* Windowed moments: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames) the
 * centred moments of the sample value x and the sample position t, from the same decoded samples as the window decode:
 * what mean, variance / standard deviation and the least-squares line through (t, x) are read from (atsc_moments_fit).
 * They are reduced by pairwise merges of centred nodes, never from sums of squares, so a window of 1e9 +- 1e-3 keeps its
 * variance.  The result is bit-exact: it depends only on the stream's samples and the window's (begin, count), not on
 * the other windows, their order, the budget, piece boundaries or the device.
 *   Node   (n, mx, M2x, mt, M2t, C).
 *   Leaf   of stream index i: (1, x[i], 0, (double)i, 0, 0); a slot outside the window or holding NaN is the empty node
 *          (n = 0).
 *   Merge(a, b)   nb == 0: a, bit for bit; na == 0: b; else
 *          n = na + nb; w = (double)nb / (double)n; f = (double)na * w; dx = mxb - mxa; dt = mtb - mta;
 *          mx = mxa + dx * w; mt = mta + dt * w;
 *          M2x = (M2xa + M2xb) + (dx * dx) * f; M2t = (M2ta + M2tb) + (dt * dt) * f; C = (Ca + Cb) + (dx * dt) * f
 *          -- every operation one correctly rounded f64 + - * /, evaluated as written, never fused.
 *   Tree   the aggregate sum's tree (above) with + replaced by Merge, the left operand as a:
 *          1. tiles of 2048 slots at multiples of 2048 in the stream index;
 *          2. in a tile, for v = 0..255: p_t = Merge(leaf[512 t + 2 v], leaf[512 t + 2 v + 1]) (t = 0..3) and
 *             s[v] = Merge(Merge(p_0, p_1), Merge(p_2, p_3)); then s[v] = Merge(s[v], s[v + h]) for v < h,
 *             h = 128, 64, 32, 16, 8, 4, 2, 1: s[0];
 *          3. the window's tile partials q[0..P-1] in tile order: q[i] = Merge(q[2 i], q[2 i + 1]) level by level (an odd
 *             last entry merges with the empty node) until one is left.
 *   Result count = n, mean = mx, m2 = M2x, t_m2 = M2t, c_tx = C, t_mean = mt - (double)begin (one subtract); when
 *          count == 0 all five doubles are NaN.  +-Inf samples give what IEEE gives under these rules; where the rule
 *          yields NaN, any NaN bit pattern conforms.
 * With u = 2^-53, L = max(1, ceil(log2 count)), kappa = sqrt(1 + count mean^2 / m2) and r = (begin + count) / count,
 * for finite data:
 *   |mean - exact| <= (L + 2) u mean|x|;              |m2 - exact| <= (L + 2) u kappa m2;
 *   |t_m2 - exact| <= (L + 2) u r t_m2;               |c_tx - exact| <= (L + 2) u r kappa sqrt(t_m2 m2);
 *   |t_mean - exact| <= (L + 2) u (begin + count);
 * m2 == 0 and c_tx == 0 exactly on a constant window.  r is the price of positions counted in the stream's index (what
 * lets windows share tiles): where a merge joins unequal counts -- a window's edges, NaN holes -- a node's mean position
 * rounds relative to its absolute position, not to the window's extent.  r == 1 for a window at the stream's start,
 * where t_mean came out exact in every NaN-free window tried; a bucket of 60 samples at sample 10^9 keeps about 8 digits
 * of t_m2, c_tx and the slope.
 * Validation and the other semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID
 * with nothing written; payloads are checked only of the frames a window touches; windows may overlap and come in any
 * order; count == 0 and n_windows == 0 are valid.  Windows may be of any length (partials merge across the pieces of the
 * scratch that atsc_ctx_set_aggregate_scratch bounds): there is no ATSC_E_CAPACITY case. */
typedef struct {
    uint64_t count; /* samples of the window that are not NaN */
    double mean;    /* of those samples */
    double m2;      /* sum (x - mean)^2 */
    double t_mean;  /* mean position of those samples, in samples from the window's begin */
    double t_m2;    /* sum (t - t_mean)^2 */
    double c_tx;    /* sum (t - t_mean)(x - mean) */
} atsc_window_moments; /* 48 bytes */
/* d_out[i] holds window i.  begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned).
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.  The plan
 * keeps the call's tables, partials and scratch: the next moments call on the same plan waits (host side) until this
 * one's work is done; atsc_dplan_destroy frees them. */
int atsc_moments_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                             const uint64_t *begin, const uint64_t *count, atsc_window_moments *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_moments_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                         const uint64_t *begin, const uint64_t *count, atsc_window_moments *out);
/* What is read off the moments, host only (no GPU); out[i] from m[i], i < n:
 *   mean; variance = m2 / (double)count, stddev = sqrt(variance) (population forms);
 *   sample_variance = m2 / (double)(count - 1), NaN when count < 2; sample_stddev = sqrt(sample_variance);
 *   slope = c_tx / t_m2, NaN unless t_m2 > 0: the least-squares trend in value units PER SAMPLE (not per second: the
 *     spacing of samples in time is the caller's, and may differ between the segments of a VSRI index);
 *   intercept = mean - slope * t_mean (not fused): the fitted value at the window's first sample.
 * count == 0 gives NaN in all seven.  ATSC_E_INVALID for a null pointer with n > 0. */
typedef struct {
    double mean, variance, stddev, sample_variance, sample_stddev, slope, intercept;
} atsc_window_fit;
int atsc_moments_fit(const atsc_window_moments *m, uint64_t n, atsc_window_fit *out);

/* Windowed pair moments: per window [begin, begin + count) the centred moments of the values x and y of TWO decoded
 * streams X and Y over the same index range, and their centred co-moment: what covariance, correlation and the
 * regression of y on x are read from (atsc_pair_fit).  Sample i of X goes with sample i of Y; the streams may differ in
 * length, framing, codecs and tiers.  The reduction is the windowed moments' with y where they have the position t, so a
 * pair of series at 1e9 +- 1e-3 keeps its covariance, and the result is bit-exact: it depends only on the two streams'
 * samples and the window's (begin, count), not on the other windows, their order, the budget, piece boundaries, either
 * stream's framing or the device.
 *   Node   (n, mx, M2x, my, M2y, C).
 *   Leaf   of stream index i: (1, x[i], 0, y[i], 0, 0); a slot outside the window, or one where x[i] or y[i] is NaN, is
 *          the empty node (n = 0).
 *   Merge(a, b)   the moments' rule with t replaced by y: nb == 0: a, bit for bit; na == 0: b; else
 *          n = na + nb; w = (double)nb / (double)n; f = (double)na * w; dx = mxb - mxa; dy = myb - mya;
 *          mx = mxa + dx * w; my = mya + dy * w;
 *          M2x = (M2xa + M2xb) + (dx * dx) * f; M2y = (M2ya + M2yb) + (dy * dy) * f; C = (Ca + Cb) + (dx * dy) * f
 *          -- every operation one correctly rounded f64 + - * /, evaluated as written, never fused.
 *   Tree   the moments' tree: tiles of 2048 slots at multiples of 2048 in the stream index, the in-tile order of the
 *          aggregate sum, then pairwise over the window's tile partials (steps 1 to 3 under "Windowed moments").
 *   Result count = n, mean_x = mx, m2_x = M2x, mean_y = my, m2_y = M2y, c_xy = C; when count == 0 all five doubles are
 *          NaN.  +-Inf samples give what IEEE gives under these rules; where the rule yields NaN, any NaN bit pattern
 *          conforms.
 * Two consequences: with X and Y swapped the record is the same with the x and y fields swapped, bit for bit; with Y
 * the same stream as X, mean_y == mean_x and m2_y == c_xy == m2_x, and they are atsc_moments_windows' mean and m2 of that
 * stream, bit for bit.
 * With u = 2^-53, L = max(1, ceil(log2 count)), kappa_x = sqrt(1 + count mean_x^2 / m2_x) and kappa_y alike, for finite
 * data:
 *   |mean_x - exact| <= (L + 2) u mean|x|;            |m2_x - exact| <= (L + 2) u kappa_x m2_x;    (and for y)
 *   |c_xy - exact| <= (L + 2) u kappa_x kappa_y sqrt(m2_x m2_y);
 * m2_x == 0 and c_xy == 0 exactly where x is constant over the window's counted samples (and for y).
 * Validation and the other semantics are atsc_moments_windows_dev's, for both streams: a window beyond the end of EITHER
 * stream gives ATSC_E_INVALID with nothing written; payloads are checked only of the frames a window touches; windows
 * may overlap and come in any order; count == 0 and n_windows == 0 are valid; windows may be of any length. */
typedef struct {
    uint64_t count; /* samples of the window where neither x nor y is NaN */
    double mean_x;  /* of x over those samples */
    double m2_x;    /* sum (x - mean_x)^2 */
    double mean_y;  /* of y over those samples */
    double m2_y;    /* sum (y - mean_y)^2 */
    double c_xy;    /* sum (x - mean_x)(y - mean_y) */
} atsc_window_pair; /* 48 bytes */
/* d_out[i] holds window i.  begin / count are HOST arrays; d_body_x, d_body_y and d_out are device memory (d_out 8-byte
 * aligned).  The two plans must belong to one context (else ATSC_E_INVALID); dp_x == dp_y is allowed.  Enqueued on
 * `stream`, not synchronised.  A malformed payload inside a window sets the status word of the plan it belongs to.
 * dp_x keeps the call's tables, partials and scratch -- one region of decoded samples per stream, which together stay
 * inside the budget of atsc_ctx_set_aggregate_scratch (raised to one piece's minimum per stream): the next pair call
 * with the same dp_x waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_pair_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp_x, const uint8_t *d_body_x, const atsc_dplan *dp_y,
                          const uint8_t *d_body_y, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                          atsc_window_pair *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records of each stream, as
 * atsc_aggregate_windows does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window in either
 * stream. */
int atsc_pair_windows(atsc_ctx *ctx, const uint8_t *body_x, uint64_t len_x, int has_count_x, const uint8_t *body_y,
                      uint64_t len_y, int has_count_y, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                      atsc_window_pair *out);
/* What is read off the pair moments, host only (no GPU); out[i] from p[i], i < n:
 *   covariance = c_xy / (double)count (population form);
 *   sample_covariance = c_xy / (double)(count - 1), NaN when count < 2;
 *   correlation = (c_xy / sqrt(m2_x)) / sqrt(m2_y), clamped to [-1, 1]; NaN unless m2_x > 0 and m2_y > 0;
 *   slope = c_xy / m2_x, NaN unless m2_x > 0: the least-squares line of y on x;
 *   intercept = mean_y - slope * mean_x (not fused);
 *   r2 = correlation * correlation;     mean_diff = mean_x - mean_y.
 * count == 0 gives NaN in all seven.  ATSC_E_INVALID for a null pointer with n > 0. */
typedef struct {
    double covariance, sample_covariance, correlation, slope, intercept, r2, mean_diff;
} atsc_window_pair_fit; /* 56 bytes */
int atsc_pair_fit(const atsc_window_pair *p, uint64_t n, atsc_window_pair_fit *out);

/* Windowed pair matrix: per window the pair moments of EVERY pair of n_streams decoded streams, 1 <= n_streams <=
 * ATSC_ACROSS_MAX_STREAMS, in one call that decodes every stream once: what the covariance and the correlation matrix
 * of a fleet's series are read from.  Streams come as lists, as the across calls take them; windows as atsc_pair_windows
 * takes them (begin[] / count[] on the host, no stride).
 * Per window the result holds P = n_streams (n_streams + 1) / 2 atsc_window_pair records, one for every pair (i, j) with
 * i <= j, window-major: window w's record of (i, j) is d_out[w * P + p], p = i (2 n_streams - i + 1) / 2 + (j - i).
 *   THE CONTRACT: record (i, j) of window w is atsc_pair_windows' record of stream i as X and stream j as Y over that
 *   window, bit for bit.
 * Leaf, the pairwise-complete NaN rule (a slot counts where neither x_i nor x_j is NaN, whatever the other streams hold
 * there), Merge and the tree are the pair's, above.  Where the rule yields NaN, any NaN bit pattern conforms; a window
 * with count == 0 gives count == 0 and five NaNs in each of its P records.  It follows that
 *   - a record depends only on its two streams' samples and the window's (begin, count): not on the other streams,
 *     their order in the list, the other windows, the budget, the pieces or either stream's framing;
 *   - (i, i) is the diagonal: there m2_y == c_xy == m2_x, and they are atsc_moments_windows' mean and m2 of stream i;
 *   - a stream listed twice gives, at its off-diagonal place, its own diagonal record;
 *   - atsc_pair_fit applies to the W * P records unchanged;
 *   - no tolerance appears anywhere: the error bounds are the pair's.
 * ATSC_E_INVALID, with nothing written and before any GPU work, for: n_streams outside [1, 64]; a null list or a null
 * entry; plans of different contexts; a window beyond the end of ANY stream; d_out not 8-byte aligned; more than
 * 2^32 - 2 records (n_windows * P).  n_windows == 0 is valid.  The calls have no ATSC_E_CAPACITY case.
 * Memory the call holds on dp[0] (its tables, partials and scratch, of a kind of their own: the next pair matrix call
 * with the same dp[0] waits, host side, until this one's work is done; atsc_dplan_destroy frees them):
 *   - decoded regions as the across calls': one input's default shared among the n_streams regions, bounded by
 *     atsc_ctx_set_aggregate_scratch, at least one piece's minimum (32 tiles of 2048 samples) per region;
 *   - a partial table of (shared full tiles + 2 n_windows + combine levels) * P * 48 bytes. */
/* host only: P of n_streams, and p of (i, j) -- ~0ull for i > j or j >= n_streams */
uint64_t atsc_pair_matrix_records(uint32_t n_streams);
uint64_t atsc_pair_matrix_index(uint32_t n_streams, uint32_t i, uint32_t j);
/* begin / count are HOST arrays, dp and d_body host lists of n_streams entries; the bodies and d_out are device memory.
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the status word of the plan it
 * belongs to. */
int atsc_pair_matrix_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                 const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                 const uint64_t *count, atsc_window_pair *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records of each stream.
 * ATSC_E_FORMAT (nothing written) for a malformed payload inside a window in any stream. */
int atsc_pair_matrix_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                             const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                             atsc_window_pair *out);

/* Windowed deltas: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames) what
 * its samples do from one to the next, from the same decoded samples as the window decode: how much a counter grew and
 * how often it reset, how much a gauge moved up and down (total variation), the largest single jump and drop.
 *   Pairs  For every stream index j with begin < j < begin + count the pair of j is (a, b) = (x[j - 1], x[j]).  A pair
 *          is counted iff neither a nor b is NaN.  Pairs are stream-adjacent: a NaN sample removes the two pairs it
 *          belongs to, and nothing reaches across it.  A counted pair is a rise iff b > a and a fall iff b < a, compared
 *          as values: -0.0, +0.0 is neither, and +Inf, +Inf is neither.
 *   Terms  b - a of a rise (up, max_rise), a - b of a fall (down, max_fall), b of a fall (after_falls): each one correctly
 *          rounded f64 subtract, or b itself.
 *   Order  The three sums take the aggregate sum's tree unchanged (atsc_aggregate_windows, steps 1-3 above).  The term
 *          of pair j sits at slot j, the index of b; every other slot holds -0.0: slots outside the window, the window's
 *          own first slot, a pair that is not counted, a pair of the wrong direction.  A sum without a term is +0.0, as
 *          the aggregate's sum is for count == 0.  The counts and the two maxima are exact in any order.
 * count <= 1 gives the all-zero record.  +-Inf samples give what IEEE gives under these rules; where that is NaN, any NaN
 * conforms.  The record is bit-exact: it depends only on the stream's samples and the window's (begin, count), not on
 * the other windows, their order, the budget, piece boundaries or the device.  With u = 2^-53 and
 * L = max(1, ceil(log2 pairs)), for finite data |up - exact| <= (L + 3) u up_exact, and likewise for down (one rounding
 * for the subtract, L + 2 for the tree); on integer samples below 2^53 in sum all three sums are exact.
 * Validation and the other semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID
 * with nothing written; payloads are checked only of the frames a window touches; windows may overlap and come in any
 * order; count == 0 and n_windows == 0 are valid.  Windows may be of any length (partials add across the pieces of the
 * scratch that atsc_ctx_set_aggregate_scratch bounds, and the last sample of a piece is carried over to the next in the
 * call's tables, not in that scratch): there is no ATSC_E_CAPACITY case. */
typedef struct {
    uint64_t pairs;     /* counted pairs */
    uint64_t rises;     /* counted pairs with b > a */
    uint64_t falls;     /* counted pairs with b < a (a counter's resets) */
    double up;          /* sum of (b - a) over the rises */
    double down;        /* sum of (a - b) over the falls: >= 0 */
    double after_falls; /* sum of b over the falls: what a counter restarted at */
    double max_rise;    /* largest b - a of a rise; +0.0 when rises == 0 */
    double max_fall;    /* largest a - b of a fall; +0.0 when falls == 0 */
} atsc_window_delta; /* 64 bytes */
/* d_out[i] holds window i.  begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned).
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.  The plan
 * keeps the call's tables, partials and scratch: the next delta call on the same plan waits (host side) until this
 * one's work is done; atsc_dplan_destroy frees them. */
int atsc_delta_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                           const uint64_t *begin, const uint64_t *count, atsc_window_delta *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_delta_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                       const uint64_t *begin, const uint64_t *count, atsc_window_delta *out);
/* What is read off the deltas, host only (no GPU); out[i] from d[i], i < n; each value one f64 operation, not fused:
 *   changes = rises + falls (64-bit unsigned);
 *   variation = up + down: the total variation of the window's counted pairs;
 *   net = up - down: last - first of a NaN-free window, up to rounding;
 *   increase = up + after_falls: the counter increase in Prometheus terms, where every fall is a restart from zero;
 *   mean_step = variation / (double)pairs, NaN when pairs == 0.
 * ATSC_E_INVALID for a null pointer with n > 0. */
typedef struct {
    uint64_t changes;
    double variation, net, increase, mean_step;
} atsc_window_delta_fit; /* 40 bytes */
int atsc_delta_derive(const atsc_window_delta *d, uint64_t n, atsc_window_delta_fit *out);

/* Windowed runs: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames) which of
 * its samples meet a condition and whether those lie together, from the same decoded samples as the window decode: was
 * the series over a limit for 300 samples in a row (an alerting rule's `for:`), how many excursions were there, how long
 * was the longest and where did it start, is the series still over the limit at the window's end and for how long.
 *   Condition  an operator and a limit, the same for every window of a call.  A sample x is INSIDE iff it is not NaN and
 *          x OP limit holds, compared as values: -0.0 equals +0.0, +-Inf samples compare like any other value.  NaN is
 *          never inside, under ATSC_RUNS_NE too, so it ends a run.  limit may be +-Inf, not NaN.
 *   Runs   A run is a maximal stretch of stream-adjacent inside samples within the window; a run that the window's edge
 *          cuts counts with the length it has inside the window.  Positions are offsets from `begin`.
 *   excess The term of an inside sample is fabs(x - limit), one correctly rounded subtract, at the sample's own slot; every
 *          other slot holds -0.0, and the sum takes the aggregate sum's tree unchanged (atsc_aggregate_windows, steps 1-3
 *          above).  inside == 0 gives +0.0.  Where IEEE gives NaN, any NaN conforms: that is Inf - Inf alone, a +Inf
 *          sample against a +Inf limit under GE / LE / EQ, and likewise with -Inf.  With u = 2^-53 and
 *          L = max(1, ceil(log2 inside)), for finite data |excess - exact| <= (L + 3) u exact (one rounding for the
 *          subtract, L + 2 for the tree, as for the delta sums).
 * A window that is inside throughout has head == tail == longest == samples and runs == 1.  count == 0 gives samples =
 * inside = runs = longest = head = tail = 0, the three positions ATSC_RUNS_NONE and excess = +0.0.  The nine integers are
 * exact, and the whole record is bit-exact: it depends only on the stream's samples, the window and the condition, not on
 * the other windows, their order, the budget, piece boundaries or the device.
 * ATSC_E_INVALID with nothing written, before any GPU work, for an unknown op or a NaN limit.  Validation and the other
 * semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID with nothing written;
 * payloads are checked only of the frames a window touches; windows may overlap and come in any order; count == 0 and
 * n_windows == 0 are valid.  Windows may be of any length (a run that crosses two pieces of the scratch that
 * atsc_ctx_set_aggregate_scratch bounds is joined when their partials merge): there is no ATSC_E_CAPACITY case. */
enum { ATSC_RUNS_GT = 0, ATSC_RUNS_GE = 1, ATSC_RUNS_LT = 2, ATSC_RUNS_LE = 3, ATSC_RUNS_EQ = 4, ATSC_RUNS_NE = 5 };
#define ATSC_RUNS_NONE UINT64_MAX
typedef struct {
    uint64_t samples;    /* count[i], NaN included */
    uint64_t inside;     /* samples that meet the condition */
    uint64_t runs;       /* maximal runs */
    uint64_t longest;    /* length of the longest run; 0 when runs == 0 */
    uint64_t longest_at; /* offset of its first sample; of equal runs the earliest; ATSC_RUNS_NONE when runs == 0 */
    uint64_t first_at;   /* offset of the first inside sample; ATSC_RUNS_NONE when inside == 0 */
    uint64_t last_at;    /* offset of the last inside sample; ATSC_RUNS_NONE when inside == 0 */
    uint64_t head;       /* length of the run that starts at the window's first sample, else 0 */
    uint64_t tail;       /* length of the run that ends at the window's last sample, else 0 */
    double excess;       /* sum of |x - limit| over the inside samples */
} atsc_window_runs; /* 80 bytes */
/* d_out[i] holds window i.  begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned).
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.  The plan
 * keeps the call's tables, partials and scratch: the next runs call on the same plan waits (host side) until this
 * one's work is done; atsc_dplan_destroy frees them. */
int atsc_runs_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                          const uint64_t *begin, const uint64_t *count, int op, double limit, atsc_window_runs *d_out,
                          void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_runs_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                      const uint64_t *begin, const uint64_t *count, int op, double limit, atsc_window_runs *out);
/* Folds the records of n adjacent windows, left to right, into the record of their union, host only (no GPU): r[i + 1]
 * begins where r[i] ends -- per-minute buckets into hours, a run that goes on from one day's file into the next.  Records
 * with samples == 0 are skipped; n == 0 gives the empty record; ATSC_E_INVALID for a null pointer with n > 0 or a null
 * out.  The merge of a followed by b, o = a.samples, both non-empty:
 *   samples and inside add;  runs = a.runs + b.runs - (a.tail && b.head ? 1 : 0);
 *   head = a.head == a.samples ? a.samples + b.head : a.head;  tail = b.tail == b.samples ? b.samples + a.tail : b.tail;
 *   first_at = a.inside ? a.first_at : (b.inside ? b.first_at + o : NONE);  last_at = b.inside ? b.last_at + o : a.last_at;
 *   longest / longest_at: a's; the joined run a.tail + b.head at o - a.tail replaces it if both parts are non-zero and it
 *   is strictly longer; then b's, at b.longest_at + o, replaces that if strictly longer (so the earliest of equal runs wins).
 * The nine integers come out as the union window's, exactly.  excess is (r[0].excess + r[1].excess) + r[2].excess ...,
 * one add per record: it may differ from the union window's own value in its last bits. */
int atsc_runs_merge(const atsc_window_runs *r, uint64_t n, atsc_window_runs *out);

/* Windowed extremes: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames) its
 * k largest and its k smallest samples and where they are, from the same decoded samples as the window decode: when was
 * the peak of each hour, what are the five worst spikes of the day and when did they happen, first / last / min / max
 * with their positions per pixel column (M4 downsampling, together with atsc_aggregate_windows' first and last).
 * One k, 1 <= k <= ATSC_EXTREMES_MAX_K, holds for every window of a call.  The record of a window is 2 + 4 k eight-byte
 * words, ATSC_EXTREMES_BYTES(k) bytes: an atsc_window_extremes_head, then largest[0 .. k), then smallest[0 .. k), each an
 * atsc_extreme; record i lies at (char *)out + i * ATSC_EXTREMES_BYTES(k).
 *   Order    largest lists the window's non-NaN samples by value descending, smallest by value ascending, in both equal
 *            values earliest position first.  Samples are compared as values: -0.0 equals +0.0, so position decides
 *            between them; +-Inf are ordinary values.  That is numpy.argsort(-x, kind="stable") and
 *            numpy.argsort(x, kind="stable") with the NaNs dropped.
 *   Entries  value is the sample's own bits (a -0.0 stays -0.0), at its offset from `begin`.  NaN is never an entry; nans
 *            counts them.  count is count[i], NaN included.  A window with fewer than k non-NaN samples fills the
 *            remaining entries with value = NaN, at = ATSC_EXTREMES_NONE.  One sample may appear in both lists.
 *            count == 0 gives zeros in the head and 2 k empty entries.
 * There is no floating-point arithmetic in the contract: the record is bit-exact, and it depends only on the stream's
 * samples, the window and k, not on the other windows, their order, the budget, piece boundaries or the device.  The
 * first j entries of a call with k are the entries of a call with j < k; largest[0].value equals atsc_aggregate_windows'
 * max as a value and smallest[0].value its min.
 * ATSC_E_INVALID with nothing written, before any GPU work, for k == 0 or k > ATSC_EXTREMES_MAX_K.  Validation and the
 * other semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID with nothing written;
 * payloads are checked only of the frames a window touches; windows may overlap and come in any order; count == 0 and
 * n_windows == 0 are valid.  Windows may be of any length: there is no ATSC_E_CAPACITY case. */
typedef struct {
    double value; /* the sample's own bits; NaN in an empty entry */
    uint64_t at;  /* its offset from the window's begin; ATSC_EXTREMES_NONE in an empty entry */
} atsc_extreme; /* 16 bytes */
typedef struct {
    uint64_t count; /* count[i], NaN included */
    uint64_t nans;  /* NaN samples */
} atsc_window_extremes_head; /* 16 bytes */
#define ATSC_EXTREMES_MAX_K 16
#define ATSC_EXTREMES_NONE UINT64_MAX
#define ATSC_EXTREMES_BYTES(k) (16u + 32u * (size_t)(k))
/* Record i at (char *)d_out + i * ATSC_EXTREMES_BYTES(k).  begin / count are HOST arrays; d_body and d_out are device
 * memory (d_out 8-byte aligned).  Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the
 * plan's status word.  The plan keeps the call's tables, partials (2 + 4 k words each) and scratch: the next extremes
 * call on the same plan waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_extremes_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                              const uint64_t *begin, const uint64_t *count, uint32_t k, void *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_extremes_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                          const uint64_t *begin, const uint64_t *count, uint32_t k, void *out);
/* Folds the records of n adjacent windows (all of the same k), left to right, into the record of their union at `out`,
 * host only (no GPU): record i + 1 begins where record i ends.  count and nans add; every `at` of record i is shifted by
 * the counts in front of it; each list is the first k of the parts' lists merged in the order above.  The k best of a
 * union are among the k best of its parts, so -- unlike atsc_runs_merge's excess -- the merged record equals the union
 * window's own record bit for bit.  Records with count == 0 are skipped; n == 0 gives the empty record.  ATSC_E_INVALID
 * for a null pointer with n > 0, a null out, or k outside 1 .. ATSC_EXTREMES_MAX_K. */
int atsc_extremes_merge(const void *records, uint64_t n, uint32_t k, void *out);

/* Windowed value counts: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames)
 * its k smallest distinct values with their exact multiplicities, from the same decoded samples as the window decode:
 * "time in each state" for every enum-like series (up, a replica count, an HTTP status, a leader id, a breaker state, a
 * config version), without knowing the values in advance (PromQL's count_values, an aggregation across series at one
 * instant, is atsc_across_values_windows, which returns this record per position).  One k, 1 <= k <= ATSC_VALUES_MAX_K,
 * holds for every window of a call.  The record of a window is ATSC_VALUES_BYTES(k) = 32 + 16 k bytes, 8-byte aligned: an
 * atsc_window_values_head, then entry[0 .. k), each an atsc_value_count; record i lies at
 * (char *)out + i * ATSC_VALUES_BYTES(k).
 *   Equality  Samples are compared as values.  -0.0 equals +0.0, and that class is reported as +0.0 (the fixed sign of
 *             the aggregates' zero extreme); every other value is reported with its own bits.  +-Inf are ordinary
 *             values.  A NaN is never a value: it is counted in nans, whatever its payload.
 *   Order     Entries are in ascending value order.
 *   above     (a double, for paging)  When above is NaN, every non-NaN sample is listed.  Otherwise only samples with
 *             x > above (as values) are listed, and the non-NaN samples that are not listed are counted in below.
 *             above = +Inf lists nothing; above = -Inf leaves out only -Inf samples; above = +-0.0 leaves out the zero
 *             class and everything negative.  Calling again with above set to the last listed value walks a window with
 *             D > k distinct values exactly, in ceil(D / k) calls.
 *   Entries   entry[j] for j < distinct is the (j + 1)-th smallest distinct listed value and the number of the window's
 *             samples equal to it; the entries from `distinct` on hold value = NaN, n = 0.  count == 0 gives an all-zero
 *             head and k such entries.  Counts are exact 64-bit integers for windows of any length.
 * There is no floating-point arithmetic in the contract: the record is bit-exact, and it depends only on the stream's
 * samples, the window, k and above, not on the other windows, their order, the scratch budget, piece boundaries, the
 * framing or the device.  Consequences:
 *   - more == 0 implies count == nans + below + the sum of the entries' n;
 *   - the first j entries of a call with k are the entries of a call with j < k (same above); that call's distinct is
 *     min(distinct_k, j) and its more is distinct_k > j || more_k;
 *   - with above NaN and at least one non-NaN sample, entry[0].value equals atsc_aggregate_windows' min as a value;
 *   - the n of a listed value v equals atsc_runs_windows(ATSC_RUNS_EQ, v).inside.
 * ATSC_E_INVALID with nothing written, before any GPU work, for k == 0 or k > ATSC_VALUES_MAX_K.  Validation and the
 * other semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID with nothing written;
 * payloads are checked only of the frames a window touches; windows may overlap and come in any order; count == 0 and
 * n_windows == 0 are valid.  Windows may be of any length: there is no ATSC_E_CAPACITY case.  Decoded samples stay inside
 * the atsc_ctx_set_aggregate_scratch budget. */
typedef struct {
    uint64_t count;    /* count[i], NaN included */
    uint64_t nans;     /* NaN samples */
    uint64_t below;    /* non-NaN samples not above `above`; 0 when `above` is NaN */
    uint32_t distinct; /* entries filled: min(D, k), D = number of distinct listed values */
    uint32_t more;     /* 1 iff D > k, else 0 */
} atsc_window_values_head; /* 32 bytes */
typedef struct {
    double value; /* the value (+0.0 for the zeros); NaN in an unused entry */
    uint64_t n;   /* the window's samples equal to it; 0 in an unused entry */
} atsc_value_count; /* 16 bytes */
#define ATSC_VALUES_MAX_K 32
#define ATSC_VALUES_BYTES(k) (32u + 16u * (size_t)(k))
/* Record i at (char *)d_out + i * ATSC_VALUES_BYTES(k).  begin / count are HOST arrays; d_body and d_out are device
 * memory (d_out 8-byte aligned).  Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the
 * plan's status word.  The plan keeps the call's tables, partials (4 + 2 k words each) and scratch, in the place of the
 * extremes call's: the next value-count or extremes call on the same plan waits (host side) until this one's work is
 * done, and so does a value-count call behind an extremes call; atsc_dplan_destroy frees them. */
int atsc_values_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                            const uint64_t *begin, const uint64_t *count, uint32_t k, double above, void *d_out,
                            void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_values_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                        const uint64_t *begin, const uint64_t *count, uint32_t k, double above, void *out);
/* Folds the records of n PAIRWISE DISJOINT windows into the record of their union at `out`, host only (no GPU).  All
 * records must share one k and one above: that is the caller's duty.  The windows may come in any order, need not be
 * adjacent, and may belong to different streams (buckets into hours, one day's file into the next, one host's series
 * into another's).  count, nans and below add; the lists merge by value, the n of equal values added, and the result is
 * cut at k; more is set iff an entry was cut or any part had more.  Records with count == 0 are skipped; n == 0 gives the
 * empty record.  The merged record equals the union's own record bit for bit: a part's distinct values are a subset of
 * the union's, so the union's k-th smallest distinct value is no greater than any part's k-th; hence every value among
 * the union's first k that occurs in a part lies inside that part's list, with its exact count, and whatever a part's
 * more hides lies above the union's cut.  ATSC_E_INVALID for a null pointer with n > 0, a null out, or k outside
 * 1 .. ATSC_VALUES_MAX_K. */
int atsc_values_merge(const void *records, uint64_t n, uint32_t k, void *out);
/* What a caller reads off the value counts most often, host only: out[i] is the listed entry of record i with the
 * largest n, of equal n the smallest value; exact = (more == 0), i.e. whether every listed value was seen;
 * distinct == 0 gives value = NaN, n = 0.  ATSC_E_INVALID for a null pointer with n > 0 or k outside
 * 1 .. ATSC_VALUES_MAX_K. */
typedef struct {
    double value;
    uint64_t n;
    uint32_t exact;
    uint32_t pad;
} atsc_value_mode; /* 24 bytes */
int atsc_values_mode(const void *records, uint64_t n, uint32_t k, atsc_value_mode *out);

/* Windowed select: per window [begin, begin + count) of the decoded stream (the indices of atsc_decompress_frames) the
 * samples that meet a condition and where they are, from the same decoded samples as the window decode: every sample
 * above 0.9 of each hour with its position, WHERE value OP limit pushed down to the device.  The result is as large as
 * the data makes it; what comes back is the selected samples, not the windows.
 *   Condition  op is one of the ATSC_RUNS_* operators and limit the same for every window of a call; the rule is
 *              atsc_runs_windows': a sample is selected iff it is not NaN and x OP limit holds, compared as values.  -0.0
 *              equals +0.0; +-Inf samples and limits are ordinary values; NaN is never selected, under NE too.
 *   Block      ATSC_SELECT_BYTES(n_windows, cap) bytes, 8-byte aligned: off[0 .. n_windows] as uint64_t, then, at byte
 *              8 (n_windows + 1), the entries e[0 .. cap), each an atsc_selected.  off[0] = 0 and off[i + 1] - off[i] is the
 *              number of selected samples of window i: the offsets are always the true numbers, whatever cap is.  The
 *              selected samples of window i, in ascending position, are the entries off[i], off[i] + 1, ..; windows go in
 *              the order given.  Entry r is written iff r < cap: a call with too small a cap returns ATSC_OK and a
 *              correct prefix, and the caller compares off[n_windows] with cap.  cap == 0 is valid and is the sizing
 *              pass: only the offsets are written.  Bytes of the block behind entry min(off[n_windows], cap) are
 *              unspecified; nothing outside the block is ever touched.
 *   Entries    value is the sample's own bits (a -0.0 stays -0.0), at its offset from `begin`.
 * There is no floating-point arithmetic in the contract: the result is bit-exact.  The entries of window i depend only on
 * the stream's samples, the window and the condition, not on the other windows, their order, cap (apart from the
 * truncation), the budget, piece boundaries or the device.  off[i + 1] - off[i] equals atsc_runs_windows' inside, and the
 * first and the last entry's at its first_at and last_at.
 * ATSC_E_INVALID with nothing written, before any GPU work, for an unknown op or a NaN limit.  Validation and the other
 * semantics are atsc_aggregate_windows_dev's: a window beyond the stream gives ATSC_E_INVALID with nothing written;
 * payloads are checked only of the frames a window touches; windows may overlap and come in any order, at most 2^32 - 2
 * of them; count == 0 is valid; n_windows == 0 is valid and writes nothing.  Windows may be of any length: there is no
 * ATSC_E_CAPACITY case, and the decoded samples stay within the budget of atsc_ctx_set_aggregate_scratch. */
typedef struct {
    double value; /* the sample's own bits (a -0.0 stays -0.0) */
    uint64_t at;  /* its offset from the window's begin */
} atsc_selected; /* 16 bytes */
#define ATSC_SELECT_BYTES(n_windows, cap) (8u * ((size_t)(n_windows) + 1u) + 16u * (size_t)(cap))
/* begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, ATSC_SELECT_BYTES(n_windows,
 * cap) bytes).  Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.
 * The plan keeps the call's tables, counts and scratch: the next select call on the same plan waits (host side) until
 * this one's work is done; atsc_dplan_destroy frees them. */
int atsc_select_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                            const uint64_t *begin, const uint64_t *count, int op, double limit, uint64_t cap,
                            void *d_out, void *stream);
/* Host bytes in, host block out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does, and brings back the offsets and the entries written, not the rest of the block.  ATSC_E_FORMAT (nothing written)
 * for a malformed payload inside a window.  When every window is empty: n_windows + 1 zero offsets. */
int atsc_select_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                        const uint64_t *begin, const uint64_t *count, int op, double limit, uint64_t cap, void *out);

/* Windowed rolling: the sliding window of one width at every position of ranges of the decoded stream (the indices of
 * atsc_decompress_frames), from the same decoded samples as the window decode.  The caller names each range once; the
 * work grows with the ranges' lengths, not with positions x width.
 *   Ranges     Range i is [begin[i], begin[i] + count[i]).  One width w, 1 <= w <= ATSC_ROLLING_MAX_WIDTH, and one stride
 *              s >= 1 hold for every range of a call.  Range i has m_i = count[i] >= w ? (count[i] - w) / s + 1 : 0
 *              positions (atsc_rolling_outputs; 0 for w == 0 or s == 0); position j is the window [begin[i] + j s,
 *              begin[i] + j s + w), which lies wholly inside the range.  Records are stored range after range, position
 *              j of range i at index m_0 + .. + m_(i-1) + j of the result.  A range shorter than w has no record;
 *              n_windows == 0 and count[i] == 0 are valid.  Ranges may overlap and come in any order.
 *   count, min, max   what atsc_aggregate_windows returns for the same window, bit for bit, the sign of a zero extreme
 *              included.
 *   sum        over the window's non-NaN samples in an order of its own, fixed by the stream's samples and the window
 *              [lo, lo + w) alone: not by the range the window came from, the stride, the other ranges, the budget, the
 *              piece boundaries, the framing or the device.
 *              term(j) = x[j], or -0.0 where x[j] is NaN.
 *              T(a, 0) = term(a); T(a, l) = T(a, l - 1) + T(a + 2^(l-1), l - 1), for a a multiple of 2^l in the stream
 *              index (never an index into the part of the stream a call happened to upload).
 *              The window's chunks, left to right: pos = lo; while pos < lo + w, take the largest l with pos % 2^l == 0
 *              and pos + 2^l <= lo + w, emit (pos, l), pos += 2^l: at most 2 ceil(log2 w) chunks (one when w == 1).
 *              sum = ((T(c_1) + T(c_2)) + T(c_3)) + ..., every operation one correctly rounded f64 add, never fused;
 *              +0.0 when count == 0; +-Inf give what IEEE gives (where that is NaN, any NaN conforms).
 *              With u = 2^-53 and L = max(1, ceil(log2 w)): |sum - exact| <= 3 L u sum|x| for finite data (the tree
 *              rounds at most L times, the chain at most 2 L - 1 times).
 *              This sum MAY DIFFER from atsc_aggregate_windows' sum of the same window in its last bits: the two are
 *              different orders of the same additions, and each lies within its own stated bound of the exact sum.
 *              Chunks never reach outside their window, so T depends on no window: every window's sum is read off one
 *              pyramid of aligned chunk sums, which is what the order is for.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for width == 0, width > ATSC_ROLLING_MAX_WIDTH,
 * stride == 0, more than 2^32 - 2 records in all, and a range beyond the stream.  Payloads are checked only of the
 * frames that a position's window touches.  Decoded samples and the chunk sums both live inside the budget of
 * atsc_ctx_set_aggregate_scratch (raised to one piece's minimum: 65536 samples, as many bytes again of chunk sums, and two
 * large frames' room); a range longer than a piece is cut into pieces that overlap by w - 1 samples, and every position
 * is computed from one piece.  A width whose window does not fit one piece under the budget gives ATSC_E_CAPACITY (the
 * quantiles' rule; never under the default budget). */
#define ATSC_ROLLING_MAX_WIDTH (1ull << 20)
typedef struct {
    uint64_t count; /* samples of the position's window that are not NaN */
    double min, max; /* over those; NaN when count == 0 */
    double sum;      /* over those, in the order above; +0.0 when count == 0 */
} atsc_window_rolling; /* 32 bytes */
/* Positions of a range of `count` samples (host only, no GPU). */
uint64_t atsc_rolling_outputs(uint64_t count, uint64_t width, uint64_t stride);
/* begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 32 bytes per record).
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a position's window sets the plan's status word.
 * The plan keeps the call's tables and scratch: the next rolling call on the same plan waits (host side) until this
 * one's work is done; atsc_dplan_destroy frees them. */
int atsc_rolling_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                             const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                             atsc_window_rolling *d_out, void *stream);
/* Host bytes in, host records out, synchronous; walks and uploads only the touched records, as atsc_aggregate_windows
 * does, and computes the device call's bits.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a
 * position's window. */
int atsc_rolling_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                         const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                         atsc_window_rolling *out);

/* Windowed rolling deltas: the deltas' record (atsc_window_delta, 64 bytes) of the sliding window at every position of
 * ranges of the decoded stream: `increase(x[5m])`, `resets(x[5m])` and the total variation evaluated at every step,
 * without listing one window per position for atsc_delta_windows.
 *   Ranges     Ranges, width, stride, the number and the order of the records (atsc_rolling_outputs), the limits
 *              1 <= width <= ATSC_ROLLING_MAX_WIDTH and 2^32 - 2 records, validation, the errors (ATSC_E_INVALID with
 *              nothing written and before any GPU work; ATSC_E_FORMAT or the plan's status word for a malformed payload
 *              inside a position's window), pieces and ATSC_E_CAPACITY are atsc_rolling_windows'.  The messages name
 *              rolling_delta_windows.
 *   Pairs      For the position whose window is [lo, lo + w) the pairs are those of the stream indices lo < j < lo + w,
 *              exactly as atsc_delta_windows defines them for (begin, count) = (lo, w): what is counted, what a rise and
 *              a fall is, the terms, and the NaN handling.
 *   pairs, rises, falls, max_rise, max_fall   atsc_delta_windows' of that window, bit for bit (exact in any order).
 *   up, down, after_falls   in the rolling's order, over pair slots.  For each sum c:
 *              term_c(j) = the deltas' term of pair j for sum c, or -0.0 (a pair that is not counted or of the wrong
 *              direction).
 *              T(a, 0) = term(a); T(a, l) = T(a, l - 1) + T(a + 2^(l-1), l - 1), for a a multiple of 2^l in the stream
 *              index.
 *              The window's chunks are the canonical chunks of [lo + 1, lo + w), left to right: pos = lo + 1; while
 *              pos < lo + w, take the largest l with pos % 2^l == 0 and pos + 2^l <= lo + w, emit (pos, l),
 *              pos += 2^l.  sum = ((T(c_1) + T(c_2)) + T(c_3)) + ..., every operation one correctly rounded f64 add.
 *              A sum without a term is +0.0: up where rises == 0, down and after_falls where falls == 0.
 *              With u = 2^-53 and L = max(1, ceil(log2 w)), for finite data |up - exact| <= (3 L + 1) u up_exact, and
 *              likewise for down (one rounding for the subtract, then the rolling's 3 L).  On integer samples whose
 *              sums stay below 2^53 all three sums are exact, and then equal atsc_delta_windows' bit for bit; otherwise
 *              they MAY DIFFER from atsc_delta_windows' in their last bits, each within its own stated bound.
 * Width 1 gives the all-zero record.  A position's bytes depend on the stream's samples and (lo, w) only: not on the
 * range the window came from, the stride, the other ranges, the budget, the piece boundaries, the framing, the host or
 * the device call.  atsc_delta_derive applies to the records unchanged.
 * The chunk partials are 48 bytes (the rolling's: 32), at most 12 bytes a sample beside the 8 of the decoded sample, inside
 * the budget of atsc_ctx_set_aggregate_scratch as the rolling's are; the default budget holds every width.
 * begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 64 bytes per record).  Enqueued
 * on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place of the plan: a rolling
 * call and a rolling delta call on the same plan wait (host side) for each other. */
int atsc_rolling_delta_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                   const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                   atsc_window_delta *d_out, void *stream);
/* Host bytes in, host records out, synchronous, as atsc_rolling_windows is; computes the device call's bits. */
int atsc_rolling_delta_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                               const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                               atsc_window_delta *out);

/* Windowed rolling runs: the runs' record (atsc_window_runs, 80 bytes) of the sliding window at every position of ranges
 * of the decoded stream under the condition x OP limit: an alerting rule's `for: 5m` (inside == samples) evaluated at
 * every step, how long the series has been over the limit (tail), the excursions of the trailing hour (runs), the time a
 * signal spent in a state (inside) -- without listing one window per position for atsc_runs_windows.
 *   Ranges     Ranges, width, stride, the number and the order of the records (atsc_rolling_outputs), the limits
 *              1 <= width <= ATSC_ROLLING_MAX_WIDTH and 2^32 - 2 records, validation, the errors (ATSC_E_INVALID with
 *              nothing written and before any GPU work; ATSC_E_FORMAT or the plan's status word for a malformed payload
 *              inside a position's window), pieces and ATSC_E_CAPACITY are atsc_rolling_windows'.  The messages name
 *              rolling_runs_windows.  In addition an unknown op or a NaN limit is ATSC_E_INVALID, nothing written and
 *              before any GPU work: atsc_runs_windows' rule.
 *   Condition  atsc_runs_windows', unchanged: op is one of the ATSC_RUNS_* operators and limit the same for every position
 *              of a call; a sample is inside iff it is not NaN and x OP limit holds.  NaN is never inside, under
 *              ATSC_RUNS_NE too; -0.0 equals +0.0; +-Inf samples and limits compare as values.
 *   samples, inside, runs, longest, longest_at, first_at, last_at, head, tail   For the position whose window is
 *              [lo, lo + w) they are atsc_runs_windows' of (begin, count) = (lo, w), exactly: samples = w, offsets count
 *              from lo, of equal longest runs the earliest wins, and ATSC_RUNS_NONE stands where that call has it.  The
 *              merge rule of the nine integers is associative, so they are exact in any order.
 *   excess     in the rolling's order, over sample slots.
 *              term(j) = fabs(x[j] - limit) where x[j] is inside (the subtract one correctly rounded operation), else
 *              -0.0.
 *              T(a, 0) = term(a); T(a, l) = T(a, l - 1) + T(a + 2^(l-1), l - 1), for a a multiple of 2^l in the stream
 *              index.  The window's chunks are the rolling's, left to right: pos = lo; while pos < lo + w, take the
 *              largest l with pos % 2^l == 0 and pos + 2^l <= lo + w, emit (pos, l), pos += 2^l.
 *              excess = ((T(c_1) + T(c_2)) + T(c_3)) + ..., every operation one correctly rounded f64 add, never fused;
 *              +0.0 where inside == 0; where IEEE gives NaN (Inf - Inf only) any NaN conforms.
 *              With u = 2^-53 and L = max(1, ceil(log2 w)), for finite data |excess - exact| <= (3 L + 1) u exact (one
 *              rounding for the subtract, then the rolling's 3 L).  On integer samples and an integer limit whose sums
 *              stay below 2^53 excess is exact, and then equals atsc_runs_windows' bit for bit; otherwise it MAY DIFFER
 *              from atsc_runs_windows' excess of the same window in its last bits, each within its own stated bound.
 * A position's 80 bytes depend on the stream's samples, (lo, w) and the condition only: not on the range the window came
 * from, the stride, the other ranges, the budget, the piece boundaries, the framing, the host, the device or the stream
 * call.  atsc_runs_merge applies unchanged to the records of adjacent disjoint positions, which needs stride == width.
 * The chunk partials are 32 bytes, the rolling's size (the nine integers without the chunk's length, packed, and
 * excess), at most 8 bytes a sample beside the 8 of the decoded sample, inside the budget of
 * atsc_ctx_set_aggregate_scratch as the rolling's are; the default budget holds every width.
 * begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 80 bytes per record).  Enqueued
 * on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place of the plan: it and the
 * other rolling calls on the same plan wait (host side) for each other. */
int atsc_rolling_runs_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                  const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride, int op,
                                  double limit, atsc_window_runs *d_out, void *stream);
/* Host bytes in, host records out, synchronous, as atsc_rolling_windows is; computes the device call's bits. */
int atsc_rolling_runs_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                              const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride, int op,
                              double limit, atsc_window_runs *out);

/* Windowed rolling moments: the moments' record (atsc_window_moments, 48 bytes) of the sliding window at every position
 * of ranges of the decoded stream: `stddev_over_time(x[5m])`, `stdvar_over_time`, `deriv(x[5m])` and `predict_linear`
 * evaluated at every step, a z-score against a trailing baseline, a moving least-squares slope -- without listing one
 * window per position for atsc_moments_windows.  atsc_moments_fit applies to the records unchanged.
 *   Ranges     Ranges, width, stride, the number and the order of the records (atsc_rolling_outputs), the limits
 *              1 <= width <= ATSC_ROLLING_MAX_WIDTH and 2^32 - 2 records, validation, the errors (ATSC_E_INVALID with
 *              nothing written and before any GPU work; ATSC_E_FORMAT or the plan's status word for a malformed payload
 *              inside a position's window), pieces and ATSC_E_CAPACITY are atsc_rolling_windows'.  The messages name
 *              rolling_moments_windows.
 *   Node, leaf, Merge   atsc_moments_windows', word for word: the node is (n, mx, M2x, mt, M2t, C); the leaf of stream
 *              index j is (1, x[j], 0, (double)j, 0, 0), a slot holding NaN the empty node (n = 0); Merge(a, b) is a,
 *              bit for bit, when nb == 0, b when na == 0, else the rule given there, every operation one correctly
 *              rounded f64 + - * /, never fused.  The position t of a leaf is its index in the stream (never an index
 *              into the part of the stream a call happened to upload), so a chunk's node depends on no window, range,
 *              piece or budget.
 *   Order      N(a, 0) = leaf(a); N(a, l) = Merge(N(a, l - 1), N(a + 2^(l-1), l - 1)), for a a multiple of 2^l in the
 *              stream index.  The window's chunks are the rolling's, left to right: pos = lo; while pos < lo + w, take
 *              the largest l with pos % 2^l == 0 and pos + 2^l <= lo + w, emit (pos, l), pos += 2^l.
 *              R = Merge(Merge(Merge(N(c_1), N(c_2)), N(c_3)), ...), the left operand as a.
 *   Record     count = n, mean = mx, m2 = M2x, t_m2 = M2t, c_tx = C, t_mean = mt - (double)lo (one subtract); when
 *              count == 0 all five doubles are NaN.  +-Inf samples give what IEEE gives under these rules; where the
 *              rule yields NaN, any NaN bit pattern conforms.
 *   count      atsc_moments_windows' of the window (lo, w), exactly.  The five doubles come from another tree than that
 *              call's and MAY DIFFER from its in their last bits; each lies within its own stated bound.
 * With u = 2^-53, L = max(1, ceil(log2 w)), kappa = sqrt(1 + count mean^2 / m2) and r = (lo + w) / w, for finite data:
 *   |mean - exact| <= (3 L + 2) u mean|x|;            |m2 - exact| <= (3 L + 2) u kappa m2;
 *   |t_m2 - exact| <= (3 L + 2) u r t_m2;             |c_tx - exact| <= (3 L + 2) u r kappa sqrt(t_m2 m2);
 *   |t_mean - exact| <= (3 L + 2) u (lo + w);
 * the windowed moments' bounds with 3 L for L: a node passes at most L merges inside a chunk and at most 2 L - 1 in the
 * chain (the rolling's count).  m2 == 0 and c_tx == 0 exactly on a constant window.
 * A position's bytes depend on the stream's samples and (lo, w) only: not on the range the window came from, the stride,
 * the other ranges, the budget, the piece boundaries, the framing, the host or the device call.
 * The chunk partials are 48 bytes (the node; the count in a 64-bit word), at most 12 bytes a sample beside the 8 of the
 * decoded sample, inside the budget of atsc_ctx_set_aggregate_scratch as the rolling deltas' are; the default budget holds
 * every width.
 * begin / count are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 48 bytes per record).  Enqueued
 * on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place of the plan: a rolling, a
 * rolling delta and a rolling moments call on the same plan wait (host side) for each other. */
int atsc_rolling_moments_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                     const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                     atsc_window_moments *d_out, void *stream);
/* Host bytes in, host records out, synchronous, as atsc_rolling_windows is; computes the device call's bits. */
int atsc_rolling_moments_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                 const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                 atsc_window_moments *out);

/* Windowed rolling quantiles: the levels q[0 .. n_q) of the sliding window at every position of ranges of the decoded
 * stream: `quantile_over_time(0.99, x[5m])` evaluated at every step, a rolling median for despiking (a Hampel filter is
 * a rolling median and a rolling MAD), a p95 band round a moving baseline -- without listing one window per position
 * for atsc_quantile_windows.
 *   Ranges     Ranges, width w, stride s, the number and the order of the positions (atsc_rolling_outputs), the limit of
 *              2^32 - 2 positions in all and validation are atsc_rolling_windows'; the width's limit is
 *              1 <= w <= ATSC_ROLLING_QUANTILE_MAX_WIDTH.  The messages name rolling_quantile_windows.
 *   Result     n_q doubles per position: with m_i = atsc_rolling_outputs(count[i], w, s), row j of range i is at
 *              out[(m_0 + .. + m_(i-1) + j) * n_q], level t of it at + t.
 *   Row        The row of the position whose window is [lo, lo + w) is, bit for bit, the row atsc_quantile_windows
 *              returns for (begin, count) = (lo, w) with the same levels and method: the window's non-NaN samples in the
 *              total order of the quantiles' key (-0.0 before +0.0), ranks and interpolation by the rule stated there
 *              (q_pick / q_interp of atsc_quantile_rule.h and nothing else); an empty or all-NaN window gives NaN at
 *              every level (any NaN bit pattern conforms).  Selection is exact: a position's bits depend on the stream's
 *              samples and (lo, w) alone, not on the range the window came from, the stride, the other ranges, the
 *              budget, the piece boundaries, how positions were grouped, the framing, the host or the device call.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_rolling_windows, for
 * width > ATSC_ROLLING_QUANTILE_MAX_WIDTH (the message says the limit and names atsc_quantile_windows with listed
 * windows, which takes any width), a null q, n_q == 0 or n_q > 64, a level that is NaN or outside [0, 1], an unknown
 * method, a d_out that is not 8-byte aligned.  ATSC_E_FORMAT (host form) or the plan's status word (device form) for a
 * malformed payload inside a position's window.
 * The limit is the length up to which one window's keys fit one workgroup's LDS (the windowed quantiles' medium tier).
 * It is far below the least piece of the scratch (65536 samples), so every window fits a piece whatever the budget of
 * atsc_ctx_set_aggregate_scratch: the call has NO ATSC_E_CAPACITY case.  The scratch holds the decoded samples only (8
 * bytes a sample).
 * begin / count / q are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 8 n_q bytes per
 * position).  Enqueued on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place of
 * the plan: it and the rolling calls on the same plan wait (host side) for each other. */
#define ATSC_ROLLING_QUANTILE_MAX_WIDTH 8192
int atsc_rolling_quantile_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                      const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                      uint32_t n_q, const double *q, int method, double *d_out, void *stream);
/* Host bytes in, host rows out, synchronous, as atsc_rolling_windows is; computes the device call's bits. */
int atsc_rolling_quantile_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                  const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                  uint32_t n_q, const double *q, int method, double *out);

/* Windowed rolling histograms: the value-bin counts of the sliding window at every position of ranges of the decoded
 * stream: a latency heat map at every step, the Prometheus `le` bucket counts over `x[5m]` at every evaluation time (the
 * input of `histogram_quantile`), an SLO's "share of samples under 200 ms over the trailing hour" at every step --
 * without listing one window per position for atsc_histogram_windows.
 *   Ranges     Ranges, width w, stride s, the number and the order of the positions (atsc_rolling_outputs),
 *              1 <= w <= ATSC_ROLLING_MAX_WIDTH, s >= 1, the limit of 2^32 - 2 positions in all and validation are
 *              atsc_rolling_windows'.  The messages name rolling_histogram_windows.
 *   Edges      edges[0 .. n_edges), closed and their validation are atsc_histogram_windows': n_edges in
 *              1 .. ATSC_HIST_MAX_EDGES, strictly ascending as values, no NaN edge, +-Inf allowed.
 *   Result     n_edges + 2 u64 counters per position, in the histograms' layout (bins 0 .. n_edges, then the NaN samples):
 *              with m_i = atsc_rolling_outputs(count[i], w, s), row j of range i is at
 *              out[(m_0 + .. + m_(i-1) + j) * (n_edges + 2)].  positions x (n_edges + 2) must be below 2^32 - 1, so that
 *              a counter's index fits 32 bits.  The caller sizes the result: sum m_i x (n_edges + 2) x 8 bytes.
 *   Row        The row of the position whose window is [lo, lo + w) is, bit for bit, the row atsc_histogram_windows
 *              returns for (begin, count) = (lo, w) with the same edges and closed; its counters sum to w.  Counts are
 *              integers: a position's bytes depend on the stream's samples, (lo, w), the edges and closed alone, not on
 *              the range the window came from, the stride, the other ranges, the budget, the piece boundaries, how
 *              positions were grouped, the framing, the host or the device call.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_rolling_windows, for every
 * case of atsc_histogram_windows' edge checks (null edges, n_edges == 0 or above ATSC_HIST_MAX_EDGES, a NaN edge, edges
 * not strictly ascending, an unknown closed), for positions x (n_edges + 2) >= 2^32 - 1 (the message says so), a d_out
 * that is not 8-byte aligned.  ATSC_E_CAPACITY when a window is longer than one scratch piece under the budget of
 * atsc_ctx_set_aggregate_scratch (the message says the budget that would hold it; the default budget holds every
 * width).  ATSC_E_FORMAT (host form) or the plan's status word (device form) for a malformed payload inside a
 * position's window.
 * The scratch holds the decoded samples only (8 bytes a sample); consecutive pieces overlap by w - 1 samples.
 * begin / count / edges are HOST arrays; d_body and d_out are device memory (d_out 8-byte aligned, 8 (n_edges + 2) bytes
 * per position).  Enqueued on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place
 * of the plan: it and the rolling calls on the same plan wait (host side) for each other. */
int atsc_rolling_histogram_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                       const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                       uint32_t n_edges, const double *edges, int closed, uint64_t *d_out, void *stream);
/* Host bytes in, host rows out, synchronous, as atsc_rolling_windows is; computes the device call's bits. */
int atsc_rolling_histogram_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                   const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                   uint32_t n_edges, const double *edges, int closed, uint64_t *out);

/* Windowed rolling pair moments: the pair moments' record (atsc_window_pair, 48 bytes) of the sliding window at every
 * position of ranges of TWO decoded streams X and Y: a rolling correlation ("does latency follow load over the last five
 * minutes, at every step"), a rolling beta (the regression slope of y on x), the covariance against a reference series
 * -- without listing one window per position for atsc_pair_windows.  Sample j of X goes with sample j of Y; the streams
 * may differ in length, framing, codecs and tiers.  atsc_pair_fit applies to the records unchanged.
 *   Ranges     Ranges, width, stride, the number and the order of the records (atsc_rolling_outputs), the limits
 *              1 <= width <= ATSC_ROLLING_MAX_WIDTH and 2^32 - 2 records, validation, the errors (ATSC_E_INVALID with
 *              nothing written and before any GPU work; ATSC_E_FORMAT or the status word of the plan it belongs to for a
 *              malformed payload inside a position's window), pieces and ATSC_E_CAPACITY are atsc_rolling_windows'.  The
 *              messages name rolling_pair_windows.  A range that reaches beyond the end of EITHER stream is
 *              ATSC_E_INVALID.  The two plans (or streams) must belong to one context, else ATSC_E_INVALID; dp_x == dp_y
 *              is allowed.
 *   Node, leaf, Merge   atsc_pair_windows', word for word: the node is (n, mx, M2x, my, M2y, C); the leaf of stream
 *              index j is (1, x[j], 0, y[j], 0, 0), the empty node (n = 0) where x[j] or y[j] is NaN; Merge(a, b) is a,
 *              bit for bit, when nb == 0, b when na == 0, else the rule given there, every operation one correctly
 *              rounded f64 + - * /, never fused.
 *   Order      atsc_rolling_moments_windows', word for word: N(a, 0) = leaf(a); N(a, l) = Merge(N(a, l - 1),
 *              N(a + 2^(l-1), l - 1)), for a a multiple of 2^l in the stream index.  The window's chunks are the
 *              rolling's, left to right: pos = lo; while pos < lo + w, take the largest l with pos % 2^l == 0 and
 *              pos + 2^l <= lo + w, emit (pos, l), pos += 2^l.  R = Merge(Merge(Merge(empty, N(c_1)), N(c_2)), ...), the
 *              left operand as a.
 *   Record     count = n, mean_x = mx, m2_x = M2x, mean_y = my, m2_y = M2y, c_xy = C; when count == 0 all five doubles
 *              are NaN.  No field is counted from lo: there is no subtract.  +-Inf samples give what IEEE gives under
 *              these rules; where the rule yields NaN, any NaN bit pattern conforms.
 * Consequences: a position's bytes depend on the two streams' samples and (lo, w) only: not on the range the window came
 * from, the stride, the other ranges, the budget, the piece boundaries, either stream's framing, the host, the device or
 * the stream call.  With X and Y swapped the record is the same with the x and y fields swapped, bit for bit.  With Y the
 * same stream as X, mean_y == mean_x and m2_y == c_xy == m2_x, and count, mean_x and m2_x are
 * atsc_rolling_moments_windows' count, mean and m2 of that stream, bit for bit (the tree and the merge are the same).
 * count is atsc_pair_windows' of the listed window (lo, w), exactly; the five doubles come from another tree than that
 * call's and MAY DIFFER from its in their last bits; each lies within its own stated bound.
 * With u = 2^-53, L = max(1, ceil(log2 w)), kappa_x = sqrt(1 + count mean_x^2 / m2_x) and kappa_y alike, for finite data:
 *   |mean_x - exact| <= (3 L + 2) u mean|x|;          |m2_x - exact| <= (3 L + 2) u kappa_x m2_x;    (and for y)
 *   |c_xy - exact| <= (3 L + 2) u kappa_x kappa_y sqrt(m2_x m2_y);
 * the pair's bounds with 3 L + 2 for L + 2, the step the rolling moments took from the windowed moments: a node passes
 * at most L merges inside a chunk and at most 2 L - 1 in the chain.  m2_x == 0 and c_xy == 0 exactly where x is constant
 * over the window's counted samples (and for y).
 * The chunk partials are the rolling moments' 48 bytes, at most 12 bytes a slot beside the 8 of each stream's decoded
 * sample: 28 bytes a slot inside the budget of atsc_ctx_set_aggregate_scratch (the rolling moments': 20); a width that
 * the budget's piece does not hold is ATSC_E_CAPACITY, and the message names the budget that would hold it,
 * (w + 4 * 2048) * 28 bytes and the spill slots of the large frames.  The default budget holds every width.
 * begin / count are HOST arrays; d_body_x, d_body_y and d_out are device memory (d_out 8-byte aligned, 48 bytes per
 * record).  Enqueued on `stream`, not synchronised.  The call keeps its tables and scratch in the rolling's place of
 * dp_x: it and the rolling, rolling delta and rolling moments calls on dp_x wait (host side) for each other. */
int atsc_rolling_pair_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp_x, const uint8_t *d_body_x, const atsc_dplan *dp_y,
                                  const uint8_t *d_body_y, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                  uint64_t width, uint64_t stride, atsc_window_pair *d_out, void *stream);
/* Host bytes in, host records out, synchronous, as atsc_pair_windows is; computes the device call's bits.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload inside a position's window in either stream. */
int atsc_rolling_pair_windows(atsc_ctx *ctx, const uint8_t *body_x, uint64_t len_x, int has_count_x, const uint8_t *body_y,
                              uint64_t len_y, int has_count_y, uint64_t n_windows, const uint64_t *begin,
                              const uint64_t *count, uint64_t width, uint64_t stride, atsc_window_pair *out);

/* Windowed across: count, min, max and sum over N streams at every position of ranges of the decoded streams (the
 * indices of atsc_decompress_frames): one value per sample index folded across many series -- `sum by (job)(x)`,
 * `max by (zone)(x)`, how many replicas report at this instant and which one is the worst -- without the decoded
 * samples leaving the library.  The streams may differ in framing, codecs and tiers.
 *   Ranges     Range i is [begin[i], begin[i] + count[i]), counted in every stream's own decoded index: sample j of
 *              stream 0 goes with sample j of every other stream, as in the pair moments.  One stride s >= 1 holds for
 *              a call.  Range i has m_i = count[i] && s ? (count[i] - 1) / s + 1 : 0 positions (atsc_across_outputs);
 *              position p is sample begin[i] + p s.  Records are stored range after range, as the rolling's are:
 *              record m_0 + .. + m_(i-1) + p is position p of range i.  Ranges may overlap, come in any order and be
 *              empty; n_windows == 0 is valid.
 *   Record     over x_k = the sample of stream k at the position, k = 0 .. N - 1 in the order of the call's list:
 *              count   the number of k with x_k not NaN;
 *              min, min_at   walk k upward: the first x_k that is not NaN starts the minimum, a later one replaces it
 *                      iff x_k < min.  Of equal values, and of zeros of either sign, the lowest k is kept; min is
 *                      stream min_at's sample bit for bit;
 *              max, max_at   the same rule with >;
 *              sum     ((t_0 + t_1) + t_2) + .. with t_k = x_k, or -0.0 where x_k is NaN: every operation one
 *                      correctly rounded f64 add, in list order, never fused or reassociated; forced to +0.0 when
 *                      count == 0.  +-Inf give what IEEE gives (where that is NaN, any NaN conforms).  The sum depends
 *                      only on the N samples and the order of the list: not on the range, the stride, the budget, the
 *                      piece boundaries, the framing or the device.
 *              No other arithmetic touches a sample: every field is bit-exact.
 *   Stride     a range is decoded whole whatever the stride: a stride does not skip frames, it thins the records.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for n_streams == 0 or n_streams >
 * ATSC_ACROSS_MAX_STREAMS, a null list or a null entry in a list, stride == 0, more than 2^32 - 2 records in all, a
 * range beyond the end of ANY of the streams, and plans or streams of different contexts.  The same plan, body or stream
 * may appear more than once in the list.  Payloads are checked only of the frames (of any stream) that a range touches.
 * Every stream is decoded piece by piece into a scratch region of its own; the budget of atsc_ctx_set_aggregate_scratch
 * is shared evenly by the N regions (each raised to one piece's minimum, 65536 samples, and two large frames' room where
 * the stream has large frames); without a budget the call's total is the default of ONE stream shared by the N regions.
 * A position needs one slot per stream, so pieces do not overlap; there is no ATSC_E_CAPACITY case. */
#define ATSC_ACROSS_MAX_STREAMS 64
typedef struct {
    uint32_t count;          /* streams whose sample at this position is not NaN */
    uint16_t min_at, max_at; /* index (into the call's stream list) of the stream that holds min / max; 0xFFFF when count == 0 */
    double min, max;         /* NaN when count == 0 */
    double sum;              /* +0.0 when count == 0 */
} atsc_across_record;        /* 32 bytes */
/* Positions of a range of `count` samples (host only, no GPU): count && stride ? (count - 1) / stride + 1 : 0. */
uint64_t atsc_across_outputs(uint64_t count, uint64_t stride);
/* dp / d_body (n_streams entries each) and begin / count are HOST arrays; d_body[k] and d_out are device memory (d_out
 * 8-byte aligned, 32 bytes per record).  Enqueued on `stream`, not synchronised.  A malformed payload in a frame of
 * stream k that a range touches sets dp[k]'s status word.  dp[0] keeps the call's tables and scratch: the next across
 * call whose first plan is dp[0] waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_across_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp, const uint8_t *const *d_body,
                            uint64_t n_windows, const uint64_t *begin, const uint64_t *count, uint64_t stride,
                            atsc_across_record *d_out, void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host records out, synchronous; walks and uploads only
 * the touched records of every stream, as atsc_aggregate_windows does, and computes the device call's bits.
 * ATSC_E_FORMAT (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                        const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                        uint64_t stride, atsc_across_record *out);

/* Windowed quantiles: exact order statistics of windows [begin, begin + count) of the decoded stream (the indices of
 * atsc_decompress_frames), from the same decoded samples as the window decode.  For window i:
 *   x  the window's non-NaN samples, n of them, sorted in IEEE total order (-0.0 before +0.0), i.e. by the keys
 *      bits(v) ^ (sign(v) ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000);
 *   v = (double)(n - 1) * q[j] (one f64 multiply); out[i * n_q + j] by the method:
 *     LOWER x[floor(v)]; HIGHER x[ceil(v)]; NEAREST x[rint(v)] (ties to even, as numpy.around);
 *     LINEAR (NumPy's default method) lo = floor(v), hi = min(lo + 1, n - 1), t = v - lo: x[lo] when t == 0 or
 *       lo == hi, else with d = x[hi] - x[lo]: t >= 0.5 ? x[hi] - d * (1 - t) : x[lo] + d * t (NumPy's _lerp, no fused
 *       multiply-add);
 *   n == 0 (an empty or all-NaN window): NaN for every level.
 * The result depends only on the window's samples, not on the other windows, the other levels, the budget or the
 * device.  It equals numpy.nanquantile as a value on finite data; where NumPy's interpolation meets Inf - Inf and gives
 * NaN, the rule above gives the Inf (np.quantile([1, inf], 1.0) is NaN, here +Inf).
 * Validation (ATSC_E_INVALID, nothing written): a null argument, a window beyond the stream, n_q == 0 or n_q > 64, a
 * level that is NaN or outside [0, 1], an unknown method.  n_windows == 0 is valid; windows may overlap and come in any
 * order.  Every window is held whole in the decoded-sample scratch that atsc_ctx_set_aggregate_scratch bounds: a window
 * longer than one piece of that budget gives ATSC_E_CAPACITY with nothing written, and atsc_ctx_last_error names the
 * budget that would hold it. */
enum { ATSC_QUANTILE_LINEAR = 0, ATSC_QUANTILE_LOWER = 1, ATSC_QUANTILE_HIGHER = 2, ATSC_QUANTILE_NEAREST = 3 };
/* begin / count / q are HOST arrays; d_body and d_out (n_windows * n_q doubles, 8-byte aligned) are device memory.
 * Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.  The plan
 * keeps the call's tables and scratch: the next quantile call on the same plan waits (host side) until this one's work
 * is done; atsc_dplan_destroy frees them. */
int atsc_quantile_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                              const uint64_t *begin, const uint64_t *count, uint32_t n_q, const double *q, int method,
                              double *d_out, void *stream);
/* Host bytes in, host results out (n_windows * n_q doubles), synchronous; walks and uploads only the touched records,
 * as atsc_aggregate_windows does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_quantile_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                          const uint64_t *begin, const uint64_t *count, uint32_t n_q, const double *q, int method,
                          double *out);

/* Windowed across quantiles: order statistics of the N samples that the streams of a call hold at every position of
 * ranges of the decoded streams -- the median replica, the p95 across a zone's hosts, `quantile by (job)(0.9, x)` --
 * without the decoded samples leaving the library.
 *   Ranges     atsc_across_windows' exactly: one stride for the call, range i has atsc_across_outputs(count[i], stride)
 *              positions, records are numbered range after range in the same order.
 *   Result     record r is a row of n_q doubles at out[r * n_q + j], level j of the call's q.
 *   Row        x_k = the sample of stream k at the position; the NaN ones are dropped, n are left, sorted in IEEE
 *              total order (the windowed quantiles' key, -0.0 before +0.0); then the windowed quantiles' rule, unchanged,
 *              over that sorted column: v = (double)(n - 1) * q[j], the ranks by the method, LINEAR by NumPy's _lerp
 *              with no fused multiply-add.  n == 0 gives NaN for every level.
 *              A row depends only on the N samples of its position, the levels and the method: not on the order of the
 *              list (a reversed list gives the same bytes), the range, the stride, the budget, the piece boundaries, the
 *              framing or the device.  Every value is bit-exact; where the rule's own arithmetic meets Inf - Inf, any
 *              NaN conforms.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_across_windows, a null q,
 * n_q == 0 or n_q > 64, a level that is NaN or outside [0, 1], an unknown method, a result pointer that is not 8-byte
 * aligned.  n_windows == 0 and empty ranges write nothing.  Scratch and pieces are the across': there is no
 * ATSC_E_CAPACITY case. */
/* dp / d_body (n_streams entries each), begin / count and q are HOST arrays; d_body[k] and d_out are device memory
 * (d_out 8-byte aligned, n_q doubles per record).  Enqueued on `stream`, not synchronised.  A malformed payload in a
 * frame of stream k that a range touches sets dp[k]'s status word.  dp[0] keeps the call's tables and scratch, apart from
 * the across': the next across quantile (or across extremes or across moments, which share the place) call whose first
 * plan is dp[0] waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_across_quantile_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                     const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                     const uint64_t *count, uint64_t stride, uint32_t n_q, const double *q, int method,
                                     double *d_out, void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host rows out, synchronous; walks and uploads only the
 * touched records of every stream, as atsc_across_windows does, and computes the device call's bits.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_quantile_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                 const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                 uint64_t stride, uint32_t n_q, const double *q, int method, double *out);

/* Windowed across extremes: the k largest and the k smallest of the N samples that the streams of a call hold at every
 * position of ranges of the decoded streams, and which streams hold them -- `topk(3, x)` / `bottomk(5, x)`, the three
 * slowest replicas at every step, who was second worst when the worst one was restarted -- without the decoded samples
 * leaving the library.
 *   Ranges     atsc_across_windows' exactly: one stride for the call, range i has atsc_across_outputs(count[i], stride)
 *              positions, records are numbered range after range in the same order.
 *   Result     record r is the ATSC_EXTREMES_BYTES(k) bytes at (char *)out + r * ATSC_EXTREMES_BYTES(k), laid out as the
 *              windowed extremes lay theirs out: an atsc_window_extremes_head, largest[0 .. k), smallest[0 .. k), each
 *              an atsc_extreme.  One k, 1 <= k <= ATSC_EXTREMES_MAX_K, holds for a call.
 *   Record     the windowed extremes' record of the column x_0 .. x_(N-1), x_j = the sample of stream j at the position,
 *              j the stream's place in the call's list: what atsc_extremes_windows gives for a window of those N samples.
 *              count is n_streams, NaN included; nans the number of j with x_j NaN.  largest lists the x_j that are not
 *              NaN by value descending, smallest by value ascending; samples are compared as values (-0.0 equals +0.0,
 *              +-Inf are ordinary values) and among equal values the lowest j comes first.  An entry's value is the
 *              sample's own bits (a -0.0 stays -0.0), its `at` is j.  NaN is never listed; unused entries -- all of them
 *              beyond N when k > N -- hold value = NaN, at = ATSC_EXTREMES_NONE.  One stream may appear in both lists.
 *              No floating-point arithmetic touches a sample: the record is bit-exact, and it depends only on the N
 *              samples of its position, the order of the list and k: not on the range, the stride, the other ranges, the
 *              budget, the piece boundaries, the framing, the codecs or the device.
 *   It follows that
 *              - the first j entries of a call with k are the entries of a call with j < k;
 *              - where atsc_across_windows' count > 0, largest[0] is its max and max_at and smallest[0] its min and
 *                min_at, bit for bit; count - nans is its count;
 *              - atsc_extremes_merge over the records of one position from calls over consecutive sub-lists L_0, L_1, ..
 *                of a list (the same k) is the record of the concatenated list, bit for bit: it shifts every `at` by the
 *                counts in front, which here are the sub-lists' sizes.  A list of more than ATSC_ACROSS_MAX_STREAMS
 *                streams is queried that way;
 *              - under a reordering of the list the listed values stay the same as values, and every `at` maps through
 *                the reordering except among equal values.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_across_windows, k == 0 or
 * k > ATSC_EXTREMES_MAX_K, a result pointer that is not 8-byte aligned.  n_windows == 0 and empty ranges write nothing.
 * Scratch and pieces are the across': there is no ATSC_E_CAPACITY case. */
/* dp / d_body (n_streams entries each) and begin / count are HOST arrays; d_body[j] and d_out are device memory (d_out
 * 8-byte aligned, ATSC_EXTREMES_BYTES(k) bytes per record).  Enqueued on `stream`, not synchronised.  A malformed
 * payload in a frame of stream j that a range touches sets dp[j]'s status word.  dp[0] keeps the call's tables and
 * scratch in the place of the across quantiles': the next across extremes, across moments or across quantile call whose
 * first plan is dp[0] waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_across_extremes_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                     const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                     const uint64_t *count, uint64_t stride, uint32_t k, void *d_out, void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host records out, synchronous; walks and uploads only
 * the touched records of every stream, as atsc_across_windows does, and computes the device call's bits.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_extremes_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                 const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                 uint64_t stride, uint32_t k, void *out);

/* Windowed across moments: count, mean and M2 = sum (x - mean)^2 of the N samples that the streams of a call hold at
 * every position of ranges of the decoded streams -- `avg`, `stdvar` and `stddev by (job)(x)`, how far apart the
 * replicas are at every step -- without the decoded samples leaving the library, and never from a sum of squares: a
 * fleet at 1e9 +- 1e-3 keeps its variance, as a window of the windowed moments does.
 *   Ranges     atsc_across_windows' exactly: one stride for the call, range i has atsc_across_outputs(count[i], stride)
 *              positions, records are numbered range after range in the same order.
 *   Record     x_k = the sample of stream k at the position, k = 0 .. N - 1 in the order of the call's list.  The record
 *              is the x half (n, mx, M2x) of
 *                  Merge(.. Merge(Merge(leaf_0, leaf_1), leaf_2) .., leaf_(N-1))
 *              with Merge the windowed moments' rule (above) and leaf_k = (1, x_k, 0), or the empty node where x_k is
 *              NaN.  For a non-empty accumulator (na, mean, m2) and a non-empty leaf the rule reads
 *                  n = na + 1; w = 1.0 / (double)n; f = (double)na * w; dx = x_k - mean;
 *                  mean = mean + dx * w; m2 = (m2 + 0.0) + (dx * dx) * f
 *              -- every operation one correctly rounded f64 operation, evaluated as written, never fused.  count = n,
 *              nans = N - n; mean and m2 are NaN when count == 0.  +-Inf samples give what IEEE gives under the rule;
 *              where it yields NaN, any NaN conforms.
 *   It follows that
 *              - a record depends only on the N samples of its position and the order of the list: not on the range, the
 *                stride, the other ranges, the budget, the piece boundaries, the framing, the codecs or the device;
 *              - count is atsc_across_windows' count at the same position;
 *              - m2 == 0.0 exactly where count == 1 and on a column of equal values;
 *              - a reordered list gives the same count and nans; its mean and m2 stay within the bounds below but are
 *                not the same bits;
 *              - for finite data, with u = 2^-53, n = count and kappa = sqrt(1 + n mean^2 / m2) as the windowed moments
 *                define it:  |mean - exact| <= (n + 2) u mean|x|;  |m2 - exact| <= (n + 2) u kappa m2.
 *                These are the moments' bounds with L replaced by n: the fold is sequential, not a tree.  A CPU trial of
 *                the fold (N = 1 .. 64, the windowed moments' input families, 20 % and 30 % NaN holes) stayed under
 *                0.55 of both; records of sub-lists of 64 merged (atsc_across_moments_merge) up to N = 400 stayed under
 *                0.07 of both.
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_across_windows and for a
 * result pointer that is not 8-byte aligned.  n_windows == 0 and empty ranges write nothing.  Scratch and pieces are the
 * across': there is no ATSC_E_CAPACITY case. */
typedef struct {
    uint32_t count; /* streams whose sample at this position is not NaN */
    uint32_t nans;  /* streams whose sample is NaN: count + nans == n_streams */
    double mean;    /* of the count samples; NaN when count == 0 */
    double m2;      /* sum (x - mean)^2 over them; NaN when count == 0 */
} atsc_across_moments; /* 24 bytes */
/* dp / d_body (n_streams entries each) and begin / count are HOST arrays; d_body[k] and d_out are device memory (d_out
 * 8-byte aligned, 24 bytes per record).  Enqueued on `stream`, not synchronised.  A malformed payload in a frame of
 * stream k that a range touches sets dp[k]'s status word.  dp[0] keeps the call's tables and scratch in the place of the
 * across quantiles', which the across extremes share: the next across moments, across extremes or across quantile call
 * whose first plan is dp[0] waits (host side) until this one's work is done; atsc_dplan_destroy frees them. */
int atsc_across_moments_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                    const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                    const uint64_t *count, uint64_t stride, atsc_across_moments *d_out, void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host records out, synchronous; walks and uploads only
 * the touched records of every stream, as atsc_across_windows does, and computes the device call's bits.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_moments_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                uint64_t stride, atsc_across_moments *out);
/* The records of ONE position from calls over consecutive sub-lists L_0, L_1, .. of a list, folded from the left by the
 * general Merge (host only, no GPU): out = Merge(.. Merge(Merge(empty, records[0]), records[1]) .., records[n - 1]), a
 * record with count == 0 being the empty node; count and nans are added.  n == 0 gives the empty record (0, 0, NaN,
 * NaN).  A list of more than ATSC_ACROSS_MAX_STREAMS streams is queried that way.  Merging the record of a list L with
 * the records of single-stream calls s_1, s_2, .. gives the record of the list L, s_1, s_2, .. bit for bit (the fold is
 * Merge with leaves); in general the merged record holds the bounds above with n the total count.  ATSC_E_INVALID for a
 * null pointer with n > 0 (out may never be null) or where a total does not fit 32 bits; out is then untouched. */
int atsc_across_moments_merge(const atsc_across_moments *records, uint64_t n, atsc_across_moments *out);
/* What is read off the across moments, host only (no GPU); out[i] from m[i], i < n, by atsc_moments_fit's definitions:
 *   mean; variance = m2 / (double)count, stddev = sqrt(variance) (population forms, PromQL's stdvar and stddev);
 *   sample_variance = m2 / (double)(count - 1), NaN when count < 2; sample_stddev = sqrt(sample_variance).
 * count == 0 gives NaN in all five.  ATSC_E_INVALID for a null pointer with n > 0. */
typedef struct {
    double mean, variance, stddev, sample_variance, sample_stddev;
} atsc_across_fit;
int atsc_across_moments_fit(const atsc_across_moments *m, uint64_t n, atsc_across_fit *out);

/* Windowed histograms: how the samples of windows [begin, begin + count) of the decoded stream (the indices of
 * atsc_decompress_frames) are distributed over value bins, from the same decoded samples as the window decode.  The
 * bins are given by n_edges ascending edges, the same for every window.  For window i:
 *   a row of n_edges + 2 counters at out[i * (n_edges + 2) ..]: bins 0 .. n_edges, then the number of NaN samples;
 *   samples are compared with the edges as values (-0.0 equals +0.0); +-Inf samples are counted like any other value;
 *   LEFT_CLOSED   a non-NaN sample v goes to bin k = the number of edges <= v: bin k holds edges[k-1] <= v < edges[k],
 *                 bin 0 v < edges[0], bin n_edges v >= edges[n_edges-1] (numpy.searchsorted(edges, v, side="right"));
 *   RIGHT_CLOSED  k = the number of edges < v: bin k holds edges[k-1] < v <= edges[k], the reading of Prometheus' `le`
 *                 buckets (side="left").
 * A row's counters always sum to count[i].  The call writes every row whole: the caller does not have to clear the
 * result, and an empty window gives a row of zeros.  The result depends only on the window's samples and the edges,
 * not on the other windows, their order, the budget or the device.  A window may be longer than one piece of the
 * decoded-sample scratch that atsc_ctx_set_aggregate_scratch bounds: counts add across pieces, there is no
 * ATSC_E_CAPACITY case.
 * Validation (ATSC_E_INVALID, nothing written): a null argument, a window beyond the stream, n_edges == 0 or
 * n_edges > ATSC_HIST_MAX_EDGES, an edge that is NaN, edges that are not strictly ascending as values (0.0, -0.0 is
 * not), an unknown `closed`, a result pointer that is not 8-byte aligned.  +-Inf edges are allowed; n_windows == 0 is
 * valid; windows may overlap and come in any order.  The edges, n_edges and `closed` are checked before any GPU work. */
enum { ATSC_HIST_LEFT_CLOSED = 0, ATSC_HIST_RIGHT_CLOSED = 1 };
enum { ATSC_HIST_MAX_EDGES = 1024 };
/* begin / count / edges are HOST arrays; d_body and d_out (n_windows * (n_edges + 2) u64, 8-byte aligned) are device
 * memory.  Enqueued on `stream`, not synchronised.  A malformed payload inside a window sets the plan's status word.
 * The plan keeps the call's tables and scratch: the next histogram call on the same plan waits (host side) until this
 * one's work is done; atsc_dplan_destroy frees them. */
int atsc_histogram_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                               const uint64_t *begin, const uint64_t *count, uint32_t n_edges, const double *edges,
                               int closed, uint64_t *d_out, void *stream);
/* Host bytes in, host rows out (n_windows * (n_edges + 2) u64), synchronous; walks and uploads only the touched
 * records, as atsc_aggregate_windows does.  ATSC_E_FORMAT (nothing written) for a malformed payload inside a window. */
int atsc_histogram_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                           const uint64_t *begin, const uint64_t *count, uint32_t n_edges, const double *edges,
                           int closed, uint64_t *out);
/* The n_bins + 1 edges of n_bins equal bins over [lo, hi], host only (no GPU):
 *   edges[k] = (double)k * ((hi - lo) / (double)n_bins) + lo for k < n_bins (one divide, then one multiply and one add
 *   per edge, not fused), edges[n_bins] = hi: numpy.linspace(lo, hi, n_bins + 1) bit for bit.
 * ATSC_E_INVALID with nothing written: edges == NULL, lo or hi not finite, hi <= lo, n_bins == 0 or
 * n_bins + 1 > ATSC_HIST_MAX_EDGES, a step of 0, or rounded edges that are not strictly ascending (a width of a few
 * ulps of lo).  Unlike numpy.histogram, whose last bin is closed on both sides, a sample equal to hi lands in the
 * overflow bin (bin n_bins + 1 of the row) under ATSC_HIST_LEFT_CLOSED. */
int atsc_histogram_edges_uniform(double lo, double hi, uint32_t n_bins, double *edges);

/* Windowed across histograms: at every position of ranges of the decoded streams, how many of the N streams of a call
 * hold a sample in each value bin -- a fleet heat map (how many of a job's 64 replicas sit in each latency band at every
 * step), `count by (job)(x > 0.9)` (one edge), an SLO's "at least 60 of 64 hosts under 200 ms" (one `le` bucket) --
 * without the decoded samples leaving the library and without one 1-sample window per position and stream.
 *   Ranges     atsc_across_windows' exactly: n_streams in 1 .. ATSC_ACROSS_MAX_STREAMS, one stride for the call, range i
 *              has atsc_across_outputs(count[i], stride) positions, rows are numbered range after range in the across'
 *              record order.  The same plan may appear in the list more than once; all plans belong to one context.
 *   Edges      edges[0 .. n_edges), closed and their validation are atsc_histogram_windows': n_edges in
 *              1 .. ATSC_HIST_MAX_EDGES, strictly ascending as values, no NaN edge, +-Inf allowed; closed is
 *              ATSC_HIST_LEFT_CLOSED or ATSC_HIST_RIGHT_CLOSED.
 *   Result     n_edges + 2 u64 counters per position, in the histograms' layout (bins 0 .. n_edges, then NaN): with
 *              m_i = atsc_across_outputs(count[i], stride), row j of range i is at
 *              out[(m_0 + .. + m_(i-1) + j) * (n_edges + 2)].  positions x (n_edges + 2) must be below 2^32 - 1, so that
 *              a counter's index fits 32 bits.  The caller sizes the result: sum m_i x (n_edges + 2) x 8 bytes.  The
 *              call writes every counter of every row: the caller does not have to clear the result.
 *   Row        The counter of bin b is the number of streams k whose sample at the position has bin b by the histograms'
 *              rule: -0.0 equals +0.0, +-Inf samples are counted like any value, NaN samples are counted apart in the
 *              last counter.  A row's counters sum to n_streams.
 *   A row depends on the N samples of its position, the edges and closed alone: not on the order of the list, the range
 *   that reached the position, the stride, the other ranges, the budget, the piece boundaries, the framing, or which of
 *   the three forms (device, host, stream) was called.  It follows that
 *              - with n_streams == 1 the row is atsc_histogram_windows' row of the window (position, 1), byte for byte;
 *              - for any N the row is the sum over k of those rows of the streams;
 *              - the NaN counter equals n_streams - atsc_across_windows' count at that position;
 *              - the rows of sub-lists add to the row of the whole list: a list of more than ATSC_ACROSS_MAX_STREAMS
 *                streams is queried that way, with plain integer addition (there is no merge function).
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_across_windows, for every
 * case of atsc_histogram_windows' edge checks (null edges, n_edges == 0 or above ATSC_HIST_MAX_EDGES, a NaN edge, edges
 * not strictly ascending, an unknown closed), for positions x (n_edges + 2) >= 2^32 - 1 (the message says so), a result
 * pointer that is not 8-byte aligned.  The messages name across_histogram_windows.  n_windows == 0 and empty ranges
 * write nothing.  Scratch and pieces are the across': there is no ATSC_E_CAPACITY case. */
/* dp / d_body (n_streams entries each), begin / count and edges are HOST arrays; d_body[k] and d_out are device memory
 * (d_out 8-byte aligned, 8 (n_edges + 2) bytes per position).  Enqueued on `stream`, not synchronised.  A malformed
 * payload in a frame of stream k that a range touches sets dp[k]'s status word.  dp[0] keeps the call's tables and scratch
 * in the place of the across quantiles', which the across extremes and moments share: the next across histogram, across
 * moments, across extremes or across quantile call whose first plan is dp[0] waits (host side) until this one's work is
 * done; atsc_dplan_destroy frees them. */
int atsc_across_histogram_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                      const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                      const uint64_t *count, uint64_t stride, uint32_t n_edges, const double *edges,
                                      int closed, uint64_t *d_out, void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host rows out, synchronous; walks and uploads only the
 * touched records of every stream, as atsc_across_windows does, and computes the device call's bytes.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_histogram_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                  const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                  uint64_t stride, uint32_t n_edges, const double *edges, int closed, uint64_t *out);

/* Windowed across value counts: at every position of ranges of the decoded streams, which values the N streams of a call
 * hold there and how many streams hold each, without knowing the values in advance.  This is PromQL's count_values
 * proper, an aggregation across series at one instant: how many replicas report each build_info version at every step,
 * how many members name each leader id, how many hosts are in each breaker state, whether the replicas of a config gauge
 * agree at all.  (atsc_values_windows is the same record over one series in time: "time in each state".)
 *   Ranges     atsc_across_windows' exactly: n_streams in 1 .. ATSC_ACROSS_MAX_STREAMS, one stride for the call, range i
 *              has atsc_across_outputs(count[i], stride) positions, records are numbered range after range in the
 *              across' record order.  The same plan may appear in the list more than once; all plans belong to one
 *              context.
 *   Result     record r is the ATSC_VALUES_BYTES(k) bytes at (char *)out + r * ATSC_VALUES_BYTES(k), in the windowed
 *              value counts' layout: an atsc_window_values_head, then entry[0 .. k) of atsc_value_count.  One k,
 *              1 <= k <= ATSC_VALUES_MAX_K, holds for a call.  The caller sizes the result: sum m_i x
 *              ATSC_VALUES_BYTES(k) bytes.  The call writes every byte of every record: the caller does not have to
 *              clear the result.
 *   Record     atsc_values_windows' rule, unchanged, applied to the column x_0 .. x_(N-1) of the streams' samples at the
 *              position as if it were a window of N samples: count = n_streams, always; nans = the NaN ones; above and
 *              below keep their windowed meaning (above NaN lists every non-NaN sample, else only x > above, and below
 *              counts the non-NaN samples not listed); -0.0 and +0.0 are one class, reported as +0.0; +-Inf are ordinary
 *              values; entries ascending, unused entries (NaN, 0); distinct = min(D, k) and more = (D > k), D the number
 *              of distinct listed values.  D can reach 64 and k only 32: calling again with above set to the last listed
 *              value walks a column exactly, in ceil(D / k) calls.
 * No arithmetic touches a sample, so the record is bit-exact.  It depends on the N samples of its position, k and above
 * alone: not on the order of the list, the range that reached the position, the stride, the other ranges, the budget,
 * the piece boundaries, the framing, the device, or which of the three forms (device, host, stream) was called.  It
 * follows that
 *              - the record equals atsc_values_merge of the N streams' atsc_values_windows records of the window
 *                (position, 1), with the same k and above (with n_streams == 1 it is that record, byte for byte);
 *              - atsc_values_merge over the records of sub-lists gives the whole list's record byte for byte (the merge
 *                already allows parts from different streams): a list of more than ATSC_ACROSS_MAX_STREAMS streams is
 *                queried that way, and there is no new merge function;
 *              - atsc_values_mode applies unchanged: the majority value at every step;
 *              - count - nans equals atsc_across_windows' count at that position;
 *              - with above NaN and a non-NaN sample, entry[0].value equals the across' min as a value;
 *              - the sum of the n of the entries whose value falls in a bin equals that bin of
 *                atsc_across_histogram_windows (more == 0, above NaN).
 * Errors: ATSC_E_INVALID with nothing written and before any GPU work for every case of atsc_across_windows, for k == 0
 * or k > ATSC_VALUES_MAX_K, a result pointer that is not 8-byte aligned.  The messages name across_values_windows.
 * n_windows == 0 and empty ranges write nothing.  Scratch and pieces are the across': there is no ATSC_E_CAPACITY case. */
/* dp / d_body (n_streams entries each), begin / count are HOST arrays; d_body[j] and d_out are device memory (d_out
 * 8-byte aligned, ATSC_VALUES_BYTES(k) bytes per position).  Enqueued on `stream`, not synchronised.  A malformed
 * payload in a frame of stream j that a range touches sets dp[j]'s status word.  dp[0] keeps the call's tables and scratch
 * in the place of the across quantiles', which the across extremes, moments and histograms share: the next across call
 * of any of these five kinds whose first plan is dp[0] waits (host side) until this one's work is done;
 * atsc_dplan_destroy frees them. */
int atsc_across_values_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                   const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                   const uint64_t *count, uint64_t stride, uint32_t k, double above, void *d_out,
                                   void *stream);
/* Host bytes in (n_streams bodies, lengths and has_count flags), host records out, synchronous; walks and uploads only
 * the touched records of every stream, as atsc_across_windows does, and computes the device call's bytes.  ATSC_E_FORMAT
 * (nothing written) for a malformed payload in a frame of any stream that a range touches. */
int atsc_across_values_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                               const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                               uint64_t stride, uint32_t k, double above, void *out);

/* ------------------------------------------------------------------------ */
/* CompressedStream mirror (atsc/src/data.rs:29-110)                          */
/* ------------------------------------------------------------------------ */
/* The reference compresses each chunk when it is added.  Here chunks are copied and queued;
 * the GPU batch runs when the bytes are asked for (atsc_stream_to_bytes) -- observable results are
 * the same, one frame per call in call order. */
int atsc_stream_new(atsc_ctx *ctx, atsc_stream **out);                           /* data.rs:30-35 */
/* data.rs:89-103 ; ATSC_E_FORMAT / ATSC_E_VERSION where the reference panics (header.rs:34-37,72-74) */
int atsc_stream_from_bytes(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, atsc_stream **out);
void atsc_stream_free(atsc_stream *s);
/* data.rs:37-44 : CompressorFrame::new(None) = the default compressor, Noop */
int atsc_stream_compress_chunk(atsc_stream *s, const double *chunk, uint64_t n);
/* data.rs:47-53 ; ATSC_AUTO here is `todo!()` in the reference -> ATSC_E_INVALID */
int atsc_stream_compress_chunk_with(atsc_stream *s, const double *chunk, uint64_t n, int compressor);
/* data.rs:56-76 */
int atsc_stream_compress_chunk_bounded_with(atsc_stream *s, const double *chunk, uint64_t n,
                                            int compressor, float max_error, int compression_speed);
uint64_t atsc_stream_frame_count(const atsc_stream *s);
/* data.rs:79-85 ; *out is malloc'd, release with atsc_free */
int atsc_stream_to_bytes(atsc_stream *s, uint8_t **out, uint64_t *len);
/* data.rs:104-109 ; *out is malloc'd, release with atsc_free */
int atsc_stream_decompress(atsc_stream *s, double **out, uint64_t *n);
/* atsc_stream_decompress of the samples [begin, begin + count) only (atsc_decompress_window); release with atsc_free */
int atsc_stream_decompress_window(atsc_stream *s, uint64_t begin, uint64_t count, double **out, uint64_t *n);
/* atsc_aggregate_windows over the stream's frames */
int atsc_stream_aggregate_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                  atsc_window_stats *out);
/* atsc_delta_windows over the stream's frames */
int atsc_stream_delta_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                              atsc_window_delta *out);
/* atsc_runs_windows over the stream's frames */
int atsc_stream_runs_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count, int op,
                             double limit, atsc_window_runs *out);
/* atsc_extremes_windows over the stream's frames */
int atsc_stream_extremes_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                 uint32_t k, void *out);
/* atsc_values_windows over the stream's frames */
int atsc_stream_values_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                               uint32_t k, double above, void *out);
/* atsc_select_windows over the stream's frames */
int atsc_stream_select_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                               int op, double limit, uint64_t cap, void *out);
/* atsc_rolling_windows over the stream's frames */
int atsc_stream_rolling_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                uint64_t width, uint64_t stride, atsc_window_rolling *out);
/* atsc_rolling_delta_windows over the stream's frames */
int atsc_stream_rolling_delta_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                      uint64_t width, uint64_t stride, atsc_window_delta *out);
/* atsc_rolling_runs_windows over the stream's frames */
int atsc_stream_rolling_runs_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                     uint64_t width, uint64_t stride, int op, double limit, atsc_window_runs *out);
/* atsc_rolling_moments_windows over the stream's frames */
int atsc_stream_rolling_moments_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                        uint64_t width, uint64_t stride, atsc_window_moments *out);
/* atsc_rolling_quantile_windows over the stream's frames */
int atsc_stream_rolling_quantile_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                         uint64_t width, uint64_t stride, uint32_t n_q, const double *q, int method,
                                         double *out);
/* atsc_rolling_histogram_windows over the stream's frames */
int atsc_stream_rolling_histogram_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                          uint64_t width, uint64_t stride, uint32_t n_edges, const double *edges, int closed,
                                          uint64_t *out);
/* atsc_rolling_pair_windows over the frames of two streams of one context (x and y may be the same stream) */
int atsc_stream_rolling_pair_windows(atsc_stream *x, atsc_stream *y, uint64_t n_windows, const uint64_t *begin,
                                     const uint64_t *count, uint64_t width, uint64_t stride, atsc_window_pair *out);
/* atsc_moments_windows over the stream's frames */
int atsc_stream_moments_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                atsc_window_moments *out);
/* atsc_pair_windows over the frames of the streams x and y, which must belong to one context (else ATSC_E_INVALID) */
int atsc_stream_pair_windows(atsc_stream *x, atsc_stream *y, uint64_t n_windows, const uint64_t *begin,
                             const uint64_t *count, atsc_window_pair *out);
/* atsc_pair_matrix_windows over the frames of the n_streams streams of the list, which must belong to one context (else
 * ATSC_E_INVALID); out: n_windows * P records */
int atsc_stream_pair_matrix_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                    const uint64_t *begin, const uint64_t *count, atsc_window_pair *out);
/* atsc_across_windows over the frames of the n_streams streams of the list, which must belong to one context (else
 * ATSC_E_INVALID) */
int atsc_stream_across_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows, const uint64_t *begin,
                               const uint64_t *count, uint64_t stride, atsc_across_record *out);
/* atsc_across_quantile_windows over the frames of the n_streams streams of the list, which must belong to one context
 * (else ATSC_E_INVALID) */
int atsc_stream_across_quantile_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                        const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t n_q,
                                        const double *q, int method, double *out);
/* atsc_across_extremes_windows over the frames of the n_streams streams of the list, which must belong to one context
 * (else ATSC_E_INVALID) */
int atsc_stream_across_extremes_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                        const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t k,
                                        void *out);
/* atsc_across_moments_windows over the frames of the n_streams streams of the list, which must belong to one context
 * (else ATSC_E_INVALID) */
int atsc_stream_across_moments_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                       const uint64_t *begin, const uint64_t *count, uint64_t stride,
                                       atsc_across_moments *out);
/* atsc_across_histogram_windows over the frames of the n_streams streams of the list, which must belong to one context
 * (else ATSC_E_INVALID) */
int atsc_stream_across_histogram_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                         const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t n_edges,
                                         const double *edges, int closed, uint64_t *out);
/* atsc_across_values_windows over the frames of the n_streams streams of the list, which must belong to one context
 * (else ATSC_E_INVALID) */
int atsc_stream_across_values_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                      const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t k,
                                      double above, void *out);
/* atsc_quantile_windows over the stream's frames */
int atsc_stream_quantile_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                 uint32_t n_q, const double *q, int method, double *out);
/* atsc_histogram_windows over the stream's frames */
int atsc_stream_histogram_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                  uint32_t n_edges, const double *edges, int closed, uint64_t *out);
void atsc_free(void *p);

/* compress_data / decompress_data of the atsc CLI (atsc/src/main.rs:130-172): clean (drop NaN/Inf),
 * chunk, compress every chunk with `compressor` (bounded with (float)error_pct/100 for
 * fft/polynomial/idw/auto, unbounded for noop/constant/rle), whole .bro image out. */
int atsc_compress_data(atsc_ctx *ctx, const double *data, uint64_t n, int compressor, uint8_t error_pct,
                       int sample_level, uint8_t **bro, uint64_t *len);
int atsc_decompress_data(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, double **out, uint64_t *n);

/* WBRO files (wavbrro/src/wavbrro.rs:103-132, read.rs:23-37, write.rs:21-27):
 * "WBRO0000WBRO" + rkyv 0.7.44 archive of {sample_count:u32, bitdepth:u8 = 5, chunks:Vec<Vec<f64>>}
 * (chunks of 2048 samples).  Byte-identical to the reference's writer. */
int atsc_wbro_from_bytes(const uint8_t *file, uint64_t len, double **out, uint64_t *n);
int atsc_wbro_to_bytes(const double *data, uint64_t n, uint8_t **out, uint64_t *len);
int atsc_wbro_read(const char *path, double **out, uint64_t *n);
int atsc_wbro_write(const char *path, const double *data, uint64_t n);
/* utils/readers/bro_reader.rs:31-46 : *out = NULL and rc 0 when the file is not a BRO file */
int atsc_bro_read_file(const char *path, uint8_t **out, uint64_t *len);
/* atsc/src/csv.rs:36-98 : value column of a comma separated file.  has_header != 0: both field names
 * must be present, values come from value_field; else column 0.  Values parse as Rust's str::parse::<f64>. */
int atsc_csv_read(const char *path, int has_header, const char *time_field, const char *value_field,
                  double **out, uint64_t *n);

/* ------------------------------------------------------------------------ */
/* host-side format helpers (no GPU needed)                                 */
/* ------------------------------------------------------------------------ */

/* OptimizerPlan::get_chunks_sizes, optimizer/mod.rs:78-98.  Returns the chunk count;
 * writes at most cap sizes. */
uint64_t atsc_chunk_sizes(uint64_t len, uint64_t *out, uint64_t cap);
/* OptimizerPlan::clean_data, optimizer/mod.rs:64-71 (drops NaN and +-Inf). Returns kept count. */
uint64_t atsc_clean_data(const double *in, uint64_t n, double *out);
/* utils::next_size, utils/mod.rs:32-38 */
uint64_t atsc_next_size(uint64_t n);
/* CompressorHeader::to_bytes + frame count varint (header.rs:60-67, data.rs:83):
 * writes "BRRO" u32le(1) u8(n_frames mod 256) varint(n_frames) into out (>= 18 bytes);
 * returns bytes written. */
uint64_t atsc_bro_prefix(uint64_t n_frames, uint8_t *out);
/* CompressedStream::from_bytes front half (data.rs:89-97, header.rs:69-84): validates magic
 * and version; returns the offset of the first frame record (after the count varint) and
 * the frame count, or ATSC_E_FORMAT / ATSC_E_VERSION. */
int atsc_bro_open(const uint8_t *bro, uint64_t len, uint64_t *body_off, uint64_t *n_frames);
/* CompressedStream::from_bytes as a dry run (data.rs:89-103): header, version, frame count and the
 * walk over every frame record (frame/mod.rs:25-33) without decoding a payload.  ATSC_E_FORMAT where
 * the reference's bincode decode `.unwrap()` panics (data.rs:98): a truncated or inflated length, a
 * count the bytes cannot hold, an unknown compressor id.  Outputs may be NULL. */
int atsc_bro_scan(const uint8_t *bro, uint64_t len, uint64_t *n_frames, uint64_t *n_samples);

/* ------------------------------------------------------------------------------------------
 * csv-compressor front end: host-only, no GPU context needed.
 * ------------------------------------------------------------------------------------------ */
/* VSRI, the timestamp index (vsri/src/lib.rs): continuous segments y = m*x + b of equally spaced
 * points, [m, x0, y0, count] each (lib.rs:100-106).  Arithmetic is Rust's release-mode i32
 * (wrapping).  Look-ups return 1 = Some(*out), 0 = None, ATSC_E_INVALID where the reference
 * panics (division by zero on a one-point segment, lib.rs:311). */
typedef struct atsc_vsri atsc_vsri;
atsc_vsri *atsc_vsri_new(void);                                      /* Vsri::new, lib.rs:110-119 */
void atsc_vsri_free(atsc_vsri *v);
int atsc_vsri_load(const char *path, atsc_vsri **out);               /* Vsri::load, lib.rs:447-486 */
int atsc_vsri_flush_to(const atsc_vsri *v, const char *path);        /* Vsri::flush_to, lib.rs:424-443 */
/* Vsri::update_for_point (lib.rs:236-273); ATSC_E_INVALID = Error::UpdateIndexForPointError */
int atsc_vsri_update_for_point(atsc_vsri *v, int32_t y);
int32_t atsc_vsri_min(const atsc_vsri *v);                           /* lib.rs:276-278 */
int32_t atsc_vsri_max(const atsc_vsri *v);                           /* lib.rs:281-283 */
uint64_t atsc_vsri_segment_count(const atsc_vsri *v);
int atsc_vsri_segment(const atsc_vsri *v, uint64_t i, int32_t out[4]);
int32_t atsc_vsri_get_sample_count(const atsc_vsri *v);              /* lib.rs:355-358 */
int atsc_vsri_get_sample(const atsc_vsri *v, int32_t y, int32_t *out);           /* lib.rs:301-317 */
int atsc_vsri_get_next_sample(const atsc_vsri *v, int32_t y, int32_t *out);      /* lib.rs:154-169 */
int atsc_vsri_get_previous_sample(const atsc_vsri *v, int32_t y, int32_t *out);  /* lib.rs:175-193 */
int atsc_vsri_get_this_or_next(const atsc_vsri *v, int32_t y, int32_t *out);     /* lib.rs:137-141 */
int atsc_vsri_get_this_or_previous(const atsc_vsri *v, int32_t y, int32_t *out); /* lib.rs:144-148 */
int atsc_vsri_get_time(const atsc_vsri *v, int32_t x, int32_t *out);             /* lib.rs:320-341 */
int atsc_vsri_is_empty(const atsc_vsri *v, int32_t t0, int32_t t1);  /* lib.rs:198-232; 1 / 0 */
int atsc_vsri_get_all_timestamps(const atsc_vsri *v, int32_t **out, uint64_t *n); /* lib.rs:344-353; atsc_free */
/* The samples whose indexed times (get_time, lib.rs:320-341) lie in [t0, t1], as a window for atsc_decompress_window:
 * begin = get_this_or_next(t0), last = get_this_or_previous(t1) (lib.rs:137-148), each end then moved inwards past
 * samples whose time falls outside [t0, t1] (an off-grid time looks up the sample in front of it).  *count = 0 when
 * no sample falls inside.  ATSC_E_INVALID where a look-up panics in the reference. */
int atsc_vsri_sample_window(const atsc_vsri *v, int32_t t0, int32_t t1, uint64_t *begin, uint64_t *count);
/* Time buckets [t0 + k*step, min(t0 + (k+1)*step - 1, t1)], k = 0.., as sample windows: atsc_vsri_sample_window of
 * each bucket (an empty bucket gives count 0).  Host only.  *n = number of buckets (0 when t1 < t0); ATSC_E_CAPACITY
 * when cap < *n (nothing written); ATSC_E_INVALID for step < 1, or where a look-up panics in the reference.
 * t0 + k*step is computed without int32 overflow. */
int atsc_vsri_step_windows(const atsc_vsri *v, int32_t t0, int32_t t1, int32_t step, uint64_t *begin,
                           uint64_t *count, uint64_t cap, uint64_t *n);
/* vsri::day_elapsed_seconds (lib.rs:49-57); ATSC_E_INVALID outside chrono's DateTime range */
int atsc_day_elapsed_seconds(int64_t timestamp_sec, int32_t *out);
/* csv-compressor/src/csv.rs:41-56: `timestamp,value` files (i64, f64; csv crate reader / writer,
 * ryu float formatting).  Arrays from the reader are released with atsc_free. */
int atsc_samples_csv_read(const char *path, int64_t **ts, double **val, uint64_t *n);
int atsc_samples_csv_write(const char *path, const int64_t *ts, const double *val, uint64_t n);
/* Metric::append_samples (metric.rs:53-65), index side: ts_ms[i] / 1000 -> seconds since midnight
 * -> update_for_point.  On failure *failed_at (may be NULL) is the offending sample. */
int atsc_metric_index_samples(atsc_vsri *index, const int64_t *ts_ms, uint64_t n, uint64_t *failed_at);
/* Metric::get_samples (metric.rs:83-97): out[i] = index.get_time(i); ATSC_E_INVALID where that is
 * None (an unwrap panic in the reference). */
int atsc_metric_sample_times(const atsc_vsri *index, uint64_t n, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif
