// Internal structures shared by the host glue and the HIP kernels.
#pragma once
#include <stdint.h>
#include <new>
#include <stdexcept>
#include <vector>

namespace atsc {

// One entry per distinct frame length in a plan.  Everything the kernels need that
// depends only on n (reference: fft.rs:298-311, utils/mod.rs:32-49, polynomial.rs:220-224).
struct DevPlan {
    uint32_t n;        // samples in the frame
    uint32_t L;        // transform length: next_size(n) if n >= 128 else n  (fft.rs:305-311)
    uint32_t pre;      // Gibbs prefix padding (fft.rs:187-190)
    uint32_t bins;     // L/2 + 1 (fft.rs:327)
    uint32_t mf;       // max(3, n/100) (fft.rs:298-302)
    uint32_t dk1;      // max(mf/2, 1)  (fft.rs:349)
    uint32_t dk2;      // max(mf/10, 1) (fft.rs:350)
    uint32_t kcap;     // min(bins, mf + 17*dk1 + 5*dk2): most bins the ladder can ever store
    uint32_t direct;   // 1: O(n^2) DFT (n < 128, any n incl. primes); 0: Stockham 2^a 3^b
    uint32_t half;     // 1: L even -> one complex FFT of length M = L/2 over the packed real signal
    uint32_t M;        // FFT length actually run through the Stockham stages (L or L/2)
    uint32_t sc;       // L / M: index scale into the length-L twiddle table
    uint32_t nstages;
    uint32_t radix[14];
    uint32_t stmagic[14];  // floor(2^32 / stride_s) + 1 for t / stride_s (stride_s = product of earlier radices)
    uint32_t p2bins;   // power of two >= bins (sort network size)
    uint32_t p2n;      // power of two >= n
    uint32_t magicL;   // floor(2^32 / L) + 1 (L >= 2): x mod L without a divide
    uint32_t f4_m1, f4_m2;  // M = f4_m1 * f4_m2, f4_m1 <= f4_m2 as close as the factors allow (0: no usable
                            // split): the large tier's LDS-tiled two-pass transform
    uint32_t sp_mf, sp_md;  // M = sp_mf * sp_md, sp_mf the largest divisor <= 992 (0: none): the large
                            // tier's inverse transform from the sparse list of admitted bins -- a direct
                            // sum over sp_md, then LDS transforms of length sp_mf (atsc_large.hip)
    uint32_t lds_bytes;
    // LDS carve offsets (bytes, 16-aligned).  AB = two FFT work buffers of ab_half bytes each,
    // later reused for spline tables, RLE run records and the RLE hash table.
    uint32_t o_xs, o_tw, o_ab, ab_half, ab_bytes, o_sel, o_aux, o_red, o_hist;
    uint64_t tw_off;   // offset (in float2 entries) of this L's table in the twiddle pool
    // The polynomial ladder of a frame of n samples (polynomial.rs:209-277) visits the same
    // (points, step, K) sequence whatever the data: points = base + jump, jump += n/10 (trips 1..17)
    // or n/100 (18..22).  Everything a trip derives from (n, step) is tabulated once per length.
    double inv_n;         // 1.0 / n
    double pry[23];       // 1.0 / step
    double pryL[23];      // 1.0 / gap of the last segment
    uint32_t pstep[23];   // max(n / points, 1)
    uint32_t pK[23];      // number of stored points: ceil(n / step) (+1 when the last sample is not a knot)
    uint32_t pmagic[23];  // floor(2^32 / step) + 1 (step >= 2): i / step without a divide
    uint32_t pgap[23];    // (n - 1) - (K - 2) * step: length of the last segment
};

// LDS carve-up of one compressor frame (bytes).  One definition for the host (DevPlan::o_*) and for
// the kernel instantiations that know the frame length at compile time.  Nothing is kept that two
// phases can share -- the footprint bounds the frames in flight per CU (160 KB / total):
//   red  reduction scratch (one-wavefront classes reduce through DPP: 16 B for the scan total)
//   xs   the frame, f64[n]
//   tw   twiddles float2[L] from the forward FFT to the end of its ladder; otherwise the RLE group
//        table u32[n] and, above it, aux u32[n + 2]
//   ab   two FFT work buffers of ab_half bytes (8 B per complex point, +8 so the second one can hold
//        M + 1 bins); later spline tables, RLE run records (>= 8n + 64 bytes) and the RLE hash table
//   sel  admitted bins, 12 B each
//   hist multi-wavefront classes only: 256 digit counters + 4 words for the radix select that picks
//        the kcap bins the ladder can ever admit before they are sorted
struct EncLds {
    uint32_t o_red, o_xs, o_tw, o_aux, o_ab, ab_half, ab_bytes, o_sel, o_hist, total;
};
#if defined(__HIPCC__)
#define ATSC_HD __host__ __device__
#else
#define ATSC_HD
#endif
ATSC_HD constexpr uint32_t enc_align16(uint32_t v) { return (v + 15u) & ~15u; }
ATSC_HD constexpr uint32_t enc_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
ATSC_HD constexpr EncLds enc_lds(uint32_t n, uint32_t L, uint32_t fft_points /* bins if direct, else M */,
                                 bool direct, uint32_t kcap, bool one_wave)
{
    EncLds e{};
    e.ab_half = enc_align16(direct ? 8 * fft_points : 8 * fft_points + 8);
    e.ab_bytes = enc_max(2 * e.ab_half, enc_align16(8 * n + 64));
    uint32_t o = 0;
    e.o_red = o; o += one_wave ? 16 : 384;
    e.o_xs = o; o += enc_align16(8 * n);
    e.o_tw = o; o += enc_align16(enc_max(8 * L, 4 * n + 4 * (n + 2)));
    e.o_aux = e.o_tw + 4 * n;
    e.o_ab = o; o += e.ab_bytes;
    e.o_sel = o; o += enc_align16(12 * enc_max(kcap, 1u));
    e.o_hist = o; o += one_wave ? 0 : 1040;
    e.total = o;
    return e;
}

struct DevFrame {
    uint64_t sample_off;
    uint64_t slot_off;  // byte offset of the frame's payload slot in the scratch arena
    uint32_t n;
    uint32_t plan;
};

struct DevResult {
    double err;
    uint32_t len;     // payload bytes in the slot
    uint32_t chosen;  // compressor wire id
};

struct KParams {
    double max_err;      // (double)(float) max_error
    double poly_target;  // round_f64(max_err, 3)  (polynomial.rs:230)
    double poly_q_hi;    // largest integer q with q / 10000.0 <= poly_target:  target < round(err,4)  <=>  round(err*1e4) > q_hi
    double poly_q_lo;    // smallest integer q with q / 10000.0 >= poly_target: target > round(err,4)  <=>  round(err*1e4) < q_lo
    int32_t max_err_m;   // (max_err * 1000.0) as i32  (fft.rs:334)
    int32_t mode;        // ATSC_* compressor id
    int32_t bounded;
    int32_t want_diag;
    int32_t debug_stop;  // profiling aid: leave the kernel after phase N (0 = run everything)
    // sample-level selection (frame/mod.rs:89-111)
    int32_t trial;               // 1: this launch is the trial on the frame prefixes: no Constant
                                 //    shortcut, no payload emission, only res[].chosen matters
    uint32_t trial_min_n;        // COMPRESSION_SPEED[level]; frames at least this long use the trial's codec
    const DevResult *trial_res;  // results of the trial launch (indexed like the frames), or null
    uint32_t *cost;              // per frame: shader clocks / 64 this launch took (scheduling hint), or null
    uint32_t large_tiled;        // large tier: in-kernel transforms take the LDS-tiled two-pass form
    uint32_t sparse_inv;         // large tier: per-trip inverse transform from the sparse bin list
    uint32_t prestats;           // large tier, split run: the statistics (LargeStats) and the chunk sums of the first
                                 // polynomial trip are in the frame's workspace slot (k_large_stats, k_large_poly1)
    uint32_t tile_stats;         // large tier, fast path: the frame statistics are the column tiles' records (TileStats)
    uint32_t fast_skip;          // large tier: k_compress_large<0> runs behind the fast path and skips the frames that
                                 // path finished (FastState::status == 2)
    uint32_t prefft;             // large tier: forward transform, untangle and norms were done by the
                                 // batched pre-pass kernels (spectrum, norm bits and non-zero count are
                                 // in the frame's workspace slot)
};
// grid extents of the large tier's pre-pass over a plan's large frames (0 tiles: no pre-pass)
struct LargePre {
    uint32_t tiles1, tiles2, chunks;  // max over frame lengths: column tiles, row tiles, 256-bin chunks
    uint32_t m1_max, m2_max;          // longest sub-transforms: size the tile buffers in LDS
    uint32_t sp_tiles;                // most tiles (8 output columns each) the sparse inverse of a frame has
    uint32_t chunks_n;                // most 4096-sample chunks a frame has (k_large_stats, k_large_poly1)
    uint32_t cols243;                 // 1: every large frame length splits as M = 243 x M2 (k_large_cols243)
    uint32_t rows9p;                  // when every large frame length has M = 243 x 9 P, P = 2 .. 32 a power of two: the
                                      // P values present, as a bit mask (k_large_rows9p<P>); else 0
    uint32_t even_off;                // 1: every large frame starts on an even sample (16-byte pairs, given an aligned base)
};
constexpr uint32_t LARGE_SPLIT_MAX = 128;  // large frames per launch up to which the first FFT trip's tiles
                                           // run as a (tile, frame) grid (launch_compress_large)

// Uniform launch: every frame of the class has the same length and frame f of the class sits at
// sample_off0 + f*n with its slot at slot_off0 + f*slot_stride; the frame descriptor is then
// computed instead of being loaded through ids[] -> frames[] (two dependent loads per workgroup).
struct UniArgs {
    uint32_t enabled;
    uint32_t adaptive;  // the class is walked in the order of ids[] (costliest frames first)
    uint32_t fid0;
    uint64_t sample_off0;
    uint64_t slot_off0;
    uint64_t slot_stride;
    uint32_t n;
    uint32_t plan;
    uint32_t spread, count;  // spread != 0: workgroup b takes frame (b * spread) % count of the class (spread coprime to count)
    uint64_t spread_m;       // 2^64 / count + 1: (b * spread) % count by two multiplies while b * spread < 2^32 (spread_mod)
    uint64_t tw_off;         // the plan's DevPlan::tw_off: a frame asks for its twiddles before it has read the plan table
};
// x % d for x < 2^32 and 1 <= d < 2^32 from m = 2^64 / d + 1 (Lemire, Kaser, Kurz: "Faster remainder by direct
// computation", 2019: exact for all 32-bit x and d): the low 64 bits of m * x are the fraction x / d, times d is the rest.
ATSC_HD constexpr uint64_t spread_magic(uint32_t d) { return d > 1 ? ~0ull / d + 1ull : 0ull; }
ATSC_HD constexpr uint32_t spread_mod(uint32_t x, uint64_t m, uint32_t d)
{
    const uint64_t frac = m * x;  // (mod 2^64)
    const uint64_t lo = (frac & 0xffffffffull) * d, hi = (frac >> 32) * d + (lo >> 32);  // (frac * d) >> 64, d < 2^32
    return (uint32_t)(hi >> 32);
}

// parsed frame record for decompression
struct DevDFrame {
    uint64_t payload_off;  // byte offset of the payload in the body
    uint64_t out_off;      // sample offset in the output
    uint32_t payload_len;
    uint32_t n;            // sample_count
    uint32_t tag;          // compressor id
    uint32_t plan;         // index into DevPlan table (by n)
};

// window decode (atsc_decompress_windows_dev): samples [lo, hi) of frame `frame` land at out[dst + j - lo]
// (k_decompress<W, SPL, true>); dst is counted in doubles from the call's d_out, modulo 2^64
struct DevWTask {
    uint64_t dst;
    uint32_t frame;  // index into the plan's DevDFrame table
    uint32_t lo, hi;
    uint32_t pad;
};
// one copy of k_window_gather: len samples from scratch[src] to out[dst]
struct DevWGather {
    uint64_t src, dst;
    uint32_t len, pad;
};

// windowed aggregates (atsc_aggregate_windows_dev, atsc_aggregate.hip): tiles of AGG_TILE samples at multiples of
// AGG_TILE in the stream index
constexpr uint32_t AGG_TILE = 2048;
// the partial of a tile or of a group of tiles: NaN-free sum / min / max / count (min = +inf, max = -inf when count == 0)
struct DevAggPart {
    double sum, mn, mx;
    uint64_t count;
};
enum : uint32_t { AGG_FIRST = 1, AGG_LAST = 2 };
// one tile of k_agg_tiles: slots [lo, hi) of the tile whose slot 0 is scratch[src] -> part[dst]; AGG_FIRST / AGG_LAST:
// also fl[2 win] = slot lo / fl[2 win + 1] = slot hi - 1
struct DevAggTile {
    uint64_t src, dst;
    uint32_t lo, hi;
    uint32_t win, flags;
};
// one group of k_agg_combine: entries j in [64 g, min(64 g + 64, n)) of a window's partial list (entry 0 at part[head],
// entry n - 1 at part[tail], entry j else at part[mid + j]) -> part[dst], or (final_) -> the stats record of window dst
struct DevAggComb {
    uint64_t head, tail, mid, dst;
    uint32_t n, g, win, final_;
};

// windowed moments (atsc_moments_windows_dev, atsc_moments.hip): the aggregates' tiles, pieces and combine passes
// (DevAggComb) over nodes of the centred moments of value and position
// the partial of a tile or of a group of tiles: the node (n, mx, M2x, mt, M2t, C) of include/atsc_hip.h
struct DevMomPart {
    double mx, m2x, mt, m2t, c;
    uint64_t n;
};
// one tile of k_mom_tiles, k_run_tiles and k_ext_tiles: slots [lo, hi) of the tile whose slot 0 is scratch[src] and
// sample t0 of the stream -> part[dst] (extremes: partial dst)
struct DevPosTile {
    uint64_t src, dst, t0;
    uint32_t lo, hi;
};

// windowed deltas (atsc_delta_windows_dev, atsc_delta.hip): the aggregates' tiles, pieces and combine passes
// (DevAggComb) over the pairs of stream-adjacent samples
// the partial of a tile or of a group of tiles: the three sums (-0.0 without a term), the largest rise and fall (+0.0
// without one) and the counts of include/atsc_hip.h
struct DevDltPart {
    double up, down, after_falls, max_rise, max_fall;
    uint64_t pairs, rises, falls;
};
// DLT_CONT: the window continues from the slot in front of the tile, so the pair at slot lo (== 0) is the window's;
// DLT_CARRY: that slot lies in the previous piece of the scratch, and its sample in the call's carry slot
enum : uint32_t { DLT_CONT = 1, DLT_CARRY = 2 };
// one tile of k_dlt_tiles: the pairs at the slots of [lo, hi) of the tile whose slot 0 is scratch[src] -> part[dst]
struct DevDltTile {
    uint64_t src, dst;
    uint32_t lo, hi;
    uint32_t flags, pad;
};

// windowed runs (atsc_runs_windows_dev, atsc_runs.hip): the aggregates' tiles, pieces and combine passes (DevAggComb)
// over the nodes of include/atsc_hip.h's merge rule
// the partial of a tile or of a group of tiles: the nine integers of its stretch of the window, the three positions as
// stream indices (~0 where the record has ATSC_RUNS_NONE), and the sum of the inside samples' terms (-0.0 without one)
struct DevRunPart {
    uint64_t samples, inside, runs, longest, longest_at, first_at, last_at, head, tail;
    double excess;
};

// windowed extremes (atsc_extremes_windows_dev, atsc_extremes.hip): the aggregates' tiles, pieces and combine passes
// (DevAggComb) over partials of 2 + 4 k eight-byte words, the record's layout with positions as stream indices: count,
// nans, k largest entries, k smallest entries, an entry being (value bits, position) and (NaN, ~0) where there is none
constexpr uint32_t EXT_MAX_K = 16;

// windowed quantiles (atsc_quantile_windows_dev, atsc_quantile.hip).  The tier of a window is chosen from its length:
// short (one wavefront, keys in registers), medium (one workgroup, keys in LDS), long (MSD radix select, 8-bit digits)
constexpr uint32_t QNT_MAX_LEVELS = 64;
constexpr uint32_t QNT_SLOTS = 2 * QNT_MAX_LEVELS;  // long tier: the ranks a window needs, two per level
constexpr uint64_t QNT_SHORT_MAX = 256;
constexpr uint64_t QNT_MEDIUM_MAX = 8192;
constexpr uint32_t QNT_CHUNK = 16384;  // long tier: samples per histogram workgroup
constexpr uint32_t QNT_PASSES = 8;
// one window: samples scratch[src, src + n) -> out[win * n_q ..]; slot: its long-tier state
struct DevQTask {
    uint64_t src, n;
    uint32_t win, slot;
};
// one histogram workgroup of the long tier: samples scratch[src, src + len) of the window in state `slot`
struct DevQChunk {
    uint64_t src;
    uint32_t len, slot;
};
// the radix select's state of one long window: n non-NaN samples; rank slot r (2 j: level j's lower rank, 2 j + 1: its
// upper one) is rank[r] among the samples whose key starts with prefix upre[ridx[r]]; upre[0, nu) ascending and distinct
struct DevQState {
    uint64_t n;
    uint32_t nr, nu;
    uint64_t rank[QNT_SLOTS];
    uint64_t upre[QNT_SLOTS];
    uint32_t ridx[QNT_SLOTS];
};

// windowed histograms (atsc_histogram_windows_dev, atsc_histogram.hip).  The tier of a task is chosen from its length:
// short (one wavefront), chunk (one workgroup; a longer stretch of a window is cut into tasks of HST_CHUNK samples)
constexpr uint32_t HST_MAX_EDGES = 1024;     // ATSC_HIST_MAX_EDGES: 8 KiB of edges in LDS
constexpr uint32_t HST_SHORT_MAX = 256;
constexpr uint32_t HST_CHUNK = 16384;        // samples per workgroup, as QNT_CHUNK
constexpr uint32_t HST_SHORT_GRID = 2048;    // the most workgroups of k_hst_short: they walk the task list in strides
constexpr uint32_t HST_OWN = 0x80000000u;    // in DevHistTask::len: the window's only task, which stores the row whole
// one task: samples scratch[src, src + (len & ~HST_OWN)) counted into row `win` of the result
struct DevHistTask {
    uint64_t src;
    uint32_t len, win;
};

// windowed select (atsc_select_windows_dev, atsc_select.hip): count, scan, ordered write.  A non-empty window is cut into
// tasks of at most SEL_TASK consecutive samples of one piece of the scratch; a task's slot is its place in (window,
// position) order, whatever piece it lies in, so the scanned counts lie in result order.
constexpr uint32_t SEL_TASK = 2048;        // samples per task: one wavefront, 16 load steps of 128 slots
constexpr uint32_t SEL_SCAN_BLOCK = 2048;  // counts per workgroup of the scan: 256 threads, eight each
// one task: samples scratch[src, src + len), the first of them `at` samples behind its window's begin -> cnt[slot], and
// the entries from pre[slot] on
struct DevSelTask {
    uint64_t src, at;
    uint32_t len, slot;
};
// words of block sums above the first level of a scan over m values: one per block of each level that has several
static inline uint64_t sel_scan_sums(uint64_t m)
{
    uint64_t words = 0;
    while (m > SEL_SCAN_BLOCK) {
        m = (m + SEL_SCAN_BLOCK - 1) / SEL_SCAN_BLOCK;
        words += m;
    }
    return words;
}

// windowed rolling (atsc_rolling_windows_dev, atsc_rolling.hip): a pyramid of the partials of the aligned chunks
// [j 2^l, (j + 1) 2^l) of the stream index over one piece of the scratch, then one record per position from its window's
// canonical chunks.  Levels below ROLL_LOW are not stored: the position kernel forms those chunks from the samples.
constexpr uint32_t ROLL_TILE_LOG = 11, ROLL_TILE = 1u << ROLL_TILE_LOG;  // samples per workgroup of the pyramid kernel
constexpr uint32_t ROLL_LOW = 3;                                        // the lowest stored level
constexpr uint32_t ROLL_MAX_LEVEL = 20;                                 // log2 ATSC_ROLLING_MAX_WIDTH
constexpr uint32_t ROLL_TASK = 256;                                     // positions per task: one wavefront, four steps
// one piece: scratch[0] is sample a0 of the stream (a multiple of ROLL_TILE), the region ends in front of sample a1 (one
// too); the chunk j of level l lies at pyr[off[l] + j - (a0 >> l)] for a0 >> l <= j <= (a1 - 1) >> l, in the call's partials
// (a chunk that sticks out of [a0, a1) has a place and no value)
struct DevRollPiece {
    uint64_t a0, a1;
    uint64_t off[ROLL_MAX_LEVEL + 1];
};
// one task: n positions of one range, the first one's window beginning at sample lo of the stream, the others' every
// `stride` samples behind it; their records from out[rec] on
struct DevRollTask {
    uint64_t lo, rec;
    uint32_t n, pad;
};

// windowed rolling deltas (atsc_rolling_delta_windows_dev, atsc_rolling_delta.hip): the rolling's pieces, tasks and
// pyramid over the pair slots of the stream, slot j holding the deltas' terms of the pair (x[j - 1], x[j]); a window's
// chunks are those of [lo + 1, lo + w), and the highest level floor(log2(w - 1))
constexpr uint32_t ROLL_DELTA_LOW = 3;    // the lowest stored level
constexpr uint32_t ROLL_DELTA_PART = 48;  // bytes of a partial: three sums, two maxima, the three counts in one word

// windowed rolling moments (atsc_rolling_moments_windows_dev, atsc_rolling_moments.hip): the rolling's pieces, tasks,
// pyramid and chunks over nodes of the centred moments of value and position (DevMomPart's fields), the position being
// the stream index; the highest level is floor(log2 w)
constexpr uint32_t ROLL_MOMENTS_LOW = 3;    // the lowest stored level
constexpr uint32_t ROLL_MOMENTS_PART = 48;  // bytes of a partial: the node's five doubles, the count in a 64-bit word

// windowed rolling runs (atsc_rolling_runs_windows_dev, atsc_rolling_runs.hip): the rolling's pieces, tasks, pyramid and
// chunks over the runs' nodes (DevRunPart's merge rule), positions counted from the chunk's first sample; the condition
// is an argument of the pyramid and the position kernels; the highest level is floor(log2 w)
constexpr uint32_t ROLL_RUNS_LOW = 3;    // the lowest stored level
constexpr uint32_t ROLL_RUNS_PART = 32;  // bytes of a partial: five 21-bit and three 20-bit fields in three words, the f64 excess

// windowed rolling quantiles (atsc_rolling_quantile_windows_dev,atsc_rolling_quantile.hip): the rolling's pieces and
// tasks without a pyramid.  A task's windows cover a span of (n - 1) stride + w samples, which one workgroup sorts in
// P slots of LDS and reads every position's levels off.  P by the width alone: the least power of two in
// [RQ_SPAN_MIN, RQ_SPAN_MAX] that holds two windows, RQ_SPAN_MAX above that; a task holds (P - w) / stride + 1 positions.
constexpr uint32_t RQ_SPAN_MIN = 512, RQ_SPAN_MAX = 8192;  // RQ_SPAN_MAX: ATSC_ROLLING_QUANTILE_MAX_WIDTH, QNT_MEDIUM_MAX
static inline uint32_t rq_span_keys(uint64_t w)
{
    uint32_t P = RQ_SPAN_MIN;
    while (P < RQ_SPAN_MAX && P < 2 * w) P <<= 1;
    return P;
}

// windowed rolling histograms (atsc_rolling_histogram_windows_dev, atsc_rolling_histogram.hip): the rolling's pieces and
// tasks without a pyramid.  One wavefront counts a task's first window and slides the row over the task's other
// positions.  B, the positions a task holds, by the width and the stride alone: eight windows' worth of positions, so
// that the first window's count is at most a sixteenth of the slide's 2 (B - 1) stride sample visits, at least
// RH_TASK_MIN (short windows still fill a task) and at most RH_TASK_MAX (a long task is one wavefront's serial work).
constexpr uint64_t RH_TASK_MIN = 64, RH_TASK_MAX = 2048;
static inline uint64_t rh_task_positions(uint64_t w, uint64_t s)
{
    const uint64_t per = w / s + (w % s ? 1 : 0);  // ceil(w / s); w <= 2^20
    const uint64_t b = 8 * per;
    return b < RH_TASK_MIN ? RH_TASK_MIN : b > RH_TASK_MAX ? RH_TASK_MAX : b;
}

// windowed across (atsc_across_windows_dev, atsc_across.hip): every stream of a call decoded into a scratch region of
// its own, the same sample at the same slot of every region, then one record per position from its slot of each.  A
// task is a DevRollTask: n positions of one range inside one piece, the first at sample lo of the streams.
constexpr uint32_t ACR_TASK = 512;  // positions per task: one wavefront, four steps of 64 pairs at stride 1

// windowed across histograms (atsc_across_histogram_windows_dev, atsc_across_histogram.hip): a wavefront counts the rows
// of G positions at a time in byte counters in LDS (a count cannot pass ATSC_ACROSS_MAX_STREAMS = 64).  A row's pitch is
// an odd number of 4-byte words, so that lanes that land in one bin of neighbouring rows meet different banks; G is what
// fits a wavefront's share of LDS, at most a lane per row:
//   words(n_edges) = ceil((n_edges + 2) / 4) | 1,  pitch = 4 words bytes,  G = min(64, floor(AH_WAVE_LDS / pitch)).
// G is 64 up to n_edges = 218, 62 at 219 and 13 at 1024; with the edges a workgroup of four wavefronts holds
// 8 n_edges + 4 G pitch <= 8192 + 4 x 14336 = 65536 bytes.
constexpr uint32_t AH_WAVE_LDS = 14336;
static inline uint32_t ah_row_pitch(uint32_t n_edges) { return 4u * (((n_edges + 2u + 3u) / 4u) | 1u); }
static inline uint32_t ah_rows_a_pass(uint32_t n_edges)
{
    const uint32_t g = AH_WAVE_LDS / ah_row_pitch(n_edges);
    return g < 64u ? g : 64u;
}

static inline uint32_t varint_len_u64(uint64_t v)
{
    return v < 251 ? 1u : v < (1ull << 16) ? 3u : v < (1ull << 32) ? 5u : 9u;
}

// No C++ exception may cross the C ABI (std::bad_alloc / std::length_error out of a container sized from
// untrusted bytes would otherwise end the host process): every extern "C" body that can allocate sits
// between these two.
#define ATSC_API_BEGIN try {
#define ATSC_API_END \
    } catch (const std::bad_alloc &) { return ATSC_E_NOMEM; } \
    catch (const std::length_error &) { return ATSC_E_NOMEM; } \
    catch (...) { return ATSC_E_INVALID; }
// One encoded frame record as it lies in a BRO body (frame/mod.rs:25-33):
// varint(frame_size) varint(sample_count) varint(compressor) varint(len) payload[len].
struct HostRecord {
    uint64_t start;        // offset of the record's first byte
    uint64_t payload_off;  // offset of the payload
    uint64_t payload_len;  // <= UINT32_MAX, and the payload lies inside the body
    uint64_t sample_count;
    uint64_t tag;
};
// bincode varint; false on a truncated field or a marker byte above 253.  `pos` only
// ever moves forward and stays <= len.
static inline bool host_varint(const uint8_t *b, uint64_t len, uint64_t &pos, uint64_t &v)
{
    if (pos >= len) return false;
    const uint8_t t = b[pos];
    uint32_t nb;
    if (t < 251) { v = t; pos += 1; return true; }
    if (t == 251) nb = 2;
    else if (t == 252) nb = 4;
    else if (t == 253) nb = 8;
    else return false;
    if (len - pos < 1ull + nb) return false;
    v = 0;
    for (uint32_t i = 0; i < nb; ++i) v |= (uint64_t)b[pos + 1 + i] << (8 * i);
    pos += 1 + nb;
    return true;
}
// Reads the record at `pos` of untrusted bytes and moves `pos` behind it.  Every bound is checked in the
// overflow-free form (a length field of 2^64 - k must not wrap `pos + len`).
static inline bool host_next_record(const uint8_t *b, uint64_t len, uint64_t &pos, HostRecord &r)
{
    uint64_t fs, p = pos;
    r.start = pos;
    if (!host_varint(b, len, p, fs) || !host_varint(b, len, p, r.sample_count) ||
        !host_varint(b, len, p, r.tag) || !host_varint(b, len, p, r.payload_len))
        return false;
    if (r.payload_len > len - p || r.payload_len > 0xFFFFFFFFull) return false;
    r.payload_off = p;
    pos = p + r.payload_len;
    return true;
}

}  // namespace atsc

// Large host results handed to the caller (decoded samples) come from big_alloc and go back through atsc_free
// -> big_release: the block released last is kept and handed out again when the next result is about the same
// size.  A fresh allocation of 84 MB is untouched address space whose pages fault in one by one during the
// device-to-host copy (milliseconds, more than the copy itself); a recycled block is resident.  At most one
// block (up to BIG_KEEP_MAX bytes) is held.
namespace atsc {
void *big_alloc(size_t bytes);
bool big_release(void *p);  // true: p was a big_alloc block and has been taken care of
void big_trim();            // frees the kept block
}  // namespace atsc

// The records of a stream one behind the other (pending chunks compressed first) and the stream's context: what
// the stream's window queries (atsc_windows.cpp) take from atsc_stream.cpp
struct atsc_ctx;
struct atsc_stream;
namespace atsc {
int stream_body(atsc_stream *s, std::vector<uint8_t> &body, atsc_ctx **ctx);
}  // namespace atsc

// atsc_compress_frames with the output allocated by the library once its length is known (*out: malloc'd,
// head_room bytes left free in front of the records) and, when nonfinite != NULL, a device-side flag for NaN /
// infinite samples (atsc_compress_data's clean_data check)
extern "C" int atsc_internal_compress_frames_scan(atsc_ctx *ctx, const double *samples, const uint64_t *frame_off,
                                                  uint64_t n_frames, int compressor, int bounded, float max_error,
                                                  int sample_level, uint64_t head_room, uint8_t **out,
                                                  uint64_t *body_len, uint64_t *rec_off, int *nonfinite);

// test hook (tests/asan): the host half of atsc_dplan_create on untrusted bytes, no GPU needed
extern "C" int atsc_internal_dplan_parse(const uint8_t *body, uint64_t body_len, int has_count,
                                         uint64_t *n_frames, uint64_t *n_samples);
// test hook: the order in which the kernels' heap replay (hp_*, atsc_device.h) pops `k` of `bins` entries
// with the given f32 norms (runs a one-wavefront kernel; needs a GPU)
extern "C" int atsc_internal_heap_order(const float *norms, uint32_t bins, uint32_t k, uint32_t *order);
