// tests/asan/sim_kernels.cpp -- strong definitions of all 45 kernel launchers of libatsc_hip.so for _build/host_sim
// (host_fuzz keeps stub_kernels.cpp).  No kernel is emulated.  A stand-in
//   (a) checks every pointer argument: its base lies in a live device block of the stand-in runtime (fake_hip.cpp), and
//       a table of n entries ends inside its block;
//   (b) reads the task table the host built and checks what each entry addresses -- the addresses a GPU would fault on;
//       the ranges are noted as the operation's reads and writes for the happens-before check;
//   (c) writes only what the host, or a later stand-in, reads back:
//         launch_pack           rec_off[0 .. n] (monotone, from the chain word), chain[1], the total; chosen and err as 0
//         launch_order_by_cost  ids_dst = ids_src (the next call's launch order must be a permutation)
//         launch_sel_count      cnt[slot] = len % 3;  launch_sel_scan: the exclusive scan and the total;
//         launch_sel_offsets    off[i] = pre[first[i]]
//         launch_copy_words     really copies (the plan tables the next stand-in reads)
//         compress / decode     the events a dispatch carries (ev0, ev1) are recorded; the decode status stays 0
//       everything else leaves its output untouched.
// Launchers left at (a), the whole block noted instead of ranges: none of the table-driven ones.  launch_qnt_pick checks
// its tasks' state and histogram slots and the result rows, not the ranks inside DevQState (the kernels' own data).
// launch_compress_large / launch_decompress_large check the workspace as ws_stride * ws_slots bytes, not the layout
// inside a slot (atsc_large.hip's own).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fake_hip.h"

#include "../../include/atsc_hip.h"
#include "../../atsc_amd/csrc/atsc_internal.h"

using namespace fake;

namespace {
struct Op {
    uint64_t before;
    Op(hipStream_t s, const char *name) : before(violations())
    {
        op_begin(s, name);
        ++n_launches;
    }
    bool clean() const { return violations() == before; }  // (a launch reports its first bad entry, not all of them)
};
// base + index * unit bytes, modulo 2^64 as the kernels' pointer arithmetic has it
const void *at(const void *base, uint64_t index, uint64_t unit) { return (const void *)((uintptr_t)base + index * unit); }
#define WHAT(buf, ...) char buf[96]; snprintf(buf, sizeof buf, __VA_ARGS__)

template <class T>
bool table(const T *t, uint64_t n, const char *name)
{
    return dev_read(t, n * sizeof(T), name);
}
// the plan entry a frame names, and its twiddle table
bool plan_entry(const atsc::DevPlan *plans, const float2 *tw, uint32_t pi, const char *who, uint64_t i)
{
    WHAT(w, "%s[%llu].plan = %u", who, (unsigned long long)i, pi);
    if (!dev_read(at(plans, pi, sizeof(atsc::DevPlan)), sizeof(atsc::DevPlan), w)) return false;
    const atsc::DevPlan &p = plans[pi];
    WHAT(w2, "%s[%llu]: twiddles of plan %u (tw_off %llu, L %u)", who, (unsigned long long)i, pi, (unsigned long long)p.tw_off, p.L);
    return dev_read(at(tw, p.tw_off, sizeof(float2)), (uint64_t)p.L * sizeof(float2), w2);
}
// one compress frame: its samples, its payload slot, its plan entry
bool cframe(const atsc::DevFrame *frames, uint64_t f, const double *samples, const uint8_t *slots, const atsc::DevPlan *plans,
            const float2 *tw)
{
    WHAT(w, "DevFrame[%llu]", (unsigned long long)f);
    if (!dev_read(frames + f, sizeof(atsc::DevFrame), w)) return false;
    const atsc::DevFrame fr = frames[f];
    WHAT(ws, "DevFrame[%llu]: samples [%llu, +%u)", (unsigned long long)f, (unsigned long long)fr.sample_off, fr.n);
    if (!dev_read(at(samples, fr.sample_off, 8), 8ull * fr.n, ws)) return false;
    WHAT(wl, "DevFrame[%llu]: slot at %llu, %llu bytes", (unsigned long long)f, (unsigned long long)fr.slot_off,
         (unsigned long long)atsc_payload_bound_bytes(fr.n));
    if (!dev_write(at(slots, fr.slot_off, 1), atsc_payload_bound_bytes(fr.n), wl)) return false;
    return plan_entry(plans, tw, fr.plan, "DevFrame", f);
}
bool compress_frames_checked(const char *, uint32_t count, const double *samples, const atsc::DevFrame *frames, const uint32_t *ids,
                             const atsc::DevPlan *plans, const float2 *tw, uint8_t *slots, atsc::DevResult *res,
                             atsc_frame_diag *diag, const atsc::KParams &prm)
{
    if (!table(ids, count, "ids")) return false;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t f = ids[i];
        if (!cframe(frames, f, samples, slots, plans, tw)) return false;
        WHAT(w, "res[%u]", f);  // (a trial's results are indexed like the frames as well)
        if (!dev_write(res + f, sizeof(atsc::DevResult), w)) return false;
        if (prm.trial_res && !dev_read(prm.trial_res + f, sizeof(atsc::DevResult), "trial_res[f]")) return false;
        if (prm.cost && !dev_write(prm.cost + f, 4, "cost[f]")) return false;
        if (diag && !dev_write(diag + f, sizeof(atsc_frame_diag), "diag[f]")) return false;
    }
    return true;
}
// one decode frame: its payload, its samples in the output, its plan entry
bool dframe(const atsc::DevDFrame *frames, uint64_t f, const uint8_t *body, const atsc::DevPlan *plans, const float2 *tw,
            atsc::DevDFrame &fr)
{
    WHAT(w, "DevDFrame[%llu]", (unsigned long long)f);
    if (!dev_read(frames + f, sizeof(atsc::DevDFrame), w)) return false;
    fr = frames[f];
    WHAT(wp, "DevDFrame[%llu]: payload [%llu, +%u)", (unsigned long long)f, (unsigned long long)fr.payload_off, fr.payload_len);
    if (!dev_read(at(body, fr.payload_off, 1), fr.payload_len, wp)) return false;
    return plan_entry(plans, tw, fr.plan, "DevDFrame", f);
}
bool dframe_out(const atsc::DevDFrame &fr, uint64_t f, double *out)
{
    WHAT(w, "DevDFrame[%llu]: output [%llu, +%u)", (unsigned long long)f, (unsigned long long)fr.out_off, fr.n);
    return dev_write(at(out, fr.out_off, 8), 8ull * fr.n, w);
}
// slots [lo, hi) of a tile at scratch[src], loaded in 16-byte pairs from an even slot (tile_load, atsc_tile_reduce.h)
bool tile_read(const double *scratch, uint64_t src, uint32_t lo, uint32_t hi, const char *who, uint64_t i)
{
    if (lo >= hi) return true;
    const uint64_t a = lo & ~1ull, b = ((uint64_t)hi + 1) & ~1ull;
    WHAT(w, "%s[%llu]: scratch[%llu + [%llu, %llu))", who, (unsigned long long)i, (unsigned long long)src, (unsigned long long)a,
         (unsigned long long)b);
    if (hi > atsc::AGG_TILE) { violation("%s[%llu]: hi = %u beyond the tile", who, (unsigned long long)i, hi); return false; }
    return dev_read(at(scratch, src + a, 8), 8 * (b - a), w);
}
// the entries of a combine group and where its result goes
bool comb(const atsc::DevAggComb *t, uint32_t n, const void *part, uint64_t part_bytes, const void *out, uint64_t rec_bytes,
          const uint64_t *begin, bool begin_always)
{
    if (!table(t, n, "DevAggComb tasks")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const atsc::DevAggComb c = t[i];
        const uint64_t j0 = 64ull * c.g, j1 = std::min<uint64_t>(j0 + 64, c.n);
        for (uint64_t j = j0; j < j1; ++j) {
            const uint64_t e = j == 0 ? c.head : j == (uint64_t)c.n - 1 ? c.tail : c.mid + j;
            WHAT(w, "DevAggComb[%u]: entry %llu at part[%llu]", i, (unsigned long long)j, (unsigned long long)e);
            if (!dev_read(at(part, e, part_bytes), part_bytes, w)) return false;
        }
        if (c.n && j0 >= c.n) { violation("DevAggComb[%u]: group %u of a list of %u", i, c.g, c.n); return false; }
        WHAT(w, "DevAggComb[%u]: dst %llu (%s)", i, (unsigned long long)c.dst, c.final_ ? "record" : "partial");
        if (c.final_ ? !dev_write(at(out, c.dst, rec_bytes), rec_bytes, w) : !dev_write(at(part, c.dst, part_bytes), part_bytes, w))
            return false;
        if (begin && c.final_ && (begin_always || c.n)) {
            WHAT(wb, "DevAggComb[%u]: begin[%u]", i, c.win);
            if (!dev_read(begin + c.win, 8, wb)) return false;
        }
    }
    return true;
}
bool pos_tiles(const atsc::DevPosTile *t, uint32_t n, const double *sx, const double *sy, void *part, uint64_t part_bytes)
{
    if (!table(t, n, "DevPosTile tasks")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        if (!tile_read(sx, t[i].src, t[i].lo, t[i].hi, "DevPosTile", i)) return false;
        if (sy && !tile_read(sy, t[i].src, t[i].lo, t[i].hi, "DevPosTile (y)", i)) return false;
        WHAT(w, "DevPosTile[%u]: part[%llu]", i, (unsigned long long)t[i].dst);
        if (!dev_write(at(part, t[i].dst, part_bytes), part_bytes, w)) return false;
    }
    return true;
}
bool agg_tiles(const atsc::DevAggTile *t, uint32_t n, const double *scratch, void *part, uint64_t part_bytes, double *fl)
{
    if (!table(t, n, "DevAggTile tasks")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        if (!tile_read(scratch, t[i].src, t[i].lo, t[i].hi, "DevAggTile", i)) return false;
        WHAT(w, "DevAggTile[%u]: part[%llu]", i, (unsigned long long)t[i].dst);
        if (!dev_write(at(part, t[i].dst, part_bytes), part_bytes, w)) return false;
        if (fl && (t[i].flags & atsc::AGG_FIRST) && !dev_write(fl + 2ull * t[i].win, 8, "DevAggTile: fl[2 win]")) return false;
        if (fl && (t[i].flags & atsc::AGG_LAST) && !dev_write(fl + 2ull * t[i].win + 1, 8, "DevAggTile: fl[2 win + 1]")) return false;
    }
    return true;
}
// the rolling pyramids (atsc_rolling.hip, atsc_rolling_delta.hip): pb bytes a partial, rb bytes a record
bool roll_piece(const atsc::DevRollPiece *pc, atsc::DevRollPiece &P)
{
    if (!dev_read(pc, sizeof(atsc::DevRollPiece), "DevRollPiece")) return false;
    P = *pc;
    if (P.a1 <= P.a0 || (P.a0 & (atsc::ROLL_TILE - 1)) || (P.a1 & (atsc::ROLL_TILE - 1))) {
        violation("DevRollPiece: [%llu, %llu) is no run of whole tiles", (unsigned long long)P.a0, (unsigned long long)P.a1);
        return false;
    }
    return true;
}
bool level_range(const void *pyr, const atsc::DevRollPiece &P, uint32_t level, uint64_t c0, uint64_t c1 /* chunk indices, inclusive */,
                 uint64_t pb, bool write)
{
    WHAT(w, "pyramid level %u, chunks [%llu, %llu] at off %llu", level, (unsigned long long)c0, (unsigned long long)c1,
         (unsigned long long)P.off[level]);
    const void *p = at(pyr, P.off[level] + (c0 - (P.a0 >> level)), pb);
    return write ? dev_write(p, (c1 - c0 + 1) * pb, w) : dev_read(p, (c1 - c0 + 1) * pb, w);
}
bool roll_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const atsc::DevRollPiece *pc, uint32_t lmax, uint64_t pb, bool delta)
{
    atsc::DevRollPiece P;
    if (!roll_piece(pc, P)) return false;
    if (!dev_read(scratch, 8ull * n_tiles * atsc::ROLL_TILE, delta ? "scratch tiles (pairs)" : "scratch tiles")) return false;
    const uint64_t span = (uint64_t)n_tiles * atsc::ROLL_TILE;
    if (P.a0 + span > P.a1) { violation("pyramid: %u tiles from sample %llu run past the piece's end %llu", n_tiles, (unsigned long long)P.a0, (unsigned long long)P.a1); return false; }
    for (uint32_t l = 3; l <= std::min(lmax, 11u); ++l)
        if (!level_range(pyr, P, l, P.a0 >> l, (P.a0 + span - 1) >> l, pb, true)) return false;
    return true;
}
bool roll_upper(void *pyr, const atsc::DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, uint64_t pb)
{
    atsc::DevRollPiece P;
    if (!roll_piece(pc, P)) return false;
    if (n == 0) return true;
    const uint64_t last = P.a1 - 1;
    // the wavefronts cover chunks [(a0 >> src) / 64 * 64, + 64 n) of level src; those inside the piece are read
    const uint64_t c_lo = P.a0 >> src, c_hi = std::min(last >> src, ((c_lo >> 6) + n) * 64 - 1);
    if (!level_range(pyr, P, src, c_lo, c_hi, pb, false)) return false;
    for (uint32_t l = src + 1; l <= std::min(src + 6, lmax); ++l) {
        const uint64_t j_lo = P.a0 >> l, j_hi = std::min(last >> l, c_hi >> (l - src));
        if (j_hi >= j_lo && !level_range(pyr, P, l, j_lo, j_hi, pb, true)) return false;
    }
    return true;
}
bool roll_positions(const atsc::DevRollTask *t, uint32_t n, const double *scratch, const void *pyr, const atsc::DevRollPiece *pc,
                    uint64_t w, uint64_t stride, void *out, uint64_t pb, uint64_t rb, bool delta)
{
    atsc::DevRollPiece P;
    if (!roll_piece(pc, P) || !table(t, n, "DevRollTask tasks")) return false;
    if (w == 0) { violation("rolling positions: width 0"); return false; }
    for (uint32_t i = 0; i < n; ++i) {
        if (t[i].n > atsc::ROLL_TASK) { violation("DevRollTask[%u]: %u positions", i, t[i].n); return false; }
        for (uint32_t p = 0; p < t[i].n; ++p) {
            const uint64_t lo = t[i].lo + (uint64_t)p * stride, hi = lo + w;
            if (lo < P.a0 || hi > P.a1) {
                violation("DevRollTask[%u] position %u: window [%llu, %llu) outside the piece [%llu, %llu)", i, p, (unsigned long long)lo,
                          (unsigned long long)hi, (unsigned long long)P.a0, (unsigned long long)P.a1);
                return false;
            }
            // the window's samples (the low levels and the zero-sign walk read them; the deltas' first pair is x[lo], x[lo + 1])
            WHAT(ws, "DevRollTask[%u] position %u: scratch [%llu, +%llu)", i, p, (unsigned long long)(lo - P.a0), (unsigned long long)w);
            if (!dev_read(at(scratch, lo - P.a0, 8), 8 * w, ws)) return false;
            for (uint64_t pos = delta ? lo + 1 : lo; pos < hi;) {
                const uint32_t up = pos ? (uint32_t)__builtin_ctzll(pos) : 63u, fit = 63u - (uint32_t)__builtin_clzll(hi - pos);
                const uint32_t l = std::min(up, fit);
                if (l > atsc::ROLL_MAX_LEVEL) { violation("DevRollTask[%u]: level %u", i, l); return false; }
                if (l >= atsc::ROLL_LOW && !level_range(pyr, P, l, pos >> l, pos >> l, pb, false)) return false;
                pos += 1ull << l;
            }
        }
        WHAT(wo, "DevRollTask[%u]: records [%llu, +%u)", i, (unsigned long long)t[i].rec, t[i].n);
        if (!dev_write(at(out, t[i].rec, rb), rb * t[i].n, wo)) return false;
    }
    return true;
}
// the across kernels: position p of a task reads slot (lo - a0) + p stride of every stream's region
bool across(const atsc::DevRollTask *t, uint32_t n, const double *scratch, const uint64_t *reg, uint32_t ns, uint64_t a0,
            uint64_t stride, void *out, uint64_t rb)
{
    if (!table(t, n, "DevRollTask tasks") || !dev_read(reg, 8ull * ns, "reg[n_streams]")) return false;
    if (ns == 0 || ns > ATSC_ACROSS_MAX_STREAMS) { violation("across: %u streams", ns); return false; }
    for (uint32_t i = 0; i < n; ++i) {
        if (t[i].n == 0) continue;
        if (t[i].lo < a0) { violation("DevRollTask[%u]: lo %llu in front of a0 %llu", i, (unsigned long long)t[i].lo, (unsigned long long)a0); return false; }
        const uint64_t s0 = t[i].lo - a0, s1 = s0 + (uint64_t)(t[i].n - 1) * stride + 1;
        // (stride 1 loads pairs from an even slot: the range's ends round outwards inside the task's own positions only)
        for (uint32_t k = 0; k < ns; ++k) {
            WHAT(w, "DevRollTask[%u]: region %u (at %llu), slots [%llu, %llu)", i, k, (unsigned long long)reg[k], (unsigned long long)s0,
                 (unsigned long long)s1);
            if (!dev_read(at(scratch, reg[k] + s0, 8), 8 * (s1 - s0), w)) return false;
        }
        WHAT(wo, "DevRollTask[%u]: records [%llu, +%u)", i, (unsigned long long)t[i].rec, t[i].n);
        if (!dev_write(at(out, t[i].rec, rb), rb * t[i].n, wo)) return false;
    }
    return true;
}
}  // namespace

namespace atsc {
// ------------------------------------------------------------------------------------------
// atsc_kernels.hip, atsc_large.hip, atsc_decode.hip: the nine launchers of atsc_host.cpp
// ------------------------------------------------------------------------------------------
hipError_t launch_compress_class(int cls, uint32_t count, uint32_t, const double *samples, const DevFrame *frames, const uint32_t *ids,
                                 const DevPlan *plans, const float2 *twpool, const KParams &prm, uint8_t *slots, DevResult *res,
                                 atsc_frame_diag *diag, const UniArgs &uni, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    if (cls < 0 || cls > 5) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (ev0) (void)hipEventRecord(ev0, s);
    Op op(s, "k_compress");
    if (compress_frames_checked("k_compress", count, samples, frames, ids, plans, twpool, slots, res, diag, prm) && uni.enabled) {
        // the uniform launch computes the descriptor: it must be the table's
        for (uint32_t i = 0; i < count && op.clean(); ++i) {
            const DevFrame &fr = frames[uni.adaptive ? ids[i] : uni.fid0 + i];
            const uint64_t k = (uni.adaptive ? ids[i] : uni.fid0 + i) - uni.fid0;
            if (fr.n != uni.n || fr.plan != uni.plan || fr.sample_off != uni.sample_off0 + k * uni.n ||
                fr.slot_off != uni.slot_off0 + k * uni.slot_stride)
                violation("k_compress: uniform arguments disagree with DevFrame[%llu]", (unsigned long long)(uni.fid0 + k));
        }
        if (uni.spread && std::__gcd(uni.spread, uni.count) != 1) violation("k_compress: spread %u not coprime to count %u", uni.spread, uni.count);
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipSuccess;
}
hipError_t launch_compress_large(uint32_t count, const double *samples, const DevFrame *frames, const uint32_t *ids, const DevPlan *plans,
                                 const float2 *twpool, const KParams &prm, uint8_t *slots, DevResult *res, atsc_frame_diag *diag,
                                 unsigned char *ws, uint64_t ws_stride, uint32_t ws_slots, hipStream_t s, const LargePre *)
{
    if (count == 0) return hipSuccess;
    Op op(s, "k_compress_large");
    if (!compress_frames_checked("k_compress_large", count, samples, frames, ids, plans, twpool, slots, res, diag, prm)) return hipSuccess;
    if (ws_slots == 0) violation("k_compress_large: no workspace slots for %u frames", count);
    else dev_write(ws, ws_stride * ws_slots, "large workspace (ws_stride x ws_slots)");
    return hipSuccess;
}
uint32_t resident_grid(int, uint32_t, uint32_t) { return 0; }
// (a bound of the same order as atsc_large.hip's; only its use as a stride matters here)
uint64_t large_ws_bytes(uint32_t n, uint32_t L, uint32_t kcap) { return 64ull * n + 32ull * L + 16ull * kcap; }
hipError_t launch_decompress_large(uint32_t count, const struct DevDFrame *frames, const uint32_t *ids, const DevPlan *plans,
                                   const float2 *twpool, const uint8_t *body, double *out, int *status, unsigned char *ws,
                                   uint64_t ws_stride, uint32_t ws_slots, int, int, hipStream_t s, const LargePre *, uint32_t)
{
    if (count == 0) return hipSuccess;
    Op op(s, "k_decompress_large");
    if (!table(ids, count, "ids")) return hipSuccess;
    for (uint32_t i = 0; i < count; ++i) {
        DevDFrame fr;
        if (!dframe(frames, ids[i], body, plans, twpool, fr) || !dframe_out(fr, ids[i], out)) return hipSuccess;
    }
    if (ws_slots == 0) violation("k_decompress_large: no workspace slots for %u frames", count);
    else dev_write(ws, ws_stride * ws_slots, "large workspace (ws_stride x ws_slots)");
    dev_write(status, sizeof(int), "status");
    return hipSuccess;
}
hipError_t launch_order_by_cost(const uint32_t *ids_src, uint32_t *ids_dst, const uint32_t *cost, uint8_t *bkt, uint32_t *hist,
                                const uint32_t *class_first, const uint32_t *class_count, int n_classes, hipStream_t s)
{
    uint32_t total = 0;
    for (int c = 0; c < n_classes; ++c)
        if (class_count[c]) {
            if (class_first[c] != total) return hipErrorInvalidValue;
            total += class_count[c];
        }
    if (!total) return hipSuccess;
    Op op(s, "k_cost_hist + k_cost_scatter");
    if (table(ids_src, total, "ids_src") && dev_write(ids_dst, 4ull * total, "ids_dst") && dev_write(bkt, total, "buckets") &&
        dev_write(hist, 2 * 8 * 64 * 4, "histogram and cursors")) {
        for (uint32_t i = 0; i < total && op.clean(); ++i) dev_read(cost + ids_src[i], 4, "cost[ids_src[i]]");
        if (op.clean()) memcpy(ids_dst, ids_src, 4ull * total);
    }
    return hipSuccess;
}
hipError_t launch_nonfinite_flag(const double *x, uint64_t n, uint32_t *flag, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_nonfinite_flag");
    if (dev_read(x, 8 * n, "samples")) dev_write(flag, 4, "flag");
    return hipSuccess;
}
hipError_t launch_pack(const DevFrame *frames, const DevResult *res, uint64_t n_frames, uint32_t *local, uint64_t *blocksum,
                       const uint8_t *slots, uint8_t *body, uint64_t body_cap, uint64_t *rec_off, uint8_t *chosen, double *err,
                       const uint32_t *big_ids, uint32_t n_big, hipStream_t s, uint64_t *chain)
{
    Op op(s, "k_pack");
    if (!table(frames, n_frames, "frames") || !table(res, n_frames, "res") || !dev_write(local, 4 * n_frames, "local") ||
        !dev_write(blocksum, 8 * ((n_frames + 1023) / 1024 + 1), "blocksum") || !dev_read_block(slots, "slots") ||
        !in_block(body, body_cap, "body[body_cap]") || !dev_write(rec_off, 8 * (n_frames + 1), "rec_off[n_frames + 1]"))
        return hipSuccess;
    if (chosen && !dev_write(chosen, n_frames, "chosen")) return hipSuccess;
    if (err && !dev_write(err, 8 * n_frames, "err")) return hipSuccess;
    if (n_big && !table(big_ids, n_big, "big_ids")) return hipSuccess;
    for (uint32_t i = 0; i < n_big; ++i)
        if (big_ids[i] >= n_frames) { violation("k_pack: big_ids[%u] = %u of %llu frames", i, big_ids[i], (unsigned long long)n_frames); return hipSuccess; }
    if (chain && (!dev_read(chain, 8, "chain[0]") || !dev_write(chain + 1, 8, "chain[1]"))) return hipSuccess;
    uint64_t off = chain ? chain[0] : 0;
    const uint64_t start = off;
    for (uint64_t f = 0; f < n_frames; ++f) {
        rec_off[f] = off;
        off += 5 + (f & 3);  // (a record of 5 .. 8 bytes: never more than the bound's 16 + payload bytes per frame)
        if (chosen) chosen[f] = 0;
        if (err) err[f] = 0.0;
    }
    rec_off[n_frames] = off;
    if (chain) chain[1] = off;
    if (off <= body_cap) dev_write(body + start, off - start, "the call's records in body");
    return hipSuccess;
}
hipError_t launch_copy_words(void *dst, const void *src, uint64_t n_words, hipStream_t s)
{
    if (n_words == 0) return hipSuccess;
    Op op(s, "k_copy_words");
    if (pinned_read(src, 4 * n_words, "source (page-locked staging)") && dev_write(dst, 4 * n_words, "destination")) memcpy(dst, src, 4 * n_words);
    return hipSuccess;
}
hipError_t launch_decompress(const struct DevDFrame *frames, uint64_t n_frames, const uint32_t *ids, int cls, uint32_t count, uint32_t,
                             const DevPlan *plans, const float2 *twpool, const uint8_t *body, double *out, int *status, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if (cls < 0 || cls > 5) return hipErrorInvalidValue;
    Op op(s, "k_decompress");
    if (ids && !table(ids, count, "ids")) return hipSuccess;
    if (!ids && count != n_frames) { violation("k_decompress: no ids for %u of %llu frames", count, (unsigned long long)n_frames); return hipSuccess; }
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t f = ids ? ids[i] : i;
        DevDFrame fr;
        if (f >= n_frames) { violation("k_decompress: ids[%u] = %llu of %llu frames", i, (unsigned long long)f, (unsigned long long)n_frames); return hipSuccess; }
        if (!dframe(frames, f, body, plans, twpool, fr) || !dframe_out(fr, f, out)) return hipSuccess;
    }
    dev_write(status, sizeof(int), "status");
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------
// the 36 launchers of atsc_windows.cpp
// ------------------------------------------------------------------------------------------
hipError_t launch_decompress_window(const DevDFrame *frames, const DevWTask *tasks, int cls, uint32_t count, uint32_t, const DevPlan *plans,
                                    const float2 *twpool, const uint8_t *body, double *out, int *status, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if (cls < 0 || cls > 5) return hipErrorInvalidValue;
    Op op(s, "k_decompress (window)");
    if (!table(tasks, count, "DevWTask tasks")) return hipSuccess;
    const uint64_t n_frames = room(frames) / sizeof(DevDFrame);
    for (uint32_t i = 0; i < count; ++i) {
        const DevWTask t = tasks[i];
        DevDFrame fr;
        if (t.frame >= n_frames) { violation("DevWTask[%u]: frame %u of %llu", i, t.frame, (unsigned long long)n_frames); return hipSuccess; }
        if (!dframe(frames, t.frame, body, plans, twpool, fr)) return hipSuccess;
        if (t.lo >= t.hi || t.hi > fr.n) { violation("DevWTask[%u]: samples [%u, %u) of a frame of %u", i, t.lo, t.hi, fr.n); return hipSuccess; }
        WHAT(w, "DevWTask[%u]: out[%llu, +%u)", i, (unsigned long long)t.dst, t.hi - t.lo);
        if (!dev_write(at(out, t.dst, 8), 8ull * (t.hi - t.lo), w)) return hipSuccess;
    }
    dev_write(status, sizeof(int), "status");
    return hipSuccess;
}
hipError_t launch_window_gather(const DevWGather *g, uint32_t n, uint32_t max_len, const double *scratch, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_window_gather");
    if (!table(g, n, "DevWGather copies")) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        if (g[i].len > max_len) { violation("DevWGather[%u]: len %u beyond the launch's %u", i, g[i].len, max_len); return hipSuccess; }
        WHAT(w, "DevWGather[%u]: %u samples, src %llu, dst %llu", i, g[i].len, (unsigned long long)g[i].src, (unsigned long long)g[i].dst);
        if (!dev_read(at(scratch, g[i].src, 8), 8ull * g[i].len, w) || !dev_write(at(out, g[i].dst, 8), 8ull * g[i].len, w)) return hipSuccess;
    }
    return hipSuccess;
}
hipError_t launch_agg_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch, DevAggPart *part, double *fl, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_agg_tiles");
    agg_tiles(tasks, n, scratch, part, sizeof(DevAggPart), fl);
    return hipSuccess;
}
hipError_t launch_agg_combine(const DevAggComb *tasks, uint32_t n, DevAggPart *part, const double *fl, void *stats, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_agg_combine");
    if (comb(tasks, n, part, sizeof(DevAggPart), stats, sizeof(atsc_window_stats), nullptr, false))
        for (uint32_t i = 0; i < n && op.clean(); ++i)
            if (tasks[i].final_ && tasks[i].n) dev_read(fl + 2ull * tasks[i].win, 16, "DevAggComb: fl[2 win, 2 win + 1]");
    return hipSuccess;
}
static bool q_tasks(const DevQTask *t, uint32_t n, const double *scratch, const double *q, uint32_t n_q, double *out, uint64_t max_n)
{
    if (!table(t, n, "DevQTask tasks") || !dev_read(q, 8ull * n_q, "q[n_q]")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        if (t[i].n > max_n) { violation("DevQTask[%u]: %llu samples in a tier of at most %llu", i, (unsigned long long)t[i].n, (unsigned long long)max_n); return false; }
        WHAT(w, "DevQTask[%u]: scratch[%llu, +%llu)", i, (unsigned long long)t[i].src, (unsigned long long)t[i].n);
        if (!dev_read(at(scratch, t[i].src, 8), 8 * t[i].n, w)) return false;
        WHAT(wo, "DevQTask[%u]: out row %u", i, t[i].win);
        if (!dev_write(at(out, (uint64_t)t[i].win * n_q, 8), 8ull * n_q, wo)) return false;
    }
    return true;
}
hipError_t launch_qnt_short(const DevQTask *tasks, uint32_t n, const double *scratch, const double *q, uint32_t n_q, int, double *out,
                            hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_qnt_short");
    q_tasks(tasks, n, scratch, q, n_q, out, QNT_SHORT_MAX);
    return hipSuccess;
}
hipError_t launch_qnt_medium(const DevQTask *tasks, uint32_t n, uint32_t P, const double *scratch, const double *q, uint32_t n_q, int,
                             double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_qnt_medium");
    q_tasks(tasks, n, scratch, q, n_q, out, P);
    return hipSuccess;
}
hipError_t launch_qnt_hist(const DevQChunk *chunks, uint32_t n, const double *scratch, const DevQState *st, uint32_t *hist, uint32_t rows,
                           uint32_t pass, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_qnt_hist");
    if (!table(chunks, n, "DevQChunk chunks")) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        if (chunks[i].len > QNT_CHUNK) { violation("DevQChunk[%u]: %u samples", i, chunks[i].len); return hipSuccess; }
        WHAT(w, "DevQChunk[%u]: scratch[%llu, +%u), slot %u", i, (unsigned long long)chunks[i].src, chunks[i].len, chunks[i].slot);
        if (!dev_read(at(scratch, chunks[i].src, 8), 8ull * chunks[i].len, w)) return hipSuccess;
        if (pass && !dev_read(st + chunks[i].slot, sizeof(DevQState), w)) return hipSuccess;
        if (!dev_write(at(hist, (uint64_t)chunks[i].slot * rows * 256u, 4), 4ull * rows * 256u, w)) return hipSuccess;
    }
    return hipSuccess;
}
hipError_t launch_qnt_pick(const DevQTask *tasks, uint32_t n, DevQState *st, uint32_t *hist, uint32_t rows, uint32_t, const double *q,
                           uint32_t n_q, int, double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_qnt_pick");
    if (!table(tasks, n, "DevQTask tasks") || !dev_read(q, 8ull * n_q, "q[n_q]")) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        WHAT(w, "DevQTask[%u]: slot %u, out row %u", i, tasks[i].slot, tasks[i].win);
        if (!dev_write(st + tasks[i].slot, sizeof(DevQState), w) ||
            !dev_write(at(hist, (uint64_t)tasks[i].slot * rows * 256u, 4), 4ull * rows * 256u, w) ||
            !dev_write(at(out, (uint64_t)tasks[i].win * n_q, 8), 8ull * n_q, w))
            return hipSuccess;
    }
    return hipSuccess;
}
static bool h_tasks(const DevHistTask *t, uint32_t n, const double *scratch, const double *edges, uint32_t n_edges, uint64_t *out, uint32_t max_len)
{
    if (!table(t, n, "DevHistTask tasks") || !dev_read(edges, 8ull * n_edges, "edges[n_edges]")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = t[i].len & ~HST_OWN;
        if (len > max_len) { violation("DevHistTask[%u]: %u samples in a tier of at most %u", i, len, max_len); return false; }
        WHAT(w, "DevHistTask[%u]: scratch[%llu, +%u), row %u", i, (unsigned long long)t[i].src, len, t[i].win);
        if (!dev_read(at(scratch, t[i].src, 8), 8ull * len, w)) return false;
        if (!dev_write(at(out, (uint64_t)t[i].win * (n_edges + 2u), 8), 8ull * (n_edges + 2u), w)) return false;
    }
    return true;
}
hipError_t launch_hst_short(const DevHistTask *tasks, uint32_t n, const double *scratch, const double *edges, uint32_t n_edges, int,
                            uint64_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_hst_short");
    h_tasks(tasks, n, scratch, edges, n_edges, out, HST_SHORT_MAX);
    return hipSuccess;
}
hipError_t launch_hst_chunk(const DevHistTask *tasks, uint32_t n, const double *scratch, const double *edges, uint32_t n_edges, int,
                            uint64_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_hst_chunk");
    h_tasks(tasks, n, scratch, edges, n_edges, out, HST_CHUNK);
    return hipSuccess;
}
hipError_t launch_mom_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, DevMomPart *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_mom_tiles");
    pos_tiles(tasks, n, scratch, nullptr, part, sizeof(DevMomPart));
    return hipSuccess;
}
hipError_t launch_mom_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, const uint64_t *begin, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_mom_combine");
    comb(tasks, n, part, sizeof(DevMomPart), out, sizeof(atsc_window_moments), begin, true);
    return hipSuccess;
}
hipError_t launch_dlt_tiles(const DevDltTile *tasks, uint32_t n, const double *scratch, const double *carry, DevDltPart *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_dlt_tiles");
    if (!table(tasks, n, "DevDltTile tasks")) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        const DevDltTile t = tasks[i];
        if (!tile_read(scratch, t.src, t.lo, t.hi, "DevDltTile", i)) return hipSuccess;
        if ((t.flags & DLT_CONT) && t.lo < t.hi) {
            if (t.lo != 0) { violation("DevDltTile[%u]: DLT_CONT with lo = %u", i, t.lo); return hipSuccess; }
            // the sample in front of the tile: the carry slot, or the slot in front of the tile in the scratch
            WHAT(w, "DevDltTile[%u]: the sample in front of scratch[%llu]", i, (unsigned long long)t.src);
            if ((t.flags & DLT_CARRY) ? !dev_read(carry, 8, "carry slot") : !dev_read(at(scratch, t.src - 1, 8), 8, w)) return hipSuccess;
        }
        WHAT(w, "DevDltTile[%u]: part[%llu]", i, (unsigned long long)t.dst);
        if (!dev_write(at(part, t.dst, sizeof(DevDltPart)), sizeof(DevDltPart), w)) return hipSuccess;
    }
    return hipSuccess;
}
hipError_t launch_dlt_combine(const DevAggComb *tasks, uint32_t n, DevDltPart *part, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_dlt_combine");
    comb(tasks, n, part, sizeof(DevDltPart), out, sizeof(atsc_window_delta), nullptr, false);
    return hipSuccess;
}
hipError_t launch_run_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, int, double, DevRunPart *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_run_tiles");
    pos_tiles(tasks, n, scratch, nullptr, part, sizeof(DevRunPart));
    return hipSuccess;
}
hipError_t launch_run_combine(const DevAggComb *tasks, uint32_t n, DevRunPart *part, const uint64_t *begin, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_run_combine");
    comb(tasks, n, part, sizeof(DevRunPart), out, sizeof(atsc_window_runs), begin, false);
    return hipSuccess;
}
hipError_t launch_ext_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, uint32_t k, void *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_ext_tiles");
    if (k < 1 || k > EXT_MAX_K) violation("k_ext_tiles: k = %u", k);
    else pos_tiles(tasks, n, scratch, nullptr, part, 8ull * (2 + 4 * k));
    return hipSuccess;
}
hipError_t launch_ext_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part, const uint64_t *begin, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_ext_combine");
    if (k < 1 || k > EXT_MAX_K) violation("k_ext_combine: k = %u", k);
    else comb(tasks, n, part, 8ull * (2 + 4 * k), out, ATSC_EXTREMES_BYTES(k), begin, false);
    return hipSuccess;
}
hipError_t launch_val_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch, uint32_t k, uint64_t, void *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_val_tiles");
    if (k < 1 || k > ATSC_VALUES_MAX_K) violation("k_val_tiles: k = %u", k);
    else agg_tiles(tasks, n, scratch, part, 8ull * (4 + 2 * k), nullptr);
    return hipSuccess;
}
hipError_t launch_val_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_val_combine");
    if (k < 1 || k > ATSC_VALUES_MAX_K) violation("k_val_combine: k = %u", k);
    else comb(tasks, n, part, 8ull * (4 + 2 * k), out, ATSC_VALUES_BYTES(k), nullptr, false);
    return hipSuccess;
}
// a select task's samples: loaded in pairs from the even slot at or in front of src (sel_span, atsc_select.hip)
static bool sel_tasks(const DevSelTask *t, uint32_t n, const double *scratch)
{
    if (!table(t, n, "DevSelTask tasks")) return false;
    for (uint32_t i = 0; i < n; ++i) {
        if (t[i].len == 0 || t[i].len > SEL_TASK) { violation("DevSelTask[%u]: %u samples", i, t[i].len); return false; }
        const uint64_t a = t[i].src & ~1ull, b = (t[i].src + t[i].len + 1) & ~1ull;
        WHAT(w, "DevSelTask[%u]: scratch[%llu, %llu)", i, (unsigned long long)a, (unsigned long long)b);
        if (!dev_read(at(scratch, a, 8), 8 * (b - a), w)) return false;
    }
    return true;
}
hipError_t launch_sel_count(const DevSelTask *tasks, uint32_t n, const double *scratch, int, double, uint64_t *cnt, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_sel_count");
    if (!sel_tasks(tasks, n, scratch)) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        WHAT(w, "DevSelTask[%u]: cnt[%u]", i, tasks[i].slot);
        if (!dev_write(cnt + tasks[i].slot, 8, w)) return hipSuccess;
        cnt[tasks[i].slot] = tasks[i].len % 3;
    }
    return hipSuccess;
}
hipError_t launch_sel_scan(uint64_t *cnt, uint64_t n, uint64_t *sums, hipStream_t s)
{
    Op op(s, "k_sel_scan");
    if (!dev_write(cnt, 8 * (n + 1), "cnt[n + 1]")) return hipSuccess;
    const uint64_t words = sel_scan_sums(n + 1);
    if (words && !dev_write(sums, 8 * words, "block sums")) return hipSuccess;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t v = cnt[i];
        cnt[i] = sum;
        sum += v;
    }
    cnt[n] = sum;
    return hipSuccess;
}
hipError_t launch_sel_offsets(const uint64_t *pre, const uint32_t *first, uint64_t n, uint64_t *off, hipStream_t s)
{
    Op op(s, "k_sel_offsets");
    if (!dev_read(first, 4 * n, "first[n_windows + 1]") || !dev_write(off, 8 * n, "off[n_windows + 1]")) return hipSuccess;
    for (uint64_t i = 0; i < n; ++i) {
        WHAT(w, "first[%llu] = %u", (unsigned long long)i, first[i]);
        if (!dev_read(pre + first[i], 8, w)) return hipSuccess;
        off[i] = pre[first[i]];
    }
    return hipSuccess;
}
hipError_t launch_sel_write(const DevSelTask *tasks, uint32_t n, const double *scratch, int, double, const uint64_t *pre, uint64_t cap,
                            void *entries, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_sel_write");
    if (!sel_tasks(tasks, n, scratch)) return hipSuccess;
    for (uint32_t i = 0; i < n; ++i) {
        // the task's entries: from pre[slot] up to the next slot's (the scan's total behind the last), those below cap
        WHAT(w, "DevSelTask[%u]: pre[%u .. %u]", i, tasks[i].slot, tasks[i].slot + 1);
        if (!dev_read(pre + tasks[i].slot, 16, w)) return hipSuccess;
        const uint64_t r0 = std::min(pre[tasks[i].slot], cap), r1 = std::min(pre[tasks[i].slot + 1], cap);
        WHAT(we, "DevSelTask[%u]: entries [%llu, %llu)", i, (unsigned long long)r0, (unsigned long long)r1);
        if (r1 > r0 && !dev_write(at(entries, r0, 16), 16 * (r1 - r0), we)) return hipSuccess;
    }
    return hipSuccess;
}
hipError_t launch_pair_tiles(const DevPosTile *tasks, uint32_t n, const double *sx, const double *sy, DevMomPart *part, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_pair_tiles");
    pos_tiles(tasks, n, sx, sy, part, sizeof(DevMomPart));
    return hipSuccess;
}
hipError_t launch_pair_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_pair_combine");
    comb(tasks, n, part, sizeof(DevMomPart), out, sizeof(atsc_window_pair), nullptr, false);
    return hipSuccess;
}
hipError_t launch_roll_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax, hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_LOW) return hipSuccess;
    Op op(s, "k_roll_pyramid");
    roll_pyramid(scratch, n_tiles, pyr, pc, lmax, 32, false);
    return hipSuccess;
}
hipError_t launch_roll_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_roll_upper");
    roll_upper(pyr, pc, n, src, lmax, 32);
    return hipSuccess;
}
hipError_t launch_roll_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr, const DevRollPiece *pc,
                                 uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_roll_positions");
    roll_positions(tasks, n, scratch, pyr, pc, w, stride, out, 32, sizeof(atsc_window_rolling), false);
    return hipSuccess;
}
hipError_t launch_rdl_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax, hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_DELTA_LOW) return hipSuccess;
    Op op(s, "k_rdl_pyramid");
    roll_pyramid(scratch, n_tiles, pyr, pc, lmax, ROLL_DELTA_PART, true);
    return hipSuccess;
}
hipError_t launch_rdl_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_rdl_upper");
    roll_upper(pyr, pc, n, src, lmax, ROLL_DELTA_PART);
    return hipSuccess;
}
hipError_t launch_rdl_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr, const DevRollPiece *pc,
                                uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_rdl_positions");
    roll_positions(tasks, n, scratch, pyr, pc, w, stride, out, ROLL_DELTA_PART, sizeof(atsc_window_delta), true);
    return hipSuccess;
}
hipError_t launch_across_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint32_t n_streams,
                                   uint64_t a0, uint64_t stride, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_across_positions");
    across(tasks, n, scratch, reg, n_streams, a0, stride, out, sizeof(atsc_across_record));
    return hipSuccess;
}
hipError_t launch_across_quantile_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                            uint32_t n_streams, uint64_t a0, uint64_t stride, const double *q, uint32_t n_q, int,
                                            double *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_across_quantile_positions");
    if (dev_read(q, 8ull * n_q, "q[n_q]")) across(tasks, n, scratch, reg, n_streams, a0, stride, out, 8ull * n_q);
    return hipSuccess;
}
hipError_t launch_across_extremes_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                            uint32_t n_streams, uint64_t a0, uint64_t stride, uint32_t k, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_across_extremes_positions");
    across(tasks, n, scratch, reg, n_streams, a0, stride, out, ATSC_EXTREMES_BYTES(k));
    return hipSuccess;
}
hipError_t launch_across_moments_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                           uint32_t n_streams, uint64_t a0, uint64_t stride, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    Op op(s, "k_across_moments_positions");
    across(tasks, n, scratch, reg, n_streams, a0, stride, out, sizeof(atsc_across_moments));
    return hipSuccess;
}
}  // namespace atsc
