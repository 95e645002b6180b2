// tests/asan/fake_hip.cpp -- a host-memory stand-in for the 27 HIP runtime functions the host sources of
// libatsc_hip.so call, so that the whole host path (pool, plan cache, parts, staging, query slots, piece cutter, task
// tables) runs on the CPU under AddressSanitizer + UBSan, against a runtime that checks what the real one lets pass in
// silence.  Linked into _build/host_sim in place of libamdhip64; the launchers are sim_kernels.cpp's.
//
// The model
//   memory   hipMalloc is malloc of exactly the requested size (the sanitizer's red zones bound every copy and every
//            table a launcher stand-in reads), hipFree is free (a dangling pool entry is a use-after-free at its next
//            use).  Freeing a pointer that is no live block's base is a violation.  Page-locked memory
//            (hipHostMalloc, hipHostRegister) is a table of ranges; hipPointerGetAttributes answers
//            hipMemoryTypeHost inside one, hipMemoryTypeDevice inside a device block and an error elsewhere.
//   work     runs at once (memcpy / memset; launcher stand-ins write what the host reads back).  The device side of a
//            copy must lie wholly inside one live device block.
//   order    a vector clock per stream (the null stream included) and one for the host.  An enqueue carries the host's
//            clock into the stream and ticks the stream's own component; hipEventRecord snapshots the stream's clock,
//            hipStreamWaitEvent joins the snapshot into the waiting stream; hipStreamSynchronize,
//            hipEventSynchronize, hipDeviceSynchronize and hipFree join into the host.  A synchronous copy or memset
//            is an operation on the null stream followed by a host join.  Streams must be created non-blocking (the
//            library creates no other kind): they have no implicit order with the null stream.
//            Every operation notes the byte ranges it reads and writes, per device block and per page-locked range.
//            Two accesses to overlapping bytes, one of them a write, neither ordered before the other: a violation.
//            hipHostFree / hipHostUnregister of a range with accesses not joined into the host: a violation.  A
//            device-to-host Async copy into pageable memory that the host is told is complete (fake::host_consumes)
//            without a join: a violation.
//            An access joined into the host is forgotten: every later operation is enqueued by the host and so ordered
//            behind it.
//   end      fake::finish: no device block, page-locked range, stream or event may remain.
// There is no allow-list.  A violation prints one line (what, which block, which two operations) and is counted.
//
// Limits.  The host's own loads and stores cannot be seen: a memcpy into page-locked staging (h_stage, QueryRes::h)
// while a kernel still reads it, or a read of a status word in page-locked memory before its copy landed, passes.
// Work "runs" in program order, so a value the host reads back is always there.  Kernel stand-ins access what their
// tables name, not what a kernel's arithmetic would make of it.
#include "fake_hip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

namespace {
typedef std::vector<uint64_t> Clock;
void join(Clock &a, const Clock &b)
{
    if (a.size() < b.size()) a.resize(b.size(), 0);
    for (size_t i = 0; i < b.size(); ++i) a[i] = std::max(a[i], b[i]);
}
uint64_t at(const Clock &c, uint32_t t) { return t < c.size() ? c[t] : 0; }

struct Stream {
    uint32_t thread;  // 1: the null stream, 2..: created streams (0 is the host)
    Clock clock;
};
struct Event {
    uint64_t id;
    bool recorded = false;
    Clock clock;
};
struct Iv {
    uint64_t lo, hi;  // bytes from the range's base
};
// what one operation read and wrote of one range: the intervals in the order they were noted (an interval that overlaps
// or adjoins the one before it widens it), and their hulls for a quick answer
struct Access {
    uint32_t thread;
    uint64_t epoch, seq;
    const char *op;
    std::vector<Iv> rd, wr;
    uint64_t rlo = ~0ull, rhi = 0, wlo = ~0ull, whi = 0;
};
struct Range {
    uintptr_t base;
    size_t size;
    int kind;  // 0: device block, 1: hipHostMalloc, 2: hipHostRegister
    uint64_t id;
    std::vector<Access> acc;
};
struct Pending {  // a device-to-host Async copy into pageable memory
    uintptr_t lo, hi;
    uint32_t thread;
    uint64_t epoch, seq;
};

Clock g_host(1, 0);
Stream g_null{1, Clock()};
std::set<Stream *> g_streams;
std::set<Event *> g_events;
std::map<uintptr_t, Range> g_dev, g_pinned;
std::vector<Pending> g_pending;
uint32_t g_next_thread = 2;
uint64_t g_next_id = 1, g_seq = 0, g_viol = 0;
uint64_t g_mallocs = 0, g_copies = 0, g_syncs = 0;
hipError_t g_last = hipSuccess;
// the current operation
Stream *g_cur = &g_null;
const char *g_cur_name = "(none)";
uint64_t g_cur_seq = 0;

const char *kind_name(int k) { return k == 0 ? "device block" : k == 1 ? "hipHostMalloc range" : "registered range"; }

Range *find_in(std::map<uintptr_t, Range> &m, const void *p)
{
    const uintptr_t a = (uintptr_t)p;
    auto it = m.upper_bound(a);
    if (it == m.begin()) return nullptr;
    --it;
    Range &r = it->second;
    // (the end counts as inside: an empty range at a block's end is addressable)
    return a <= r.base + r.size ? &r : nullptr;
}
Stream *stream_of(hipStream_t s, const char *call)
{
    if (!s) return &g_null;
    Stream *st = (Stream *)s;
    if (!g_streams.count(st)) {
        fake::violation("%s: stream %p is no live stream", call, (void *)s);
        return &g_null;
    }
    return st;
}
bool ordered_before_host(const Access &a) { return at(g_host, a.thread) >= a.epoch; }
void host_join(const Clock &c)
{
    ++g_syncs;
    join(g_host, c);
    for (auto *m : {&g_dev, &g_pinned})
        for (auto &kv : *m) {
            auto &v = kv.second.acc;
            v.erase(std::remove_if(v.begin(), v.end(), ordered_before_host), v.end());
        }
    g_pending.erase(std::remove_if(g_pending.begin(), g_pending.end(),
                                   [](const Pending &p) { return at(g_host, p.thread) >= p.epoch; }),
                    g_pending.end());
}
void host_join_all()
{
    Clock all = g_null.clock;
    for (Stream *s : g_streams) join(all, s->clock);
    host_join(all);
}
void enqueue(Stream *s)  // the host's clock goes into the stream
{
    join(s->clock, g_host);
}
// the first interval of v that overlaps [lo, hi), or null
const Iv *overlap(const std::vector<Iv> &v, uint64_t vlo, uint64_t vhi, uint64_t lo, uint64_t hi)
{
    if (vhi <= lo || hi <= vlo) return nullptr;
    for (const Iv &i : v)
        if (i.lo < hi && lo < i.hi) return &i;
    return nullptr;
}
void note(Range &r, uint64_t lo, uint64_t hi, bool write, const char *what)
{
    if (lo >= hi) return;
    const uint32_t t = g_cur->thread;
    const uint64_t e = at(g_cur->clock, t);
    Access *mine = nullptr;
    for (Access &a : r.acc) {
        if (a.thread == t) {  // the same stream: in order
            if (a.epoch == e) mine = &a;
            continue;
        }
        if (at(g_cur->clock, a.thread) >= a.epoch) continue;  // ordered before the current operation
        const Iv *w = overlap(a.wr, a.wlo, a.whi, lo, hi), *rd = write ? overlap(a.rd, a.rlo, a.rhi, lo, hi) : nullptr;
        const Iv *hit = w ? w : rd;
        if (!hit) continue;
        fake::violation("unordered %s after %s: %s #%llu (%zu bytes), bytes [%llu, %llu) x [%llu, %llu): op %llu '%s' on stream %u "
                        "and op %llu '%s' (%s) on stream %u",
                        write ? "write" : "read", w ? "write" : "read", kind_name(r.kind), (unsigned long long)r.id, r.size,
                        (unsigned long long)hit->lo, (unsigned long long)hit->hi, (unsigned long long)lo, (unsigned long long)hi,
                        (unsigned long long)a.seq, a.op, a.thread, (unsigned long long)g_cur_seq, g_cur_name, what, t);
        break;  // one line per access
    }
    if (!mine) {
        r.acc.push_back(Access{t, e, g_cur_seq, g_cur_name, {}, {}});
        mine = &r.acc.back();
    }
    std::vector<Iv> &v = write ? mine->wr : mine->rd;
    uint64_t &vlo = write ? mine->wlo : mine->rlo, &vhi = write ? mine->whi : mine->rhi;
    vlo = std::min(vlo, lo);
    vhi = std::max(vhi, hi);
    if (!v.empty() && lo <= v.back().hi && v.back().lo <= hi) {  // a table's entries one after the other stay one interval
        v.back().lo = std::min(v.back().lo, lo);
        v.back().hi = std::max(v.back().hi, hi);
        return;
    }
    v.push_back(Iv{lo, hi});
}
bool touch(std::map<uintptr_t, Range> &m, const void *p, uint64_t bytes, int mode /* 0 check, 1 read, 2 write */, const char *what)
{
    Range *r = find_in(m, p);
    if (!r) {
        fake::violation("op %llu '%s': %s = %p lies in no live device block", (unsigned long long)g_cur_seq, g_cur_name, what, p);
        return false;
    }
    const uint64_t lo = (uintptr_t)p - r->base;
    if (bytes > r->size - lo) {
        fake::violation("op %llu '%s': %s = block #%llu + %llu, %llu bytes, runs %llu bytes past the block's %zu",
                        (unsigned long long)g_cur_seq, g_cur_name, what, (unsigned long long)r->id, (unsigned long long)lo,
                        (unsigned long long)bytes, (unsigned long long)(lo + bytes - r->size), r->size);
        return false;
    }
    if (mode) note(*r, lo, lo + bytes, mode == 2, what);
    return true;
}
// the host side of a copy: inside a page-locked range it is noted there; pageable otherwise
void host_side(const void *p, uint64_t bytes, bool write, bool async, const char *what)
{
    Range *r = find_in(g_pinned, p);
    if (r && (uintptr_t)p + bytes <= r->base + r->size) {
        note(*r, (uintptr_t)p - r->base, (uintptr_t)p - r->base + bytes, write, what);
        return;
    }
    if (async && write && bytes)
        g_pending.push_back(Pending{(uintptr_t)p, (uintptr_t)p + bytes, g_cur->thread, at(g_cur->clock, g_cur->thread), g_cur_seq});
}
hipError_t copy(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s, bool async)
{
    Stream *st = async ? stream_of(s, "hipMemcpyAsync") : &g_null;
    fake::op_begin((hipStream_t)(st == &g_null ? nullptr : st), async ? "hipMemcpyAsync" : "hipMemcpy");
    ++g_copies;
    bool dd = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
    bool sd = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    if (kind == hipMemcpyDefault) {
        dd = find_in(g_dev, dst) != nullptr;
        sd = find_in(g_dev, src) != nullptr;
    }
    bool ok = true;
    if (dd) ok = touch(g_dev, dst, n, 2, "copy destination") && ok;
    else host_side(dst, n, true, async, "copy destination (host)");
    if (sd) ok = touch(g_dev, src, n, 1, "copy source") && ok;
    else host_side(src, n, false, async, "copy source (host)");
    if (!ok) return g_last = hipErrorInvalidValue;  // (the bytes stay where they are: the sanitizer would stop the run)
    if (n) memcpy(dst, src, n);
    if (!async) host_join(g_null.clock);
    return hipSuccess;
}
hipError_t fill(void *dst, int v, size_t n, hipStream_t s, bool async)
{
    Stream *st = async ? stream_of(s, "hipMemsetAsync") : &g_null;
    fake::op_begin((hipStream_t)(st == &g_null ? nullptr : st), async ? "hipMemsetAsync" : "hipMemset");
    if (!touch(g_dev, dst, n, 2, "memset destination")) return g_last = hipErrorInvalidValue;
    if (n) memset(dst, v, n);
    if (!async) host_join(g_null.clock);
    return hipSuccess;
}
bool joined_into_host(const Range &r, const char *call)
{
    for (const Access &a : r.acc)
        if (!ordered_before_host(a)) {
            fake::violation("%s of %s #%llu (%zu bytes) with op %llu '%s' on stream %u in flight (not joined into the host)", call,
                            kind_name(r.kind), (unsigned long long)r.id, r.size, (unsigned long long)a.seq, a.op, a.thread);
            return false;
        }
    return true;
}
}  // namespace

namespace fake {
uint64_t n_launches = 0;
void violation(const char *fmt, ...)
{
    ++g_viol;
    fprintf(stderr, "fake_hip: VIOLATION: ");
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
uint64_t violations() { return g_viol; }
void op_begin(hipStream_t s, const char *name)
{
    Stream *st = stream_of(s, name);
    enqueue(st);
    if (st->clock.size() <= st->thread) st->clock.resize(st->thread + 1, 0);
    ++st->clock[st->thread];
    g_cur = st;
    g_cur_name = name;
    g_cur_seq = ++g_seq;
}
bool in_block(const void *p, uint64_t bytes, const char *what) { return touch(g_dev, p, bytes, 0, what); }
bool dev_read(const void *p, uint64_t bytes, const char *what) { return touch(g_dev, p, bytes, 1, what); }
bool dev_write(const void *p, uint64_t bytes, const char *what) { return touch(g_dev, p, bytes, 2, what); }
bool dev_read_block(const void *p, const char *what)
{
    Range *r = find_in(g_dev, p);
    return touch(g_dev, r ? (const void *)r->base : p, r ? r->size : 0, 1, what);
}
bool dev_write_block(const void *p, const char *what)
{
    Range *r = find_in(g_dev, p);
    return touch(g_dev, r ? (const void *)r->base : p, r ? r->size : 0, 2, what);
}
bool pinned_read(const void *p, uint64_t bytes, const char *what)
{
    Range *r = find_in(g_pinned, p);
    if (!r || (uintptr_t)p + bytes > r->base + r->size) {
        violation("op %llu '%s': %s = %p, %llu bytes, is not inside one page-locked range", (unsigned long long)g_cur_seq, g_cur_name, what,
                  p, (unsigned long long)bytes);
        return false;
    }
    note(*r, (uintptr_t)p - r->base, (uintptr_t)p - r->base + bytes, false, what);
    return true;
}
bool quiescent(const void *p, uint64_t bytes, const char *what)
{
    auto it = g_dev.find((uintptr_t)p);
    if (it == g_dev.end() || it->second.size != bytes) {
        violation("%s: %p (%llu bytes) is no live device block of that size (dangling or mis-sized entry)", what, p, (unsigned long long)bytes);
        return false;
    }
    for (const Access &a : it->second.acc)
        if (!ordered_before_host(a)) {
            violation("%s: device block #%llu (%zu bytes) with op %llu '%s' on stream %u not joined into the host", what,
                      (unsigned long long)it->second.id, it->second.size, (unsigned long long)a.seq, a.op, a.thread);
            return false;
        }
    return true;
}
uint64_t room(const void *p)
{
    Range *r = find_in(g_dev, p);
    return r ? r->base + r->size - (uintptr_t)p : 0;
}
void host_consumes(const void *p, uint64_t bytes, const char *what)
{
    const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
    for (const Pending &q : g_pending)
        if (q.lo < hi && lo < q.hi && at(g_host, q.thread) < q.epoch)
            violation("%s handed to the host as complete while op %llu 'hipMemcpyAsync' (device to pageable host memory) on stream %u "
                      "is not joined into the host", what, (unsigned long long)q.seq, q.thread);
}
uint64_t finish(const char *scenario)
{
    for (auto &kv : g_dev) violation("end of scenario: device block #%llu (%zu bytes) was never freed", (unsigned long long)kv.second.id, kv.second.size);
    for (auto &kv : g_pinned)
        violation("end of scenario: %s #%llu (%zu bytes) remains", kind_name(kv.second.kind), (unsigned long long)kv.second.id, kv.second.size);
    if (!g_streams.empty()) violation("end of scenario: %zu streams remain", g_streams.size());
    if (!g_events.empty()) violation("end of scenario: %zu events remain", g_events.size());
    // what remains is released, so that the sanitizer's leak check speaks of the product's blocks only
    for (auto &kv : g_dev) free((void *)kv.second.base);
    for (auto &kv : g_pinned)
        if (kv.second.kind == 1) free((void *)kv.second.base);
    for (Stream *s : g_streams) delete s;
    for (Event *e : g_events) delete e;
    g_dev.clear(); g_pinned.clear(); g_streams.clear(); g_events.clear();
    printf("fake_hip: scenario=%s ops=%llu launches=%llu copies=%llu mallocs=%llu host_joins=%llu violations=%llu\n", scenario,
           (unsigned long long)g_seq, (unsigned long long)n_launches, (unsigned long long)g_copies, (unsigned long long)g_mallocs,
           (unsigned long long)g_syncs, (unsigned long long)g_viol);
    return g_viol;
}
}  // namespace fake

// ------------------------------------------------------------------------------------------
// the 27 functions
// ------------------------------------------------------------------------------------------
hipError_t hipGetDeviceCount(int *count) { *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : (g_last = hipErrorInvalidDevice); }
const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument (stand-in)";
    case hipErrorOutOfMemory: return "out of memory (stand-in)";
    case hipErrorNotReady: return "device not ready (stand-in)";
    default: return "error (stand-in)";
    }
}
hipError_t hipGetLastError(void)
{
    const hipError_t e = g_last;
    g_last = hipSuccess;
    return e;
}
hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b)
{
    *free_b = (size_t)64 << 30;
    *total_b = (size_t)288 << 30;
    return hipSuccess;
}

hipError_t hipMalloc(void **ptr, size_t size)
{
    if (!ptr) return g_last = hipErrorInvalidValue;
    *ptr = nullptr;
    if (size == 0) return hipSuccess;
    void *p = malloc(size);
    if (!p) return g_last = hipErrorOutOfMemory;
    memset(p, 0xEE, size);  // (what a kernel stand-in reads before anything wrote it is garbage that fails its checks)
    ++g_mallocs;
    g_dev[(uintptr_t)p] = Range{(uintptr_t)p, size, 0, g_next_id++, {}};
    *ptr = p;
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    if (!p) return hipSuccess;
    auto it = g_dev.find((uintptr_t)p);
    if (it == g_dev.end()) {
        Range *r = find_in(g_dev, p);
        if (r) fake::violation("hipFree(%p): inside device block #%llu, not its base", p, (unsigned long long)r->id);
        else fake::violation("hipFree(%p): no live device block (unknown or already freed)", p);
        return g_last = hipErrorInvalidValue;
    }
    host_join_all();  // hipFree synchronises the device (the product relies on it: "as hipFree would")
    free(p);
    g_dev.erase(it);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int)
{
    if (!ptr || !size) return g_last = hipErrorInvalidValue;
    void *p = malloc(size);
    if (!p) return g_last = hipErrorOutOfMemory;
    g_pinned[(uintptr_t)p] = Range{(uintptr_t)p, size, 1, g_next_id++, {}};
    *ptr = p;
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    if (!p) return hipSuccess;
    auto it = g_pinned.find((uintptr_t)p);
    if (it == g_pinned.end() || it->second.kind != 1) {
        fake::violation("hipHostFree(%p): no hipHostMalloc range", p);
        return g_last = hipErrorInvalidValue;
    }
    joined_into_host(it->second, "hipHostFree");
    free(p);
    g_pinned.erase(it);
    return hipSuccess;
}
hipError_t hipHostRegister(void *p, size_t size, unsigned int)
{
    if (!p || !size) return g_last = hipErrorInvalidValue;
    const uintptr_t lo = (uintptr_t)p, hi = lo + size;
    for (auto &kv : g_pinned)
        if (kv.second.base < hi && lo < kv.second.base + kv.second.size) {
            fake::violation("hipHostRegister(%p, %zu): overlaps %s #%llu (double registration)", p, size, kind_name(kv.second.kind),
                            (unsigned long long)kv.second.id);
            return g_last = hipErrorHostMemoryAlreadyRegistered;
        }
    g_pinned[lo] = Range{lo, size, 2, g_next_id++, {}};
    return hipSuccess;
}
hipError_t hipHostUnregister(void *p)
{
    auto it = g_pinned.find((uintptr_t)p);
    if (it == g_pinned.end() || it->second.kind != 2) {
        fake::violation("hipHostUnregister(%p): no registered range", p);
        return g_last = hipErrorHostMemoryNotRegistered;
    }
    joined_into_host(it->second, "hipHostUnregister");
    g_pinned.erase(it);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p)
{
    memset(a, 0, sizeof(*a));
    Range *r = find_in(g_pinned, p);
    if (r && (uintptr_t)p < r->base + r->size) {
        a->type = hipMemoryTypeHost;
        a->hostPointer = (void *)p;
        a->devicePointer = (void *)p;
        return hipSuccess;
    }
    r = find_in(g_dev, p);
    if (r && (uintptr_t)p < r->base + r->size) {
        a->type = hipMemoryTypeDevice;
        a->devicePointer = (void *)p;
        return hipSuccess;
    }
    return g_last = hipErrorInvalidValue;  // pageable memory: an error the callers take as an answer
}

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) { return copy(dst, src, n, kind, nullptr, false); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s) { return copy(dst, src, n, kind, s, true); }
hipError_t hipMemset(void *dst, int v, size_t n) { return fill(dst, v, n, nullptr, false); }
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) { return fill(dst, v, n, s, true); }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags)
{
    if (flags != hipStreamNonBlocking) fake::violation("hipStreamCreateWithFlags(%u): the library creates non-blocking streams only", flags);
    Stream *st = new Stream{g_next_thread++, Clock()};
    g_streams.insert(st);
    *s = (hipStream_t)st;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    Stream *st = (Stream *)s;
    if (!s || !g_streams.count(st)) {
        fake::violation("hipStreamDestroy(%p): no live stream", (void *)s);
        return g_last = hipErrorInvalidHandle;
    }
    // (the real call returns at once and lets queued work finish: no join; the stream's accesses keep their epochs)
    g_streams.erase(st);
    delete st;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    host_join(stream_of(s, "hipStreamSynchronize")->clock);
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t s)
{
    Stream *st = stream_of(s, "hipStreamQuery");
    if (at(g_host, st->thread) < at(st->clock, st->thread)) return g_last = hipErrorNotReady;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void)
{
    host_join_all();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int)
{
    Event *ev = new Event();
    ev->id = g_next_id++;
    g_events.insert(ev);
    *e = (hipEvent_t)ev;
    return hipSuccess;
}
static Event *event_of(hipEvent_t e, const char *call)
{
    Event *ev = (Event *)e;
    if (!e || !g_events.count(ev)) {
        fake::violation("%s: event %p is no live event", call, (void *)e);
        return nullptr;
    }
    return ev;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    Event *ev = event_of(e, "hipEventDestroy");
    if (!ev) return g_last = hipErrorInvalidHandle;
    g_events.erase(ev);
    delete ev;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    Event *ev = event_of(e, "hipEventRecord");
    if (!ev) return g_last = hipErrorInvalidHandle;
    Stream *st = stream_of(s, "hipEventRecord");
    enqueue(st);
    ev->clock = st->clock;
    ev->recorded = true;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    Event *ev = event_of(e, "hipEventSynchronize");
    if (!ev) return g_last = hipErrorInvalidHandle;
    if (ev->recorded) host_join(ev->clock);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    Event *ea = event_of(a, "hipEventElapsedTime"), *eb = event_of(b, "hipEventElapsedTime");
    if (!ea || !eb) return g_last = hipErrorInvalidHandle;
    if (!ea->recorded || !eb->recorded) return g_last = hipErrorInvalidHandle;
    *ms = 0.001f;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    Event *ev = event_of(e, "hipStreamWaitEvent");
    if (!ev) return g_last = hipErrorInvalidHandle;
    Stream *st = stream_of(s, "hipStreamWaitEvent");
    enqueue(st);
    if (ev->recorded) join(st->clock, ev->clock);
    return hipSuccess;
}
