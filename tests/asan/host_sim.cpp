// tests/asan/host_sim.cpp -- runs the host path of libatsc_hip.so (atsc_host.cpp, atsc_windows.cpp, atsc_stream.cpp)
// on the CPU, under AddressSanitizer + UBSan, against the checking stand-in runtime (fake_hip.cpp) and the launcher
// stand-ins (sim_kernels.cpp): the pool, the plan cache, compress and decode in parts, the page-locked staging, the
// per-query slots of a decode plan, the piece cutter and every task table, scenario by scenario.  A scenario runs in
// a process of its own (several switches of the library are read once per process); tests/test_host_sim.py writes the
// corpus -- valid streams from the oracle -- and runs them all.
// Usage: host_sim <scenario> <corpus dir>     scenarios: selfcheck compress decode faulted pipelined windows
// Exit status 0: the scenario ran, the stand-in counted no violation and nothing was left behind.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "fake_hip.h"

#include "../../atsc_amd/csrc/atsc_host_private.h"

static const float ME5 = 5.0f / 100.0f;
static atsc_ctx *g_ctx = nullptr;

#define OK(call)                                                                                                       \
    do {                                                                                                               \
        const int rc__ = (call);                                                                                       \
        if (rc__ != ATSC_OK) {                                                                                         \
            fprintf(stderr, "host_sim: %s:%d: %s = %d (%s)\n", __FILE__, __LINE__, #call, rc__,                        \
                    g_ctx ? atsc_ctx_last_error(g_ctx) : "");                                                          \
            exit(3);                                                                                                   \
        }                                                                                                              \
    } while (0)
#define EXPECT(cond)                                                                                                   \
    do {                                                                                                               \
        if (!(cond)) { fprintf(stderr, "host_sim: %s:%d: expected %s\n", __FILE__, __LINE__, #cond); exit(3); }      \
    } while (0)
#define HIP(call) EXPECT((call) == hipSuccess)

// what the pool promises after every call that returned: its entries are live blocks of the recorded size, and a block
// on the free list has no work in flight
static void check_pool(atsc_ctx *ctx, const char *after)
{
    char what[128];
    for (auto &b : ctx->pool_free_list) {
        snprintf(what, sizeof what, "pool free list after %s", after);
        fake::quiescent(b.first, b.second, what);
    }
    for (auto &b : ctx->pool_live) {
        snprintf(what, sizeof what, "pool live entry after %s", after);
        if (fake::room(b.first) != b.second) fake::violation("%s: %p is no live device block of %zu bytes", what, b.first, b.second);
    }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static std::vector<double> series(uint64_t n, int seed)
{
    std::vector<double> x(n);
    for (uint64_t i = 0; i < n; ++i) x[i] = 100.0 + 10.0 * std::sin(0.01 * (double)i + seed) + (double)((i * 7 + (uint64_t)seed) % 13);
    return x;
}
static std::vector<uint64_t> offsets(const std::vector<uint32_t> &lens)
{
    std::vector<uint64_t> off(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    return off;
}
static uint64_t body_bound(const std::vector<uint64_t> &off)
{
    uint64_t b = 0;
    for (size_t i = 0; i + 1 < off.size(); ++i) b += atsc_payload_bound_bytes(off[i + 1] - off[i]) + 16;
    return b;
}

// a .bro file of the corpus: rec() are its records (no count in front), counted() the same with the count
struct Bro {
    std::vector<uint8_t> file;
    uint64_t body_off = 0, nf = 0, ns = 0;
    const uint8_t *rec() const { return file.data() + body_off; }
    uint64_t rec_len() const { return file.size() - body_off; }
    const uint8_t *counted() const { return file.data() + 9; }
    uint64_t counted_len() const { return file.size() - 9; }
};
static std::string g_corpus;
static Bro load(const char *name)
{
    Bro b;
    const std::string path = g_corpus + "/" + name;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { perror(path.c_str()); exit(2); }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) b.file.insert(b.file.end(), buf, buf + got);
    fclose(f);
    uint64_t nf2 = 0;
    OK(atsc_bro_open(b.file.data(), b.file.size(), &b.body_off, &b.nf));
    OK(atsc_bro_scan(b.file.data(), b.file.size(), &nf2, &b.ns));
    EXPECT(nf2 == b.nf);
    return b;
}

// ------------------------------------------------------------------------------------------
// self-check of the stand-in: misuse through its own API, each case counted once
// ------------------------------------------------------------------------------------------
static int selfcheck()
{
    int counted = 0;
    auto step = [&](const char *what, uint64_t before) {
        const bool ok = fake::violations() == before + 1;
        printf("selfcheck: %-44s %s\n", what, ok ? "counted" : "NOT counted once");
        counted += ok;
    };
    void *a = nullptr, *b = nullptr;
    HIP(hipMalloc(&a, 256));
    HIP(hipMalloc(&b, 256));
    uint64_t v = fake::violations();
    HIP(hipFree(a));
    (void)hipFree(a);
    step("a double free", v);

    unsigned char host[512] = {};
    v = fake::violations();
    (void)hipMemcpy(b, host, 257, hipMemcpyHostToDevice);
    step("a copy one byte past a block", v);

    hipStream_t s1, s2;
    HIP(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    void *pinned = nullptr;
    HIP(hipHostMalloc(&pinned, 512, hipHostMallocDefault));
    v = fake::violations();
    HIP(hipMemcpyAsync(pinned, b, 128, hipMemcpyDeviceToHost, s1));   // s1 reads b
    HIP(hipMemsetAsync(b, 0, 64, s2));                                  // s2 writes b: no order with s1
    step("an unordered write after a read on two streams", v);
    HIP(hipDeviceSynchronize());
    // the same with an event between them is in order
    hipEvent_t ev;
    HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    v = fake::violations();
    HIP(hipMemcpyAsync(pinned, b, 128, hipMemcpyDeviceToHost, s1));
    HIP(hipEventRecord(ev, s1));
    HIP(hipStreamWaitEvent(s2, ev, 0));
    HIP(hipMemsetAsync(b, 0, 64, s2));
    EXPECT(fake::violations() == v);
    HIP(hipDeviceSynchronize());

    static unsigned char reg[4096];
    HIP(hipHostRegister(reg, sizeof reg, hipHostRegisterDefault));
    v = fake::violations();
    HIP(hipMemcpyAsync(b, reg, 256, hipMemcpyHostToDevice, s1));
    (void)hipHostUnregister(reg);
    step("an unregister with a copy in flight", v);

    // a device-to-host Async copy into pageable memory handed on without a join, and with one
    v = fake::violations();
    HIP(hipMemcpyAsync(host, b, 64, hipMemcpyDeviceToHost, s1));
    fake::host_consumes(host, 64, "selfcheck's buffer");
    step("a pageable result handed on before its copy joined", v);
    HIP(hipStreamSynchronize(s1));
    v = fake::violations();
    fake::host_consumes(host, 64, "selfcheck's buffer");
    EXPECT(fake::violations() == v);

    HIP(hipEventDestroy(ev));
    HIP(hipStreamDestroy(s1));
    HIP(hipStreamDestroy(s2));
    HIP(hipHostFree(pinned));
    HIP(hipFree(b));
    const uint64_t total = fake::finish("selfcheck");
    printf("selfcheck: %d of 5 misuses counted, %llu violations in all\n", counted, (unsigned long long)total);
    return counted == 5 && total == 5 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------
// compress
// ------------------------------------------------------------------------------------------
struct Compressed {
    uint64_t total = 0;
    std::vector<uint64_t> rec_off;
};
static Compressed compress(atsc_ctx *ctx, const double *x, const std::vector<uint64_t> &off, int comp, int bounded, int level,
                           uint8_t *body, uint64_t cap, int expect = ATSC_OK)
{
    const uint64_t nf = off.size() - 1;
    Compressed c;
    c.rec_off.assign(nf + 1, ~0ull);
    std::vector<uint8_t> chosen(nf);
    std::vector<double> err(nf);
    const int rc = atsc_compress_frames(ctx, x, off.data(), nf, comp, bounded, ME5, level, body, cap, &c.total, c.rec_off.data(),
                                        chosen.data(), err.data());
    if (rc != expect) {
        fprintf(stderr, "host_sim: atsc_compress_frames = %d, expected %d (%s)\n", rc, expect, atsc_ctx_last_error(ctx));
        exit(3);
    }
    check_pool(ctx, "atsc_compress_frames");
    if (rc == ATSC_OK) {
        fake::host_consumes(body, c.total, "atsc_compress_frames' records");
        EXPECT(c.rec_off[0] == 0 && c.rec_off[nf] == c.total);
        for (uint64_t f = 0; f < nf; ++f) EXPECT(c.rec_off[f] < c.rec_off[f + 1]);
    }
    return c;
}
static void compress_round(atsc_ctx *ctx)
{
    // 16384 frames of 256 samples: 2^22 samples, the least that gives two parts
    {
        const uint64_t n = 1ull << 22;
        std::vector<double> x = series(n, 1);
        const std::vector<uint64_t> off = offsets(std::vector<uint32_t>(16384, 256));
        const uint64_t bound = body_bound(off);
        std::vector<uint8_t> body(bound);
        const Compressed a = compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
        // a capacity one byte short: ATSC_E_CAPACITY, and no block lost (check_pool; the leak check at the end)
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), a.total - 1, ATSC_E_CAPACITY);
        // the same from registered buffers: the records come back part by part
        OK(atsc_host_register(x.data(), n * sizeof(double)));
        OK(atsc_host_register(body.data(), bound));
        const Compressed b = compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
        EXPECT(b.total == a.total && b.rec_off == a.rec_off);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), a.total - 1, ATSC_E_CAPACITY);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), a.rec_off[9000], ATSC_E_CAPACITY);  // short by a part
        OK(atsc_host_unregister(body.data()));
        OK(atsc_host_unregister(x.data()));
    }
    // mixed lengths: every class, the large tier among them; the trial sub-plans and the unpadded transform's
    {
        std::vector<uint32_t> lens;
        for (int r = 0; r < 6; ++r)
            for (uint32_t l : {12u, 64u, 100u, 127u, 128u, 256u, 511u, 1000u, 2048u, 4096u, 4097u, 5000u, 16384u}) lens.push_back(l + (uint32_t)r);
        const std::vector<uint64_t> off = offsets(lens);
        std::vector<double> x = series(off.back(), 2);
        const uint64_t bound = body_bound(off);
        std::vector<uint8_t> body(bound);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 3, body.data(), bound);
        (void)compress(ctx, x.data(), off, ATSC_FFT, 0, 0, body.data(), bound);
        (void)compress(ctx, x.data(), off, ATSC_RLE, 0, 0, body.data(), bound);
    }
    // 64 frames of 8192 samples (two parts of 32) and 3 of 131072
    for (auto shape : {std::pair<uint32_t, uint32_t>(64, 8192), std::pair<uint32_t, uint32_t>(3, 131072)}) {
        const std::vector<uint64_t> off = offsets(std::vector<uint32_t>(shape.first, shape.second));
        std::vector<double> x = series(off.back(), 3);
        const uint64_t bound = body_bound(off);
        std::vector<uint8_t> body(bound);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
        OK(atsc_host_register(x.data(), x.size() * sizeof(double)));
        OK(atsc_host_register(body.data(), bound));
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
        OK(atsc_host_unregister(body.data()));
        OK(atsc_host_unregister(x.data()));
    }
    // six distinct layouts in a row: the plan cache (four entries) evicts; then the first again
    for (int r = 0; r < 7; ++r) {
        const std::vector<uint64_t> off = offsets(std::vector<uint32_t>(10 + (r % 6), 300 + 100 * (uint32_t)(r % 6)));
        std::vector<double> x = series(off.back(), 4 + r);
        const uint64_t bound = body_bound(off);
        std::vector<uint8_t> body(bound);
        (void)compress(ctx, x.data(), off, ATSC_AUTO, 1, 0, body.data(), bound);
    }
}
static int scenario_compress()
{
    OK(atsc_ctx_create(&g_ctx, 0));
    compress_round(g_ctx);
    OK(atsc_ctx_trim(g_ctx));
    check_pool(g_ctx, "atsc_ctx_trim");
    EXPECT(g_ctx->pool_free_list.empty() && g_ctx->plan_cache.empty());
    atsc_release_caches();
    compress_round(g_ctx);
    EXPECT(!g_ctx->plan_cache.empty());
    atsc_ctx_destroy(g_ctx);  // with cached plans
    g_ctx = nullptr;
    atsc_release_caches();
    return 0;
}

// ------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------
static const char *SMALL_STREAMS[] = {"auto_12.bro", "fft_64.bro", "poly_256.bro", "idw_256.bro", "rle_1000.bro", "noop_256.bro",
                                      "constant_1000.bro", "auto_1000.bro", "large_16384.bro"};
static void decode_host(atsc_ctx *ctx, const Bro &b, bool registered, int expect = ATSC_OK, const uint8_t *rec = nullptr,
                        uint64_t rec_len = 0, uint64_t cap_short = 0)
{
    if (!rec) { rec = b.rec(); rec_len = b.rec_len(); }
    std::vector<double> out(b.ns + 1, -1.0);
    std::vector<uint8_t> bytes(rec, rec + rec_len);  // a heap copy of the exact length
    if (registered) {
        OK(atsc_host_register(out.data(), out.size() * sizeof(double)));
        OK(atsc_host_register(bytes.data(), bytes.size()));
    }
    uint64_t n = 0;
    const int rc = atsc_decompress_frames(ctx, bytes.data(), bytes.size(), 0, out.data(), b.ns - cap_short, &n);
    if (rc != expect) {
        fprintf(stderr, "host_sim: atsc_decompress_frames = %d, expected %d (%s)\n", rc, expect, atsc_ctx_last_error(ctx));
        exit(3);
    }
    check_pool(ctx, "atsc_decompress_frames");
    if (rc == ATSC_OK) {
        EXPECT(n == b.ns);
        fake::host_consumes(out.data(), n * sizeof(double), "atsc_decompress_frames' samples");
    } else {
        EXPECT(n == 0);
    }
    if (registered) {
        OK(atsc_host_unregister(bytes.data()));
        OK(atsc_host_unregister(out.data()));
    }
}
// the offset of the payload-length field of the last record that starts at or behind `from`
static uint64_t last_len_field(const Bro &b, uint64_t from, uint64_t *rec_start)
{
    uint64_t pos = 0, at = 0;
    const uint8_t *p = b.rec();
    while (pos < b.rec_len()) {
        atsc::HostRecord hr;
        const uint64_t start = pos;
        EXPECT(atsc::host_next_record(p, b.rec_len(), pos, hr));
        if (start >= from || pos >= b.rec_len()) {
            uint64_t q = start, v;
            for (int i = 0; i < 3; ++i) EXPECT(atsc::host_varint(p, b.rec_len(), q, v));
            at = q;
            *rec_start = start;
        }
    }
    return at;
}
static void decode_round(atsc_ctx *ctx)
{
    // pageable, one plan: every codec and tier; with the count in front; the allocating form
    for (const char *name : SMALL_STREAMS) {
        const Bro b = load(name);
        decode_host(ctx, b, false);
        std::vector<double> out(b.ns);
        uint64_t n = 0;
        OK(atsc_decompress_frames(ctx, b.counted(), b.counted_len(), 1, out.data(), out.size(), &n));
        EXPECT(n == b.ns);
        double *alloc = nullptr;
        OK(atsc_decompress_frames_alloc(ctx, b.rec(), b.rec_len(), 0, &alloc, &n));
        EXPECT(n == b.ns && alloc);
        atsc_free(alloc);
        check_pool(ctx, "atsc_decompress_frames_alloc");
        // a plan of the caller's and device buffers of the caller's, on a stream of the caller's
        atsc_dplan *dp = nullptr;
        OK(atsc_dplan_create(ctx, b.rec(), b.rec_len(), 0, &dp));
        void *d_body = nullptr, *d_out = nullptr;
        hipStream_t s;
        HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP(hipMalloc(&d_body, b.rec_len()));
        HIP(hipMalloc(&d_out, b.ns * sizeof(double)));
        HIP(hipMemcpyAsync(d_body, b.rec(), b.rec_len(), hipMemcpyHostToDevice, s));
        OK(atsc_decompress_plan_dev(ctx, dp, (const uint8_t *)d_body, (double *)d_out, s));
        HIP(hipMemcpyAsync(out.data(), d_out, b.ns * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP(hipStreamSynchronize(s));
        fake::host_consumes(out.data(), b.ns * sizeof(double), "the caller's samples");
        atsc_dplan_destroy(dp);
        HIP(hipFree(d_body));
        HIP(hipFree(d_out));
        HIP(hipStreamDestroy(s));
    }
    // registered: the parts form (at least 2^20 record bytes; a record longer than a part's stride)
    for (const char *name : {"noop3.bro", "rle5.bro"}) {
        const Bro b = load(name);
        EXPECT(b.rec_len() >= (1u << 20));
        decode_host(ctx, b, false);
        decode_host(ctx, b, true);
        // a later part with a broken length; a truncated tail; a destination one sample short: every error path returns
        // every block (check_pool, the leak check), and the same context then decodes the intact stream
        uint64_t start = 0;
        const uint64_t at = last_len_field(b, b.rec_len() / 2, &start);
        std::vector<uint8_t> bad(b.rec(), b.rec() + b.rec_len());
        EXPECT(bad[at] >= 251);
        for (unsigned i = 1; i <= (bad[at] == 251 ? 2u : bad[at] == 252 ? 4u : 8u); ++i) bad[at + i] = 0xFF;
        decode_host(ctx, b, true, ATSC_E_FORMAT, bad.data(), bad.size());
        decode_host(ctx, b, false, ATSC_E_FORMAT, bad.data(), bad.size());
        decode_host(ctx, b, true, ATSC_E_FORMAT, b.rec(), b.rec_len() - 100);
        decode_host(ctx, b, true, ATSC_E_CAPACITY, nullptr, 0, 1);
        decode_host(ctx, b, false, ATSC_E_CAPACITY, nullptr, 0, 1);
        decode_host(ctx, b, true);
    }
}
static int scenario_decode()
{
    OK(atsc_ctx_create(&g_ctx, 0));
    decode_round(g_ctx);
    atsc_ctx_destroy(g_ctx);
    g_ctx = nullptr;
    atsc_release_caches();
    return 0;
}

// ------------------------------------------------------------------------------------------
// the sequence of tests/test_gpu_parity.py::test_decode_in_parts_with_records_longer_than_a_part, behind the calls above
// in one process: per codec, a compress of 131072-sample frames, the pageable decode of the records, then the same
// decode into registered memory, with the register and unregister pairs of each round.  (The records the decodes walk
// are the oracle's: the compress stand-ins write offsets, not payloads.  The test's third codec, Fft, is compressed
// here and decoded from large_16384.bro, the corpus' large-tier Fft stream.)
// ------------------------------------------------------------------------------------------
static int scenario_faulted()
{
    OK(atsc_ctx_create(&g_ctx, 0));
    atsc_ctx *ctx = g_ctx;
    compress_round(ctx);
    decode_round(ctx);
    const struct { int comp; uint32_t nfr; const char *stream; } rounds[] = {
        {ATSC_NOOP, 3, "noop3.bro"}, {ATSC_RLE, 5, "rle5.bro"}, {ATSC_FFT, 4, "large_16384.bro"}};
    for (const auto &r : rounds) {
        const std::vector<uint64_t> off = offsets(std::vector<uint32_t>(r.nfr, 131072));
        std::vector<double> x = series(off.back(), 60);
        const uint64_t bound = body_bound(off);
        std::vector<uint8_t> body(bound);
        (void)compress(ctx, x.data(), off, r.comp, r.comp == ATSC_FFT, 0, body.data(), bound);
        const Bro b = load(r.stream);
        decode_host(ctx, b, false);  // ref = ctx.decompress_host(rec): a pageable destination, one plan
        decode_host(ctx, b, true);   // register dec and recarr, atsc_decompress_frames, unregister both
    }
    atsc_ctx_destroy(ctx);
    g_ctx = nullptr;
    atsc_release_caches();
    return 0;
}

// ------------------------------------------------------------------------------------------
// pipelined
// ------------------------------------------------------------------------------------------
struct OutSet {
    uint8_t *body;
    uint64_t *rec_off;
    uint8_t *chosen;
    double *err;
};
static void pipelined_plan(atsc_ctx *ctx, uint32_t nf, uint32_t F, int chains, bool adaptive)
{
    OK(atsc_ctx_set_chains(ctx, chains));
    OK(atsc_ctx_set_adaptive_order(ctx, adaptive ? 1 : 0));
    const std::vector<uint64_t> off = offsets(std::vector<uint32_t>(nf, F));
    const uint64_t n = off.back();
    atsc_plan *plan = nullptr;
    OK(atsc_plan_create(ctx, off.data(), nf, &plan));
    const uint64_t bound = atsc_plan_body_bound(plan);
    hipStream_t side;
    HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    double *buf = nullptr;
    HIP(hipMalloc((void **)&buf, n * sizeof(double)));
    OutSet o[8];
    for (auto &s : o) {
        HIP(hipMalloc((void **)&s.body, bound));
        HIP(hipMalloc((void **)&s.rec_off, (nf + 1) * sizeof(uint64_t)));
        HIP(hipMalloc((void **)&s.chosen, nf));
        HIP(hipMalloc((void **)&s.err, nf * sizeof(double)));
    }
    std::vector<double> x = series(n, 5);
    std::vector<uint64_t> h_off(nf + 1);
    // 24 calls over eight output sets through ONE input buffer, refilled behind atsc_plan_input_release; a plain call
    // in the middle; the caller reuses an output set only behind an atsc_plan_join
    for (int b = 0; b < 24; ++b) {
        if (b % 8 == 0) OK(atsc_plan_join(ctx, plan, side));
        OK(atsc_plan_input_release(ctx, plan, side));
        HIP(hipMemcpyAsync(buf, x.data(), n * sizeof(double), hipMemcpyHostToDevice, side));
        OutSet &s = o[b % 8];
        if (b == 12)
            OK(atsc_compress_plan_dev(ctx, plan, buf, ATSC_AUTO, 1, ME5, 0, s.body, bound, s.rec_off, s.chosen, s.err, side));
        else
            OK(atsc_compress_plan_dev_pipelined(ctx, plan, buf, b == 5 ? ATSC_FFT : ATSC_AUTO, b == 5 ? 0 : 1, ME5, b == 7 ? 3 : 0, s.body,
                                                bound, s.rec_off, s.chosen, s.err, side));
        check_pool(ctx, "atsc_compress_plan_dev_pipelined");
    }
    OK(atsc_plan_join(ctx, plan, side));
    for (auto &s : o) HIP(hipMemcpyAsync(h_off.data(), s.rec_off, (nf + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, side));
    HIP(hipStreamSynchronize(side));
    fake::host_consumes(h_off.data(), h_off.size() * 8, "the caller's offsets");
    EXPECT(h_off[0] == 0 && h_off[nf] > 0);
    atsc_plan_destroy(plan);
    check_pool(ctx, "atsc_plan_destroy");
    for (auto &s : o) { HIP(hipFree(s.body)); HIP(hipFree(s.rec_off)); HIP(hipFree(s.chosen)); HIP(hipFree(s.err)); }
    HIP(hipFree(buf));
    HIP(hipStreamDestroy(side));
}
static int scenario_pipelined()
{
    OK(atsc_ctx_create(&g_ctx, 0));
    for (int chains = 1; chains <= 4; ++chains) {
        pipelined_plan(g_ctx, 4096, 256, chains, chains >= 3);
        pipelined_plan(g_ctx, 12, 131072, chains, chains == 2);
        pipelined_plan(g_ctx, 300, 1000, chains, true);
    }
    // down again: a context that has run four chains and is set to one
    pipelined_plan(g_ctx, 4096, 256, 1, false);
    atsc_ctx_destroy(g_ctx);
    g_ctx = nullptr;
    return 0;
}

// ------------------------------------------------------------------------------------------
// windows
// ------------------------------------------------------------------------------------------
struct Windows {
    std::vector<uint64_t> begin, count;
    uint64_t n() const { return begin.size(); }
};
// nw windows inside [0, ns): scattered short ones, empty ones, and (whole) one over everything
static Windows make_windows(uint64_t ns, uint64_t nw, uint64_t max_len, bool whole)
{
    Windows w;
    for (uint64_t i = 0; i < nw; ++i) {
        const uint64_t c = i % 7 == 3 ? 0 : 1 + rnd() % std::min(max_len, ns);
        w.begin.push_back(rnd() % (ns - c + 1));
        w.count.push_back(c);
    }
    if (whole) { w.begin.push_back(0); w.count.push_back(ns); }
    return w;
}
// a query kind: its device call into d_out, its host call and its stream call into out, and the bytes of a result
struct Kind {
    const char *name;
    std::function<size_t(const Windows &)> bytes;
    std::function<int(const atsc_dplan *const *, const uint8_t *const *, const Windows &, void *, void *)> dev;
    std::function<int(const Bro &, const Windows &, void *)> host;
    std::function<int(atsc_stream *const *, const Windows &, void *)> stream;
    uint32_t inputs = 1;       // plans / bodies / streams the call reads
    uint64_t max_len = ~0ull;  // the longest window the lists hold (the rolling's and across' results grow with it)
};
struct DevSide {
    std::vector<atsc_dplan *> dp;
    std::vector<uint8_t *> d_body;
};
static bool g_small_budget = false;
static void run_dev(atsc_ctx *ctx, const Kind &k, const DevSide &D, const Windows &w, hipStream_t s, bool destroy_after = false)
{
    const size_t bytes = std::max<size_t>(k.bytes(w), 8);
    void *d_out = nullptr;
    HIP(hipMalloc(&d_out, bytes));
    const int rc = k.dev(D.dp.data(), D.d_body.data(), w, d_out, s);
    // (a quantile's window must fit one piece: under a small budget the whole-stream window is refused, with every block back)
    if (rc == ATSC_E_CAPACITY && g_small_budget && !strcmp(k.name, "quantile")) {
        check_pool(ctx, k.name);
        HIP(hipFree(d_out));
        return;
    }
    if (rc != ATSC_OK) { fprintf(stderr, "host_sim: %s (device call) = %d (%s)\n", k.name, rc, atsc_ctx_last_error(ctx)); exit(3); }
    check_pool(ctx, k.name);
    if (destroy_after) return (void)hipFree(d_out);  // (the caller frees; hipFree waits for the device)
    std::vector<uint8_t> out(bytes);
    HIP(hipMemcpyAsync(out.data(), d_out, bytes, hipMemcpyDeviceToHost, s));
    HIP(hipStreamSynchronize(s));
    fake::host_consumes(out.data(), bytes, "the caller's result");
    HIP(hipFree(d_out));
}
static void run_host(atsc_ctx *ctx, const Kind &k, const Bro &b, const Windows &w)
{
    std::vector<uint8_t> out(std::max<size_t>(k.bytes(w), 8));
    const int rc = k.host(b, w, out.data());
    if (rc == ATSC_E_CAPACITY && g_small_budget && !strcmp(k.name, "quantile")) return check_pool(ctx, k.name);
    if (rc != ATSC_OK) { fprintf(stderr, "host_sim: %s (host call) = %d (%s)\n", k.name, rc, atsc_ctx_last_error(ctx)); exit(3); }
    check_pool(ctx, k.name);
    fake::host_consumes(out.data(), out.size(), "a host call's result");
}
static std::vector<Kind> kinds(atsc_ctx *ctx, uint32_t n_across)
{
    static const double q[3] = {0.1, 0.5, 0.99};
    static double edges[9];
    for (int i = 0; i < 9; ++i) edges[i] = 90.0 + 5.0 * i;
    const uint64_t RW = 300, RS = 7, AS = 3;  // rolling width and stride, across stride
    auto rolling_bytes = [=](const Windows &w, size_t rec) {
        size_t n = 0;
        for (uint64_t i = 0; i < w.n(); ++i) n += atsc_rolling_outputs(w.count[i], RW, RS);
        return n * rec;
    };
    auto across_bytes = [=](const Windows &w, size_t rec) {
        size_t n = 0;
        for (uint64_t i = 0; i < w.n(); ++i) n += atsc_across_outputs(w.count[i], AS);
        return n * rec;
    };
    std::vector<Kind> K;
#define B const_cast<uint64_t *>(w.begin.data())
#define C const_cast<uint64_t *>(w.count.data())
#define ONE(NAME, BYTES, DEVCALL, HOSTCALL, STREAMCALL)                                                                  \
    K.push_back(Kind{NAME, [=](const Windows &w) -> size_t { return BYTES; },                                            \
                     [=](const atsc_dplan *const *dp, const uint8_t *const *db, const Windows &w, void *out, void *s) { return DEVCALL; }, \
                     [=](const Bro &b, const Windows &w, void *out) { return HOSTCALL; },                                \
                     [=](atsc_stream *const *st, const Windows &w, void *out) { return STREAMCALL; }})
    ONE("aggregate", w.n() * sizeof(atsc_window_stats),
        atsc_aggregate_windows_dev(ctx, dp[0], db[0], w.n(), B, C, (atsc_window_stats *)out, s),
        atsc_aggregate_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, (atsc_window_stats *)out),
        atsc_stream_aggregate_windows(st[0], w.n(), B, C, (atsc_window_stats *)out));
    ONE("moments", w.n() * sizeof(atsc_window_moments),
        atsc_moments_windows_dev(ctx, dp[0], db[0], w.n(), B, C, (atsc_window_moments *)out, s),
        atsc_moments_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, (atsc_window_moments *)out),
        atsc_stream_moments_windows(st[0], w.n(), B, C, (atsc_window_moments *)out));
    ONE("delta", w.n() * sizeof(atsc_window_delta),
        atsc_delta_windows_dev(ctx, dp[0], db[0], w.n(), B, C, (atsc_window_delta *)out, s),
        atsc_delta_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, (atsc_window_delta *)out),
        atsc_stream_delta_windows(st[0], w.n(), B, C, (atsc_window_delta *)out));
    ONE("runs", w.n() * sizeof(atsc_window_runs),
        atsc_runs_windows_dev(ctx, dp[0], db[0], w.n(), B, C, ATSC_RUNS_GT, 105.0, (atsc_window_runs *)out, s),
        atsc_runs_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, ATSC_RUNS_GT, 105.0, (atsc_window_runs *)out),
        atsc_stream_runs_windows(st[0], w.n(), B, C, ATSC_RUNS_GT, 105.0, (atsc_window_runs *)out));
    ONE("extremes k=1", w.n() * ATSC_EXTREMES_BYTES(1),
        atsc_extremes_windows_dev(ctx, dp[0], db[0], w.n(), B, C, 1, out, s),
        atsc_extremes_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, 1, out),
        atsc_stream_extremes_windows(st[0], w.n(), B, C, 1, out));
    ONE("values k=32", w.n() * ATSC_VALUES_BYTES(32),
        atsc_values_windows_dev(ctx, dp[0], db[0], w.n(), B, C, 32, 100.0, out, s),
        atsc_values_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, 32, 100.0, out),
        atsc_stream_values_windows(st[0], w.n(), B, C, 32, 100.0, out));
    ONE("extremes k=16", w.n() * ATSC_EXTREMES_BYTES(16),
        atsc_extremes_windows_dev(ctx, dp[0], db[0], w.n(), B, C, 16, out, s),
        atsc_extremes_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, 16, out),
        atsc_stream_extremes_windows(st[0], w.n(), B, C, 16, out));
    ONE("select", ATSC_SELECT_BYTES(w.n(), 500),
        atsc_select_windows_dev(ctx, dp[0], db[0], w.n(), B, C, ATSC_RUNS_GE, 100.0, 500, out, s),
        atsc_select_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, ATSC_RUNS_GE, 100.0, 500, out),
        atsc_stream_select_windows(st[0], w.n(), B, C, ATSC_RUNS_GE, 100.0, 500, out));
    ONE("quantile", w.n() * 3 * sizeof(double),
        atsc_quantile_windows_dev(ctx, dp[0], db[0], w.n(), B, C, 3, q, ATSC_QUANTILE_LINEAR, (double *)out, s),
        atsc_quantile_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, 3, q, ATSC_QUANTILE_LINEAR, (double *)out),
        atsc_stream_quantile_windows(st[0], w.n(), B, C, 3, q, ATSC_QUANTILE_LINEAR, (double *)out));
    ONE("histogram", w.n() * (9 + 2) * sizeof(uint64_t),
        atsc_histogram_windows_dev(ctx, dp[0], db[0], w.n(), B, C, 9, edges, ATSC_HIST_LEFT_CLOSED, (uint64_t *)out, s),
        atsc_histogram_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, 9, edges, ATSC_HIST_LEFT_CLOSED, (uint64_t *)out),
        atsc_stream_histogram_windows(st[0], w.n(), B, C, 9, edges, ATSC_HIST_LEFT_CLOSED, (uint64_t *)out));
    ONE("rolling", rolling_bytes(w, sizeof(atsc_window_rolling)),
        atsc_rolling_windows_dev(ctx, dp[0], db[0], w.n(), B, C, RW, RS, (atsc_window_rolling *)out, s),
        atsc_rolling_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, RW, RS, (atsc_window_rolling *)out),
        atsc_stream_rolling_windows(st[0], w.n(), B, C, RW, RS, (atsc_window_rolling *)out));
    ONE("rolling delta", rolling_bytes(w, sizeof(atsc_window_delta)),
        atsc_rolling_delta_windows_dev(ctx, dp[0], db[0], w.n(), B, C, RW, RS, (atsc_window_delta *)out, s),
        atsc_rolling_delta_windows(ctx, b.rec(), b.rec_len(), 0, w.n(), B, C, RW, RS, (atsc_window_delta *)out),
        atsc_stream_rolling_delta_windows(st[0], w.n(), B, C, RW, RS, (atsc_window_delta *)out));
    ONE("pair", w.n() * sizeof(atsc_window_pair),
        atsc_pair_windows_dev(ctx, dp[0], db[0], dp[1], db[1], w.n(), B, C, (atsc_window_pair *)out, s),
        atsc_pair_windows(ctx, b.rec(), b.rec_len(), 0, b.rec(), b.rec_len(), 0, w.n(), B, C, (atsc_window_pair *)out),
        atsc_stream_pair_windows(st[0], st[1], w.n(), B, C, (atsc_window_pair *)out));
    K.back().inputs = 2;
    // the across calls read n_across streams: the same records under every pointer (each gets a plan of its own)
#define BODIES                                                                   \
    std::vector<const uint8_t *> bodies(n_across, b.rec());                      \
    std::vector<uint64_t> lens(n_across, b.rec_len());                           \
    std::vector<int> hc(n_across, 0)
    ONE("across", across_bytes(w, sizeof(atsc_across_record)),
        atsc_across_windows_dev(ctx, n_across, dp, db, w.n(), B, C, AS, (atsc_across_record *)out, s),
        ([&] { BODIES; return atsc_across_windows(ctx, n_across, bodies.data(), lens.data(), hc.data(), w.n(), B, C, AS, (atsc_across_record *)out); })(),
        atsc_stream_across_windows(st, n_across, w.n(), B, C, AS, (atsc_across_record *)out));
    K.back().inputs = n_across;
    ONE("across quantile", across_bytes(w, 3 * sizeof(double)),
        atsc_across_quantile_windows_dev(ctx, n_across, dp, db, w.n(), B, C, AS, 3, q, ATSC_QUANTILE_LINEAR, (double *)out, s),
        ([&] { BODIES; return atsc_across_quantile_windows(ctx, n_across, bodies.data(), lens.data(), hc.data(), w.n(), B, C, AS, 3, q, ATSC_QUANTILE_LINEAR, (double *)out); })(),
        atsc_stream_across_quantile_windows(st, n_across, w.n(), B, C, AS, 3, q, ATSC_QUANTILE_LINEAR, (double *)out));
    K.back().inputs = n_across;
    ONE("across extremes k=16", across_bytes(w, ATSC_EXTREMES_BYTES(std::min(16u, n_across))),
        atsc_across_extremes_windows_dev(ctx, n_across, dp, db, w.n(), B, C, AS, std::min(16u, n_across), out, s),
        ([&] { BODIES; return atsc_across_extremes_windows(ctx, n_across, bodies.data(), lens.data(), hc.data(), w.n(), B, C, AS, std::min(16u, n_across), out); })(),
        atsc_stream_across_extremes_windows(st, n_across, w.n(), B, C, AS, std::min(16u, n_across), out));
    K.back().inputs = n_across;
    ONE("across moments", across_bytes(w, sizeof(atsc_across_moments)),
        atsc_across_moments_windows_dev(ctx, n_across, dp, db, w.n(), B, C, AS, (atsc_across_moments *)out, s),
        ([&] { BODIES; return atsc_across_moments_windows(ctx, n_across, bodies.data(), lens.data(), hc.data(), w.n(), B, C, AS, (atsc_across_moments *)out); })(),
        atsc_stream_across_moments_windows(st, n_across, w.n(), B, C, AS, (atsc_across_moments *)out));
    K.back().inputs = n_across;
#undef ONE
#undef BODIES
#undef B
#undef C
    return K;
}
static const Kind &kind(const std::vector<Kind> &K, const char *name)
{
    for (const Kind &k : K)
        if (!strcmp(k.name, name)) return k;
    fprintf(stderr, "host_sim: no kind %s\n", name);
    exit(2);
}
static DevSide dev_side(atsc_ctx *ctx, const Bro &b, uint32_t n)
{
    DevSide D;
    for (uint32_t i = 0; i < n; ++i) {
        atsc_dplan *dp = nullptr;
        OK(atsc_dplan_create(ctx, b.rec(), b.rec_len(), 0, &dp));
        void *d = nullptr;
        HIP(hipMalloc(&d, b.rec_len()));
        HIP(hipMemcpy(d, b.rec(), b.rec_len(), hipMemcpyHostToDevice));
        D.dp.push_back(dp);
        D.d_body.push_back((uint8_t *)d);
    }
    return D;
}
static void free_dev_side(DevSide &D)
{
    for (atsc_dplan *dp : D.dp) atsc_dplan_destroy(dp);
    for (uint8_t *d : D.d_body) HIP(hipFree(d));
    D.dp.clear();
    D.d_body.clear();
}
// the window decode has a call shape of its own
static void window_decode(atsc_ctx *ctx, const Bro &b, const DevSide &D, hipStream_t s)
{
    for (uint64_t nw : {3ull, 40ull, 2ull, 120ull}) {
        const Windows w = make_windows(b.ns, nw, 3000, nw == 2);
        std::vector<uint64_t> out_off(w.n());
        uint64_t total = 0;
        for (uint64_t i = 0; i < w.n(); ++i) { out_off[i] = total; total += w.count[i]; }
        void *d_out = nullptr;
        HIP(hipMalloc(&d_out, std::max<uint64_t>(total, 1) * sizeof(double)));
        OK(atsc_decompress_windows_dev(ctx, D.dp[0], D.d_body[0], w.n(), w.begin.data(), w.count.data(), out_off.data(), (double *)d_out, s));
        check_pool(ctx, "atsc_decompress_windows_dev");
        HIP(hipStreamSynchronize(s));
        HIP(hipFree(d_out));
        std::vector<double> out(w.count[0] + 1);
        uint64_t n = 0;
        OK(atsc_decompress_window(ctx, b.rec(), b.rec_len(), 0, w.begin[0], w.count[0], out.data(), out.size(), &n));
        EXPECT(n == w.count[0]);
        fake::host_consumes(out.data(), n * sizeof(double), "atsc_decompress_window's samples");
    }
}
static void windows_on(atsc_ctx *ctx, const char *stream_name, uint32_t n_across, bool all_forms)
{
    const Bro b = load(stream_name);
    const std::vector<Kind> K = kinds(ctx, n_across);
    hipStream_t s;
    HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevSide D = dev_side(ctx, b, std::max(2u, n_across));
    std::vector<atsc_stream *> st(std::max(2u, n_across), nullptr);
    if (all_forms)
        for (auto &p : st) OK(atsc_stream_from_bytes(ctx, b.file.data(), b.file.size(), &p));
    // the default budget, then budgets that cut the whole-stream window into 2, 3 and 5 pieces (a piece is at least 32
    // tiles: 65536 samples); the window lists grow, shrink and grow again on one plan
    const uint64_t tiles = (b.ns + atsc::AGG_TILE - 1) / atsc::AGG_TILE;
    for (uint64_t pieces : {1ull, 2ull, 3ull, 5ull}) {
        const uint64_t piece_tiles = (tiles + pieces - 1) / pieces;
        if (pieces > 1 && piece_tiles < 32) continue;  // (the stream is too short to be cut that often)
        OK(atsc_ctx_set_aggregate_scratch(ctx, pieces == 1 ? 0 : piece_tiles * atsc::AGG_TILE * sizeof(double)));
        g_small_budget = pieces > 1;
        for (const Kind &k : K) {
            const bool wide = k.inputs > 2 || !strncmp(k.name, "rolling", 7);  // a result per position: shorter lists
            for (uint64_t nw : {3ull, 40ull, 2ull, 90ull}) {
                if (pieces > 1 && nw != 2) continue;
                const Windows w = make_windows(b.ns, wide ? std::min<uint64_t>(nw, 12) : nw, wide ? 5000 : 20000, nw == 2);
                run_dev(ctx, k, D, w, s);
                if (all_forms && (pieces == 1 || pieces == 3)) {
                    run_host(ctx, k, b, w);
                    if (nw <= 3) {
                        std::vector<uint8_t> out(std::max<size_t>(k.bytes(w), 8));
                        const int src = k.stream(st.data(), w, out.data());
                        EXPECT(src == ATSC_OK || (src == ATSC_E_CAPACITY && g_small_budget && !strcmp(k.name, "quantile")));
                        check_pool(ctx, k.name);
                    }
                }
            }
        }
    }
    OK(atsc_ctx_set_aggregate_scratch(ctx, 0));
    g_small_budget = false;
    if (all_forms) window_decode(ctx, b, D, s);
    // the kinds that share a slot of the plan, alternately and with changing sizes: reserve regrows under the other
    const char *shared[][3] = {{"extremes k=1", "values k=32", nullptr},
                               {"across quantile", "across extremes k=16", "across moments"},
                               {"rolling", "rolling delta", nullptr}};
    for (auto &grp : shared)
        for (uint64_t nw : {2ull, 30ull, 1ull, 60ull, 4ull})
            for (const char *name : grp) {
                if (!name) continue;
                const Kind &k = kind(K, name);
                const bool wide = k.inputs > 2 || !strncmp(k.name, "rolling", 7);
                run_dev(ctx, k, D, make_windows(b.ns, wide ? std::min<uint64_t>(nw, 10) : nw, wide ? 2000 + 500 * nw : 4000 * nw, nw == 1), s);
            }
    // a plan destroyed straight after an enqueue
    {
        DevSide D2 = dev_side(ctx, b, 2);
        run_dev(ctx, kind(K, "aggregate"), D2, make_windows(b.ns, 10, 9000, true), s, true);
        run_dev(ctx, kind(K, "rolling"), D2, make_windows(b.ns, 4, 9000, false), s, true);
        free_dev_side(D2);
    }
    for (auto p : st)
        if (p) atsc_stream_free(p);
    free_dev_side(D);
    HIP(hipStreamDestroy(s));
}
static int scenario_windows(const char *which)
{
    OK(atsc_ctx_create(&g_ctx, 0));
    if (!strcmp(which, "windows")) {
        windows_on(g_ctx, "win_small.bro", 2, true);
        windows_on(g_ctx, "auto_1000.bro", 3, true);
    } else if (!strcmp(which, "windows_large")) {
        windows_on(g_ctx, "noop3.bro", 2, false);
        windows_on(g_ctx, "large_16384.bro", 2, true);
    } else {  // windows_across64: N = 64, and a second context in the same process
        windows_on(g_ctx, "auto_1000.bro", 64, true);
        atsc_ctx *first = g_ctx, *second = nullptr;
        OK(atsc_ctx_create(&second, 0));
        const Bro b = load("win_small.bro");
        const std::vector<Kind> K1 = kinds(first, 2), K2 = kinds(second, 2);
        for (int r = 0; r < 3; ++r) {
            const Windows w = make_windows(b.ns, 5 + 10 * r, 30000, r == 1);
            g_ctx = first;
            run_host(first, kind(K1, "aggregate"), b, w);
            g_ctx = second;
            run_host(second, kind(K2, "aggregate"), b, w);
            run_host(second, kind(K2, "quantile"), b, w);
        }
        atsc_ctx_destroy(second);
        g_ctx = first;
    }
    atsc_ctx_destroy(g_ctx);
    g_ctx = nullptr;
    atsc_release_caches();
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: host_sim <scenario> <corpus dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_corpus = argv[2];
    if (sc == "selfcheck") return selfcheck();
    int rc;
    if (sc == "compress") rc = scenario_compress();
    else if (sc == "decode") rc = scenario_decode();
    else if (sc == "faulted") rc = scenario_faulted();
    else if (sc == "pipelined") rc = scenario_pipelined();
    else if (sc.rfind("windows", 0) == 0) rc = scenario_windows(sc.c_str());
    else { fprintf(stderr, "host_sim: unknown scenario %s\n", sc.c_str()); return 2; }
    const uint64_t v = fake::finish(sc.c_str());
    return rc || v ? 1 : 0;
}
