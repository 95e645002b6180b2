// csv-compressor -- command line front end over libatsc_hip.so with the reference's flags, file
// naming and exit behaviour (csv-compressor/src/main.rs:31-232): `timestamp,value` CSV in,
// .bro (+ .vsri index, + .wavbro samples) out; `-u` turns .bro + .vsri back into .wbro + .csv.
// Compression and decompression run on the GPU; the index and the text formats are host code.
//
//   csv-compressor [-o OUT] [-u [--from T0 --to T1 [--step S [--quantiles Q,Q,.. [--quantile-method M]]
//                  [--histogram E,E,..|LO:HI:N [--histogram-closed left|right]] [--moments] [--deltas] [--runs OP:LIMIT]
//                  [--extremes K] [--values K[:ABOVE]]] [--where OP:LIMIT] [--rolling W[:S] [--rolling-deltas] [--rolling-moments] [--rolling-runs OP:LIMIT]
//                  [--rolling-quantiles Q,Q,.. [--rolling-quantile-method M]] [--rolling-histogram E,E,..|LO:HI:N]]]]
//                  [--no-compression] [--output-vsri] [--output-wavbrro]
//                  [--output-csv] [--compressor auto|noop|fft|constant|polynomial|idw] [-e 0..50] [-c 0..6] <INPUT>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atsc_hip.h"
#include "atsc_cli_buckets.h"

namespace {

struct Args {
    std::string input, output;
    bool has_output = false, uncompress = false, no_compression = false;
    bool output_vsri = false, output_wavbrro = false, output_csv = false;
    int compressor = ATSC_AUTO;  // default_value = "auto" (main.rs:66)
    int error = 5;               // default_value_t = 5 (main.rs:73)
    int level = 0;
    bool window = false;  // --from / --to (with -u): only the samples whose indexed times lie in [t0, t1]
    int32_t t0 = 0, t1 = 0;
    int32_t step = 0;  // --step S (with --from / --to): summaries of S-second buckets into <out>.agg.csv
    BucketOptions q;   // with --step: the queries beside the summaries (atsc_cli_buckets.h)
};

constexpr int PANIC = 101;  // exit status of a Rust panic: every failure below is an expect()/panic!()

void usage()
{
    fprintf(stderr,
            "A Time-Series compressor utilizes Brro Compressor for CSV format\n\n"
            "Usage: csv-compressor [OPTIONS] <INPUT>\n\nOptions:\n"
            "  -o, --output <OUTPUT>          where the result will be stored\n"
            "  -u                             uncompress the input\n"
            "      --from <T0> --to <T1>      with -u: only the samples indexed at T0..=T1 (seconds since midnight)\n"
            "      --step <S>                 with --from/--to: count,min,max,sum,first,last of every S seconds to .agg.csv\n"
            "      --quantiles <Q,Q,..>       with --step: also the levels Q (0..1, at most 64) of every bucket\n"
            "      --quantile-method <M>      linear | lower | higher | nearest [default: linear]\n"
            "      --histogram <SPEC>         with --step: also every bucket's counts over the value bins of the edges\n"
            "                                 E,E,.. (ascending, at most 1024) or LO:HI:N (N equal bins over LO..HI)\n"
            "      --histogram-closed <SIDE>  left: E[k-1] <= v < E[k] | right: E[k-1] < v <= E[k] [default: left]\n"
            "      --moments                  with --step: also every bucket's mean, stdvar, stddev (population forms) and\n"
            "                                 least-squares slope (value units per SAMPLE, not per second) and intercept\n"
            "                                 (at its first sample)\n"
            "      --deltas                   with --step: also every bucket's steps from one sample to the next: counted\n"
            "                                 pairs, rises, falls (a counter's resets), the sums of the rises (up) and of the\n"
            "                                 falls (down), the counter increase (every fall a restart from zero), the total\n"
            "                                 variation (up + down) and the largest single rise and fall\n"
            "      --runs <OP:LIMIT>          with --step: also every bucket's samples with value OP LIMIT (OP: gt ge lt le eq\n"
            "                                 ne, e.g. gt:0.9) and their runs of adjacent samples, as the last columns: inside,\n"
            "                                 runs, longest (in samples), longest_at, first_at, last_at (the indexed times of\n"
            "                                 those samples, empty where there is none), head, tail (in samples), excess (the\n"
            "                                 sum of |value - LIMIT| over them)\n"
            "      --extremes <K>             with --step: also every bucket's K largest and K smallest samples (K: 1..16) and\n"
            "                                 when they happened, as the last columns: nans, max1, max1_at .. maxK, maxK_at,\n"
            "                                 min1, min1_at .. minK, minK_at (equal values earliest first; *_at the indexed\n"
            "                                 time of the sample; both cells empty where the bucket has fewer samples)\n"
            "      --values <K[:ABOVE]>       with --step: also every bucket's K smallest distinct values (K: 1..32) and how often\n"
            "                                 each occurs, as the last columns: nans, below, distinct, more, v1, n1 .. vK, nK\n"
            "                                 (values ascending, -0.0 counted with 0.0; with ABOVE only values greater than it\n"
            "                                 are listed and the others counted in below; more is 1 where the bucket has more\n"
            "                                 than K such values; both cells empty where it has fewer)\n"
            "      --where <OP:LIMIT>         with --from/--to, without --step: write the window's samples with value OP LIMIT\n"
            "                                 (as --runs) to .sel.csv instead of the .wbro and .csv: timestamp,value, one row\n"
            "                                 per selected sample, timestamp its indexed time\n"
            "      --rolling <W[:S]>          with --from/--to, without --step: write the window of W samples at every S-th\n"
            "                                 position of the window's samples (S: 1) to .roll.csv instead of the .wbro and\n"
            "                                 .csv: timestamp,count,min,max,sum,mean, timestamp the indexed time of the\n"
            "                                 position's LAST sample; mean is sum / count, empty where count is 0\n"
            "      --rolling-deltas           with --rolling: also every position's steps from one sample to the next, as the\n"
            "                                 last columns: pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase\n"
            "                                 (as --deltas; increase = up + after_falls, the counter increase of the window)\n"
            "      --rolling-moments          with --rolling: also every position's mean, spread and trend, as the last\n"
            "                                 columns: nonnan,avg,stdvar,stddev,slope,intercept (as --moments: population\n"
            "                                 forms, slope per sample, intercept at the position's first sample; all empty\n"
            "                                 where the window holds no sample)\n"
            "      --rolling-runs <OP:LIMIT>  with --rolling: also every position's samples with value OP LIMIT and their runs (as\n"
            "                                 --runs), behind those columns: samples,inside,runs,longest,longest_at,first_at,\n"
            "                                 last_at,head,tail,excess; the three positions count samples from the position's\n"
            "                                 first one and are empty where there is none (inside == samples: every sample of\n"
            "                                 the window meets the condition, an alert's `for:`)\n"
            "      --rolling-quantiles <Q,Q,..>  with --rolling, W at most 8192: also every position's levels (0 <= Q <= 1, as\n"
            "                                 --quantiles), as the last columns: one q<Q> per level as typed; NaN where the\n"
            "                                 window holds no sample\n"
            "      --rolling-quantile-method <M>  with --rolling-quantiles: linear (default), lower, higher or nearest\n"
            "      --rolling-histogram <SPEC> with --rolling: also every position's counts over the value bins of the edges\n"
            "                                 (SPEC and --histogram-closed as --histogram), as the last columns:\n"
            "                                 h0 .. h<n_edges>,hnan; a row's counters sum to W\n"
            "      --no-compression           do not write the .bro\n"
            "      --output-vsri              write the generated VSRI index\n"
            "      --output-wavbrro           write the generated WavBrro\n"
            "      --output-csv               (accepted; the reference never reads it)\n"
            "      --compressor <COMPRESSOR>  auto, noop, fft, constant, polynomial, idw [default: auto]\n"
            "  -e, --error <ERROR>            maximum allowed error in %% (0..50) [default: 5]\n"
            "  -c, --compression-selection-sample-level <0..6>  [default: 0]\n"
            "  -h, --help    -V, --version\n");
}

bool parse_compressor(const std::string &v, int &out)  // main.rs:85-94: no rle here
{
    static const struct { const char *n; int id; } T[] = {
        {"auto", ATSC_AUTO}, {"noop", ATSC_NOOP}, {"fft", ATSC_FFT}, {"constant", ATSC_CONSTANT},
        {"polynomial", ATSC_POLYNOMIAL}, {"idw", ATSC_IDW}};
    for (auto &t : T)
        if (v == t.n) { out = t.id; return true; }
    return false;
}
int die(const char *what, int rc = 0, const char *detail = "")
{
    fprintf(stderr, "thread 'main' panicked: %s%s%s%s\n", what, rc ? ": " : "", rc ? atsc_strerror(rc) : "", detail);
    return PANIC;
}

// -u --from T0 --to T1: the index finds the window, only its samples are decoded; .wbro and .csv hold those samples,
// their timestamps from the same get_time path as the whole file's (Metric::get_samples)
int uncompress_window(const Args &a, const std::string &output_base, uint8_t *bro, uint64_t len)
{
    atsc_vsri *index = nullptr;
    int rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
    if (rc) { atsc_free(bro); return die("failed to read vsri", rc); }
    uint64_t begin = 0, count = 0;
    rc = atsc_vsri_sample_window(index, a.t0, a.t1, &begin, &count);
    if (rc) { atsc_free(bro); atsc_vsri_free(index); return die("vsri window", rc); }
    std::vector<int64_t> ts(begin + count + 1);
    rc = atsc_metric_sample_times(index, begin + count, ts.data());
    atsc_vsri_free(index);
    if (rc) { atsc_free(bro); return die("called `Option::unwrap()` on a `None` value (index has no time for a sample)"); }
    std::vector<double> data(count ? count : 1);
    uint64_t n = 0;
    if (count) {
        atsc_ctx *ctx = nullptr;
        rc = atsc_ctx_create(&ctx, 0);
        if (rc) { atsc_free(bro); return die("no GPU context", rc); }
        rc = atsc_bro_open(bro, len, nullptr, nullptr);
        if (!rc) rc = atsc_decompress_window(ctx, bro + 9, len - 9, 1, begin, count, data.data(), count, &n);
        if (rc) { int e = die("decompress", rc, atsc_ctx_last_error(ctx)); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
        atsc_ctx_destroy(ctx);
    }
    atsc_free(bro);
    const std::string wbro_path = with_ext(output_base, "wbro");
    rc = atsc_wbro_write(wbro_path.c_str(), data.data(), n);
    if (rc) return die("writing wavbrro", rc);
    rc = atsc_samples_csv_write(with_ext(wbro_path, "csv").c_str(), ts.data() + begin, data.data(), n);
    if (rc) return die("failed to write samples to file", rc);
    return 0;
}

// -u --from T0 --to T1 --where OP:LIMIT: the index finds the window, the GPU its samples that meet the condition; their
// timestamps come from the same get_time path as the window's .csv; <out>.sel.csv is all that is written
int uncompress_where(const Args &a, const std::string &output_base, uint8_t *bro, uint64_t len)
{
    atsc_vsri *index = nullptr;
    int rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
    if (rc) { atsc_free(bro); return die("failed to read vsri", rc); }
    uint64_t begin = 0, count = 0;
    rc = atsc_vsri_sample_window(index, a.t0, a.t1, &begin, &count);
    if (rc) { atsc_free(bro); atsc_vsri_free(index); return die("vsri window", rc); }
    std::vector<int64_t> ts(begin + count + 1);
    rc = atsc_metric_sample_times(index, begin + count, ts.data());
    atsc_vsri_free(index);
    if (rc) { atsc_free(bro); return die("called `Option::unwrap()` on a `None` value (index has no time for a sample)"); }
    std::vector<atsc_selected> rows;
    if (count) {
        atsc_ctx *ctx = nullptr;
        rc = atsc_ctx_create(&ctx, 0);
        if (rc) { atsc_free(bro); return die("no GPU context", rc); }
        rc = atsc_bro_open(bro, len, nullptr, nullptr);
        if (!rc) rc = where_select(ctx, bro, len, a.q, begin, count, rows);
        if (rc) { int e = die("select", rc, atsc_ctx_last_error(ctx)); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
        atsc_ctx_destroy(ctx);
    }
    atsc_free(bro);
    if (!where_write(with_ext(output_base, "sel.csv"), "timestamp", rows,
                     [&](uint64_t at) { return std::to_string((long long)ts[begin + at]); }))
        return die("failed to write selected samples to file");
    return 0;
}

// -u --from T0 --to T1 --rolling W[:S]: the index finds the window, the GPU the sliding window's record at every position
// of it; a row carries the indexed time of its window's LAST sample, where a trailing average is plotted, from the same
// get_time path as the window's .csv; <out>.roll.csv is all that is written
int uncompress_rolling(const Args &a, const std::string &output_base, uint8_t *bro, uint64_t len)
{
    atsc_vsri *index = nullptr;
    int rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
    if (rc) { atsc_free(bro); return die("failed to read vsri", rc); }
    uint64_t begin = 0, count = 0;
    rc = atsc_vsri_sample_window(index, a.t0, a.t1, &begin, &count);
    if (rc) { atsc_free(bro); atsc_vsri_free(index); return die("vsri window", rc); }
    std::vector<int64_t> ts(begin + count + 1);
    rc = atsc_metric_sample_times(index, begin + count, ts.data());
    atsc_vsri_free(index);
    if (rc) { atsc_free(bro); return die("called `Option::unwrap()` on a `None` value (index has no time for a sample)"); }
    std::vector<atsc_window_rolling> rows;
    std::vector<atsc_window_delta> deltas;
    std::vector<atsc_window_delta_fit> fits;
    std::vector<atsc_window_moments> moments;
    std::vector<atsc_window_runs> runs;
    std::vector<double> levels;
    std::vector<uint64_t> hist;
    if (count) {
        atsc_ctx *ctx = nullptr;
        rc = atsc_ctx_create(&ctx, 0);
        if (rc) { atsc_free(bro); return die("no GPU context", rc); }
        rc = atsc_bro_open(bro, len, nullptr, nullptr);
        if (!rc) rc = rolling_query(ctx, bro, len, a.q, begin, count, rows, deltas, fits, moments, levels, runs, nullptr, &hist);
        if (rc) { int e = die("rolling", rc, atsc_ctx_last_error(ctx)); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
        atsc_ctx_destroy(ctx);
    }
    atsc_free(bro);
    const uint64_t w = a.q.rolling, stride = a.q.rolling_stride;
    if (!rolling_write(with_ext(output_base, "roll.csv"), "timestamp", rows, a.q.rolling_deltas, deltas, fits, a.q.rolling_moments, moments, a.q.rolling_level_names, levels, a.q.rolling_runs, runs, nullptr,
                       [&](uint64_t j) { return std::to_string((long long)ts[begin + j * stride + w - 1]); },
                       a.q.rolling_hist ? &hist : nullptr, a.q.rolling_edges.size() + 2))
        return die("failed to write rolling records to file");
    return 0;
}

// -u --from T0 --to T1 --step S: the time buckets [T0 + k S, min(T0 + (k + 1) S - 1, T1)] as sample windows of the index,
// one atsc_window_stats row each (timestamp = the bucket's start) into <out>.agg.csv; nothing else is written
int uncompress_buckets(const Args &a, const std::string &output_base, uint8_t *bro, uint64_t len)
{
    atsc_vsri *index = nullptr;
    int rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
    if (rc) { atsc_free(bro); return die("failed to read vsri", rc); }
    uint64_t nb = 0;
    rc = atsc_vsri_step_windows(index, a.t0, a.t1, a.step, nullptr, nullptr, 0, &nb);
    std::vector<uint64_t> b(nb ? nb : 1), c(nb ? nb : 1);
    if (rc == ATSC_E_CAPACITY || rc == ATSC_OK) rc = atsc_vsri_step_windows(index, a.t0, a.t1, a.step, b.data(), c.data(), nb, &nb);
    atsc_vsri_free(index);
    if (rc) { atsc_free(bro); return die("vsri buckets", rc); }
    atsc_ctx *ctx = nullptr;
    rc = atsc_ctx_create(&ctx, 0);
    if (rc) { atsc_free(bro); return die("no GPU context", rc); }
    BucketResults r;
    const char *failed = "aggregate";
    rc = atsc_bro_open(bro, len, nullptr, nullptr);
    if (!rc) rc = bucket_queries(ctx, bro, len, a.q, nb, b.data(), c.data(), r, &failed);
    if (rc) { int e = die(failed, rc, atsc_ctx_last_error(ctx)); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
    const std::vector<atsc_window_runs> &rv = r.rv;
    // "when did it start": the three positions as the indexed times of their samples, get_time(begin + offset)
    std::vector<std::string> rt(3 * nb);
    if (a.q.have_runs && nb) {
        index = nullptr;
        rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
        for (uint64_t k = 0; !rc && k < nb; ++k) {
            const uint64_t at[3] = {rv[k].longest_at, rv[k].first_at, rv[k].last_at};
            for (int j = 0; !rc && j < 3; ++j) {
                if (at[j] == ATSC_RUNS_NONE) continue;
                int32_t t = 0;
                const int got = atsc_vsri_get_time(index, (int32_t)(b[k] + at[j]), &t);  // 1: Some(t), 0: None
                if (got < 0) rc = got;
                if (got == 1) rt[3 * k + j] = std::to_string(t);
            }
        }
        if (index) atsc_vsri_free(index);
        if (rc) { int e = die("runs: indexed time", rc); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
    }
    // "when was the peak": the extremes' places as the indexed times of their samples, likewise
    if (a.q.extremes && nb) {
        index = nullptr;
        rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
        if (!rc)
            rc = bucket_extreme_places(r, nb, [&](uint64_t k, uint64_t at, std::string &cell) {
                int32_t t = 0;
                const int got = atsc_vsri_get_time(index, (int32_t)(b[k] + at), &t);  // 1: Some(t), 0: None
                if (got == 1) cell = std::to_string(t);
                return got < 0 ? got : 0;
            });
        if (index) atsc_vsri_free(index);
        if (rc) { int e = die("extremes: indexed time", rc); atsc_ctx_destroy(ctx); atsc_free(bro); return e; }
    }
    atsc_ctx_destroy(ctx);
    atsc_free(bro);
    FILE *f = fopen(with_ext(output_base, "agg.csv").c_str(), "w");
    if (!f) return die("failed to write aggregates to file");
    bucket_header(f, "timestamp", a.q, r);
    for (uint64_t k = 0; k < nb; ++k) bucket_row(f, std::to_string((long long)a.t0 + (long long)k * a.step), a.q, r, k, &rt[3 * k]);
    if (fclose(f) != 0) return die("failed to write aggregates to file");
    return 0;
}

int uncompress(const Args &a, const std::string &output_base)  // main.rs:139-173
{
    uint8_t *bro = nullptr;
    uint64_t len = 0;
    int rc = atsc_bro_read_file(a.input.c_str(), &bro, &len);
    if (rc) return die("failed to read bro file", rc);
    if (!bro) return 0;  // not a BRO file: nothing happens
    if (a.step) return uncompress_buckets(a, output_base, bro, len);
    if (a.q.have_where) return uncompress_where(a, output_base, bro, len);
    if (a.q.rolling) return uncompress_rolling(a, output_base, bro, len);
    if (a.window) return uncompress_window(a, output_base, bro, len);
    atsc_ctx *ctx = nullptr;
    rc = atsc_ctx_create(&ctx, 0);
    if (rc) { atsc_free(bro); return die("no GPU context", rc); }
    double *data = nullptr;
    uint64_t n = 0;
    rc = atsc_decompress_data(ctx, bro, len, &data, &n);
    atsc_free(bro);
    if (rc) { int e = die("decompress", rc, atsc_ctx_last_error(ctx)); atsc_ctx_destroy(ctx); return e; }
    atsc_ctx_destroy(ctx);
    atsc_vsri *index = nullptr;
    rc = atsc_vsri_load(with_ext(a.input, "vsri").c_str(), &index);
    if (rc) { atsc_free(data); return die("failed to read vsri", rc); }
    const std::string wbro_path = with_ext(output_base, "wbro");
    rc = atsc_wbro_write(wbro_path.c_str(), data, n);
    if (rc) { atsc_free(data); atsc_vsri_free(index); return die("writing wavbrro", rc); }
    std::vector<int64_t> ts(n ? n : 1);
    rc = atsc_metric_sample_times(index, n, ts.data());  // Metric::get_samples: get_time(i).unwrap()
    atsc_vsri_free(index);
    if (rc) { atsc_free(data); return die("called `Option::unwrap()` on a `None` value (index has no time for a sample)"); }
    rc = atsc_samples_csv_write(with_ext(wbro_path, "csv").c_str(), ts.data(), data, n);
    atsc_free(data);
    if (rc) return die("failed to write samples to file", rc);
    return 0;
}

int compress(const Args &a, const std::string &output_base)  // main.rs:174-207
{
    int64_t *ts = nullptr;
    double *vals = nullptr;
    uint64_t n = 0;
    int rc = atsc_samples_csv_read(a.input.c_str(), &ts, &vals, &n);
    if (rc) return die("failed to read samples from file", rc);
    atsc_vsri *index = atsc_vsri_new();
    if (!index) { atsc_free(ts); atsc_free(vals); return die("out of memory"); }
    uint64_t bad = 0;
    rc = atsc_metric_index_samples(index, ts, n, &bad);
    atsc_free(ts);
    if (rc) {
        fprintf(stderr, "updating for point failed, sample: %llu\n", (unsigned long long)bad);
        atsc_free(vals);
        atsc_vsri_free(index);
        return die("failed to create metric from samples");
    }
    int status = 0;
    if (a.output_wavbrro && atsc_wbro_write(with_ext(output_base, "wavbro").c_str(), vals, n)) status = die("writing wavbrro");
    if (!status && a.output_vsri && (rc = atsc_vsri_flush_to(index, with_ext(output_base, "vsri").c_str())))
        status = die("failed to flush vsri to the file", rc);
    atsc_vsri_free(index);
    if (!status && !a.no_compression) {
        atsc_ctx *ctx = nullptr;
        rc = atsc_ctx_create(&ctx, 0);
        if (rc) { atsc_free(vals); return die("no GPU context", rc); }
        uint8_t *bro = nullptr;
        uint64_t len = 0;
        rc = atsc_compress_data(ctx, vals, n, a.compressor, (uint8_t)a.error, a.level, &bro, &len);
        if (rc) {
            status = die("compress", rc, atsc_ctx_last_error(ctx));
        } else {
            FILE *f = fopen(with_ext(output_base, "bro").c_str(), "wb");
            if (!f || fwrite(bro, 1, len, f) != len) status = die("failed to write compressed data");
            if (f) fclose(f);
            atsc_free(bro);
        }
        atsc_ctx_destroy(ctx);
    }
    atsc_free(vals);
    return status;
}

}  // namespace

int main(int argc, char **argv)
{
    Args a;
    bool have_from = false, have_to = false;
    for (int i = 1; i < argc; ++i) {
        std::string s = argv[i], v;
        auto value = [&](const char *name) -> bool {
            const std::string pre = std::string(name) + "=";
            if (s.rfind(pre, 0) == 0) { v = s.substr(pre.size()); return true; }
            if (s == name && i + 1 < argc) { v = argv[++i]; return true; }
            return false;
        };
        if (s == "-h" || s == "--help") { usage(); return 0; }
        if (s == "-V" || s == "--version") { printf("csv-compressor 0.7.2 (%s)\n", atsc_version()); return 0; }
        if (s == "-u") a.uncompress = true;
        else if (s == "--no-compression") a.no_compression = true;
        else if (s == "--output-vsri") a.output_vsri = true;
        else if (s == "--output-wavbrro") a.output_wavbrro = true;
        else if (s == "--output-csv") a.output_csv = true;
        else if (value("--output") || value("-o")) { a.output = v; a.has_output = true; }
        else if (value("--from") || value("--to")) {
            const bool from = s.rfind("--from", 0) == 0;
            char *end = nullptr;
            const long long t = strtoll(v.c_str(), &end, 10);
            if (v.empty() || *end || t < INT32_MIN || t > INT32_MAX) {
                fprintf(stderr, "error: invalid value '%s' for '%s'\n", v.c_str(), from ? "--from" : "--to");
                return 2;
            }
            (from ? a.t0 : a.t1) = (int32_t)t;
            (from ? have_from : have_to) = true;
        }
        else if (value("--step")) {
            char *end = nullptr;
            const long long t = strtoll(v.c_str(), &end, 10);
            if (v.empty() || *end || t < 1 || t > INT32_MAX) {
                fprintf(stderr, "error: invalid value '%s' for '--step': expected 1..=%d\n", v.c_str(), INT32_MAX);
                return 2;
            }
            a.step = (int32_t)t;
        }
        else if (const int k = bucket_option(s, v, value, a.q)) { if (k == 2) return 2; }
        else if (value("--compressor")) { if (!parse_compressor(v, a.compressor)) { fprintf(stderr, "error: invalid value '%s' for '--compressor'\n", v.c_str()); return 2; } }
        else if (value("--error") || value("-e")) { if (!parse_int(v, 0, 50, a.error)) { fprintf(stderr, "error: invalid value '%s' for '--error': not in 0..=50\n", v.c_str()); return 2; } }
        else if (value("--compression-selection-sample-level") || value("-c")) { if (!parse_int(v, 0, 6, a.level)) { fprintf(stderr, "error: invalid value '%s' for '-c': not in 0..=6\n", v.c_str()); return 2; } }
        else if (!s.empty() && s[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); usage(); return 2; }
        else a.input = s;
    }
    if (a.input.empty()) { usage(); return 2; }
    if (have_from != have_to || ((have_from || have_to) && !a.uncompress)) {
        fprintf(stderr, "error: '--from' and '--to' go together, with '-u'\n");
        return 2;
    }
    if (a.step && !have_from) {
        fprintf(stderr, "error: '--step' needs '--from' and '--to'\n");
        return 2;
    }
    if (!bucket_options_complete(a.q, "--step", a.step != 0)) return 2;
    if (!where_option_complete(a.q, "--from' and '--to", have_from, "--step", a.step != 0)) return 2;
    if (!rolling_option_complete(a.q, "--from' and '--to", have_from, "--step", a.step != 0)) return 2;
    a.window = have_from;
    struct stat st;
    if (stat(a.input.c_str(), &st) != 0) return die("Failed to retrieve metadata of the input");  // main.rs:226-229
    if (!S_ISREG(st.st_mode)) return die("Input is not a file");                                 // main.rs:219-221
    const std::string output_base = a.has_output ? a.output : a.input;                            // main.rs:133-137
    return a.uncompress ? uncompress(a, output_base) : compress(a, output_base);
}
