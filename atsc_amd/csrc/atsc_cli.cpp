// atsc -- command line front end over libatsc_hip.so with the reference's flags and file naming
// (atsc/src/main.rs:29-127,176-243).  Every frame is compressed / decompressed on the GPU.
//
//   atsc [--compressor auto|noop|fft|constant|polynomial|idw|rle] [-e 0..50] [-u [--samples BEGIN:COUNT] [--buckets N
//        [--quantiles Q,Q,.. [--quantile-method linear|lower|higher|nearest]]
//        [--histogram E,E,..|LO:HI:N [--histogram-closed left|right]] [--moments] [--deltas] [--runs OP:LIMIT] [--extremes K] [--values K[:ABOVE]]
//        [--pair OTHER.bro | --pair-matrix A.bro,B.bro,..]] [--where OP:LIMIT] [--rolling W[:S] [--rolling-deltas] [--rolling-moments] [--rolling-runs OP:LIMIT]
//        [--rolling-quantiles Q,Q,.. [--rolling-quantile-method M]] [--rolling-pair OTHER.bro]
//        [--rolling-histogram E,E,..|LO:HI:N]]
//        [--across A.bro,B.bro,.. [--across-stride S] [--across-quantiles Q,Q,.. [--across-quantile-method M]]
//        [--across-extremes K] [--across-moments] [--across-histogram E,E,..|LO:HI:N] [--across-values K[:ABOVE]]]]
//        [-c 0..6] [--verbose] [--csv] [--no-header] [--fields=TIME,VALUE] <file-or-directory>
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/atsc_hip.h"
#include "atsc_cli_buckets.h"

namespace {

struct Args {
    std::string input;
    int compressor = ATSC_AUTO;  // default_value = "auto" (main.rs:180)
    int error = 3;               // default_value_t = 3 (main.rs:187)
    bool uncompress = false;
    int level = 0;
    bool verbose = false, csv = false, no_header = false;
    std::string fields = "time,value";  // main.rs:218
    bool window = false;                // --samples BEGIN:COUNT (with -u): decode only that window
    uint64_t win_begin = 0, win_count = 0;
    uint64_t buckets = 0;               // --buckets N (with -u): summaries of N-sample buckets into <file>.agg.csv
    BucketOptions q;                    // with --buckets: the queries beside the summaries (atsc_cli_buckets.h)
};

void usage()
{
    fprintf(stderr,
            "A Time-Series compressor\n\nUsage: atsc [OPTIONS] <INPUT>\n\nOptions:\n"
            "      --compressor <COMPRESSOR>  auto, noop, fft, constant, polynomial, idw, rle [default: auto]\n"
            "  -e, --error <ERROR>            maximum allowed error in %% (0..50) [default: 3]\n"
            "  -u                             uncompress the input file/directory\n"
            "      --samples <BEGIN:COUNT>    with -u: write only the samples [BEGIN, BEGIN+COUNT) to the .wbro\n"
            "      --buckets <N>              with -u: write count,min,max,sum,first,last of every N samples to .agg.csv\n"
            "      --quantiles <Q,Q,..>       with --buckets: also the levels Q (0..1, at most 64) of every bucket\n"
            "      --quantile-method <M>      linear | lower | higher | nearest [default: linear]\n"
            "      --histogram <SPEC>         with --buckets: also every bucket's counts over the value bins of the edges\n"
            "                                 E,E,.. (ascending, at most 1024) or LO:HI:N (N equal bins over LO..HI)\n"
            "      --histogram-closed <SIDE>  left: E[k-1] <= v < E[k] | right: E[k-1] < v <= E[k] [default: left]\n"
            "      --moments                  with --buckets: also every bucket's mean, stdvar, stddev (population forms) and\n"
            "                                 least-squares slope (value units per sample) and intercept (at its first sample)\n"
            "      --deltas                   with --buckets: also every bucket's steps from one sample to the next: counted\n"
            "                                 pairs, rises, falls (a counter's resets), the sums of the rises (up) and of the\n"
            "                                 falls (down), the counter increase (every fall a restart from zero), the total\n"
            "                                 variation (up + down) and the largest single rise and fall\n"
            "      --runs <OP:LIMIT>          with --buckets: also every bucket's samples with value OP LIMIT (OP: gt ge lt le eq\n"
            "                                 ne, e.g. gt:0.9) and their runs of adjacent samples, as the last columns: inside,\n"
            "                                 runs, longest, longest_at, first_at, last_at (sample offsets in the bucket, empty\n"
            "                                 where there is none), head, tail, excess (the sum of |value - LIMIT| over them)\n"
            "      --extremes <K>             with --buckets: also every bucket's K largest and K smallest samples (K: 1..16) and\n"
            "                                 where they are, as the last columns: nans, max1, max1_at .. maxK, maxK_at, min1,\n"
            "                                 min1_at .. minK, minK_at (equal values earliest first; *_at the sample's offset\n"
            "                                 in the bucket; both cells empty where the bucket has fewer samples)\n"
            "      --pair <OTHER.bro>         with --buckets: also every bucket's pair moments against the samples of OTHER.bro at\n"
            "                                 the same sample indices (OTHER must reach the bucketed range's end), as the last\n"
            "                                 columns: pair_count (samples where neither value is NaN), covariance (population\n"
            "                                 form), correlation, and slope and intercept of OTHER's value on this file's\n"
            "      --pair-matrix <A.bro,B.bro,..>  with --buckets, without --pair: also the pair moments of every pair of this file\n"
            "                                 (stream 0) and the listed files (streams 1.., at most 63; each must reach the\n"
            "                                 bucketed range's end) over every bucket, one row per (bucket, i, j), i <= j, to\n"
            "                                 .pairs.csv: bucket,begin,count,i,j,pair_count,mean_i,mean_j,covariance,correlation,\n"
            "                                 slope,intercept (of stream j's value on stream i's; i == j: the stream's own moments)\n"
            "      --values <K[:ABOVE]>       with --buckets: also every bucket's K smallest distinct values (K: 1..32) and how often\n"
            "                                 each occurs, as the last columns: nans, below, distinct, more, v1, n1 .. vK, nK\n"
            "                                 (values ascending, -0.0 counted with 0.0; with ABOVE only values greater than it\n"
            "                                 are listed and the others counted in below; more is 1 where the bucket has more\n"
            "                                 than K such values; both cells empty where it has fewer)\n"
            "      --where <OP:LIMIT>         with -u --samples, without --buckets: write the window's samples with value OP LIMIT\n"
            "                                 (as --runs) to .sel.csv instead of the .wbro: sample,value, one row per selected\n"
            "                                 sample, sample its index in the stream\n"
            "      --rolling <W[:S]>          with -u --samples, without --buckets: write the window of W samples at every\n"
            "                                 S-th position of the samples (S: 1) to .roll.csv instead of the .wbro:\n"
            "                                 offset,count,min,max,sum,mean, offset the position's first sample counted\n"
            "                                 from BEGIN; mean is sum / count, empty where count is 0\n"
            "      --rolling-deltas           with --rolling: also every position's steps from one sample to the next, as the\n"
            "                                 last columns: pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase\n"
            "                                 (as --deltas; increase = up + after_falls, the counter increase of the window)\n"
            "      --rolling-moments          with --rolling: also every position's mean, spread and trend, as the last\n"
            "                                 columns: nonnan,avg,stdvar,stddev,slope,intercept (as --moments: population\n"
            "                                 forms, slope per sample, intercept at the position's first sample; all empty\n"
            "                                 where the window holds no sample)\n"
            "      --rolling-runs <OP:LIMIT>  with --rolling: also every position's samples with value OP LIMIT and their runs (as\n"
            "                                 --runs), behind those columns: samples,inside,runs,longest,longest_at,first_at,\n"
            "                                 last_at,head,tail,excess; the three positions count from the position's first\n"
            "                                 sample and are empty where there is none (inside == samples: every sample of the\n"
            "                                 window meets the condition, an alert's `for:`)\n"
            "      --rolling-quantiles <Q,Q,..>  with --rolling, W at most 8192: also every position's levels (0 <= Q <= 1, as\n"
            "                                 --quantiles), as the last columns: one q<Q> per level as typed; NaN where the\n"
            "                                 window holds no sample\n"
            "      --rolling-quantile-method <M>  with --rolling-quantiles: linear (default), lower, higher or nearest\n"
            "      --rolling-histogram <SPEC> with --rolling: also every position's counts over the value bins of the edges\n"
            "                                 (SPEC and --histogram-closed as --histogram), as the last columns:\n"
            "                                 h0 .. h<n_edges>,hnan; a row's counters sum to W\n"
            "      --rolling-pair <OTHER.bro> with --rolling: also every position's pair moments against the samples of\n"
            "                                 OTHER.bro at the same indices (x: this file, y: OTHER), as the last columns:\n"
            "                                 pair_count,covariance,correlation,slope,intercept (as --pair; the four empty\n"
            "                                 where pair_count is 0).  OTHER must not end before a position's window\n"
            "      --across <A.bro,B.bro,..>  with -u --samples, without --buckets, --rolling and --where: fold this file (stream\n"
            "                                 0) and the listed files (streams 1.., at most 63) at the same sample indices and\n"
            "                                 write one row per sample to .across.csv instead of the .wbro:\n"
            "                                 offset,count,min,min_at,max,max_at,sum,mean -- offset counted from BEGIN, count the\n"
            "                                 streams whose sample is not NaN, min_at / max_at the stream that holds the extreme\n"
            "                                 (the first of equal ones), sum in list order; min_at, max_at and mean (sum / count)\n"
            "                                 empty where count is 0.  Every file must reach the window's end\n"
            "      --across-stride <S>        with --across: every S-th sample of the window only [default: 1]\n"
            "      --across-quantiles <Q,Q,..> with --across: also the levels Q (0..1, at most 64) of the streams' samples at\n"
            "                                 every row's sample index, NaN samples left out: one column q<Q> per level\n"
            "                                 behind mean, NaN where every stream's sample is NaN\n"
            "      --across-quantile-method <M>  linear | lower | higher | nearest [default: linear]\n"
            "      --across-extremes <K>      with --across: also the K (1..16) largest and the K smallest of the streams' samples\n"
            "                                 at every row's sample index and the streams that hold them (of equal values the\n"
            "                                 first in the list first), NaN samples left out and counted: nans,top1,top1_at,..,\n"
            "                                 topK,topK_at,bottom1,bottom1_at,..,bottomK,bottomK_at behind the columns above,\n"
            "                                 the cells of unused entries empty\n"
            "      --across-moments           with --across: also nonnan,avg,stdvar,stddev behind the columns above: how many of the\n"
            "                                 streams' samples at every row's sample index are not NaN, their mean and their\n"
            "                                 variance and standard deviation (population forms), merged from centred moments and\n"
            "                                 never from a sum of squares; the four cells empty where every sample is NaN\n"
            "      --across-histogram <SPEC>  with --across: also how many of the streams' samples at every row's sample index\n"
            "                                 lie in each value bin of the edges (SPEC and --histogram-closed as --histogram), as\n"
            "                                 the last columns: h0 .. h<n_edges>,hnan; a row's counters sum to the number of streams\n"
            "      --across-values <K[:ABOVE]>  with --across: also which values the streams hold at every row's sample index and\n"
            "                                 how many streams hold each (count_values), behind every other column:\n"
            "                                 vcount,vnans,vbelow,vdistinct,vmore,v0,n0 .. v<K-1>,n<K-1>: the streams, those whose\n"
            "                                 sample is NaN, those whose sample is not above ABOVE, the entries filled, whether more\n"
            "                                 distinct values follow, then the K (1..=32) smallest distinct values above ABOVE (all\n"
            "                                 without it; -0.0 counts as +0.0) and the number of streams that hold each, the cells\n"
            "                                 of unused entries empty; page on with ABOVE = the last value listed\n"
            "  -c, --compression-selection-sample-level <0..6>  [default: 0]\n"
            "      --verbose                  dump every sample\n"
            "      --csv                      input is a CSV file\n"
            "      --no-header                the CSV has no header\n"
            "      --fields <TIME,VALUE>      CSV field names [default: time,value]\n"
            "  -h, --help    -V, --version\n");
}

bool parse_compressor(const std::string &v, int &out)
{
    static const struct { const char *n; int id; } T[] = {
        {"auto", ATSC_AUTO}, {"noop", ATSC_NOOP}, {"fft", ATSC_FFT}, {"constant", ATSC_CONSTANT},
        {"polynomial", ATSC_POLYNOMIAL}, {"idw", ATSC_IDW}, {"rle", ATSC_RLE}};
    for (auto &t : T)
        if (v == t.n) { out = t.id; return true; }
    return false;
}
void dump(const char *tag, const double *d, uint64_t n)
{
    printf("%s=[", tag);
    for (uint64_t i = 0; i < n; ++i) printf("%s%s", i ? ", " : "", debug_f64(d[i]).c_str());
    printf("]\n");
}

// -u --buckets N: one atsc_window_stats row per bucket of N samples of [begin, begin + count), the last bucket shorter
int write_buckets(atsc_ctx *ctx, const std::string &path, const Args &a, const uint8_t *bro, uint64_t len, uint64_t begin,
                  uint64_t count)
{
    const uint64_t nb = (count + a.buckets - 1) / a.buckets;
    std::vector<uint64_t> b(nb), c(nb);
    for (uint64_t k = 0; k < nb; ++k) {
        b[k] = begin + k * a.buckets;
        c[k] = std::min(a.buckets, begin + count - b[k]);
    }
    BucketResults r;
    const char *failed;  // (not reported: the context's message names the call)
    const int rc = bucket_queries(ctx, bro, len, a.q, nb, b.data(), c.data(), r, &failed);
    if (rc) return rc;
    auto pos = [](uint64_t p) { return p == ATSC_RUNS_NONE ? std::string() : std::to_string(p); };
    FILE *f = fopen(with_ext(path, "agg.csv").c_str(), "w");
    if (!f) return ATSC_E_IO;
    bucket_header(f, "begin", a.q, r);
    for (uint64_t k = 0; k < nb; ++k) {
        std::string at[3];  // the three run positions: sample offsets in the bucket
        if (a.q.have_runs) {
            at[0] = pos(r.rv[k].longest_at);
            at[1] = pos(r.rv[k].first_at);
            at[2] = pos(r.rv[k].last_at);
        }
        bucket_row(f, std::to_string(b[k]), a.q, r, k, at);
    }
    if (fclose(f) != 0) return ATSC_E_IO;
    if (a.q.pair_matrix.empty()) return ATSC_OK;
    // --pair-matrix: beside the .agg.csv, every pair's row of every bucket
    std::vector<atsc_window_pair> recs;
    uint32_t n_streams = 0;
    const int rcm = pair_matrix_query(ctx, bro, len, a.q, nb, b.data(), c.data(), recs, &n_streams);
    if (rcm) return rcm;
    return pair_matrix_write(with_ext(path, "pairs.csv"), nb, b.data(), c.data(), n_streams, recs) ? ATSC_OK : ATSC_E_IO;
}

int process_single_file(atsc_ctx *ctx, const std::string &path, const Args &a)
{
    if (a.uncompress) {  // main.rs:72-83
        uint8_t *bro = nullptr;
        uint64_t len = 0;
        int rc = atsc_bro_read_file(path.c_str(), &bro, &len);
        if (rc) return rc;
        if (!bro) return ATSC_OK;  // not a BRO file: skipped silently
        if (a.buckets) {
            uint64_t ns = 0;
            rc = atsc_bro_open(bro, len, nullptr, nullptr);
            if (!rc && !a.window) rc = atsc_bro_scan(bro, len, nullptr, &ns);
            if (!rc) rc = write_buckets(ctx, path, a, bro, len, a.window ? a.win_begin : 0, a.window ? a.win_count : ns);
            atsc_free(bro);
            return rc;
        }
        if (a.q.have_where) {  // (with --samples) the window's selected samples, no .wbro
            std::vector<atsc_selected> rows;
            rc = atsc_bro_open(bro, len, nullptr, nullptr);
            if (!rc) rc = where_select(ctx, bro, len, a.q, a.win_begin, a.win_count, rows);
            atsc_free(bro);
            if (rc) return rc;
            const uint64_t b0 = a.win_begin;
            return where_write(with_ext(path, "sel.csv"), "sample", rows, [b0](uint64_t at) { return std::to_string(b0 + at); })
                       ? ATSC_OK
                       : ATSC_E_IO;
        }
        if (a.q.rolling) {  // (with --samples) the window's rolling records, no .wbro
            std::vector<atsc_window_rolling> rows;
            std::vector<atsc_window_delta> deltas;
            std::vector<atsc_window_delta_fit> fits;
            std::vector<atsc_window_moments> moments;
            std::vector<double> levels;
            rc = atsc_bro_open(bro, len, nullptr, nullptr);
            std::vector<atsc_window_pair> pairs;
            std::vector<atsc_window_runs> runs;
            std::vector<uint64_t> hist;
            if (!rc) rc = rolling_query(ctx, bro, len, a.q, a.win_begin, a.win_count, rows, deltas, fits, moments, levels, runs, &pairs, &hist);
            atsc_free(bro);
            if (rc) return rc;
            const uint64_t stride = a.q.rolling_stride;  // a position's first sample, counted from the window's begin
            return rolling_write(with_ext(path, "roll.csv"), "offset", rows, a.q.rolling_deltas, deltas, fits, a.q.rolling_moments, moments, a.q.rolling_level_names, levels,
                                 a.q.rolling_runs, runs, a.q.rolling_pair.empty() ? nullptr : &pairs,
                                 [stride](uint64_t j) { return std::to_string(j * stride); }, a.q.rolling_hist ? &hist : nullptr,
                                 a.q.rolling_edges.size() + 2)
                       ? ATSC_OK
                       : ATSC_E_IO;
        }
        if (!a.q.across.empty()) {  // (with --samples) the window's across records over this file and the listed ones, no .wbro
            std::vector<atsc_across_record> rows;
            std::vector<double> levels;
            std::vector<uint64_t> extremes;
            std::vector<atsc_across_moments> moments;
            std::vector<uint64_t> hist, values;
            rc = atsc_bro_open(bro, len, nullptr, nullptr);
            if (!rc) rc = across_query(ctx, bro, len, a.q, a.win_begin, a.win_count, rows, levels, extremes, moments, hist, values);
            atsc_free(bro);
            if (rc) return rc;
            const bool ok = across_write(with_ext(path, "across.csv"), rows, a.q.across_stride, a.q.across_level_names, levels,
                                         (uint32_t)a.q.across_extremes, extremes, a.q.across_moments, moments,
                                         a.q.across_hist ? &hist : nullptr, a.q.across_edges.size() + 2,
                                         (uint32_t)a.q.across_values, &values);
            return ok ? ATSC_OK : ATSC_E_IO;
        }
        double *out = nullptr;
        uint64_t n = 0;
        if (a.window) {
            // the records from the frame-count varint on, as atsc_decompress_data reads them
            rc = atsc_bro_open(bro, len, nullptr, nullptr);
            if (!rc) {
                out = (double *)malloc((a.win_count ? a.win_count : 1) * sizeof(double));
                rc = out ? atsc_decompress_window(ctx, bro + 9, len - 9, 1, a.win_begin, a.win_count, out, a.win_count, &n)
                         : ATSC_E_NOMEM;
            }
        } else {
            rc = atsc_decompress_data(ctx, bro, len, &out, &n);
        }
        atsc_free(bro);
        if (rc) { atsc_free(out); return rc; }
        if (a.verbose) dump("Output", out, n);
        rc = atsc_wbro_write(with_ext(path, "wbro").c_str(), out, n);
        atsc_free(out);
        return rc;
    }
    double *data = nullptr;
    uint64_t n = 0;
    int rc;
    if (a.csv) {  // main.rs:84-100
        const size_t comma = a.fields.find(',');
        const std::string tf = a.fields.substr(0, comma);
        const std::string vf = comma == std::string::npos ? std::string() : a.fields.substr(comma + 1);
        rc = atsc_csv_read(path.c_str(), a.no_header ? 0 : 1, tf.c_str(), vf.c_str(), &data, &n);
    } else {
        rc = atsc_wbro_read(path.c_str(), &data, &n);  // main.rs:112
    }
    if (rc) return rc;
    if (a.verbose) dump("Input", data, n);
    uint8_t *bro = nullptr;
    uint64_t len = 0;
    rc = atsc_compress_data(ctx, data, n, a.compressor, (uint8_t)a.error, a.level, &bro, &len);
    atsc_free(data);
    if (rc) return rc;
    FILE *f = fopen(with_ext(path, "bro").c_str(), "wb");  // main.rs:121-124
    if (!f) { atsc_free(bro); return ATSC_E_IO; }
    const size_t w = fwrite(bro, 1, len, f);
    fclose(f);
    atsc_free(bro);
    return w == len ? ATSC_OK : ATSC_E_IO;
}

bool has_ext(const std::string &p, const char *ext)
{
    const size_t dot = p.find_last_of('.');
    return dot != std::string::npos && p.substr(dot + 1) == ext;
}

// main.rs:50-68 walks read_dir while it writes into the same directory and calls
// process_single_file twice per entry; here the listing is taken once and every input file
// (.wbro / .csv when compressing, anything BRO-tagged when uncompressing) is handled once.
int process_directory(atsc_ctx *ctx, const Args &a)
{
    std::vector<std::string> files;
    DIR *d = opendir(a.input.c_str());
    if (!d) return ATSC_E_IO;
    while (dirent *e = readdir(d)) {
        std::string p = a.input + "/" + e->d_name;
        struct stat st;
        if (stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode)) files.push_back(p);
    }
    closedir(d);
    int last = ATSC_OK;
    for (const std::string &p : files) {
        if (!a.uncompress && !(a.csv ? has_ext(p, "csv") : has_ext(p, "wbro"))) continue;
        int rc = process_single_file(ctx, p, a);
        if (rc) {
            fprintf(stderr, "[ERROR] %s File: %s\n", atsc_strerror(rc), p.c_str());
            last = rc;
        }
    }
    return last;
}

}  // namespace

int main(int argc, char **argv)
{
    Args a;
    a.q.pair_allowed = true;
    a.q.across_allowed = true;
    for (int i = 1; i < argc; ++i) {
        std::string s = argv[i], v;
        auto value = [&](const char *name) -> bool {
            const std::string pre = std::string(name) + "=";
            if (s.rfind(pre, 0) == 0) { v = s.substr(pre.size()); return true; }
            if (s == name && i + 1 < argc) { v = argv[++i]; return true; }
            return false;
        };
        if (s == "-h" || s == "--help") { usage(); return 0; }
        if (s == "-V" || s == "--version") { printf("atsc 0.7.2 (%s)\n", atsc_version()); return 0; }
        if (s == "-u") a.uncompress = true;
        else if (s == "--verbose") a.verbose = true;
        else if (s == "--csv") a.csv = true;
        else if (s == "--no-header") a.no_header = true;
        else if (value("--compressor")) { if (!parse_compressor(v, a.compressor)) { fprintf(stderr, "error: invalid value '%s' for '--compressor'\n", v.c_str()); return 2; } }
        else if (value("--error") || value("-e")) { if (!parse_int(v, 0, 50, a.error)) { fprintf(stderr, "error: invalid value '%s' for '--error': not in 0..=50\n", v.c_str()); return 2; } }
        else if (value("--compression-selection-sample-level") || value("-c")) { if (!parse_int(v, 0, 6, a.level)) { fprintf(stderr, "error: invalid value '%s' for '-c': not in 0..=6\n", v.c_str()); return 2; } }
        else if (value("--fields")) a.fields = v;
        else if (value("--samples")) {
            const size_t colon = v.find(':');
            char *e1 = nullptr, *e2 = nullptr;
            const std::string b = colon == std::string::npos ? std::string() : v.substr(0, colon);
            const std::string c = colon == std::string::npos ? std::string() : v.substr(colon + 1);
            a.win_begin = strtoull(b.c_str(), &e1, 10);
            a.win_count = strtoull(c.c_str(), &e2, 10);
            if (b.empty() || c.empty() || *e1 || *e2 || b[0] == '-' || c[0] == '-') {
                fprintf(stderr, "error: invalid value '%s' for '--samples': expected BEGIN:COUNT\n", v.c_str());
                return 2;
            }
            a.window = true;
        }
        else if (value("--buckets")) {
            char *e = nullptr;
            a.buckets = strtoull(v.c_str(), &e, 10);
            if (v.empty() || *e || v[0] == '-' || a.buckets == 0) {
                fprintf(stderr, "error: invalid value '%s' for '--buckets': expected a positive sample count\n", v.c_str());
                return 2;
            }
        }
        else if (const int k = bucket_option(s, v, value, a.q)) { if (k == 2) return 2; }
        else if (!s.empty() && s[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); usage(); return 2; }
        else a.input = s;
    }
    if (a.input.empty()) { usage(); return 2; }
    if (a.window && !a.uncompress) { fprintf(stderr, "error: '--samples' needs '-u'\n"); return 2; }
    if (a.buckets && !a.uncompress) { fprintf(stderr, "error: '--buckets' needs '-u'\n"); return 2; }
    if (!bucket_options_complete(a.q, "--buckets", a.buckets != 0)) return 2;
    if (!where_option_complete(a.q, "--samples", a.window, "--buckets", a.buckets != 0)) return 2;
    if (!rolling_option_complete(a.q, "--samples", a.window, "--buckets", a.buckets != 0)) return 2;
    if (!across_option_complete(a.q, "--samples", a.window, "--buckets", a.buckets != 0)) return 2;
    struct stat st;
    if (stat(a.input.c_str(), &st) != 0) { fprintf(stderr, "[ERROR] %s: No such file or directory\n", a.input.c_str()); return 1; }
    atsc_ctx *ctx = nullptr;
    int rc = atsc_ctx_create(&ctx, 0);
    if (rc) { fprintf(stderr, "[ERROR] %s\n", atsc_strerror(rc)); return 1; }
    if (S_ISREG(st.st_mode)) rc = process_single_file(ctx, a.input, a);
    else if (S_ISDIR(st.st_mode)) rc = process_directory(ctx, a);
    else { fprintf(stderr, "[ERROR] The provided path is neither a file nor a directory.\n"); rc = ATSC_E_IO; }
    if (rc) fprintf(stderr, "[ERROR] %s (%s)\n", atsc_strerror(rc), atsc_ctx_last_error(ctx));
    atsc_ctx_destroy(ctx);
    return rc ? 1 : 0;  // main.rs:239-242
}
