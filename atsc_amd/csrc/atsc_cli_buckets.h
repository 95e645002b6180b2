// atsc_cli_buckets.h -- what the two command lines (atsc_cli.cpp, csv_compressor_cli.cpp) share: the small text helpers
// and the bucket queries behind `atsc -u --buckets N` and `csv-compressor -u --from --to --step S`: their options, the
// usage errors, the calls over the buckets and the columns of the .agg.csv; `--rolling W[:S]`, the sliding window's
// records at every position of a window (with `--rolling-deltas`, its deltas beside them, with `--rolling-moments`, its
// moments, with `--rolling-quantiles Q,Q,..`, its levels, with `--rolling-pair OTHER.bro` (atsc only), its pair moments
// against another file, with `--rolling-histogram E,E,..|LO:HI:N`, its value-bin counts); `--where OP:LIMIT`, the selected samples
// of the window itself into a .sel.csv; and `--across A.bro,B.bro,..` (atsc only), the across records of the window over
// several files into an .across.csv (the end of this file).  The two differ in the row's first cell,
// in how a failure is reported and in how a position inside a bucket is written: the three run positions, which the
// caller hands in, and the extremes' positions, which csv-compressor rewrites as times (bucket_extreme_places).
#pragma once
#include <cctype>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/atsc_hip.h"

namespace {

bool parse_int(const std::string &v, int lo, int hi, int &out)
{
    if (v.empty()) return false;
    char *end = nullptr;
    long x = strtol(v.c_str(), &end, 10);
    if (*end || x < lo || x > hi) return false;
    out = (int)x;
    return true;
}

// Rust `{:?}` of an f64: shortest round-trip digits (exponent form where that is shorter), ".0" appended to integers
std::string debug_f64(double v)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), v);
    std::string s(buf, r.ptr);
    if (s.find('e') == std::string::npos && s.find('.') == std::string::npos) s += ".0";
    return s;
}

std::string with_ext(const std::string &path, const char *ext)  // PathBuf::set_extension
{
    const size_t slash = path.find_last_of('/');
    const size_t dot = path.find_last_of('.');
    std::string base = (dot != std::string::npos && (slash == std::string::npos || dot > slash + 1)) ? path.substr(0, dot) : path;
    return base + "." + ext;
}

// The queries beside the buckets' count,min,max,sum,first,last, each with the .agg.csv columns it adds
struct BucketOptions {
    std::vector<double> levels;  // --quantiles: one column per level
    std::vector<std::string> level_names;
    int method = ATSC_QUANTILE_LINEAR;  // --quantile-method
    bool have_method = false;
    std::vector<double> edges;  // --histogram: h0 .. h<n_edges>,hnan
    bool have_hist = false;
    int closed = ATSC_HIST_LEFT_CLOSED;  // --histogram-closed
    bool have_closed = false;
    bool moments = false;  // --moments: mean,stdvar,stddev,slope,intercept
    bool deltas = false;   // --deltas: pairs,rises,falls,up,down,increase,variation,max_rise,max_fall
    bool have_runs = false;  // --runs OP:LIMIT: inside,runs,longest,longest_at,first_at,last_at,head,tail,excess
    int runs_op = ATSC_RUNS_GT;
    double runs_limit = 0.0;
    int extremes = 0;  // --extremes K: nans,max1,max1_at,..,maxK,maxK_at,min1,min1_at,..,minK,minK_at
    int values = 0;  // --values K[:ABOVE]: nans,below,distinct,more,v1,n1,..,vK,nK
    double values_above = std::nan("");  // NaN: every value is listed
    bool pair_allowed = false;  // the front end takes --pair (atsc; csv-compressor does not: DESIGN.md "Windowed pair moments")
    std::string pair;           // --pair OTHER.bro: pair_count,covariance,correlation,slope,intercept against that stream
    std::vector<std::string> pair_matrix;  // --pair-matrix A.bro,B.bro,.. (where pair_allowed): every pair's row per bucket into .pairs.csv
    bool have_where = false;  // --where OP:LIMIT: no bucket query; the window's selected samples into .sel.csv
    int where_op = ATSC_RUNS_GT;
    double where_limit = 0.0;
    uint64_t rolling = 0;  // --rolling W[:S]: no bucket query; the window's rolling records into .roll.csv
    uint64_t rolling_stride = 1;
    bool rolling_deltas = false;  // --rolling-deltas: pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase behind .roll.csv's own
    bool rolling_moments = false;  // --rolling-moments: nonnan,avg,stdvar,stddev,slope,intercept behind those
    bool rolling_runs = false;  // --rolling-runs OP:LIMIT: samples,inside,runs,longest,longest_at,first_at,last_at,head,tail,excess behind those
    int rolling_runs_op = ATSC_RUNS_GT;
    double rolling_runs_limit = 0.0;
    std::vector<double> rolling_levels;  // --rolling-quantiles Q,Q,..: one column per level behind those
    std::vector<std::string> rolling_level_names;
    std::vector<double> rolling_edges;  // --rolling-histogram E,E,..|LO:HI:N: h0 .. h<n_edges>,hnan as the last columns (closed: --histogram-closed)
    bool rolling_hist = false;
    std::string rolling_pair;  // --rolling-pair OTHER.bro (where pair_allowed): pair_count,covariance,correlation,slope,intercept as the last columns
    int rolling_method = ATSC_QUANTILE_LINEAR;  // --rolling-quantile-method
    bool have_rolling_method = false;
    bool across_allowed = false;      // the front end takes --across (atsc; csv-compressor does not: DESIGN.md "Windowed across")
    std::vector<std::string> across;  // --across A.bro,B.bro,..: no bucket query; the window's across records into .across.csv
    uint64_t across_stride = 1;       // --across-stride S
    bool have_across_stride = false;
    std::vector<double> across_levels;  // --across-quantiles Q,Q,..: one column per level behind .across.csv's own
    std::vector<std::string> across_level_names;
    int across_method = ATSC_QUANTILE_LINEAR;  // --across-quantile-method
    bool have_across_method = false;
    int across_extremes = 0;  // --across-extremes K: nans,top1,top1_at,..,topK,topK_at,bottom1,bottom1_at,..,bottomK,bottomK_at
    bool across_moments = false;  // --across-moments: nonnan,avg,stdvar,stddev
    std::vector<double> across_edges;  // --across-histogram E,E,..|LO:HI:N: h0 .. h<n_edges>,hnan as the last columns (closed: --histogram-closed)
    bool across_hist = false;
    int across_values = 0;  // --across-values K[:ABOVE]: vcount,vnans,vbelow,vdistinct,vmore,v0,n0,..,v<K-1>,n<K-1> as the last columns
    double across_values_above = std::nan("");  // NaN: every value is listed
};

// --quantiles Q,Q,..: levels in [0, 1] as typed (the column names), at most ATSC's 64
bool parse_levels(const std::string &v, std::vector<double> &q, std::vector<std::string> &names)
{
    q.clear();
    names.clear();
    for (size_t p = 0;;) {
        const size_t c = v.find(',', p);
        const std::string t = v.substr(p, c == std::string::npos ? std::string::npos : c - p);
        char *e = nullptr;
        const double x = strtod(t.c_str(), &e);
        if (t.empty() || isspace((unsigned char)t[0]) || *e || !(x >= 0.0 && x <= 1.0)) return false;
        q.push_back(x);
        names.push_back(t);
        if (c == std::string::npos) return true;
        p = c + 1;
    }
}

bool parse_method(const std::string &v, int &m)
{
    static const char *names[] = {"linear", "lower", "higher", "nearest"};  // ATSC_QUANTILE_* order
    for (int k = 0; k < 4; ++k)
        if (v == names[k]) { m = k; return true; }
    return false;
}

// --histogram SPEC: explicit edges E,E,.. or LO:HI:N, N equal bins over [LO, HI] (atsc_histogram_edges_uniform).
// 0: fine; 1: unparsable, NaN or not ascending, or a bad uniform spec; 2: more than ATSC_HIST_MAX_EDGES edges
int parse_histogram(const std::string &v, std::vector<double> &edges)
{
    edges.clear();
    auto number = [](const std::string &t, double &x) {
        char *e = nullptr;
        x = strtod(t.c_str(), &e);
        return !t.empty() && !isspace((unsigned char)t[0]) && !*e && x == x;
    };
    const size_t c1 = v.find(':');
    if (c1 != std::string::npos) {
        const size_t c2 = v.find(':', c1 + 1);
        if (c2 == std::string::npos) return 1;
        double lo, hi;
        const std::string ns = v.substr(c2 + 1);
        char *e = nullptr;
        const unsigned long long n = strtoull(ns.c_str(), &e, 10);
        if (!number(v.substr(0, c1), lo) || !number(v.substr(c1 + 1, c2 - c1 - 1), hi) || ns.empty() || *e ||
            !isdigit((unsigned char)ns[0]))
            return 1;
        if (n >= ATSC_HIST_MAX_EDGES) return 2;
        edges.resize(n + 1);
        return atsc_histogram_edges_uniform(lo, hi, (uint32_t)n, edges.data()) ? 1 : 0;
    }
    for (size_t p = 0;;) {
        const size_t c = v.find(',', p);
        double x;
        if (!number(v.substr(p, c == std::string::npos ? std::string::npos : c - p), x)) return 1;
        if (!edges.empty() && !(edges.back() < x)) return 1;
        edges.push_back(x);
        if (c == std::string::npos) return edges.size() > (size_t)ATSC_HIST_MAX_EDGES ? 2 : 0;
        p = c + 1;
    }
}

// the value of --histogram, --rolling-histogram or --across-histogram (`name`) into edges.  false: a usage error, reported
bool histogram_option(const char *name, const std::string &v, std::vector<double> &edges)
{
    const int bad = parse_histogram(v, edges);
    if (bad == 1) fprintf(stderr, "error: invalid value '%s' for '%s': expected ascending edges E,E,.. or LO:HI:N\n", v.c_str(), name);
    if (bad == 2) fprintf(stderr, "error: invalid value for '%s': more than %d edges\n", name, (int)ATSC_HIST_MAX_EDGES);
    return bad == 0;
}

// --runs OP:LIMIT: OP one of gt ge lt le eq ne, LIMIT a number that is not NaN, nothing behind it
bool parse_runs(const std::string &v, int &op, double &limit)
{
    static const char *const OPS[] = {"gt", "ge", "lt", "le", "eq", "ne"};
    const size_t c = v.find(':');
    if (c == std::string::npos) return false;
    const std::string o = v.substr(0, c), t = v.substr(c + 1);
    int k = 0;
    while (k < 6 && o != OPS[k]) ++k;
    char *e = nullptr;
    const double x = strtod(t.c_str(), &e);
    if (k == 6 || t.empty() || isspace((unsigned char)t[0]) || *e || x != x) return false;
    op = k;  // ATSC_RUNS_GT .. ATSC_RUNS_NE in this order
    limit = x;
    return true;
}

// --values K[:ABOVE]: K in 1 .. ATSC_VALUES_MAX_K; ABOVE, where given, a number that is not NaN, nothing behind it
bool parse_values(const std::string &v, int &k, double &above)
{
    const size_t c = v.find(':');
    if (!parse_int(v.substr(0, c), 1, ATSC_VALUES_MAX_K, k)) return false;
    above = std::nan("");
    if (c == std::string::npos) return true;
    const std::string t = v.substr(c + 1);
    char *e = nullptr;
    const double x = strtod(t.c_str(), &e);
    if (t.empty() || isspace((unsigned char)t[0]) || *e || x != x) return false;
    above = x;
    return true;
}

// --rolling W[:S]: the width, 1 .. ATSC_ROLLING_MAX_WIDTH, and the stride, at least 1 (1 where it is left out)
bool parse_rolling(const std::string &v, uint64_t &width, uint64_t &stride)
{
    const size_t c = v.find(':');
    auto number = [](const std::string &t, uint64_t &x) {
        char *e = nullptr;
        x = strtoull(t.c_str(), &e, 10);
        return !t.empty() && isdigit((unsigned char)t[0]) && !*e && t.size() <= 19 && x >= 1;
    };
    stride = 1;
    if (!number(v.substr(0, c), width) || width > ATSC_ROLLING_MAX_WIDTH) return false;
    return c == std::string::npos || number(v.substr(c + 1), stride);
}

// --across A.bro,B.bro,..: one to ATSC_ACROSS_MAX_STREAMS - 1 paths (the input file is stream 0), none of them empty
bool parse_across(const std::string &v, std::vector<std::string> &files)
{
    files.clear();
    for (size_t p = 0;;) {
        const size_t c = v.find(',', p);
        const std::string t = v.substr(p, c == std::string::npos ? std::string::npos : c - p);
        if (t.empty()) return false;
        files.push_back(t);
        if (c == std::string::npos) return files.size() < (size_t)ATSC_ACROSS_MAX_STREAMS;
        p = c + 1;
    }
}

// --pair OTHER.bro, --pair-matrix, --across and --across-stride are taken only where the front end allows them (o.pair_allowed,
// o.across_allowed).
// One argument of the command line, where it is a bucket-query option.  s: the argument; value(name): whether s is the
// option `name` with a value, which it leaves in v (the callers' lambda).  0: none of them; 1: taken; 2: a usage error,
// reported on stderr.
template <class Value>
int bucket_option(const std::string &s, const std::string &v, Value value, BucketOptions &o)
{
    if (value("--quantiles")) {
        if (!parse_levels(v, o.levels, o.level_names)) {
            fprintf(stderr, "error: invalid value '%s' for '--quantiles': expected levels in 0..=1, comma separated\n", v.c_str());
            return 2;
        }
        if (o.levels.size() > 64) {
            fprintf(stderr, "error: invalid value for '--quantiles': %zu levels, at most 64\n", o.levels.size());
            return 2;
        }
    } else if (value("--quantile-method")) {
        if (!parse_method(v, o.method)) {
            fprintf(stderr, "error: invalid value '%s' for '--quantile-method': linear, lower, higher or nearest\n", v.c_str());
            return 2;
        }
        o.have_method = true;
    } else if (value("--histogram")) {
        if (!histogram_option("--histogram", v, o.edges)) return 2;
        o.have_hist = true;
    } else if (value("--histogram-closed")) {
        if (v != "left" && v != "right") {
            fprintf(stderr, "error: invalid value '%s' for '--histogram-closed': left or right\n", v.c_str());
            return 2;
        }
        o.closed = v == "right" ? ATSC_HIST_RIGHT_CLOSED : ATSC_HIST_LEFT_CLOSED;
        o.have_closed = true;
    } else if (s == "--moments") {
        o.moments = true;
    } else if (s == "--deltas") {
        o.deltas = true;
    } else if (value("--runs")) {
        if (!parse_runs(v, o.runs_op, o.runs_limit)) {
            fprintf(stderr, "error: invalid value '%s': '--runs' wants OP:LIMIT (OP: gt ge lt le eq ne)\n", v.c_str());
            return 2;
        }
        o.have_runs = true;
    } else if (value("--where")) {
        if (!parse_runs(v, o.where_op, o.where_limit)) {
            fprintf(stderr, "error: invalid value '%s': '--where' wants OP:LIMIT (OP: gt ge lt le eq ne)\n", v.c_str());
            return 2;
        }
        o.have_where = true;
    } else if (value("--rolling")) {
        if (!parse_rolling(v, o.rolling, o.rolling_stride)) {
            fprintf(stderr, "error: invalid value '%s' for '--rolling': expected W[:S], W in 1..=%llu, S at least 1\n", v.c_str(),
                    (unsigned long long)ATSC_ROLLING_MAX_WIDTH);
            return 2;
        }
    } else if (s == "--rolling-deltas") {
        o.rolling_deltas = true;
    } else if (s == "--rolling-moments") {
        o.rolling_moments = true;
    } else if (value("--rolling-runs")) {
        if (!parse_runs(v, o.rolling_runs_op, o.rolling_runs_limit)) {
            fprintf(stderr, "error: invalid value '%s': '--rolling-runs' wants OP:LIMIT (OP: gt ge lt le eq ne)\n", v.c_str());
            return 2;
        }
        o.rolling_runs = true;
    } else if (value("--rolling-quantiles")) {
        if (!parse_levels(v, o.rolling_levels, o.rolling_level_names)) {
            fprintf(stderr, "error: invalid value '%s' for '--rolling-quantiles': expected levels in 0..=1, comma separated\n",
                    v.c_str());
            return 2;
        }
        if (o.rolling_levels.size() > 64) {
            fprintf(stderr, "error: invalid value for '--rolling-quantiles': %zu levels, at most 64\n", o.rolling_levels.size());
            return 2;
        }
    } else if (value("--rolling-histogram")) {
        if (!histogram_option("--rolling-histogram", v, o.rolling_edges)) return 2;
        o.rolling_hist = true;
    } else if (value("--rolling-quantile-method")) {
        if (!parse_method(v, o.rolling_method)) {
            fprintf(stderr, "error: invalid value '%s' for '--rolling-quantile-method': linear, lower, higher or nearest\n",
                    v.c_str());
            return 2;
        }
        o.have_rolling_method = true;
    } else if (value("--extremes")) {
        if (!parse_int(v, 1, ATSC_EXTREMES_MAX_K, o.extremes)) {
            fprintf(stderr, "error: invalid value '%s' for '--extremes': expected 1..=%d\n", v.c_str(), (int)ATSC_EXTREMES_MAX_K);
            return 2;
        }
    } else if (value("--values")) {
        if (!parse_values(v, o.values, o.values_above)) {
            fprintf(stderr, "error: invalid value '%s' for '--values': expected K[:ABOVE], K in 1..=%d, ABOVE a number\n", v.c_str(),
                    (int)ATSC_VALUES_MAX_K);
            return 2;
        }
    } else if (o.pair_allowed && value("--pair")) {
        if (v.empty()) {
            fprintf(stderr, "error: invalid value '' for '--pair': expected the path of a .bro file\n");
            return 2;
        }
        o.pair = v;
    } else if (o.pair_allowed && value("--pair-matrix")) {
        if (!parse_across(v, o.pair_matrix)) {
            fprintf(stderr, "error: invalid value '%s' for '--pair-matrix': expected 1..=%d paths of .bro files, comma separated\n",
                    v.c_str(), (int)ATSC_ACROSS_MAX_STREAMS - 1);
            return 2;
        }
    } else if (o.pair_allowed && value("--rolling-pair")) {
        if (v.empty()) {
            fprintf(stderr, "error: invalid value '' for '--rolling-pair': expected the path of a .bro file\n");
            return 2;
        }
        o.rolling_pair = v;
    } else if (o.across_allowed && value("--across")) {
        if (!parse_across(v, o.across)) {
            fprintf(stderr, "error: invalid value '%s' for '--across': expected 1..=%d paths of .bro files, comma separated\n",
                    v.c_str(), (int)ATSC_ACROSS_MAX_STREAMS - 1);
            return 2;
        }
    } else if (o.across_allowed && value("--across-stride")) {
        char *e = nullptr;
        o.across_stride = strtoull(v.c_str(), &e, 10);
        if (v.empty() || !isdigit((unsigned char)v[0]) || *e || v.size() > 19 || o.across_stride == 0) {
            fprintf(stderr, "error: invalid value '%s' for '--across-stride': expected a stride of at least 1\n", v.c_str());
            return 2;
        }
        o.have_across_stride = true;
    } else if (o.across_allowed && value("--across-quantiles")) {
        if (!parse_levels(v, o.across_levels, o.across_level_names)) {
            fprintf(stderr, "error: invalid value '%s' for '--across-quantiles': expected levels in 0..=1, comma separated\n",
                    v.c_str());
            return 2;
        }
        if (o.across_levels.size() > 64) {
            fprintf(stderr, "error: invalid value for '--across-quantiles': %zu levels, at most 64\n", o.across_levels.size());
            return 2;
        }
    } else if (o.across_allowed && value("--across-quantile-method")) {
        if (!parse_method(v, o.across_method)) {
            fprintf(stderr, "error: invalid value '%s' for '--across-quantile-method': linear, lower, higher or nearest\n",
                    v.c_str());
            return 2;
        }
        o.have_across_method = true;
    } else if (o.across_allowed && value("--across-extremes")) {
        if (!parse_int(v, 1, ATSC_EXTREMES_MAX_K, o.across_extremes)) {
            fprintf(stderr, "error: invalid value '%s' for '--across-extremes': expected 1..=%d\n", v.c_str(), (int)ATSC_EXTREMES_MAX_K);
            return 2;
        }
    } else if (o.across_allowed && s == "--across-moments") {
        o.across_moments = true;
    } else if (o.across_allowed && value("--across-histogram")) {
        if (!histogram_option("--across-histogram", v, o.across_edges)) return 2;
        o.across_hist = true;
    } else if (o.across_allowed && value("--across-values")) {
        if (!parse_values(v, o.across_values, o.across_values_above)) {
            fprintf(stderr, "error: invalid value '%s' for '--across-values': expected K[:ABOVE], K in 1..=%d, ABOVE a number\n",
                    v.c_str(), (int)ATSC_VALUES_MAX_K);
            return 2;
        }
    } else {
        return 0;
    }
    return 1;
}

// The options that need another one.  bucketing: the caller's option that cuts the buckets ("--buckets" or "--step"),
// given: whether it was there.  false: a usage error, reported on stderr.
bool bucket_options_complete(const BucketOptions &o, const char *bucketing, bool given)
{
    const struct {
        bool have, needed;
        const char *name, *needs;
    } T[] = {{!o.levels.empty(), given, "--quantiles", bucketing},
             {o.have_method, !o.levels.empty(), "--quantile-method", "--quantiles"},
             {o.have_hist, given, "--histogram", bucketing},
             {o.have_closed, o.have_hist || o.rolling_hist || o.across_hist, "--histogram-closed", "--histogram"},
             {o.moments, given, "--moments", bucketing},
             {o.deltas, given, "--deltas", bucketing},
             {o.have_runs, given, "--runs", bucketing},
             {o.extremes != 0, given, "--extremes", bucketing},
             {o.values != 0, given, "--values", bucketing},
             {!o.pair.empty(), given, "--pair", bucketing},
             {!o.pair_matrix.empty(), given, "--pair-matrix", bucketing}};
    for (const auto &t : T)
        if (t.have && !t.needed) {
            fprintf(stderr, "error: '%s' needs '%s'\n", t.name, t.needs);
            return false;
        }
    // (--pair's columns are the matrix' pair (0, 1) of that file: one or the other)
    if (!o.pair_matrix.empty() && !o.pair.empty()) {
        fprintf(stderr, "error: '--pair-matrix' cannot be used with '--pair'\n");
        return false;
    }
    return true;
}

// --where goes with the option that names the window (window: "--samples", or "--from' and '--to"; windowed: whether it
// was there) and without the one that cuts buckets.  false: a usage error, reported on stderr.
bool where_option_complete(const BucketOptions &o, const char *window, bool windowed, const char *bucketing, bool bucketed)
{
    if (!o.have_where) return true;
    if (!windowed) {
        fprintf(stderr, "error: '--where' needs '%s'\n", window);
        return false;
    }
    if (bucketed) {
        fprintf(stderr, "error: '--where' cannot be used with '%s'\n", bucketing);
        return false;
    }
    return true;
}

// --rolling goes with the option that names the window and without the one that cuts buckets, as --where does, and
// not with --where; --rolling-deltas, --rolling-moments, --rolling-runs, --rolling-quantiles, --rolling-histogram and --rolling-pair go with --rolling, --rolling-quantile-method
// with --rolling-quantiles, and --rolling-quantiles with a W of at most ATSC_ROLLING_QUANTILE_MAX_WIDTH.  false: a usage
// error, reported on stderr.
bool rolling_option_complete(const BucketOptions &o, const char *window, bool windowed, const char *bucketing, bool bucketed)
{
    if (o.have_rolling_method && o.rolling_levels.empty()) {
        fprintf(stderr, "error: '--rolling-quantile-method' needs '--rolling-quantiles'\n");
        return false;
    }
    if (!o.rolling) {
        if (o.rolling_deltas) fprintf(stderr, "error: '--rolling-deltas' needs '--rolling'\n");
        if (o.rolling_moments) fprintf(stderr, "error: '--rolling-moments' needs '--rolling'\n");
        if (o.rolling_runs) fprintf(stderr, "error: '--rolling-runs' needs '--rolling'\n");
        if (!o.rolling_levels.empty()) fprintf(stderr, "error: '--rolling-quantiles' needs '--rolling'\n");
        if (!o.rolling_pair.empty()) fprintf(stderr, "error: '--rolling-pair' needs '--rolling'\n");
        if (o.rolling_hist) fprintf(stderr, "error: '--rolling-histogram' needs '--rolling'\n");
        return !o.rolling_deltas && !o.rolling_moments && !o.rolling_runs && o.rolling_levels.empty() && o.rolling_pair.empty() &&
               !o.rolling_hist;
    }
    if (!o.rolling_levels.empty() && o.rolling > ATSC_ROLLING_QUANTILE_MAX_WIDTH) {
        fprintf(stderr, "error: '--rolling-quantiles' needs a '--rolling' W in 1..=%llu\n",
                (unsigned long long)ATSC_ROLLING_QUANTILE_MAX_WIDTH);
        return false;
    }
    if (!windowed) {
        fprintf(stderr, "error: '--rolling' needs '%s'\n", window);
        return false;
    }
    if (bucketed || o.have_where) {
        fprintf(stderr, "error: '--rolling' cannot be used with '%s'\n", bucketed ? bucketing : "--where");
        return false;
    }
    return true;
}

// --across goes with the option that names the window and without the one that cuts buckets, --rolling and --where;
// --across-stride, --across-quantiles, --across-extremes, --across-moments, --across-histogram and --across-values go with --across,
// --across-quantile-method with --across-quantiles.  false: a usage error, reported on stderr.
bool across_option_complete(const BucketOptions &o, const char *window, bool windowed, const char *bucketing, bool bucketed)
{
    if (o.have_across_method && o.across_levels.empty()) {
        fprintf(stderr, "error: '--across-quantile-method' needs '--across-quantiles'\n");
        return false;
    }
    if (o.across.empty()) {
        if (o.have_across_stride) fprintf(stderr, "error: '--across-stride' needs '--across'\n");
        else if (!o.across_levels.empty()) fprintf(stderr, "error: '--across-quantiles' needs '--across'\n");
        else if (o.across_extremes) fprintf(stderr, "error: '--across-extremes' needs '--across'\n");
        else if (o.across_moments) fprintf(stderr, "error: '--across-moments' needs '--across'\n");
        else if (o.across_hist) fprintf(stderr, "error: '--across-histogram' needs '--across'\n");
        else if (o.across_values) fprintf(stderr, "error: '--across-values' needs '--across'\n");
        return !o.have_across_stride && o.across_levels.empty() && !o.across_extremes && !o.across_moments && !o.across_hist &&
               !o.across_values;
    }
    if (!windowed) {
        fprintf(stderr, "error: '--across' needs '%s'\n", window);
        return false;
    }
    if (bucketed || o.rolling || o.have_where) {
        fprintf(stderr, "error: '--across' cannot be used with '%s'\n", bucketed ? bucketing : o.rolling ? "--rolling" : "--where");
        return false;
    }
    return true;
}

// what the queries gave, per bucket
struct BucketResults {
    std::vector<atsc_window_stats> st;
    uint64_t nq = 0, nh = 0;  // levels and counters per bucket
    std::vector<double> qv;
    std::vector<uint64_t> hv;
    std::vector<atsc_window_moments> mv;
    std::vector<atsc_window_fit> fv;
    std::vector<atsc_window_delta> dv;
    std::vector<atsc_window_delta_fit> df;
    std::vector<atsc_window_runs> rv;
    uint32_t ek = 0;                  // --extremes: entries per list
    std::vector<unsigned char> ev;    // the buckets' records, ATSC_EXTREMES_BYTES(ek) each
    std::vector<std::string> eat;     // 2 ek cells per bucket: the entries' places, as offsets in the bucket
    std::vector<atsc_window_pair> pv;  // --pair
    std::vector<atsc_window_pair_fit> pf;
    uint32_t vk = 0;                  // --values: entries per record
    std::vector<unsigned char> vv;    // the buckets' records, ATSC_VALUES_BYTES(vk) each
    const atsc_window_values_head &val_head(uint64_t k) const
    {
        return *(const atsc_window_values_head *)(vv.data() + k * ATSC_VALUES_BYTES(vk));
    }
    const atsc_value_count &val_entry(uint64_t k, uint32_t j) const { return ((const atsc_value_count *)(&val_head(k) + 1))[j]; }
    const atsc_window_extremes_head &ext_head(uint64_t k) const
    {
        return *(const atsc_window_extremes_head *)(ev.data() + k * ATSC_EXTREMES_BYTES(ek));
    }
    // entry j of bucket k: j < ek the largest, then the smallest
    const atsc_extreme &ext_entry(uint64_t k, uint32_t j) const { return ((const atsc_extreme *)(&ext_head(k) + 1))[j]; }
};

// With --extremes: writes the cell of every entry's place: place(k, at, cell) for the sample at offset `at` of bucket k
// (non-zero: a failure, which ends it); an empty entry's cell stays empty, as a run position that is ATSC_RUNS_NONE.
template <class Place>
int bucket_extreme_places(BucketResults &r, uint64_t nb, Place place)
{
    r.eat.assign(2 * (size_t)r.ek * nb, std::string());
    for (uint64_t k = 0; k < nb; ++k)
        for (uint32_t j = 0; j < 2 * r.ek; ++j) {
            const uint64_t at = r.ext_entry(k, j).at;
            if (at == ATSC_EXTREMES_NONE) continue;
            const int rc = place(k, at, r.eat[2 * (size_t)r.ek * k + j]);
            if (rc) return rc;
        }
    return 0;
}

// Runs the aggregates and the selected queries over the nb buckets (b, c) of a .bro image, the records from the
// frame-count varint on, as atsc_decompress_data reads them.  A failure ends it: its rc, and *failed names the query.
int bucket_queries(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, const BucketOptions &o, uint64_t nb, const uint64_t *b,
                   const uint64_t *c, BucketResults &r, const char **failed)
{
    const uint8_t *body = bro + 9;
    const uint64_t body_len = len - 9;
    r.st.resize(nb ? nb : 1);
    *failed = "aggregate";
    int rc = atsc_aggregate_windows(ctx, body, body_len, 1, nb, b, c, r.st.data());
    if (rc) return rc;
    *failed = "quantiles";
    r.nq = o.levels.size();
    r.qv.resize(nb * r.nq ? nb * r.nq : 1);
    if (r.nq) rc = atsc_quantile_windows(ctx, body, body_len, 1, nb, b, c, (uint32_t)r.nq, o.levels.data(), o.method, r.qv.data());
    if (rc) return rc;
    *failed = "histogram";
    r.nh = o.have_hist ? o.edges.size() + 2 : 0;
    r.hv.resize(nb * r.nh ? nb * r.nh : 1);
    if (r.nh) rc = atsc_histogram_windows(ctx, body, body_len, 1, nb, b, c, (uint32_t)o.edges.size(), o.edges.data(), o.closed,
                                          r.hv.data());
    if (rc) return rc;
    *failed = "moments";
    r.mv.resize(o.moments && nb ? nb : 1);
    r.fv.resize(r.mv.size());
    if (o.moments) rc = atsc_moments_windows(ctx, body, body_len, 1, nb, b, c, r.mv.data());
    if (!rc && o.moments) rc = atsc_moments_fit(r.mv.data(), nb, r.fv.data());
    if (rc) return rc;
    *failed = "deltas";
    r.dv.resize(o.deltas && nb ? nb : 1);
    r.df.resize(r.dv.size());
    if (o.deltas) rc = atsc_delta_windows(ctx, body, body_len, 1, nb, b, c, r.dv.data());
    if (!rc && o.deltas) rc = atsc_delta_derive(r.dv.data(), nb, r.df.data());
    if (rc) return rc;
    *failed = "runs";
    r.rv.resize(o.have_runs && nb ? nb : 1);
    if (o.have_runs) rc = atsc_runs_windows(ctx, body, body_len, 1, nb, b, c, o.runs_op, o.runs_limit, r.rv.data());
    if (rc) return rc;
    *failed = "extremes";
    r.ek = (uint32_t)o.extremes;
    r.ev.resize(r.ek && nb ? nb * ATSC_EXTREMES_BYTES(r.ek) : 8);
    if (r.ek) rc = atsc_extremes_windows(ctx, body, body_len, 1, nb, b, c, r.ek, r.ev.data());
    if (!rc && r.ek)
        rc = bucket_extreme_places(r, nb, [](uint64_t, uint64_t at, std::string &cell) { cell = std::to_string(at); return 0; });
    if (rc) return rc;
    *failed = "pair";
    const bool pair = !o.pair.empty();
    r.pv.resize(pair && nb ? nb : 1);
    r.pf.resize(r.pv.size());
    if (pair) {  // the other stream: sample i of it goes with sample i of this one
        uint8_t *other = nullptr;
        uint64_t olen = 0;
        rc = atsc_bro_read_file(o.pair.c_str(), &other, &olen);
        if (!rc && !other) rc = ATSC_E_FORMAT;  // not a BRO file
        if (!rc) rc = atsc_bro_open(other, olen, nullptr, nullptr);
        if (!rc) rc = atsc_pair_windows(ctx, body, body_len, 1, other + 9, olen - 9, 1, nb, b, c, r.pv.data());
        if (!rc) rc = atsc_pair_fit(r.pv.data(), nb, r.pf.data());
        atsc_free(other);
    }
    if (rc) return rc;
    *failed = "values";
    r.vk = (uint32_t)o.values;
    r.vv.resize(r.vk && nb ? nb * ATSC_VALUES_BYTES(r.vk) : 8);
    if (r.vk) rc = atsc_values_windows(ctx, body, body_len, 1, nb, b, c, r.vk, o.values_above, r.vv.data());
    return rc;
}

// the .agg.csv header; first: the name of the rows' first cell
void bucket_header(FILE *f, const char *first, const BucketOptions &o, const BucketResults &r)
{
    fprintf(f, "%s,count,min,max,sum,first,last", first);
    for (const std::string &n : o.level_names) fprintf(f, ",q%s", n.c_str());
    for (uint64_t j = 0; j + 1 < r.nh; ++j) fprintf(f, ",h%llu", (unsigned long long)j);
    if (r.nh) fprintf(f, ",hnan");
    if (o.moments) fprintf(f, ",mean,stdvar,stddev,slope,intercept");
    if (o.deltas) fprintf(f, ",pairs,rises,falls,up,down,increase,variation,max_rise,max_fall");
    if (o.have_runs) fprintf(f, ",inside,runs,longest,longest_at,first_at,last_at,head,tail,excess");
    if (o.extremes) {
        fprintf(f, ",nans");
        for (int e = 0; e < 2; ++e)
            for (int j = 1; j <= o.extremes; ++j) fprintf(f, ",%s%d,%s%d_at", e ? "min" : "max", j, e ? "min" : "max", j);
    }
    if (!o.pair.empty()) fprintf(f, ",pair_count,covariance,correlation,slope,intercept");
    if (o.values) {
        fprintf(f, ",nans,below,distinct,more");
        for (int j = 1; j <= o.values; ++j) fprintf(f, ",v%d,n%d", j, j);
    }
    fprintf(f, "\n");
}

// the row of bucket k; first: its first cell; run_at: with --runs, the cells longest_at, first_at, last_at
void bucket_row(FILE *f, const std::string &first, const BucketOptions &o, const BucketResults &r, uint64_t k,
                const std::string *run_at)
{
    const atsc_window_stats &st = r.st[k];
    fprintf(f, "%s,%llu,%s,%s,%s,%s,%s", first.c_str(), (unsigned long long)st.count, debug_f64(st.min).c_str(),
            debug_f64(st.max).c_str(), debug_f64(st.sum).c_str(), debug_f64(st.first).c_str(), debug_f64(st.last).c_str());
    for (uint64_t j = 0; j < r.nq; ++j) fprintf(f, ",%s", debug_f64(r.qv[k * r.nq + j]).c_str());
    for (uint64_t j = 0; j < r.nh; ++j) fprintf(f, ",%llu", (unsigned long long)r.hv[k * r.nh + j]);
    if (o.moments) {
        const atsc_window_fit &fv = r.fv[k];
        fprintf(f, ",%s,%s,%s,%s,%s", debug_f64(fv.mean).c_str(), debug_f64(fv.variance).c_str(), debug_f64(fv.stddev).c_str(),
                debug_f64(fv.slope).c_str(), debug_f64(fv.intercept).c_str());
    }
    if (o.deltas) {
        const atsc_window_delta &dv = r.dv[k];
        fprintf(f, ",%llu,%llu,%llu,%s,%s,%s,%s,%s,%s", (unsigned long long)dv.pairs, (unsigned long long)dv.rises,
                (unsigned long long)dv.falls, debug_f64(dv.up).c_str(), debug_f64(dv.down).c_str(),
                debug_f64(r.df[k].increase).c_str(), debug_f64(r.df[k].variation).c_str(), debug_f64(dv.max_rise).c_str(),
                debug_f64(dv.max_fall).c_str());
    }
    if (o.have_runs) {
        const atsc_window_runs &rv = r.rv[k];
        fprintf(f, ",%llu,%llu,%llu,%s,%s,%s,%llu,%llu,%s", (unsigned long long)rv.inside, (unsigned long long)rv.runs,
                (unsigned long long)rv.longest, run_at[0].c_str(), run_at[1].c_str(), run_at[2].c_str(),
                (unsigned long long)rv.head, (unsigned long long)rv.tail, debug_f64(rv.excess).c_str());
    }
    if (o.extremes) {
        fprintf(f, ",%llu", (unsigned long long)r.ext_head(k).nans);
        for (uint32_t j = 0; j < 2 * r.ek; ++j) {
            const atsc_extreme &x = r.ext_entry(k, j);
            fprintf(f, ",%s,%s", x.at == ATSC_EXTREMES_NONE ? "" : debug_f64(x.value).c_str(),
                    r.eat[2 * (size_t)r.ek * k + j].c_str());
        }
    }
    if (!o.pair.empty()) {
        const atsc_window_pair_fit &pf = r.pf[k];
        fprintf(f, ",%llu,%s,%s,%s,%s", (unsigned long long)r.pv[k].count, debug_f64(pf.covariance).c_str(),
                debug_f64(pf.correlation).c_str(), debug_f64(pf.slope).c_str(), debug_f64(pf.intercept).c_str());
    }
    if (o.values) {
        const atsc_window_values_head &h = r.val_head(k);
        fprintf(f, ",%llu,%llu,%u,%u", (unsigned long long)h.nans, (unsigned long long)h.below, h.distinct, h.more);
        for (uint32_t j = 0; j < r.vk; ++j) {
            const atsc_value_count &x = r.val_entry(k, j);
            if (j < h.distinct) fprintf(f, ",%s,%llu", debug_f64(x.value).c_str(), (unsigned long long)x.n);
            else fprintf(f, ",,");
        }
    }
    fprintf(f, "\n");
}

// --where: the samples of [begin, begin + count) of a .bro image that meet the condition, in stream order; cap is the
// window's sample count, so nothing is cut off.
int where_select(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, const BucketOptions &o, uint64_t begin, uint64_t count,
                 std::vector<atsc_selected> &rows)
{
    std::vector<uint64_t> block(ATSC_SELECT_BYTES(1, count) / 8);
    const int rc = atsc_select_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.where_op, o.where_limit, count, block.data());
    if (rc) return rc;
    const atsc_selected *e = (const atsc_selected *)(block.data() + 2);
    rows.assign(e, e + block[1]);
    return ATSC_OK;
}

// the .sel.csv: `first`,value and one row per selected sample; place(at): the first cell of the sample at offset `at` of
// the window; values as the .agg.csv writes them.  false: the file could not be written.
template <class Place>
bool where_write(const std::string &path, const char *first, const std::vector<atsc_selected> &rows, Place place)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    fprintf(f, "%s,value\n", first);
    for (const atsc_selected &r : rows) fprintf(f, "%s,%s\n", place(r.at).c_str(), debug_f64(r.value).c_str());
    return fclose(f) == 0;
}

// --rolling: one record per position of the range [begin, begin + count) of a .bro image; deltas: with --rolling-deltas,
// the same positions' rolling deltas and what atsc_delta_derive reads off them; moments: with --rolling-moments, the
// same positions' rolling moments; levels: with --rolling-quantiles, the same positions' rows of levels; runs: with
// --rolling-runs OP:LIMIT, the same positions' rolling runs under that condition; pairs: with
// --rolling-pair OTHER.bro, the same positions' rolling pair moments against that file's samples (sample i of it goes
// with sample i of this one; a file that ends before a window fails as --pair's does); hist: with
// --rolling-histogram, the same positions' rows of o.rolling_edges.size() + 2 counters (--histogram-closed's side)
int rolling_query(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, const BucketOptions &o, uint64_t begin, uint64_t count,
                  std::vector<atsc_window_rolling> &rows, std::vector<atsc_window_delta> &deltas,
                  std::vector<atsc_window_delta_fit> &fits, std::vector<atsc_window_moments> &moments,
                  std::vector<double> &levels, std::vector<atsc_window_runs> &runs, std::vector<atsc_window_pair> *pairs = nullptr,
                  std::vector<uint64_t> *hist = nullptr)
{
    rows.assign(atsc_rolling_outputs(count, o.rolling, o.rolling_stride), atsc_window_rolling{});
    atsc_window_rolling none;
    int rc = atsc_rolling_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride,
                                  rows.empty() ? &none : rows.data());
    if (!rc && o.rolling_deltas) {
        deltas.assign(rows.size(), atsc_window_delta{});
        fits.assign(rows.size(), atsc_window_delta_fit{});
        atsc_window_delta none_d;
        rc = atsc_rolling_delta_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride,
                                        deltas.empty() ? &none_d : deltas.data());
        if (!rc && !deltas.empty()) rc = atsc_delta_derive(deltas.data(), deltas.size(), fits.data());
    }
    if (!rc && o.rolling_moments) {
        moments.assign(rows.size(), atsc_window_moments{});
        atsc_window_moments none_m;
        rc = atsc_rolling_moments_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride,
                                          moments.empty() ? &none_m : moments.data());
    }
    if (!rc && !o.rolling_levels.empty()) {
        levels.assign(rows.size() * o.rolling_levels.size(), 0.0);
        double none_q;
        rc = atsc_rolling_quantile_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride,
                                           (uint32_t)o.rolling_levels.size(), o.rolling_levels.data(), o.rolling_method,
                                           levels.empty() ? &none_q : levels.data());
    }
    if (!rc && o.rolling_runs) {
        runs.assign(rows.size(), atsc_window_runs{});
        atsc_window_runs none_r;
        rc = atsc_rolling_runs_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride, o.rolling_runs_op,
                                       o.rolling_runs_limit, runs.empty() ? &none_r : runs.data());
    }
    if (!rc && pairs && !o.rolling_pair.empty()) {
        pairs->assign(rows.size(), atsc_window_pair{});
        atsc_window_pair none_p;
        uint8_t *other = nullptr;
        uint64_t olen = 0;
        rc = atsc_bro_read_file(o.rolling_pair.c_str(), &other, &olen);
        if (!rc && !other) rc = ATSC_E_FORMAT;  // not a BRO file
        if (!rc) rc = atsc_bro_open(other, olen, nullptr, nullptr);
        if (!rc)
            rc = atsc_rolling_pair_windows(ctx, bro + 9, len - 9, 1, other + 9, olen - 9, 1, 1, &begin, &count, o.rolling,
                                           o.rolling_stride, pairs->empty() ? &none_p : pairs->data());
        atsc_free(other);
    }
    if (!rc && hist && o.rolling_hist) {
        hist->assign(rows.size() * (o.rolling_edges.size() + 2), 0);
        uint64_t none_h;
        rc = atsc_rolling_histogram_windows(ctx, bro + 9, len - 9, 1, 1, &begin, &count, o.rolling, o.rolling_stride,
                                            (uint32_t)o.rolling_edges.size(), o.rolling_edges.data(), o.closed,
                                            hist->empty() ? &none_h : hist->data());
    }
    return rc;
}

// the .roll.csv: `first`,count,min,max,sum,mean and one row per position; place(j): the first cell of position j; values
// as the .agg.csv writes them, mean = sum / count and empty where count == 0.  with_deltas (--rolling-deltas): behind
// them pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase.  with_moments (--rolling-moments): behind those
// nonnan,avg,stdvar,stddev,slope,intercept from the position's record of `moments`: its count and the mean, the
// population variance and standard deviation, and the least-squares line (slope per sample, intercept at the position's
// first sample) that atsc_moments_fit reads off it, all six empty where the count is 0 (the count column says so); the
// column is avg because mean is taken: sum / count in the rolling's order.  names (--rolling-quantiles): behind those a
// column q<level as typed> per level, from the position's row of `levels` (NaN where the window holds no sample).
// with_runs (--rolling-runs): behind those samples,inside,runs,longest,longest_at,first_at,last_at,head,tail,excess from
// the position's record of `runs`, the three positions counted from the position's first sample and empty where the
// record has ATSC_RUNS_NONE, as --runs' cells are.
// pairs (--rolling-pair; null without it): as the last columns pair_count,covariance,correlation,slope,intercept, --pair's
// columns, from the position's record and what atsc_pair_fit reads off it; the four cells empty where pair_count is 0.
// hist (--rolling-histogram; null without it): behind all of those h0 .. h<n_edges>,hnan, --histogram's columns, from the
// position's row of n_hist = n_edges + 2 counters.
// false: the file could not be written.
template <class Place>
bool rolling_write(const std::string &path, const char *first, const std::vector<atsc_window_rolling> &rows, bool with_deltas,
                   const std::vector<atsc_window_delta> &deltas, const std::vector<atsc_window_delta_fit> &fits,
                   bool with_moments, const std::vector<atsc_window_moments> &moments, const std::vector<std::string> &names,
                   const std::vector<double> &levels, bool with_runs, const std::vector<atsc_window_runs> &runs,
                   const std::vector<atsc_window_pair> *pairs, Place place, const std::vector<uint64_t> *hist = nullptr,
                   size_t n_hist = 0)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    fprintf(f, "%s,count,min,max,sum,mean%s%s", first,
            with_deltas ? ",pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase" : "",
            with_moments ? ",nonnan,avg,stdvar,stddev,slope,intercept" : "");
    for (const std::string &n : names) fprintf(f, ",q%s", n.c_str());
    if (with_runs) fprintf(f, ",samples,inside,runs,longest,longest_at,first_at,last_at,head,tail,excess");
    if (pairs) fprintf(f, ",pair_count,covariance,correlation,slope,intercept");
    if (hist) {
        for (size_t k = 0; k + 1 < n_hist; ++k) fprintf(f, ",h%zu", k);
        fprintf(f, ",hnan");
    }
    fprintf(f, "\n");
    for (size_t j = 0; j < rows.size(); ++j) {
        const atsc_window_rolling &r = rows[j];
        fprintf(f, "%s,%llu,%s,%s,%s,%s", place(j).c_str(), (unsigned long long)r.count, debug_f64(r.min).c_str(),
                debug_f64(r.max).c_str(), debug_f64(r.sum).c_str(), r.count ? debug_f64(r.sum / (double)r.count).c_str() : "");
        if (with_deltas) {
            const atsc_window_delta &d = deltas[j];
            fprintf(f, ",%llu,%llu,%llu,%s,%s,%s,%s,%s,%s", (unsigned long long)d.pairs, (unsigned long long)d.rises,
                    (unsigned long long)d.falls, debug_f64(d.up).c_str(), debug_f64(d.down).c_str(),
                    debug_f64(d.after_falls).c_str(), debug_f64(d.max_rise).c_str(), debug_f64(d.max_fall).c_str(),
                    debug_f64(fits[j].increase).c_str());
        }
        if (with_moments) {
            atsc_window_fit fit;
            atsc_moments_fit(&moments[j], 1, &fit);
            if (moments[j].count == 0) fprintf(f, ",,,,,,");
            else fprintf(f, ",%llu,%s,%s,%s,%s,%s", (unsigned long long)moments[j].count, debug_f64(fit.mean).c_str(),
                         debug_f64(fit.variance).c_str(), debug_f64(fit.stddev).c_str(), debug_f64(fit.slope).c_str(),
                         debug_f64(fit.intercept).c_str());
        }
        for (size_t q = 0; q < names.size(); ++q) fprintf(f, ",%s", debug_f64(levels[j * names.size() + q]).c_str());
        if (with_runs) {
            const atsc_window_runs &rv = runs[j];
            auto pos = [](uint64_t p) { return p == ATSC_RUNS_NONE ? std::string() : std::to_string(p); };
            fprintf(f, ",%llu,%llu,%llu,%llu,%s,%s,%s,%llu,%llu,%s", (unsigned long long)rv.samples, (unsigned long long)rv.inside,
                    (unsigned long long)rv.runs, (unsigned long long)rv.longest, pos(rv.longest_at).c_str(), pos(rv.first_at).c_str(),
                    pos(rv.last_at).c_str(), (unsigned long long)rv.head, (unsigned long long)rv.tail, debug_f64(rv.excess).c_str());
        }
        if (pairs) {
            const atsc_window_pair &p = (*pairs)[j];
            atsc_window_pair_fit pf;
            atsc_pair_fit(&p, 1, &pf);
            if (p.count == 0) fprintf(f, ",0,,,,");
            else fprintf(f, ",%llu,%s,%s,%s,%s", (unsigned long long)p.count, debug_f64(pf.covariance).c_str(),
                         debug_f64(pf.correlation).c_str(), debug_f64(pf.slope).c_str(), debug_f64(pf.intercept).c_str());
        }
        if (hist)
            for (size_t k = 0; k < n_hist; ++k) fprintf(f, ",%llu", (unsigned long long)(*hist)[j * n_hist + k]);
        fprintf(f, "\n");
    }
    return fclose(f) == 0;
}

// --across: one record per position of the range [begin, begin + count) over the .bro image (stream 0) and the listed
// files (stream 1 and on): sample i of each goes with sample i of the others.  levels: with --across-quantiles, the
// same positions' rows of o.across_levels.size() levels; extremes: with --across-extremes K, the same positions'
// extremes records of k = K, ATSC_EXTREMES_BYTES(K) / 8 words each; moments: with --across-moments, the same
// positions' across moments; hist: with --across-histogram, the same positions' rows of o.across_edges.size() + 2 counters
// (--histogram-closed's side); values: with --across-values K[:ABOVE], the same positions' value-count records of k = K,
// ATSC_VALUES_BYTES(K) / 8 words each
int across_query(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, const BucketOptions &o, uint64_t begin, uint64_t count,
                 std::vector<atsc_across_record> &rows, std::vector<double> &levels, std::vector<uint64_t> &extremes,
                 std::vector<atsc_across_moments> &moments, std::vector<uint64_t> &hist, std::vector<uint64_t> &values)
{
    std::vector<uint8_t *> image(o.across.size(), nullptr);
    std::vector<const uint8_t *> body{bro + 9};
    std::vector<uint64_t> body_len{len - 9};
    int rc = ATSC_OK;
    for (size_t k = 0; k < o.across.size() && !rc; ++k) {
        uint64_t n = 0;
        rc = atsc_bro_read_file(o.across[k].c_str(), &image[k], &n);
        if (!rc && !image[k]) rc = ATSC_E_FORMAT;  // not a BRO file
        if (!rc) rc = atsc_bro_open(image[k], n, nullptr, nullptr);
        if (rc) break;
        body.push_back(image[k] + 9);
        body_len.push_back(n - 9);
    }
    if (!rc) {
        const std::vector<int> has_count(body.size(), 1);
        rows.assign(atsc_across_outputs(count, o.across_stride), atsc_across_record{});
        atsc_across_record none;
        rc = atsc_across_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin, &count,
                                 o.across_stride, rows.empty() ? &none : rows.data());
        if (!rc && !o.across_levels.empty()) {
            const uint32_t n_q = (uint32_t)o.across_levels.size();
            levels.assign(rows.size() * n_q, 0.0);
            double no_row;
            rc = atsc_across_quantile_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin,
                                              &count, o.across_stride, n_q, o.across_levels.data(), o.across_method,
                                              levels.empty() ? &no_row : levels.data());
        }
        if (!rc && o.across_extremes) {
            extremes.assign(rows.size() * (ATSC_EXTREMES_BYTES(o.across_extremes) / 8), 0);
            uint64_t no_record;
            rc = atsc_across_extremes_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin,
                                              &count, o.across_stride, (uint32_t)o.across_extremes,
                                              extremes.empty() ? &no_record : extremes.data());
        }
        if (!rc && o.across_moments) {
            moments.assign(rows.size(), atsc_across_moments{});
            atsc_across_moments no_moments;
            rc = atsc_across_moments_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin,
                                             &count, o.across_stride, moments.empty() ? &no_moments : moments.data());
        }
        if (!rc && o.across_hist) {
            hist.assign(rows.size() * (o.across_edges.size() + 2), 0);
            uint64_t no_row;
            rc = atsc_across_histogram_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin,
                                               &count, o.across_stride, (uint32_t)o.across_edges.size(), o.across_edges.data(),
                                               o.closed, hist.empty() ? &no_row : hist.data());
        }
        if (!rc && o.across_values) {
            values.assign(rows.size() * (ATSC_VALUES_BYTES(o.across_values) / 8), 0);
            uint64_t no_record;
            rc = atsc_across_values_windows(ctx, (uint32_t)body.size(), body.data(), body_len.data(), has_count.data(), 1, &begin,
                                            &count, o.across_stride, (uint32_t)o.across_values, o.across_values_above,
                                            values.empty() ? &no_record : values.data());
        }
    }
    for (uint8_t *p : image) atsc_free(p);
    return rc;
}

// the .across.csv: offset,count,min,min_at,max,max_at,sum,mean and one row per position; offset: the position's sample
// counted from the window's begin; values as the .agg.csv writes them; min_at and max_at (the stream's place in the
// list, the input file 0) and mean = sum / count empty where count == 0.  names: with --across-quantiles, a column
// q<level as typed> per level behind them, from the position's row of `levels`.  k: with --across-extremes K, behind
// those nans,top1,top1_at,..,topK,topK_at,bottom1,bottom1_at,..,bottomK,bottomK_at from the position's record of
// `extremes`: the K largest and the K smallest samples and the streams that hold them, the cells of unused entries
// empty.  with_moments: with --across-moments, behind those nonnan,avg,stdvar,stddev from the position's record of
// `moments`: its count, mean and the population variance and standard deviation that atsc_across_moments_fit reads off
// it, all four empty where count == 0 (the count column says so).  hist (--across-histogram; null without it): as the
// columns behind those h0 .. h<n_edges>,hnan, --histogram's columns, from the position's row of n_hist = n_edges + 2
// counters.  vk: with --across-values K[:ABOVE], as the last columns vcount,vnans,vbelow,vdistinct,vmore,v0,n0,..,
// v<K-1>,n<K-1> from the position's record of `values` (null without it): the number of streams, those whose sample is
// NaN, those whose sample is not above ABOVE, the entries filled, whether more distinct values lie above them, then the
// K smallest distinct values and the number of streams that hold each, the cells of unused entries empty.
// false: the file could not be written.
bool across_write(const std::string &path, const std::vector<atsc_across_record> &rows, uint64_t stride,
                  const std::vector<std::string> &names, const std::vector<double> &levels, uint32_t k,
                  const std::vector<uint64_t> &extremes, bool with_moments, const std::vector<atsc_across_moments> &moments,
                  const std::vector<uint64_t> *hist = nullptr, size_t n_hist = 0, uint32_t vk = 0,
                  const std::vector<uint64_t> *values = nullptr)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    fprintf(f, "offset,count,min,min_at,max,max_at,sum,mean");
    for (const std::string &n : names) fprintf(f, ",q%s", n.c_str());
    if (k) {
        fprintf(f, ",nans");
        for (uint32_t e = 0; e < k; ++e) fprintf(f, ",top%u,top%u_at", e + 1, e + 1);
        for (uint32_t e = 0; e < k; ++e) fprintf(f, ",bottom%u,bottom%u_at", e + 1, e + 1);
    }
    if (with_moments) fprintf(f, ",nonnan,avg,stdvar,stddev");
    if (hist) {
        for (size_t b = 0; b + 1 < n_hist; ++b) fprintf(f, ",h%zu", b);
        fprintf(f, ",hnan");
    }
    if (vk) {
        fprintf(f, ",vcount,vnans,vbelow,vdistinct,vmore");
        for (uint32_t e = 0; e < vk; ++e) fprintf(f, ",v%u,n%u", e, e);
    }
    fprintf(f, "\n");
    for (size_t j = 0; j < rows.size(); ++j) {
        const atsc_across_record &r = rows[j];
        const std::string mn_at = r.count ? std::to_string(r.min_at) : std::string(), mx_at = r.count ? std::to_string(r.max_at) : std::string();
        fprintf(f, "%llu,%u,%s,%s,%s,%s,%s,%s", (unsigned long long)(j * stride), r.count, debug_f64(r.min).c_str(), mn_at.c_str(),
                debug_f64(r.max).c_str(), mx_at.c_str(), debug_f64(r.sum).c_str(),
                r.count ? debug_f64(r.sum / (double)r.count).c_str() : "");
        for (size_t q = 0; q < names.size(); ++q) fprintf(f, ",%s", debug_f64(levels[j * names.size() + q]).c_str());
        if (k) {
            const uint64_t *rec = extremes.data() + j * (ATSC_EXTREMES_BYTES(k) / 8);
            const atsc_extreme *x = (const atsc_extreme *)(rec + 2);
            fprintf(f, ",%llu", (unsigned long long)((const atsc_window_extremes_head *)rec)->nans);
            for (uint32_t e = 0; e < 2 * k; ++e) {
                if (x[e].at == ATSC_EXTREMES_NONE) fprintf(f, ",,");
                else fprintf(f, ",%s,%llu", debug_f64(x[e].value).c_str(), (unsigned long long)x[e].at);
            }
        }
        if (with_moments) {
            atsc_across_fit fit;
            atsc_across_moments_fit(&moments[j], 1, &fit);
            if (moments[j].count == 0) fprintf(f, ",,,,");
            else fprintf(f, ",%u,%s,%s,%s", moments[j].count, debug_f64(fit.mean).c_str(), debug_f64(fit.variance).c_str(),
                         debug_f64(fit.stddev).c_str());
        }
        if (hist)
            for (size_t b = 0; b < n_hist; ++b) fprintf(f, ",%llu", (unsigned long long)(*hist)[j * n_hist + b]);
        if (vk) {
            const uint64_t *rec = values->data() + j * (ATSC_VALUES_BYTES(vk) / 8);
            const atsc_window_values_head &h = *(const atsc_window_values_head *)rec;
            const atsc_value_count *x = (const atsc_value_count *)(&h + 1);
            fprintf(f, ",%llu,%llu,%llu,%u,%u", (unsigned long long)h.count, (unsigned long long)h.nans, (unsigned long long)h.below,
                    h.distinct, h.more);
            for (uint32_t e = 0; e < vk; ++e) {
                if (e < h.distinct) fprintf(f, ",%s,%llu", debug_f64(x[e].value).c_str(), (unsigned long long)x[e].n);
                else fprintf(f, ",,");
            }
        }
        fprintf(f, "\n");
    }
    return fclose(f) == 0;
}

// --pair-matrix: the pair moments of every pair of the .bro image (stream 0) and the listed files (stream 1 and on) over
// the nb buckets (b, c): sample i of each goes with sample i of the others, and a file that ends before a bucket fails
// as --pair's does.  recs: nb rows of atsc_pair_matrix_records(*n_streams) records.
int pair_matrix_query(atsc_ctx *ctx, const uint8_t *bro, uint64_t len, const BucketOptions &o, uint64_t nb, const uint64_t *b,
                      const uint64_t *c, std::vector<atsc_window_pair> &recs, uint32_t *n_streams)
{
    std::vector<uint8_t *> image(o.pair_matrix.size(), nullptr);
    std::vector<const uint8_t *> body{bro + 9};
    std::vector<uint64_t> body_len{len - 9};
    int rc = ATSC_OK;
    for (size_t k = 0; k < o.pair_matrix.size() && !rc; ++k) {
        uint64_t n = 0;
        rc = atsc_bro_read_file(o.pair_matrix[k].c_str(), &image[k], &n);
        if (!rc && !image[k]) rc = ATSC_E_FORMAT;  // not a BRO file
        if (!rc) rc = atsc_bro_open(image[k], n, nullptr, nullptr);
        if (rc) break;
        body.push_back(image[k] + 9);
        body_len.push_back(n - 9);
    }
    if (!rc) {
        const std::vector<int> has_count(body.size(), 1);
        *n_streams = (uint32_t)body.size();
        recs.assign(nb * atsc_pair_matrix_records(*n_streams), atsc_window_pair{});
        atsc_window_pair none;
        rc = atsc_pair_matrix_windows(ctx, *n_streams, body.data(), body_len.data(), has_count.data(), nb, b, c,
                                      recs.empty() ? &none : recs.data());
    }
    for (uint8_t *p : image) atsc_free(p);
    return rc;
}

// the .pairs.csv: bucket,begin,count,i,j,pair_count,mean_i,mean_j,covariance,correlation,slope,intercept and one row per
// (bucket, i, j), i <= j, in the records' order: the bucket's number, first sample and length, the two streams' places in
// the list (the input file 0), the record's count and means and what atsc_pair_fit reads off it (the slope and intercept
// of stream j on stream i); values as the .agg.csv writes them.  false: the file could not be written.
bool pair_matrix_write(const std::string &path, uint64_t nb, const uint64_t *b, const uint64_t *c, uint32_t n_streams,
                       const std::vector<atsc_window_pair> &recs)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    fprintf(f, "bucket,begin,count,i,j,pair_count,mean_i,mean_j,covariance,correlation,slope,intercept\n");
    const uint64_t P = atsc_pair_matrix_records(n_streams);
    for (uint64_t k = 0; k < nb; ++k)
        for (uint32_t i = 0; i < n_streams; ++i)
            for (uint32_t j = i; j < n_streams; ++j) {
                const atsc_window_pair &p = recs[k * P + atsc_pair_matrix_index(n_streams, i, j)];
                atsc_window_pair_fit pf;
                atsc_pair_fit(&p, 1, &pf);
                fprintf(f, "%llu,%llu,%llu,%u,%u,%llu,%s,%s,%s,%s,%s,%s\n", (unsigned long long)k, (unsigned long long)b[k],
                        (unsigned long long)c[k], i, j, (unsigned long long)p.count, debug_f64(p.mean_x).c_str(),
                        debug_f64(p.mean_y).c_str(), debug_f64(pf.covariance).c_str(), debug_f64(pf.correlation).c_str(),
                        debug_f64(pf.slope).c_str(), debug_f64(pf.intercept).c_str());
            }
    return fclose(f) == 0;
}

}  // namespace
