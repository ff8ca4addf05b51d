// mcl_host.cpp -- the homolog-group rule of include/peprml.h in plain C++: the graph front end, Markov clustering in dense loops
// (pml_mcl_cluster_host: the CPU tests' subject and the timing baseline of tools/measure_mcl.py; a component of 256
// nodes or more shares its columns among up to 16 threads), the reading of a limit matrix
// and the Java's filters and set selection.  No HIP, no context: builds alone under host sanitizers.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <thread>

#include "../../include/peprml.h"
#include "mcl.hpp"

namespace pml {

MclOpts mcl_resolve(const pml_mcl_opts *o) {
    MclOpts r{1.5, 10000.0, 1e-3, 10000};
    if (o) {
        if (o->inflation != 0) r.inflation = o->inflation;
        if (o->prune_inverse != 0) r.prune_inverse = o->prune_inverse;
        if (o->chaos_eps != 0) r.chaos_eps = o->chaos_eps;
        if (o->max_iter != 0) r.max_iter = o->max_iter;
    }
    return r;
}

namespace {
struct Dsu {
    std::vector<int> p;
    explicit Dsu(int n) : p((size_t)n) { std::iota(p.begin(), p.end(), 0); }
    int find(int x) { while (p[(size_t)x] != x) { p[(size_t)x] = p[(size_t)p[(size_t)x]]; x = p[(size_t)x]; } return x; }
    void unite(int a, int b) { a = find(a); b = find(b); if (a != b) p[(size_t)std::max(a, b)] = std::min(a, b); }     // the root is the smallest member
};
struct Arc { int a, b; double w; };
}  // namespace

bool mcl_build_graph(int n, long long narcs, const int *a, const int *b, const double *w, MclGraph &g, std::string &err) {
    std::vector<Arc> arcs;
    arcs.reserve((size_t)narcs * 2);
    Dsu dsu(n);
    for (long long i = 0; i < narcs; ++i) {
        if (a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n) { err = "arc " + std::to_string(i) + " names a node outside 0.." + std::to_string(n - 1); return false; }
        if (!std::isfinite(w[i]) || w[i] <= 0) { err = "arc " + std::to_string(i) + " has the weight " + std::to_string(w[i]) + ": weights are finite and > 0"; return false; }
        if (a[i] == b[i]) continue;                                  // a self hit only makes its label a node
        arcs.push_back({a[i], b[i], w[i]});
        arcs.push_back({b[i], a[i], w[i]});
        dsu.unite(a[i], b[i]);
    }
    std::sort(arcs.begin(), arcs.end(), [](const Arc &x, const Arc &y) { return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.w > y.w; });
    arcs.erase(std::unique(arcs.begin(), arcs.end(), [](const Arc &x, const Arc &y) { return x.a == y.a && x.b == y.b; }), arcs.end());   // the first of equals is the largest
    // components in order of their smallest member (the root), members ascending
    g.n = n;
    std::vector<int> comp_of((size_t)n, -1), count;
    for (int i = 0; i < n; ++i) {
        const int r = dsu.find(i);
        if (comp_of[(size_t)r] < 0) { comp_of[(size_t)r] = (int)count.size(); count.push_back(0); }      // r <= i: a root is met first
        comp_of[(size_t)i] = comp_of[(size_t)r];
        count[(size_t)comp_of[(size_t)i]]++;
    }
    g.comp_off.assign(count.size() + 1, 0);
    for (size_t c = 0; c < count.size(); ++c) g.comp_off[c + 1] = g.comp_off[c] + count[c];
    g.nodes.assign((size_t)n, 0);
    std::vector<int> at(g.comp_off.begin(), g.comp_off.end() - 1), local((size_t)n), pos((size_t)n);
    for (int i = 0; i < n; ++i) { const int c = comp_of[(size_t)i]; pos[(size_t)i] = at[(size_t)c]++; g.nodes[(size_t)pos[(size_t)i]] = i; local[(size_t)i] = pos[(size_t)i] - g.comp_off[(size_t)c]; }
    g.ptr.assign((size_t)n + 1, 0);
    for (const Arc &e : arcs) g.ptr[(size_t)pos[(size_t)e.a] + 1]++;
    for (int p = 0; p < n; ++p) g.ptr[(size_t)p + 1] += g.ptr[(size_t)p];
    g.row.resize(arcs.size()); g.val.resize(arcs.size());
    std::vector<long long> fill(g.ptr.begin(), g.ptr.end() - 1);
    for (const Arc &e : arcs) { const long long k = fill[(size_t)pos[(size_t)e.a]]++; g.row[(size_t)k] = local[(size_t)e.b]; g.val[(size_t)k] = e.w; }   // ascending rows: arcs are sorted
    return true;
}

void mcl_fill_host(const MclGraph &g, int c, std::vector<double> &M) {
    const int n = g.size(c), p0 = g.comp_off[(size_t)c];
    M.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double mx = 0, sum = 0;
        for (long long k = g.ptr[(size_t)(p0 + j)]; k < g.ptr[(size_t)(p0 + j) + 1]; ++k) { mx = std::max(mx, g.val[(size_t)k]); sum += g.val[(size_t)k]; }
        const double loop = mx > 0 ? mx : 1.0;
        sum += loop;
        for (long long k = g.ptr[(size_t)(p0 + j)]; k < g.ptr[(size_t)(p0 + j) + 1]; ++k) M[(size_t)j * n + g.row[(size_t)k]] = g.val[(size_t)k] / sum;
        M[(size_t)j * n + j] = loop / sum;
    }
}

namespace {
// columns [j0, j1) of one iteration; returns their chaos
double step_columns(int n, const std::vector<double> &M, std::vector<double> &tmp, const MclOpts &o, int j0, int j1) {
    const double thr = 1.0 / o.prune_inverse;
    double chaos = -1e300;
    for (int j = j0; j < j1; ++j) {
        double *c = &tmp[(size_t)j * n];
        std::fill(c, c + n, 0.0);
        for (int k = 0; k < n; ++k) {                                // column j of M M = sum_k M[:, k] M[k][j]
            const double m = M[(size_t)j * n + k];
            if (m == 0) continue;
            const double *col = &M[(size_t)k * n];
            for (int i = 0; i < n; ++i) c[i] += col[i] * m;
        }
        double s = 0;
        for (int i = 0; i < n; ++i) { if (c[i] < thr) c[i] = 0; s += c[i]; }
        double mx = 0, sq = 0;
        for (int i = 0; i < n; ++i) { c[i] /= s; mx = std::max(mx, c[i]); sq += c[i] * c[i]; }
        chaos = std::max(chaos, mx - sq);
        s = 0;
        for (int i = 0; i < n; ++i) { c[i] = c[i] > 0 ? std::pow(c[i], o.inflation) : 0.0; s += c[i]; }
        for (int i = 0; i < n; ++i) c[i] /= s;
    }
    return chaos;
}
}  // namespace

// a large component's columns are shared among up to 16 threads: a column's arithmetic does not depend on the split
double mcl_step_host(int n, std::vector<double> &M, std::vector<double> &tmp, const MclOpts &o) {
    tmp.resize((size_t)n * n);
    const int T = n < 256 ? 1 : (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)n / 64u}));
    double chaos = -1e300;
    if (T == 1) chaos = step_columns(n, M, tmp, o, 0, n);
    else {
        std::vector<double> part((size_t)T, -1e300);
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t)
            th.emplace_back([&, t] { part[(size_t)t] = step_columns(n, M, tmp, o, (int)((long long)n * t / T), (int)((long long)n * (t + 1) / T)); });
        for (auto &x : th) x.join();
        for (double p : part) chaos = std::max(chaos, p);
    }
    M.swap(tmp);
    return chaos;
}

void mcl_read_host(int n, const std::vector<double> &M, int *best, unsigned *mask) {
    const int W = mcl_words(n);
    std::fill(mask, mask + (size_t)n * W, 0u);
    for (int j = 0; j < n; ++j) {
        int bst = -1;
        const bool att_j = M[(size_t)j * n + j] > 0;
        for (int a = 0; a < n; ++a) {
            if (!(M[(size_t)a * n + a] > 0)) continue;
            const double v = M[(size_t)j * n + a];
            if (bst < 0 || v > M[(size_t)j * n + bst]) bst = a;
            if (att_j && v > 0) mask[(size_t)j * W + (a >> 5)] |= 1u << (a & 31);
        }
        best[j] = bst;
    }
}

void mcl_finish(const MclGraph &g, const int *best, const unsigned *mask, int *cluster_of, int *nclusters) {
    const int n = g.n;
    Dsu dsu(n);                                                      // over renumbered nodes; a root is its cluster's smallest member
    size_t moff = 0;
    for (int c = 0; c < g.ncomp(); ++c) {
        const int m = g.size(c), p0 = g.comp_off[(size_t)c], W = mcl_words(m);
        for (int b = 0; b < m; ++b)
            for (int a = 0; a < m; ++a)
                if (mask[moff + (size_t)b * W + (a >> 5)] >> (a & 31) & 1u) dsu.unite(p0 + a, p0 + b);
        moff += (size_t)m * W;
    }
    // a node joins its best attractor's system; the systems' roots may not be the clusters' smallest members, so group by root first
    std::vector<int> sys((size_t)n);
    for (int c = 0; c < g.ncomp(); ++c) {
        const int m = g.size(c), p0 = g.comp_off[(size_t)c];
        for (int j = 0; j < m; ++j) sys[(size_t)(p0 + j)] = best[p0 + j] >= 0 ? dsu.find(p0 + best[p0 + j]) : -(p0 + j) - 1;
    }
    std::map<int, std::vector<int>> groups;                          // members by the call's node index
    for (int p = 0; p < n; ++p) groups[sys[(size_t)p]].push_back(g.nodes[(size_t)p]);
    std::vector<std::vector<int>> cl;
    for (auto &kv : groups) { std::sort(kv.second.begin(), kv.second.end()); cl.push_back(std::move(kv.second)); }
    std::sort(cl.begin(), cl.end(), [](const std::vector<int> &x, const std::vector<int> &y) { return x.size() != y.size() ? x.size() > y.size() : x[0] < y[0]; });
    for (size_t k = 0; k < cl.size(); ++k) for (int v : cl[k]) cluster_of[v] = (int)k;
    *nclusters = (int)cl.size();
}

// ---- the Java around MCL ----
std::string java_float_to_string(float v) {
    if (v == 0) return std::signbit(v) ? "-0.0" : "0.0";
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-Infinity" : "Infinity";
    char buf[64];
    int prec = 0;
    for (; prec < 9; ++prec) {                                       // the shortest digits that read back as v
        std::snprintf(buf, sizeof buf, "%.*e", prec, (double)v);
        if (std::strtof(buf, nullptr) == v) break;
    }
    std::string s(buf);
    const size_t epos = s.find('e');
    const int e = std::atoi(s.c_str() + epos + 1);
    std::string sign, digits;
    for (size_t i = 0; i < epos; ++i) { if (s[i] == '-') sign = "-"; else if (s[i] != '.') digits += s[i]; }
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const double av = std::fabs((double)v);
    if (av >= 1e-3 && av < 1e7) {
        std::string whole, frac;
        if (e >= 0) {
            whole = digits.substr(0, std::min(digits.size(), (size_t)e + 1));
            whole.append((size_t)e + 1 - whole.size(), '0');
            if (digits.size() > (size_t)e + 1) frac = digits.substr((size_t)e + 1);
        } else { whole = "0"; frac = std::string((size_t)(-e - 1), '0') + digits; }
        return sign + whole + "." + (frac.empty() ? "0" : frac);
    }
    return sign + digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(e);
}

namespace {
// the lines of a text (the last one may lack its newline), each split at tabs with trailing empty fields dropped, as Java's split does
template <class F> void each_line(const char *t, size_t n, F f) {
    size_t at = 0;
    std::vector<std::string> fields;
    while (at < n) {
        const char *nl = (const char *)std::memchr(t + at, '\n', n - at);
        const size_t end = nl ? (size_t)(nl - t) : n;
        fields.clear();
        size_t s = at;
        for (size_t i = at; i <= end; ++i) if (i == end || t[i] == '\t') { fields.emplace_back(t + s, i - s); s = i + 1; }
        while (!fields.empty() && fields.back().empty()) fields.pop_back();
        f(fields);
        at = end + 1;
    }
}
}  // namespace

bool hits_filter(const char *t, size_t n, std::string &out, std::string &err) {
    bool ok = true; long long line = 0;
    each_line(t, n, [&](const std::vector<std::string> &f) {
        ++line;
        if (f.size() > 1) {                                          // :1008
            if (f.size() < 12) { if (ok) err = "line " + std::to_string(line) + " of the hit table has " + std::to_string(f.size()) + " fields, the score is field 11"; ok = false; return; }
            out += f[0] + "\t" + f[1] + "\t" + f[11] + "\n";         // :1009-1010
        }
    });
    return ok;
}

void hits_bidirectional(const char *t, size_t n, int score_field, std::string &out) {
    std::map<std::pair<std::string, std::string>, float> stored;    // :947; IntPair.java:12-21: unordered
    each_line(t, n, [&](const std::vector<std::string> &f) {
        if ((int)f.size() > score_field) {                           // :951
            const auto key = f[0] < f[1] ? std::make_pair(f[0], f[1]) : std::make_pair(f[1], f[0]);
            auto it = stored.find(key);
            if (it == stored.end()) stored[key] = std::strtof(f[(size_t)score_field].c_str(), nullptr);       // :958-961
            else {                                                   // :962-973
                out += f[0] + "\t" + f[1] + "\t" + f[(size_t)score_field] + "\n";
                out += f[1] + "\t" + f[0] + "\t" + java_float_to_string(it->second) + "\n";
                stored.erase(it);
            }
        }
    });
}

bool abc_parse(const char *t, size_t n, std::vector<std::string> &labels, std::vector<int> &a, std::vector<int> &b, std::vector<double> &w, std::string &err) {
    std::map<std::string, int> index;
    size_t at = 0; long long line = 0;
    while (at < n) {
        const char *nl = (const char *)std::memchr(t + at, '\n', n - at);
        const size_t end = nl ? (size_t)(nl - t) : n;
        ++line;
        std::vector<std::string> f;
        for (size_t i = at; i < end;) {
            while (i < end && (t[i] == ' ' || t[i] == '\t' || t[i] == '\r')) ++i;
            size_t s = i;
            while (i < end && !(t[i] == ' ' || t[i] == '\t' || t[i] == '\r')) ++i;
            if (i > s) f.emplace_back(t + s, i - s);
        }
        at = end + 1;
        if (f.size() < 2) continue;
        int id[2];
        for (int k = 0; k < 2; ++k) {
            auto it = index.find(f[(size_t)k]);
            if (it == index.end()) { it = index.emplace(f[(size_t)k], (int)labels.size()).first; labels.push_back(f[(size_t)k]); }
            id[k] = it->second;
        }
        double weight = 1.0;
        if (f.size() > 2) {
            char *e = nullptr;
            weight = std::strtod(f[2].c_str(), &e);
            if (e == f[2].c_str() || *e) { err = "line " + std::to_string(line) + ": the weight '" + f[2] + "' is not a number"; return false; }
        }
        a.push_back(id[0]); b.push_back(id[1]); w.push_back(weight);
    }
    return true;
}

void homolog_select(int nclusters, const long long *off, const int *members, const int *taxon_of_node, int min_taxa, int max_taxa, bool rep_only, int target_ntax,
                    int target_min_gene, std::vector<int> &kept) {
    kept.clear();
    std::vector<int> ntax((size_t)nclusters, 0);
    for (int k = 0; k < nclusters; ++k) {
        const long long size = off[k + 1] - off[k];
        if (size < min_taxa || size > max_taxa) continue;            // SequenceSetProviderImpl.java:126-127: a sequence count
        std::set<int> taxa;
        for (long long i = off[k]; i < off[k + 1]; ++i) taxa.insert(taxon_of_node[members[i]]);
        ntax[(size_t)k] = (int)taxa.size();
        if (rep_only && (long long)taxa.size() != size) continue;    // :223-247
        kept.push_back(k);
    }
    if ((int)kept.size() > target_min_gene)                          // PhylogenomicPipeline2.java:580
        for (int t = min_taxa + 1; t <= target_ntax; ++t) {          // :583
            int have = 0;
            for (int k : kept) have += ntax[(size_t)k] >= t;         // :584, SequenceSetProviderImpl.java:320-329
            if (have >= target_min_gene)                             // :591, :295-312
                kept.erase(std::remove_if(kept.begin(), kept.end(), [&](int k) { return ntax[(size_t)k] < t; }), kept.end());
        }
}

}  // namespace pml

using namespace pml;

extern "C" int pml_mcl_class_limits(int *limits_out) {
    if (!limits_out) return PML_EINVAL;
    limits_out[0] = MCL_PACKED_MAX; limits_out[1] = MCL_LDS_MAX; limits_out[2] = MCL_TILE; limits_out[3] = 0;
    return PML_OK;
}

extern "C" int pml_mcl_cluster_host(int n, long long narcs, const int *a, const int *b, const double *w, const pml_mcl_opts *opts, int *cluster_of_out,
                                    int *nclusters_out, int *iters_out) {
    if (n < 0 || narcs < 0 || (narcs > 0 && (!a || !b || !w)) || (n > 0 && !cluster_of_out) || !nclusters_out) return PML_EINVAL;
    try {
        const MclOpts o = mcl_resolve(opts);
        if (!(o.inflation > 0) || !(o.prune_inverse > 0) || o.max_iter < 1) return PML_EINVAL;
        MclGraph g; std::string err;
        if (!mcl_build_graph(n, narcs, a, b, w, g, err)) return PML_EINVAL;
        std::vector<int> best((size_t)n);
        std::vector<unsigned> mask;
        std::vector<double> M, tmp;
        int iters = 0;
        for (int c = 0; c < g.ncomp(); ++c) {
            const int m = g.size(c);
            mcl_fill_host(g, c, M);
            int it = 0;
            while (it < o.max_iter) { const double chaos = mcl_step_host(m, M, tmp, o); ++it; if (chaos < o.chaos_eps) break; }
            iters = std::max(iters, it);
            const size_t moff = mask.size();
            mask.resize(moff + (size_t)m * mcl_words(m));
            mcl_read_host(m, M, best.data() + g.comp_off[(size_t)c], mask.data() + moff);
        }
        mcl_finish(g, best.data(), mask.data(), cluster_of_out, nclusters_out);
        if (iters_out) *iters_out = iters;
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

static char *dup_text(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }

extern "C" int pml_hits_filter_host(const char *table, long long table_bytes, char **text_out) {
    if (table_bytes < 0 || (table_bytes > 0 && !table) || !text_out) return PML_EINVAL;
    try {
        std::string out, err;
        if (!hits_filter(table, (size_t)table_bytes, out, err)) return PML_EINVAL;
        if (!(*text_out = dup_text(out))) return PML_ENOMEM;
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_hits_bidirectional_host(const char *table, long long table_bytes, int score_field, char **text_out) {
    if (table_bytes < 0 || (table_bytes > 0 && !table) || score_field < 2 || !text_out) return PML_EINVAL;
    try {
        std::string out;
        hits_bidirectional(table, (size_t)table_bytes, score_field, out);
        if (!(*text_out = dup_text(out))) return PML_ENOMEM;
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_homolog_select_host(int nclusters, const long long *cluster_off, const int *members, const int *taxon_of_node, int min_taxa, int max_taxa,
                                       int rep_only, int target_ntax, int target_min_gene, int *kept_out, int *nkept_out) {
    if (nclusters < 0 || !cluster_off || (nclusters > 0 && (!members || !taxon_of_node || !kept_out)) || !nkept_out) return PML_EINVAL;
    try {
        std::vector<int> kept;
        homolog_select(nclusters, cluster_off, members, taxon_of_node, min_taxa, max_taxa, rep_only != 0, target_ntax, target_min_gene, kept);
        std::copy(kept.begin(), kept.end(), kept_out);
        *nkept_out = (int)kept.size();
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}
