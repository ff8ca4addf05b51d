// sw_host.cpp -- the homology-search rule of include/peprml.h ("Homology search") in plain C++: encoding, the row-by-row affine-gap
// Smith-Waterman score, the per-genome selection, statistics, the table text and the traceback (pml_sw_search_host: the CPU
// tests' subject and the timing baseline of tools/measure_sw.py).  The device driver (sw.cpp) shares the encoding and everything
// behind the selection keys.  No HIP, no context: builds alone under host sanitizers.
#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "nj.hpp"
#include "sw.hpp"

namespace pml {

bool sw_resolve(const pml_sw_opts *o, SwOpts &r, std::string &err) {
    r.open = 11; r.ext = 1; r.lambda = 0.267; r.K = 0.041; r.evalue = 0.1; r.traceback = false;
    const int *tab = nullptr;
    if (o) {
        if (o->gap_open < 0 || o->gap_extend < 0) { err = "gap costs must not be negative"; return false; }
        if (o->gap_open > (1 << 20) || o->gap_extend > (1 << 20)) { err = "gap costs above 2^20 are not supported"; return false; }
        if (o->hits_per_query != 0 && o->hits_per_query != 1) { err = "hits_per_query other than 1 is not built"; return false; }
        if (o->traceback != 0 && o->traceback != 1) { err = "traceback is 0 or 1"; return false; }
        if (o->gap_open) r.open = o->gap_open;
        if (o->gap_extend) r.ext = o->gap_extend;
        if (o->lambda != 0) r.lambda = o->lambda;
        if (o->K != 0) r.K = o->K;
        if (o->evalue != 0) r.evalue = o->evalue;
        if (!(r.lambda > 0) || !(r.K > 0) || !(r.evalue > 0) || !std::isfinite(r.lambda) || !std::isfinite(r.K)) { err = "lambda, K and evalue must be > 0"; return false; }
        r.traceback = o->traceback != 0;
        tab = o->table576;
    }
    if (tab) std::memcpy(r.table, tab, sizeof r.table); else blosum62_as_loaded(r.table);
    for (int i = 0; i < 576; ++i) if (r.table[i] < -128 || r.table[i] > 127) { err = "a table entry does not fit int8"; return false; }
    return true;
}

int sw_encode_residues(const char *text, size_t n, uint8_t *out, long long *bad_pos) {
    static const struct Lut { int8_t code[256]; Lut() {
        static const char order[] = "ARNDCQEGHILKMFPSTWYVBZX";
        for (int i = 0; i < 256; ++i) code[i] = -1;
        for (int i = 0; order[i]; ++i) { code[(unsigned char)order[i]] = (int8_t)i; code[(unsigned char)(order[i] - 'A' + 'a')] = (int8_t)i; }
        for (const char *c = "JOUjou"; *c; ++c) code[(unsigned char)*c] = 22;
    } } lut;
    for (size_t k = 0; k < n; ++k) {
        const int c = lut.code[(unsigned char)text[k]];
        if (c < 0) { if (bad_pos) *bad_pos = (long long)k; return -1; }
        out[k] = (uint8_t)c;
    }
    return 0;
}

bool sw_encode(const pml_proteome_set *set, SwSet &s, std::string &err) {
    if (!set || set->ngenomes < 0 || (set->ngenomes > 0 && !set->genome_off)) { err = "the proteome set is malformed"; return false; }
    s.G = set->ngenomes;
    s.genome_off.assign(1, 0);
    for (int g = 0; g < s.G; ++g) {
        if (set->genome_off[g + 1] < set->genome_off[g] || set->genome_off[0] != 0) { err = "genome_off must start at 0 and not decrease"; return false; }
        s.genome_off.push_back(set->genome_off[g + 1]);
    }
    s.np = s.G ? s.genome_off.back() : 0;
    if (s.np > 0 && (!set->labels || !set->residues)) { err = "the proteome set is malformed"; return false; }
    s.off.assign(1, 0);
    s.genome_res.assign((size_t)s.G, 0);
    for (int g = 0; g < s.G; ++g)
        for (int p = s.genome_off[(size_t)g]; p < s.genome_off[(size_t)g + 1]; ++p) {
            const char *lab = set->labels[p], *res = set->residues[p];
            if (!lab || !res) { err = "protein " + std::to_string(p) + ": a null label or sequence"; return false; }
            size_t a = 0;
            while (lab[a] && std::isspace((unsigned char)lab[a])) ++a;
            size_t b = a;
            while (lab[b] && !std::isspace((unsigned char)lab[b])) ++b;
            s.label.emplace_back(lab + a, b - a);
            const size_t n = std::strlen(res);
            if (n > (size_t)SW_MAX_LEN) { err = "protein " + std::to_string(p) + " ('" + s.label.back() + "') has " + std::to_string(n) + " residues, the limit is 65535"; return false; }
            const size_t at = s.codes.size();
            s.codes.resize(at + n);
            long long bad = 0;
            if (sw_encode_residues(res, n, s.codes.data() + at, &bad)) {
                err = "protein " + std::to_string(p) + " ('" + s.label.back() + "'): byte " + std::to_string((int)(unsigned char)res[bad]) + " at position " + std::to_string(bad) + " is no residue";
                return false;
            }
            s.off.push_back((long long)s.codes.size());
            s.genome_of.push_back(g); s.pos_in_genome.push_back(p - s.genome_off[(size_t)g]);
            s.genome_res[(size_t)g] += (long long)n;
        }
    return true;
}

long long sw_total_cells(const SwSet &s) {
    long long all = 0, total = 0;
    for (int g = 0; g < s.G; ++g) all += s.genome_res[(size_t)g];
    for (int p = 0; p < s.np; ++p) total += (long long)s.len(p) * all;
    return total;
}

int sw_score_host(const uint8_t *q, int m, const uint8_t *t, int n, const SwOpts &o) {
    if (m <= 0 || n <= 0) return 0;
    const int NEG = INT32_MIN / 2, oe = o.open + o.ext;
    std::vector<int> H((size_t)n + 1, 0), F((size_t)n + 1, NEG);       // the previous row's H, this column's F
    int best = 0;
    for (int i = 0; i < m; ++i) {
        const int *row = o.table + q[i] * 24;
        int diag = 0, left = 0, e = NEG;                                // H[i-1][j-1], H[i][j-1], E[i][j-1]
        for (int j = 1; j <= n; ++j) {
            e = std::max(e - o.ext, left - oe);
            const int f = F[(size_t)j] = std::max(F[(size_t)j] - o.ext, H[(size_t)j] - oe);
            const int h = std::max(std::max(0, diag + row[t[j - 1]]), std::max(e, f));
            diag = H[(size_t)j]; H[(size_t)j] = left = h;
            best = std::max(best, h);
        }
    }
    return best;
}

namespace {

struct Trace { int length = 0, ident = 0, mismatch = 0, gapopen = 0, qs = 0, qe = 0, ss = 0, se = 0; };

bool sw_traceback(const uint8_t *q, int m, const uint8_t *t, int n, const SwOpts &o, Trace &tr) {
    const size_t W = (size_t)n + 1, cells = ((size_t)m + 1) * W;
    if (cells > ((size_t)1 << 28)) return false;
    const int NEG = INT32_MIN / 2, oe = o.open + o.ext;
    std::vector<int> H(cells, 0), E(cells, NEG), F(cells, NEG);
    int best = 0, bi = 0, bj = 0;
    for (int i = 1; i <= m; ++i)
        for (int j = 1; j <= n; ++j) {
            const size_t c = (size_t)i * W + j;
            E[c] = std::max(E[c - 1] - o.ext, H[c - 1] - oe);
            F[c] = std::max(F[c - W] - o.ext, H[c - W] - oe);
            H[c] = std::max(std::max(0, H[c - W - 1] + o.table[q[i - 1] * 24 + t[j - 1]]), std::max(E[c], F[c]));
            if (H[c] > best) { best = H[c]; bi = i; bj = j; }          // strict: the first maximal cell in row-major order
        }
    tr = Trace();
    if (best <= 0) return true;
    int i = bi, j = bj, state = 0;                                      // 0 H, 1 E, 2 F
    tr.qe = bi; tr.se = bj;
    for (;;) {
        const size_t c = (size_t)i * W + j;
        if (state == 0) {
            if (H[c] == 0) break;
            if (H[c] == H[c - W - 1] + o.table[q[i - 1] * 24 + t[j - 1]]) {
                tr.length++; if (q[i - 1] == t[j - 1]) tr.ident++; else tr.mismatch++;
                --i; --j;
            } else if (H[c] == E[c]) { state = 1; tr.gapopen++; }
            else { state = 2; tr.gapopen++; }
        } else if (state == 1) {
            tr.length++;
            if (E[c] == H[c - 1] - oe) state = 0;
            --j;
        } else {
            tr.length++;
            if (F[c] == H[c - W] - oe) state = 0;
            --i;
        }
    }
    tr.qs = i + 1; tr.ss = j + 1;
    return true;
}

template <class T> T *dup_array(const std::vector<T> &v) {
    T *p = (T *)std::malloc(sizeof(T) * std::max<size_t>(v.size(), 1));
    if (p && !v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

}  // namespace

int sw_finish(const SwSet &s, const SwOpts &o, const std::vector<unsigned long long> &best, long long cells, pml_sw_result *res, std::string &err) {
    std::vector<int> hq, hs, hg, hsc; std::vector<double> hb, he;
    std::string text;
    char buf[256];
    for (int g = 0; g < s.G; ++g)
        for (int q = 0; q < s.np; ++q) {
            const unsigned long long key = best[(size_t)q * s.G + g];
            const int S = sw_key_score(key);
            if (!key || S <= 0 || s.len(q) == 0) continue;
            const int pos = sw_key_pos(key);
            if (pos < 0 || pos >= s.genome_off[(size_t)g + 1] - s.genome_off[(size_t)g]) { err = "internal: a winner's position is " + std::to_string(pos); return PML_EDEVICE; }
            const int sub = s.genome_off[(size_t)g] + pos;
            const double ev = o.K * (double)s.len(q) * (double)s.genome_res[(size_t)g] * std::exp(-o.lambda * (double)S);
            if (!(ev <= o.evalue)) continue;
            const double bits = (o.lambda * (double)S - std::log(o.K)) / std::log(2.0);
            Trace tr;
            if (o.traceback && !sw_traceback(s.codes.data() + s.off[(size_t)q], s.len(q), s.codes.data() + s.off[(size_t)sub], s.len(sub), o, tr)) {
                err = "the traceback of '" + s.label[(size_t)q] + "' against '" + s.label[(size_t)sub] + "' needs more than 2^28 cells"; return PML_ENOMEM;
            }
            text += s.label[(size_t)q]; text += '\t'; text += s.label[(size_t)sub];
            if (o.traceback) std::snprintf(buf, sizeof buf, "\t%.2f\t%d\t%d\t%d\t%d\t%d\t%d\t%d", tr.length ? 100.0 * tr.ident / tr.length : 0.0, tr.length, tr.mismatch, tr.gapopen, tr.qs, tr.qe, tr.ss, tr.se);
            else std::snprintf(buf, sizeof buf, "\t0\t0\t0\t0\t0\t0\t0\t0");
            text += buf;
            std::snprintf(buf, sizeof buf, "\t%.2e\t%.1f\n", ev, bits);
            text += buf;
            hq.push_back(q); hs.push_back(sub); hg.push_back(g); hsc.push_back(S); hb.push_back(bits); he.push_back(ev);
        }
    res->nhits = (long long)hq.size(); res->cells = cells;
    res->query = dup_array(hq); res->subject = dup_array(hs); res->target_genome = dup_array(hg); res->score = dup_array(hsc);
    res->bits = dup_array(hb); res->evalue = dup_array(he);
    res->table = (char *)std::malloc(text.size() + 1);
    res->table_bytes = (long long)text.size();
    if (!res->query || !res->subject || !res->target_genome || !res->score || !res->bits || !res->evalue || !res->table) { err = "host allocation failed"; return PML_ENOMEM; }
    std::memcpy(res->table, text.c_str(), text.size() + 1);
    return PML_OK;
}

}  // namespace pml

using namespace pml;

extern "C" void pml_sw_result_free(pml_sw_result *r) {
    if (!r) return;
    std::free(r->query); std::free(r->subject); std::free(r->target_genome); std::free(r->score); std::free(r->bits); std::free(r->evalue); std::free(r->table);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_sw_class_limits(int *limits_out) {
    if (!limits_out) return PML_EINVAL;
    for (int c = 0; c < SW_CLASSES; ++c) { limits_out[2 * c] = SW_LANES[c]; limits_out[2 * c + 1] = SW_LANES[c] * SW_STRIP; }
    limits_out[6] = SW_STRIP; limits_out[7] = SW_CHUNK_DEFAULT;
    return PML_OK;
}

extern "C" int pml_sw_search_host(const pml_proteome_set *set, const pml_sw_opts *opts, pml_sw_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!set || !result) return PML_EINVAL;
    int rc = PML_OK;
    try {
        SwOpts o; SwSet s; std::string err;
        if (!sw_resolve(opts, o, err) || !sw_encode(set, s, err)) return PML_EINVAL;
        std::vector<unsigned long long> best((size_t)s.np * std::max(s.G, 1), 0ull);
        for (int q = 0; q < s.np; ++q) {
            if (!s.len(q)) continue;
            for (int g = 0; g < s.G; ++g)
                for (int p = s.genome_off[(size_t)g]; p < s.genome_off[(size_t)g + 1]; ++p) {
                    if (!s.len(p)) continue;
                    const int S = sw_score_host(s.codes.data() + s.off[(size_t)q], s.len(q), s.codes.data() + s.off[(size_t)p], s.len(p), o);
                    unsigned long long &b = best[(size_t)q * s.G + g];
                    b = std::max(b, sw_key(S, s.pos_in_genome[(size_t)p]));
                }
        }
        rc = sw_finish(s, o, best, sw_total_cells(s), result, err);
    } catch (const std::bad_alloc &) { rc = PML_ENOMEM; }
    if (rc) pml_sw_result_free(result);
    return rc;
}
