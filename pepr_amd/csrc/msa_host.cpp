// msa_host.cpp -- the multiple-alignment rule of include/peprml.h ("Multiple alignment") in plain C++: encoding, the guide tree, the
// profile-profile DP with its traceback, the merge of two clusters' rows and the progressive alignment of whole sets
// (pml_msa_align_host: the CPU tests' subject and the timing baseline of tools/measure_msa.py).  The device driver (msa.cpp)
// shares the encoding, the tree, the bound and the result's layout.  No HIP, no context: builds alone (with sw_host.cpp and
// nj.cpp) under host sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "msa.hpp"
#include "nj.hpp"
#include "sw.hpp"

namespace pml {

bool msa_resolve(const pml_msa_opts *o, MsaOpts &r, std::string &err) {
    r.open = 11; r.ext = 1; r.maxabs = 0;
    const int *tab = nullptr;
    if (o) {
        if (o->gap_open < 0 || o->gap_extend < 0) { err = "gap costs must not be negative"; return false; }
        if (o->gap_open > (1 << 20) || o->gap_extend > (1 << 20)) { err = "gap costs above 2^20 are not supported"; return false; }
        if (o->gap_open) r.open = o->gap_open;
        if (o->gap_extend) r.ext = o->gap_extend;
        tab = o->table576;
    }
    if (tab) std::memcpy(r.table, tab, sizeof r.table); else blosum62_as_loaded(r.table);
    for (int i = 0; i < 576; ++i) {
        if (r.table[i] < -128 || r.table[i] > 127) { err = "a table entry does not fit int8"; return false; }
        if (i / 24 < MSA_GAP && i % 24 < MSA_GAP) r.maxabs = std::max(r.maxabs, std::abs(r.table[i]));
    }
    return true;
}

void msa_guide_tree(int n, const long long *S, std::vector<MsaMerge> &merges) {
    merges.clear();
    if (n < 2) return;
    std::vector<long long> sum((size_t)n * n, 0);                        // symmetric: the sum of S over the cross pairs of two live clusters
    for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) sum[(size_t)a * n + b] = sum[(size_t)b * n + a] = S[(size_t)a * n + b];
    std::vector<int> size((size_t)n, 1), level((size_t)n, 0);
    std::vector<char> live((size_t)n, 1);
    for (int step = 0; step + 1 < n; ++step) {
        int ba = -1, bb = -1;
        for (int a = 0; a < n; ++a) {
            if (!live[(size_t)a]) continue;
            for (int b = a + 1; b < n; ++b) {
                if (!live[(size_t)b]) continue;
                if (ba >= 0) {                                           // strictly larger average only: ties stay with the lowest ids
                    const __int128 lhs = (__int128)sum[(size_t)a * n + b] * ((__int128)size[(size_t)ba] * size[(size_t)bb]);
                    const __int128 rhs = (__int128)sum[(size_t)ba * n + bb] * ((__int128)size[(size_t)a] * size[(size_t)b]);
                    if (!(lhs > rhs)) continue;
                }
                ba = a; bb = b;
            }
        }
        const int lv = 1 + std::max(level[(size_t)ba], level[(size_t)bb]);
        merges.push_back({ba, bb, lv});
        for (int k = 0; k < n; ++k) {
            if (!live[(size_t)k] || k == ba || k == bb) continue;
            sum[(size_t)ba * n + k] = sum[(size_t)k * n + ba] = sum[(size_t)ba * n + k] + sum[(size_t)bb * n + k];
        }
        size[(size_t)ba] += size[(size_t)bb]; level[(size_t)ba] = lv; live[(size_t)bb] = 0;
    }
}

void msa_member_orders(int n, const std::vector<MsaMerge> &merges, std::vector<std::vector<int>> &order) {
    order.assign((size_t)n, std::vector<int>());
    for (int i = 0; i < n; ++i) order[(size_t)i].push_back(i);
    for (const MsaMerge &m : merges) {
        order[(size_t)m.x].insert(order[(size_t)m.x].end(), order[(size_t)m.y].begin(), order[(size_t)m.y].end());
        order[(size_t)m.y].clear();
    }
}

std::string msa_refusal(int nX, int nY, int LX, int LY, const MsaOpts &o) {
    const __int128 w = (__int128)nX * nY;
    const __int128 need = w * ((__int128)(o.maxabs + o.open) * (std::min(LX, LY) + 1) + (__int128)o.ext * ((long long)LX + LY));
    if (need >= ((__int128)1 << 30))
        return "profiles of " + std::to_string(nX) + " x " + std::to_string(LX) + " and " + std::to_string(nY) + " x " + std::to_string(LY) +
               " (rows x columns): w ((M + gap_open) (min(LX, LY) + 1) + gap_extend (LX + LY)) = " +
               (need > (__int128)INT64_MAX ? std::string("more than 2^63") : std::to_string((long long)need)) + " is not below the int32 bound 2^30 = 1073741824";
    if (nX > MSA_MAX_NX || nY > MSA_MAX_NY)
        return "profiles of " + std::to_string(nX) + " and " + std::to_string(nY) + " rows: the int16 counts take at most " + std::to_string(MSA_MAX_NX) + " rows of X and " +
               std::to_string(MSA_MAX_NY) + " of Y";
    return std::string();
}

namespace {

void column_counts(const MsaProfile &P, std::vector<int> &c) {
    c.assign((size_t)P.L * MSA_GAP, 0);
    for (int r = 0; r < P.n; ++r)
        for (int i = 0; i < P.L; ++i) { const int a = P.rows[(size_t)r * P.L + i]; if (a < MSA_GAP) c[(size_t)i * MSA_GAP + a]++; }
}

}  // namespace

long long msa_profile_align_rule(const MsaProfile &X, const MsaProfile &Y, const MsaOpts &o, std::vector<uint8_t> &path) {
    const int LX = X.L, LY = Y.L, NEG = MSA_NEG;
    const int w = X.n * Y.n, GO = o.open * w, GE = o.ext * w;
    std::vector<int> cX, cY;
    column_counts(X, cX); column_counts(Y, cY);
    std::vector<int> V((size_t)LY * MSA_GAP, 0);                         // V_j[a] = Sum_b cY[j][b] T[a][b]
    for (int j = 0; j < LY; ++j)
        for (int a = 0; a < MSA_GAP; ++a) {
            int v = 0;
            for (int b = 0; b < MSA_GAP; ++b) v += cY[(size_t)j * MSA_GAP + b] * o.table[a * 24 + b];
            V[(size_t)j * MSA_GAP + a] = v;
        }
    auto s = [&](int i, int j) {                                         // 1-based
        int v = 0;
        const int *c = &cX[(size_t)(i - 1) * MSA_GAP], *vj = &V[(size_t)(j - 1) * MSA_GAP];
        for (int a = 0; a < MSA_GAP; ++a) v += c[a] * vj[a];
        return v;
    };
    const size_t W = (size_t)LY + 1, cells = ((size_t)LX + 1) * W;
    std::vector<int> H(cells, NEG), E(cells, NEG), F(cells, NEG);
    H[0] = 0;
    for (int i = 0; i <= LX; ++i) {
        const int oe = (i == 0 || i == LX ? 0 : GO) + GE;
        for (int j = 0; j <= LY; ++j) {
            if (i == 0 && j == 0) continue;
            const size_t c = (size_t)i * W + j;
            const int of = (j == 0 || j == LY ? 0 : GO) + GE;
            int h = NEG;
            if (j >= 1) { E[c] = std::max(E[c - 1] - GE, H[c - 1] - oe); h = E[c]; }
            if (i >= 1) { F[c] = std::max(F[c - W] - GE, H[c - W] - of); h = std::max(h, F[c]); }
            if (i >= 1 && j >= 1) h = std::max(h, H[c - W - 1] + s(i, j));
            H[c] = h;
        }
    }
    path.clear();
    int i = LX, j = LY, state = 0;                                        // 0 H, 1 E, 2 F
    while (i > 0 || j > 0) {
        const size_t c = (size_t)i * W + j;
        if (state == 0) {
            if (i > 0 && j > 0 && H[c] == H[c - W - 1] + s(i, j)) { path.push_back(0); --i; --j; }
            else if (j > 0 && H[c] == E[c]) state = 1;
            else state = 2;
        } else if (state == 1) {
            const int oe = (i == 0 || i == LX ? 0 : GO) + GE;
            path.push_back(1);
            if (E[c] == H[c - 1] - oe) state = 0;
            --j;
        } else {
            const int of = (j == 0 || j == LY ? 0 : GO) + GE;
            path.push_back(2);
            if (F[c] == H[c - W] - of) state = 0;
            --i;
        }
    }
    std::reverse(path.begin(), path.end());
    return H[cells - 1];
}

void msa_merge_rows(const MsaProfile &X, const MsaProfile &Y, const std::vector<uint8_t> &path, MsaProfile &out) {
    out.n = X.n + Y.n; out.L = (int)path.size();
    out.rows.assign((size_t)out.n * out.L, (uint8_t)MSA_GAP);
    int i = 0, j = 0;
    for (int c = 0; c < out.L; ++c) {
        if (path[(size_t)c] != 1) { for (int r = 0; r < X.n; ++r) out.rows[(size_t)r * out.L + c] = X.rows[(size_t)r * X.L + i]; ++i; }
        if (path[(size_t)c] != 2) { for (int r = 0; r < Y.n; ++r) out.rows[(size_t)(X.n + r) * out.L + c] = Y.rows[(size_t)r * Y.L + j]; ++j; }
    }
}

bool msa_encode_sets(int nsets, const pml_msa_set *sets, MsaInput &in, std::string &err) {
    in.set_off.assign(1, 0); in.off.assign(1, 0); in.codes.clear();
    for (int s = 0; s < nsets; ++s) {
        if (sets[s].nseq < 1 || !sets[s].residues) { err = "set " + std::to_string(s) + " has no sequence"; return false; }
        for (int k = 0; k < sets[s].nseq; ++k) {
            const char *res = sets[s].residues[k];
            const std::string who = "set " + std::to_string(s) + ", sequence " + std::to_string(k);
            if (!res) { err = who + ": a null sequence"; return false; }
            const size_t n = std::strlen(res), at = in.codes.size();
            if (n == 0) { err = who + " is empty"; return false; }
            if (n > (size_t)SW_MAX_LEN) { err = who + " has " + std::to_string(n) + " residues, the limit is 65535"; return false; }
            in.codes.resize(at + n);
            long long bad = 0;
            if (sw_encode_residues(res, n, in.codes.data() + at, &bad)) {
                err = who + ": byte " + std::to_string((int)(unsigned char)res[bad]) + " at position " + std::to_string(bad) + " is no residue";
                return false;
            }
            in.off.push_back((long long)in.codes.size());
        }
        in.set_off.push_back((int)in.off.size() - 1);
    }
    return true;
}

bool msa_encode_profile(const pml_msa_set *a, const char *what, MsaProfile &p, std::string &err) {
    if (!a || a->nseq < 1 || !a->residues) { err = std::string("profile ") + what + " has no row"; return false; }
    p.n = a->nseq; p.L = -1;
    for (int r = 0; r < p.n; ++r) {
        const char *row = a->residues[r];
        const std::string who = std::string("profile ") + what + ", row " + std::to_string(r);
        if (!row) { err = who + ": a null row"; return false; }
        const size_t n = std::strlen(row);
        if (p.L < 0) {
            if (n == 0) { err = who + " is empty"; return false; }
            if (n > (size_t)SW_MAX_LEN) { err = who + " has " + std::to_string(n) + " columns, the limit is 65535"; return false; }
            p.L = (int)n; p.rows.assign((size_t)p.n * n, (uint8_t)MSA_GAP);
        } else if ((int)n != p.L) { err = who + " has " + std::to_string(n) + " columns, row 0 has " + std::to_string(p.L); return false; }
        for (size_t k = 0; k < n; ++k) {
            if (row[k] == '-') continue;
            long long bad = 0;
            if (sw_encode_residues(row + k, 1, &p.rows[(size_t)r * n + k], &bad)) {
                err = who + ": byte " + std::to_string((int)(unsigned char)row[k]) + " at position " + std::to_string(k) + " is neither a residue nor `-`";
                return false;
            }
        }
    }
    return true;
}

int msa_fill_result(pml_msa_result *res, const MsaProfile &fin, const std::vector<int> &members, const MsaPlan &plan, const std::vector<uint8_t> *path) {
    static const char letters[] = "ARNDCQEGHILKMFPSTWYVBZX-";
    const size_t nm = plan.merges.size();
    res->nrows = fin.n; res->ncols = fin.L; res->nmerges = (int)nm;
    res->rows = (char *)std::malloc((size_t)fin.n * ((size_t)fin.L + 1));
    res->merge_x = (int *)std::malloc(sizeof(int) * std::max<size_t>(nm, 1));
    res->merge_y = (int *)std::malloc(sizeof(int) * std::max<size_t>(nm, 1));
    res->merge_level = (int *)std::malloc(sizeof(int) * std::max<size_t>(nm, 1));
    res->merge_score = (long long *)std::malloc(sizeof(long long) * std::max<size_t>(nm, 1));
    res->path = path ? (unsigned char *)std::malloc(std::max<size_t>(path->size(), 1)) : nullptr;
    if (!res->rows || !res->merge_x || !res->merge_y || !res->merge_level || !res->merge_score || (path && !res->path)) return PML_ENOMEM;
    for (int r = 0; r < fin.n; ++r) {
        char *out = res->rows + (size_t)members[(size_t)r] * ((size_t)fin.L + 1);
        for (int c = 0; c < fin.L; ++c) out[c] = letters[std::min<int>(fin.rows[(size_t)r * fin.L + c], MSA_GAP)];
        out[fin.L] = 0;
    }
    for (size_t m = 0; m < nm; ++m) {
        res->merge_x[m] = plan.merges[m].x; res->merge_y[m] = plan.merges[m].y; res->merge_level[m] = plan.merges[m].level;
        res->merge_score[m] = plan.score[m];
    }
    if (path && !path->empty()) std::memcpy(res->path, path->data(), path->size());
    return PML_OK;
}

}  // namespace pml

using namespace pml;

namespace {

int host_fail(int code, const std::string &msg, char *err, int cap) {
    if (err && cap > 0) std::snprintf(err, (size_t)cap, "%s", msg.c_str());
    return code;
}

}  // namespace

extern "C" void pml_msa_result_free(pml_msa_result *r) {
    if (!r) return;
    std::free(r->rows); std::free(r->merge_x); std::free(r->merge_y); std::free(r->merge_level); std::free(r->merge_score); std::free(r->path);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_msa_limits(int *limits_out) {
    if (!limits_out) return PML_EINVAL;
    for (int c = 0; c < MSA_CLASSES; ++c) { limits_out[2 * c] = MSA_LANES[c]; limits_out[2 * c + 1] = MSA_LANES[c] * MSA_STRIP; }
    limits_out[6] = MSA_STRIP; limits_out[7] = MSA_THREADS;
    return PML_OK;
}

extern "C" int pml_msa_guide_tree_host(int n, const long long *scores, int *merge_x, int *merge_y, int *merge_level) {
    if (n < 1 || (n > 1 && (!scores || !merge_x || !merge_y || !merge_level))) return PML_EINVAL;
    try {
        std::vector<MsaMerge> merges;
        msa_guide_tree(n, scores, merges);
        for (size_t m = 0; m < merges.size(); ++m) { merge_x[m] = merges[m].x; merge_y[m] = merges[m].y; merge_level[m] = merges[m].level; }
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_msa_align_host(int nsets, const pml_msa_set *sets, const pml_msa_opts *opts, pml_msa_result *results, char *err, int err_cap) {
    if (results && nsets > 0) std::memset(results, 0, sizeof *results * (size_t)nsets);
    if (nsets < 0 || (nsets > 0 && (!sets || !results))) return host_fail(PML_EINVAL, "null arguments", err, err_cap);
    int rc = PML_OK; std::string msg;
    try {
        MsaOpts o; MsaInput in;
        if (!msa_resolve(opts, o, msg) || !msa_encode_sets(nsets, sets, in, msg)) return host_fail(PML_EINVAL, msg, err, err_cap);
        SwOpts so = SwOpts(); so.open = o.open; so.ext = o.ext; std::memcpy(so.table, o.table, sizeof so.table);
        for (int s = 0; s < nsets && !rc; ++s) {
            const int q0 = in.set_off[(size_t)s], n = in.set_off[(size_t)s + 1] - q0;
            std::vector<long long> S((size_t)n * n, 0);
            for (int a = 0; a < n; ++a)
                for (int b = a + 1; b < n; ++b)
                    S[(size_t)a * n + b] = sw_score_host(in.codes.data() + in.off[(size_t)q0 + a], in.len(q0 + a), in.codes.data() + in.off[(size_t)q0 + b], in.len(q0 + b), so);
            MsaPlan plan;
            msa_guide_tree(n, S.data(), plan.merges);
            std::vector<MsaProfile> cl((size_t)n);
            for (int k = 0; k < n; ++k) {
                cl[(size_t)k].n = 1; cl[(size_t)k].L = in.len(q0 + k);
                cl[(size_t)k].rows.assign(in.codes.begin() + in.off[(size_t)q0 + k], in.codes.begin() + in.off[(size_t)q0 + k + 1]);
            }
            for (const MsaMerge &m : plan.merges) {
                MsaProfile &X = cl[(size_t)m.x], &Y = cl[(size_t)m.y];
                const std::string why = msa_refusal(X.n, Y.n, X.L, Y.L, o);
                if (!why.empty()) { rc = PML_EINVAL; msg = "set " + std::to_string(s) + ", merge of clusters " + std::to_string(m.x) + " and " + std::to_string(m.y) + ": " + why; break; }
                std::vector<uint8_t> path; MsaProfile out;
                plan.score.push_back(msa_profile_align_rule(X, Y, o, path));
                msa_merge_rows(X, Y, path, out);
                X = std::move(out); Y = MsaProfile();
            }
            if (rc) break;
            std::vector<std::vector<int>> order;
            msa_member_orders(n, plan.merges, order);
            rc = msa_fill_result(results + s, cl[0], order[0], plan, nullptr);
            if (rc) msg = "host allocation failed";
        }
    } catch (const std::bad_alloc &) { rc = PML_ENOMEM; msg = "host allocation failed"; }
    if (rc) { for (int s = 0; s < nsets; ++s) pml_msa_result_free(results + s); return host_fail(rc, msg, err, err_cap); }
    return PML_OK;
}

extern "C" int pml_msa_profile_align_host(const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, long long *score_out, pml_msa_result *result,
                                          char *err, int err_cap) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!a || !b || !result) return host_fail(PML_EINVAL, "null arguments", err, err_cap);
    int rc = PML_OK; std::string msg;
    try {
        MsaOpts o; MsaProfile X, Y;
        if (!msa_resolve(opts, o, msg) || !msa_encode_profile(a, "a", X, msg) || !msa_encode_profile(b, "b", Y, msg)) return host_fail(PML_EINVAL, msg, err, err_cap);
        const std::string why = msa_refusal(X.n, Y.n, X.L, Y.L, o);
        if (!why.empty()) return host_fail(PML_EINVAL, "set 0: " + why, err, err_cap);
        std::vector<uint8_t> path; MsaProfile out; MsaPlan plan;
        plan.merges.push_back({0, X.n, 1});
        plan.score.push_back(msa_profile_align_rule(X, Y, o, path));
        msa_merge_rows(X, Y, path, out);
        std::vector<int> members((size_t)out.n);
        for (int r = 0; r < out.n; ++r) members[(size_t)r] = r;
        if (score_out) *score_out = plan.score[0];
        rc = msa_fill_result(result, out, members, plan, &path);
        if (rc) msg = "host allocation failed";
    } catch (const std::bad_alloc &) { rc = PML_ENOMEM; msg = "host allocation failed"; }
    if (rc) { pml_msa_result_free(result); return host_fail(rc, msg, err, err_cap); }
    return PML_OK;
}
