// nj.cpp -- the reference's `nj` tree-building method on the host, restated from the Java (package edu.vt.vbi.ci.pepr):
//   alignment/AlignmentUtilities.java:174-342   convertAminaAcidSequenceToInts     -> nj_encode24
//   alignment/AlignmentUtilities.java:371-398   loadScoringMatrixFromResource      -> blosum62_as_loaded
//   tree/TreeBuilder.java:152-344, 346-362      getNJTreeString, convertSimilarityToDistanceMatrix -> nj_tree_string
//   tree/TreeBuilder.java:34-140                getNJTopology                      -> nj_topology
//   tree/TreeBuilder.java:702-748               getMinValueCoordinates / getMaxValueCoordinates
// The trees are a fixed sequence of IEEE double operations: every expression below keeps the Java's operand order and
// grouping, and contraction into fused multiply-adds is off, so that a length is the same bits as the Java's.  The quirks
// are kept (they are the contract): the similarity-to-distance shift leaves a non-zero diagonal, row sums include it, the
// merged node gets a zero diagonal, the last three lengths are not clamped.
// Plain C++, no HIP include: `g++ -c nj.cpp` builds it alone (tests/nj_standalone).
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)
#endif              // g++ knows neither pragma: build this file with -ffp-contract=off there (x86-64 without -mfma has no FMA to contract into)
#include "nj.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../include/peprml.h"

namespace pml {

namespace {
struct Lut24 {
    int8_t code[256];
    Lut24() {
        static const char order[] = "ARNDCQEGHILKMFPSTWYVBZX";
        for (int i = 0; i < 256; ++i) code[i] = -1;
        for (int i = 0; order[i]; ++i) { code[(unsigned char)order[i]] = (int8_t)i; code[(unsigned char)(order[i] - 'A' + 'a')] = (int8_t)i; }
        code[(unsigned char)'-'] = NJ_GAP; code[(unsigned char)'?'] = NJ_GAP;
    }
};
}  // namespace

int nj_encode24(const char *row, int n, uint8_t *out, int *bad_col, int *bad_byte) {
    static const Lut24 lut;                             // a function-local static: initialised once, thread-safe (C++11)
    for (int k = 0; k < n; ++k) {
        const int c = lut.code[(unsigned char)row[k]];
        if (c < 0) { if (bad_col) *bad_col = k; if (bad_byte) *bad_byte = (unsigned char)row[k]; return -1; }
        out[k] = (uint8_t)c;
    }
    return 0;
}

// BLOSUM62 (Henikoff & Henikoff 1992) as NCBI publishes it with the J column, at a scale of ln(2)/2: the rows and columns
// A R N D C Q E G H I L K M F P S T W Y V B J Z.  The X and * lines of the file never reach the Java's table.
static const int8_t BLOSUM62_FILE[23][23] = {
    {  4, -1, -2, -2,  0, -1, -1,  0, -2, -1, -1, -1, -1, -2, -1,  1,  0, -3, -2,  0, -2, -1, -1},   // A
    { -1,  5,  0, -2, -3,  1,  0, -2,  0, -3, -2,  2, -1, -3, -2, -1, -1, -3, -2, -3, -1, -2,  0},   // R
    { -2,  0,  6,  1, -3,  0,  0,  0,  1, -3, -3,  0, -2, -3, -2,  1,  0, -4, -2, -3,  4, -3,  0},   // N
    { -2, -2,  1,  6, -3,  0,  2, -1, -1, -3, -4, -1, -3, -3, -1,  0, -1, -4, -3, -3,  4, -3,  1},   // D
    {  0, -3, -3, -3,  9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1, -3, -1, -3},   // C
    { -1,  1,  0,  0, -3,  5,  2, -2,  0, -3, -2,  1,  0, -3, -1,  0, -1, -2, -1, -2,  0, -2,  4},   // Q
    { -1,  0,  0,  2, -4,  2,  5, -2,  0, -3, -3,  1, -2, -3, -1,  0, -1, -3, -2, -2,  1, -3,  4},   // E
    {  0, -2,  0, -1, -3, -2, -2,  6, -2, -4, -4, -2, -3, -3, -2,  0, -2, -2, -3, -3, -1, -4, -2},   // G
    { -2,  0,  1, -1, -3,  0,  0, -2,  8, -3, -3, -1, -2, -1, -2, -1, -2, -2,  2, -3,  0, -3,  0},   // H
    { -1, -3, -3, -3, -1, -3, -3, -4, -3,  4,  2, -3,  1,  0, -3, -2, -1, -3, -1,  3, -3,  3, -3},   // I
    { -1, -2, -3, -4, -1, -2, -3, -4, -3,  2,  4, -2,  2,  0, -3, -2, -1, -2, -1,  1, -4,  3, -3},   // L
    { -1,  2,  0, -1, -3,  1,  1, -2, -1, -3, -2,  5, -1, -3, -1,  0, -1, -3, -2, -2,  0, -3,  1},   // K
    { -1, -1, -2, -3, -1,  0, -2, -3, -2,  1,  2, -1,  5,  0, -2, -1, -1, -1, -1,  1, -3,  2, -1},   // M
    { -2, -3, -3, -3, -2, -3, -3, -3, -1,  0,  0, -3,  0,  6, -4, -2, -2,  1,  3, -1, -3,  0, -3},   // F
    { -1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4,  7, -1, -1, -4, -3, -2, -2, -3, -1},   // P
    {  1, -1,  1,  0, -1,  0,  0,  0, -1, -2, -2,  0, -1, -2, -1,  4,  1, -3, -2, -2,  0, -2,  0},   // S
    {  0, -1,  0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1,  1,  5, -2, -2,  0, -1, -1, -1},   // T
    { -3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1,  1, -4, -3, -2, 11,  2, -3, -4, -2, -2},   // W
    { -2, -2, -2, -3, -2, -1, -2, -3,  2, -1, -1, -2, -1,  3, -3, -2, -2,  2,  7, -1, -3, -1, -2},   // Y
    {  0, -3, -3, -3, -1, -2, -2, -3, -3,  3,  1, -2,  1, -1, -2, -2,  0, -3, -1,  4, -3,  2, -2},   // V
    { -2, -1,  4,  4, -3,  0,  1, -1,  0, -3, -4,  0, -3, -3, -2,  0, -1, -4, -3, -3,  4, -3,  0},   // B
    { -1, -2, -3, -3, -1, -2, -3, -4, -3,  3,  3, -3,  2,  0, -3, -2, -1, -2, -1,  2, -3,  3, -3},   // J
    { -1,  0,  0,  1, -3,  4,  4, -2,  0, -3, -3,  1, -1, -3, -1,  0, -1, -2, -2, -2,  0, -3,  4},   // Z
};

// The loader copies file row i, column j to r[i][j] for i, j < 23 (:385-392) while the codes run A..V, B, Z, X, gap: code Z
// (21) therefore reads the file's J line and code X (22) the file's Z line; row and column 23 (gap) are never written.
void blosum62_as_loaded(int table[NJ_CODES * NJ_CODES]) {
    for (int i = 0; i < NJ_CODES; ++i)
        for (int j = 0; j < NJ_CODES; ++j) table[i * NJ_CODES + j] = (i < 23 && j < 23) ? BLOSUM62_FILE[i][j] : 0;
}

std::string nj_number(double x) {
    char buf[40];
    for (int prec = 15; prec <= 17; ++prec) {
        std::snprintf(buf, sizeof buf, "%.*g", prec, x);
        if (prec == 17 || std::strtod(buf, nullptr) == x) break;
    }
    return buf;
}

namespace {
// Math.max(x, 0): NaN stays NaN, -0.0 becomes 0.0
inline double java_max0(double x) { return x > 0 ? x : (x != x ? x : 0.0); }

// :702-748, row-major over i < j, strict comparison: the first extreme wins
bool extreme_pair(const std::vector<double> &M, int n, bool want_min, int &bi, int &bj) {
    bi = bj = -1;
    double best = want_min ? DBL_MAX : -std::numeric_limits<double>::infinity();
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double v = M[(size_t)i * n + j];
            if (want_min ? v < best : v > best) { best = v; bi = i; bj = j; }
        }
    return bi >= 0;
}

// the new index of every node after merging (mi, mj) into index 0 (:253-262, :88-97)
void new_indices(int n, int mi, int mj, std::vector<int> &idx) {
    idx.assign((size_t)n, 0);
    int offset = 1;
    for (int i = 0; i < n; ++i) {
        if (i == mi || i == mj) { --offset; idx[i] = 0; }
        else idx[i] = i + offset;
    }
}

// "copy unchanged values" (:265-278, :100-113): the upper triangle of the old matrix, mirrored; the entries it writes into
// row / column 0 are overwritten by the caller's means, [0][0] is never written and stays 0
void copy_unchanged(const std::vector<double> &D, int n, int mi, int mj, const std::vector<int> &idx, std::vector<double> &N) {
    const int m = n - 1;
    N.assign((size_t)m * m, 0.0);
    for (int i = 0; i < n; ++i) {
        if (i == mi) continue;
        const int ni = idx[i];
        for (int j = i; j < n; ++j) {
            if (j == mj) continue;
            const int nj = idx[j];
            N[(size_t)ni * m + nj] = D[(size_t)i * n + j];
            N[(size_t)nj * m + ni] = D[(size_t)i * n + j];
        }
    }
}

bool check_args(int n, const std::vector<std::string> &names, const double *m, int type, std::string &err) {
    if (n < 4) { err = "neighbor joining needs at least 4 taxa (the reference returns null for 3)"; return false; }
    if ((int)names.size() != n || !m) { err = "names / matrix do not match n"; return false; }
    if (type != NJ_DISTANCE && type != NJ_SIMILARITY) { err = "matrixType must be DISTANCE or SIMILARITY"; return false; }
    return true;
}
}  // namespace

bool nj_tree_string(int n0, const std::vector<std::string> &names, const double *m, int type, std::string &out, std::string &err) {
    if (!check_args(n0, names, m, type, err)) return false;
    int n = n0;
    std::vector<std::string> nodes(names);
    std::vector<double> D((size_t)n * n), N, sums, Q;
    std::vector<int> idx;
    if (type == NJ_SIMILARITY) {                       // :346-362: the maximum starts from 0 and looks at the diagonal only
        double max_sim = 0;
        for (int i = 0; i < n; ++i) if (m[(size_t)i * n + i] > max_sim) max_sim = m[(size_t)i * n + i];
        for (size_t k = 0; k < D.size(); ++k) D[k] = max_sim - m[k];
    } else D.assign(m, m + (size_t)n * n);
    for (;;) {
        sums.assign((size_t)n, 0.0);                   // :166-172, the diagonal included
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) sums[i] += D[(size_t)i * n + j];
        const int r_minus2 = n - 2;
        Q.assign((size_t)n * n, 0.0);                  // :176-185
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) {
                const double value = (r_minus2 * D[(size_t)i * n + j]) - sums[i] - sums[j];
                Q[(size_t)i * n + j] = value; Q[(size_t)j * n + i] = value;
            }
        int mi, mj;
        if (!extreme_pair(Q, n, true, mi, mj)) { err = "no pair of nodes has a Q below Double.MAX_VALUE"; return false; }
        const double dij = D[(size_t)mi * n + mj];
        double to_i = (dij / 2) + ((1 / (2.0 * r_minus2)) * (sums[mi] - sums[mj]));     // :221-222
        double to_j = dij - to_i;                                                         // :225
        to_i = java_max0(to_i); to_j = java_max0(to_j);                                   // :228-229
        const std::string combined = "(" + nodes[mi] + ":" + nj_number(to_i) + "," + nodes[mj] + ":" + nj_number(to_j) + ")";
        new_indices(n, mi, mj, idx);
        copy_unchanged(D, n, mi, mj, idx, N);
        const int nn = n - 1;
        for (int i = 0; i < n; ++i) {                  // :281-289
            if (idx[i] == 0) continue;
            const double vi = D[(size_t)mi * n + i], vj = D[(size_t)mj * n + i];
            const double mean = (vi + vj - dij) / 2;
            N[idx[i]] = mean; N[(size_t)idx[i] * nn] = mean;
        }
        std::vector<std::string> nn_nodes((size_t)nn);
        for (int i = 0; i < n; ++i) if (idx[i] != 0) nn_nodes[idx[i]].swap(nodes[i]);
        nn_nodes[0] = combined;
        nodes.swap(nn_nodes); D.swap(N); n = nn;
        if (n > 3) continue;
        double s[3];                                   // :317-340, three nodes left: lengths from the row sums, not clamped
        for (int i = 0; i < 3; ++i) { s[i] = 0; for (int j = 0; j < 3; ++j) s[i] += D[(size_t)i * 3 + j]; }
        const double d0 = (D[0 * 3 + 1] / 2) + (0.5 * (s[0] - s[1]));
        const double d1 = (D[1 * 3 + 2] / 2) + (0.5 * (s[1] - s[2]));
        const double d2 = (D[2 * 3 + 0] / 2) + (0.5 * (s[2] - s[0]));
        out = "(" + nodes[0] + ":" + nj_number(d0) + "," + nodes[1] + ":" + nj_number(d1) + "," + nodes[2] + ":" + nj_number(d2) + ");";
        return true;
    }
}

bool nj_topology(int n0, const std::vector<std::string> &names, const double *m, int type, std::string &out, std::string &err) {
    if (!check_args(n0, names, m, type, err)) return false;
    int n = n0;
    std::vector<std::string> nodes(names);
    std::vector<double> D(m, m + (size_t)n * n), N;
    std::vector<int> idx;
    for (;;) {
        int mi, mj;
        if (!extreme_pair(D, n, type == NJ_DISTANCE, mi, mj)) { err = "no pair of nodes passes the strict comparison"; return false; }
        const std::string combined = "(" + nodes[mi] + "," + nodes[mj] + ")";
        if (n == 2) { out = combined + ";"; return true; }      // :133-138
        new_indices(n, mi, mj, idx);
        copy_unchanged(D, n, mi, mj, idx, N);
        const int nn = n - 1;
        for (int i = 0; i < n; ++i) {                  // :116-124, plain means
            if (idx[i] == 0) continue;
            const double mean = (D[(size_t)mi * n + i] + D[(size_t)mj * n + i]) / 2;
            N[idx[i]] = mean; N[(size_t)idx[i] * nn] = mean;
        }
        std::vector<std::string> nn_nodes((size_t)nn);
        for (int i = 0; i < n; ++i) if (idx[i] != 0) nn_nodes[idx[i]].swap(nodes[i]);
        nn_nodes[0] = combined;
        nodes.swap(nn_nodes); D.swap(N); n = nn;
    }
}

}  // namespace pml

static char *nj_dup(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) { for (size_t i = 0; i <= s.size(); ++i) p[i] = s.c_str()[i]; } return p; }

extern "C" int pml_pairscore_table_blosum62(int table_out[576]) {
    if (!table_out) return PML_EINVAL;
    pml::blosum62_as_loaded(table_out);
    return PML_OK;
}

extern "C" int pml_nj_from_matrix(int n, const char *const *names, const double *m, int matrix_type, int form, char **newick_out) {
    if (newick_out) *newick_out = nullptr;
    if (n < 4 || !names || !m || !newick_out) return PML_EINVAL;
    if (form != PML_NJ_TREE && form != PML_NJ_TOPOLOGY) return PML_EINVAL;
    try {
        std::vector<std::string> nm((size_t)n);
        for (int i = 0; i < n; ++i) { if (!names[i]) return PML_EINVAL; nm[i] = names[i]; }
        std::string out, err;
        const bool ok = form == PML_NJ_TREE ? pml::nj_tree_string(n, nm, m, matrix_type, out, err) : pml::nj_topology(n, nm, m, matrix_type, out, err);
        if (!ok) return PML_EINVAL;
        *newick_out = nj_dup(out);
    } catch (const std::exception &) { return PML_ENOMEM; }
    return *newick_out ? PML_OK : PML_ENOMEM;
}
