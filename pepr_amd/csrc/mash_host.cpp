// mash_host.cpp -- the MinHash rule of include/peprml.h on the host (window, canonical form, hash, sketch, pair, distance) and the
// selection routines of util/NeighborMasher.java restated.  Plain C++: no HIP include, so it builds and runs alone
// (tests/mash_standalone); the library's host-only doors are at the end.  The rule is written here over BYTES (the window and its
// reverse complement as strings, MurmurHash3 over any length); the kernels use the packed form of mash.hpp, and the tests hold the
// two against each other.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../include/peprml.h"
#include "mash.hpp"

namespace pml {

void mash_murmur3_x64_128(const void *key, size_t len, uint32_t seed, uint64_t out[2]) {
    const unsigned char *data = (const unsigned char *)key;
    const size_t nblocks = len / 16;
    uint64_t h1 = seed, h2 = seed;
    const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
    auto rd = [](const unsigned char *p, size_t n) { uint64_t v = 0; for (size_t i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i); return v; };
    for (size_t i = 0; i < nblocks; ++i) {
        uint64_t k1 = rd(data + 16 * i, 8), k2 = rd(data + 16 * i + 8, 8);
        k1 *= c1; k1 = mash_rotl(k1, 31); k1 *= c2; h1 ^= k1; h1 = mash_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = mash_rotl(k2, 33); k2 *= c1; h2 ^= k2; h2 = mash_rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    const unsigned char *tail = data + 16 * nblocks;
    const size_t t = len & 15;
    if (t > 8) { uint64_t k2 = rd(tail + 8, t - 8); k2 *= c2; k2 = mash_rotl(k2, 33); k2 *= c1; h2 ^= k2; }
    if (t > 0) { uint64_t k1 = rd(tail, t > 8 ? 8 : t); k1 *= c1; k1 = mash_rotl(k1, 31); k1 *= c2; h1 ^= k1; }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = mash_fmix(h1); h2 = mash_fmix(h2);
    h1 += h2; h2 += h1;
    out[0] = h1; out[1] = h2;
}

void mash_record_values(const unsigned char *rec, long long len, int k, uint64_t *out) {
    static const char comp[4] = {'T', 'G', 'C', 'A'};
    static const char base[4] = {'A', 'C', 'G', 'T'};
    char fw[32], rc[32];
    long long bad = -1;                                // the last position before p + k that holds no ACGT
    for (long long p = 0; p < len && p < k - 1; ++p) if (mash_code(rec[p]) > 3) bad = p;
    for (long long p = 0; p < len; ++p) {
        out[p] = MASH_INVALID;
        if (p + k > len) continue;
        if (mash_code(rec[p + k - 1]) > 3) bad = p + k - 1;
        if (bad >= p) continue;
        for (int j = 0; j < k; ++j) {
            fw[j] = base[mash_code(rec[p + j])];
            rc[j] = comp[mash_code(rec[p + k - 1 - j])];
        }
        const char *canon = std::memcmp(rc, fw, (size_t)k) < 0 ? rc : fw;
        uint64_t h[2];
        mash_murmur3_x64_128(canon, (size_t)k, MASH_SEED, h);
        out[p] = k <= 16 ? (h[0] & 0xFFFFFFFFull) : h[0];
    }
}

void mash_sketch_host(const MashGenome &g, int k, int s, std::vector<uint64_t> &out) {
    std::set<uint64_t> low;                            // the s smallest distinct values so far
    std::vector<uint64_t> v;
    for (const std::string &r : g.records) {
        v.resize(r.size());
        mash_record_values((const unsigned char *)r.data(), (long long)r.size(), k, v.data());
        for (size_t p = 0; p + (size_t)k <= r.size(); ++p) {
            // a window is valid or not by its bytes; the value 2^64 - 1 of a valid window is kept here (the device cannot tell it
            // from its own mark: include/peprml.h)
            bool valid = true;
            if (v[p] == MASH_INVALID) for (int j = 0; j < k && valid; ++j) valid = mash_code((unsigned char)r[p + (size_t)j]) <= 3;
            if (!valid) continue;
            if ((long long)low.size() < s) low.insert(v[p]);
            else if (v[p] < *low.rbegin() && low.insert(v[p]).second) low.erase(std::prev(low.end()));
        }
    }
    out.assign(low.begin(), low.end());
}

void mash_pair_host(const uint64_t *a, long long na, const uint64_t *b, long long nb, int s, int &common, int &denom) {
    long long i = 0, j = 0, c = 0, d = 0;
    while (d < s && i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (b[j] < a[i]) ++j;
        else { ++i; ++j; ++c; }
        ++d;
    }
    if (d < s) d = std::min<long long>(s, d + (na - i) + (nb - j));
    common = (int)c; denom = (int)d;
}

double mash_distance_of(int common, int denom, int k) {
    if (common == denom) return 0.0;
    if (common == 0) return 1.0;
    const double j = (double)common / (double)denom;
    const double d = -std::log(2.0 * j / (1.0 + j)) / (double)k;
    return d < 1.0 ? d : 1.0;
}

double mash_round_digits(double d, int digits) {
    if (digits <= 0 || d != d) return d;
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.*g", digits > 17 ? 17 : digits, d);
    return std::strtod(buf, nullptr);
}

// getDistanceFromIngroup :360-382 (an array filled with 1.0, sorted, its last element) and the loop of
// getMaxDistanceForEachOutgroupToIngroupSketch :760-768 (null, or a strictly larger distance, replaces): both are the maximum
double mash_candidate_max(const double *row, int n_in) {
    double mx = row[0];
    for (int i = 1; i < n_in; ++i) if (row[i] > mx) mx = row[i];
    return mx;
}

// GenomeCandidate.compareTo :1064-1072 under Arrays.sort's stable merge sort
static std::vector<int> stable_order(int n, const double *dist) {
    std::vector<int> idx((size_t)n);
    for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return dist[x] < dist[y]; });
    return idx;
}

// expandIngroup :281-324
void mash_expand_ingroup(int n_in, int n_pool, const double *d, const unsigned char *pool_is_ingroup, int target, std::vector<int> &added) {
    added.clear();
    std::vector<double> cand((size_t)n_pool);
    for (int p = 0; p < n_pool; ++p) cand[(size_t)p] = mash_candidate_max(d + (size_t)p * n_in, n_in);     // :292-296
    const std::vector<int> order = stable_order(n_pool, cand.data());                                       // :298
    for (int i = 0; i < n_pool && n_in + (int)added.size() < target; ++i) {                                 // :312
        const int p = order[(size_t)i];
        if (cand[(size_t)p] < 1.0 && !(pool_is_ingroup && pool_is_ingroup[p])) added.push_back(p);          // :314-316
    }
}

// StatisticsUtilities.getMean :158-173 (NaN entries are skipped, 0 / 0 for none), getStandardDeviation :831-840 (n - 1 in the
// divisor: NaN for one value, -0.0 for none), getMax :938-949 (NaN for none)
void mash_pair_stats(const std::vector<double> &d, double &mean, double &sd, double &mx) {
    double r = 0.0; int den = 0;
    for (double x : d) if (x == x) { r += x; ++den; }
    mean = r / (double)den;
    double sos = 0.0;
    for (double x : d) { const double diff = mean - x; sos += diff * diff; }
    sd = std::sqrt(sos / (double)((long long)d.size() - 1));
    mx = std::nan("");
    if (!d.empty()) { mx = d[0]; for (double x : d) if (x > mx) mx = x; }
}

// selectOutgroupCandidates :483-568.  The Java groups candidates by distance in HashMaps of HashSets; a group's order is the
// JVM's, here it is the sorted (input) order.
void mash_select_outgroup(int n, const double *cand, double max_ingroup, double sd, int count, std::vector<int> &selected) {
    selected.clear();
    const std::vector<int> order = stable_order(n, cand);                                     // :485
    const double minimum = max_ingroup + (sd * 0);                                            // :486 (NaN when sd is NaN)
    std::vector<std::pair<double, std::vector<int>>> ok, near;                                // distinct distances in first-seen order
    auto group = [](std::vector<std::pair<double, std::vector<int>>> &m, double dist) -> std::vector<int> & {
        for (auto &e : m) if (e.first == dist) return e.second;
        m.push_back({dist, {}});
        return m.back().second;
    };
    for (int i = 0; i < n && (int)ok.size() < count; ++i) {                                   // :493
        const int c = order[(size_t)i];
        const double dist = cand[c];
        if (dist < 1.0) {
            if (dist > minimum) group(ok, dist).push_back(c);                                 // :496-502
            else group(near, dist).push_back(c);                                              // :503-512
        }                                                                                     // :514-516 too far: only counted
    }
    std::stable_sort(ok.begin(), ok.end(), [](const auto &x, const auto &y) { return x.first < y.first; });      // :521-522
    for (auto &e : ok) {                                                                      // :529-541
        for (int c : e.second) {
            selected.push_back(c);
            if ((int)selected.size() == count) break;
        }
        if ((int)selected.size() == count) break;
    }
    if (selected.empty() && !near.empty()) {                                                  // :543-563: the farthest, one only
        std::stable_sort(near.begin(), near.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        selected.push_back(near.back().second[0]);
    }
}

}  // namespace pml

using namespace pml;

static bool genome_ok(const pml_genome *g) {
    if (!g || g->nrecords < 0 || (g->nrecords > 0 && (!g->records || !g->lengths))) return false;
    for (int r = 0; r < g->nrecords; ++r) if (g->lengths[r] < 0 || (g->lengths[r] > 0 && !g->records[r])) return false;
    return true;
}

extern "C" int pml_mash_tile(void) { return MASH_TILE; }
extern "C" int pml_mash_chunk(void) { return MASH_CHUNK; }

extern "C" int pml_mash_sketch_host(const pml_genome *genome, int k, int s, unsigned long long *values_out, int *len_out) {
    if (!genome_ok(genome) || k < 1 || k > 32 || s < 1 || !values_out || !len_out) return PML_EINVAL;
    try {
        MashGenome g;
        for (int r = 0; r < genome->nrecords; ++r) g.records.emplace_back(genome->records[r] ? genome->records[r] : "", (size_t)genome->lengths[r]);
        std::vector<uint64_t> sk;
        mash_sketch_host(g, k, s, sk);
        for (size_t i = 0; i < sk.size(); ++i) values_out[i] = sk[i];
        *len_out = (int)sk.size();
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_mash_hashes_host(const pml_genome *genome, int k, unsigned long long *values_out) {
    if (!genome_ok(genome) || k < 1 || k > 32 || !values_out) return PML_EINVAL;
    size_t at = 0;
    for (int r = 0; r < genome->nrecords; ++r) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit values");
        mash_record_values((const unsigned char *)genome->records[r], genome->lengths[r], k, (uint64_t *)values_out + at);
        at += (size_t)genome->lengths[r];
    }
    return PML_OK;
}

extern "C" int pml_mash_murmur3(const void *key, long long len, unsigned seed, unsigned long long out[2]) {
    if (len < 0 || (len > 0 && !key) || !out) return PML_EINVAL;
    uint64_t h[2];
    mash_murmur3_x64_128(key, (size_t)len, seed, h);
    out[0] = h[0]; out[1] = h[1];
    return PML_OK;
}

extern "C" int pml_mash_pair_host(const unsigned long long *a, int na, const unsigned long long *b, int nb, int s, int *common_out, int *denom_out) {
    if (na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b) || s < 1 || !common_out || !denom_out) return PML_EINVAL;
    mash_pair_host((const uint64_t *)a, na, (const uint64_t *)b, nb, s, *common_out, *denom_out);
    return PML_OK;
}

extern "C" double pml_mash_distance_of(int common, int denom, int k, int digits) {
    return mash_round_digits(mash_distance_of(common, denom, k), digits);
}

extern "C" int pml_mash_candidate_distances(int n_in, int n_pool, const double *d, double *cand_out) {
    if (n_in < 1 || n_pool < 0 || (n_pool > 0 && (!d || !cand_out))) return PML_EINVAL;
    for (int p = 0; p < n_pool; ++p) cand_out[p] = mash_candidate_max(d + (size_t)p * n_in, n_in);
    return PML_OK;
}

extern "C" int pml_mash_expand_ingroup(int n_in, int n_pool, const double *d, const unsigned char *pool_is_ingroup, int target, int *added_out, int *nadded_out) {
    if (n_in < 1 || n_pool < 0 || (n_pool > 0 && (!d || !added_out)) || !nadded_out) return PML_EINVAL;
    try {
        std::vector<int> added;
        mash_expand_ingroup(n_in, n_pool, d, pool_is_ingroup, target, added);
        for (size_t i = 0; i < added.size(); ++i) added_out[i] = added[i];
        *nadded_out = (int)added.size();
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_mash_select_outgroup(int n, const double *cand, double max_ingroup, double sd, int count, int *selected_out, int *nselected_out) {
    if (n < 0 || (n > 0 && (!cand || !selected_out)) || !nselected_out) return PML_EINVAL;
    try {
        std::vector<int> sel;
        mash_select_outgroup(n, cand, max_ingroup, sd, count, sel);
        for (size_t i = 0; i < sel.size(); ++i) selected_out[i] = sel[i];
        *nselected_out = (int)sel.size();
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_mash_pair_stats(int n, const double *d, double out3[3]) {
    if (n < 0 || (n > 0 && !d) || !out3) return PML_EINVAL;
    try {
        std::vector<double> v(d, d + n);
        mash_pair_stats(v, out3[0], out3[1], out3[2]);
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}
