// mash.hpp -- what the MinHash path's host rule (mash_host.cpp), its device driver (mash.cpp) and its kernels (mash.hip) share: the
// constants of the layout, the byte classes, and the hash of a canonical window held as four little-endian words.  Plain C++
// outside hipcc; no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PML_MASH_HD __host__ __device__ inline __attribute__((always_inline))      // mash_host.cpp includes no HIP header
#else
#define PML_MASH_HD inline
#endif

namespace pml {

constexpr int MASH_TILE = 1024;            // window starts a k_mash_hash workgroup stages at a time (pml_mash_tile)
constexpr int MASH_THREADS = 256;          // its threads: MASH_TILE / MASH_THREADS window starts each
constexpr int MASH_SPAN_TILES = 64;        // tiles one workgroup works through (one genome; its histogram is flushed once)
constexpr int MASH_BIN_BITS = 12;          // leading bits of a value that the cut histogram keeps
constexpr int MASH_BINS = 1 << MASH_BIN_BITS;
constexpr int MASH_CHUNK = 256;            // sketch values of the row genome a k_mash_pairs workgroup takes at a time (pml_mash_chunk)
constexpr uint32_t MASH_SEED = 42;
constexpr uint64_t MASH_INVALID = ~0ull;   // what k_mash_hash writes for a window that is not valid: above every 32-bit value, and
                                           // above every 64-bit value but 2^64 - 1 itself (include/peprml.h says what that means)
constexpr unsigned char MASH_SEP = '\n';   // the byte between records and between genomes of a batch

// bits of a value: 4^k <= 2^32 keeps the low 32 bits of h1
PML_MASH_HD int mash_value_bits(int k) { return k <= 16 ? 32 : 64; }

// A, C, G, T in either case = 0..3, everything else 4
PML_MASH_HD unsigned mash_code(unsigned b) {
    const unsigned u = b & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

PML_MASH_HD uint64_t mash_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
PML_MASH_HD uint64_t mash_fmix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// h1 of MurmurHash3_x64_128 over len <= 32 bytes given as four little-endian words (bytes from len on are 0)
PML_MASH_HD uint64_t mash_murmur_h1(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, int len, uint32_t seed) {
    const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
    uint64_t h1 = seed, h2 = seed;
    const int nblocks = len >> 4;
    if (nblocks >= 1) {
        uint64_t k1 = w0, k2 = w1;
        k1 *= c1; k1 = mash_rotl(k1, 31); k1 *= c2; h1 ^= k1; h1 = mash_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = mash_rotl(k2, 33); k2 *= c1; h2 ^= k2; h2 = mash_rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    if (nblocks >= 2) {
        uint64_t k1 = w2, k2 = w3;
        k1 *= c1; k1 = mash_rotl(k1, 31); k1 *= c2; h1 ^= k1; h1 = mash_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = mash_rotl(k2, 33); k2 *= c1; h2 ^= k2; h2 = mash_rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    const int tail = len & 15;
    const uint64_t t1 = nblocks == 0 ? w0 : w2, t2 = nblocks == 0 ? w1 : w3;     // nblocks == 2 has no tail
    if (tail > 8) { uint64_t k2 = t2; k2 *= c2; k2 = mash_rotl(k2, 33); k2 *= c1; h2 ^= k2; }
    if (tail > 0) { uint64_t k1 = t1; k1 *= c1; k1 = mash_rotl(k1, 31); k1 *= c2; h1 ^= k1; }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = mash_fmix(h1); h2 = mash_fmix(h2);
    h1 += h2;
    return h1;
}

// the value of a valid window from its two 2-bit packings (first base in the highest of the 2k bits): fw the window, rc its
// reverse complement.  A < C < G < T is the byte order, so the smaller packing is the smaller byte string.
PML_MASH_HD uint64_t mash_value(uint64_t fw, uint64_t rc, int k) {
    const uint64_t canon = rc < fw ? rc : fw;
    const uint64_t left = canon << (64 - 2 * k);                                // base j in bits 63 - 2j, 62 - 2j
    uint64_t w[4] = {0, 0, 0, 0};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 32; ++j) {                                              // all 32 places with constant shifts ...
        const unsigned c = (unsigned)(left >> (62 - 2 * j)) & 3u;
        const uint64_t byte = (0x54474341u >> (8 * c)) & 0xFFu;                 // "ACGT"
        w[j >> 3] |= byte << (8 * (j & 7));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {                                               // ... then the bytes from k on are cleared
        const int nb = k - 8 * i;
        w[i] &= nb >= 8 ? ~0ull : nb <= 0 ? 0ull : ((1ull << (8 * nb)) - 1ull);
    }
    const uint64_t h = mash_murmur_h1(w[0], w[1], w[2], w[3], k, MASH_SEED);
    return k <= 16 ? (h & 0xFFFFFFFFull) : h;
}

// ---- host rule (mash_host.cpp) ----
struct MashGenome { std::vector<std::string> records; };
void mash_murmur3_x64_128(const void *key, size_t len, uint32_t seed, uint64_t out[2]);     // any length
// one value per byte of the record; MASH_INVALID where no valid window starts
void mash_record_values(const unsigned char *rec, long long len, int k, uint64_t *out);
void mash_sketch_host(const MashGenome &g, int k, int s, std::vector<uint64_t> &out);
void mash_pair_host(const uint64_t *a, long long na, const uint64_t *b, long long nb, int s, int &common, int &denom);
double mash_distance_of(int common, int denom, int k);
double mash_round_digits(double d, int digits);            // digits <= 0: d itself; else strtod of "%.<digits>g"

// the Java half (util/NeighborMasher.java); candidates are indices, ties follow input order
double mash_candidate_max(const double *row, int n_in);                                   // :360-382 and :760-768
void mash_expand_ingroup(int n_in, int n_pool, const double *d, const unsigned char *pool_is_ingroup, int target, std::vector<int> &added);
void mash_pair_stats(const std::vector<double> &d, double &mean, double &sd, double &mx); // StatisticsUtilities
void mash_select_outgroup(int n, const double *cand, double max_ingroup, double sd, int count, std::vector<int> &selected);

}  // namespace pml
