// trim.hpp -- MSATrimmer's three column filters as ONE decision function, compiled for the device (k_colclass, trim.hip) and
// for the host (pml_trim_column_flags_host, trim.cpp): the two cannot disagree.  Plain C++ outside hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PML_TRIM_HD __host__ __device__ __forceinline__
#else
#define PML_TRIM_HD inline
#endif

namespace pml {

// one flag byte per column: bits 0, 1, 2 = kept under PML_TRIM_UNIFORM, PML_TRIM_GAP_UNIFORM, PML_TRIM_TOPOLOGICAL;
// bit 3 = the column holds nothing but '-' and '?' (the Java's trimUniformColumns dereferences null there)
enum { TRIM_KEEP_UNIFORM = 1, TRIM_KEEP_GAP_UNIFORM = 2, TRIM_KEEP_TOPOLOGICAL = 4, TRIM_ALL_GAP = 8 };
constexpr int TRIM_COLS = 256;        // columns per k_colclass workgroup, one per thread
constexpr int TRIM_CHUNKS = 64;       // 16-byte chunks of an output row per k_colgather workgroup, one per lane
constexpr int TRIM_ROWS = 64;         // rows per k_colgather workgroup

// A column's state is two sets of bytes, each eight 32-bit words (byte b = bit b & 31 of word b >> 5), and one count:
// seen1 = the bytes that occur, seen2 = the bytes that occur at least twice, shown = the rows whose byte is neither '-' nor
// '?'; n = the gene's rows.
PML_TRIM_HD void trim_note(uint32_t seen1[8], uint32_t seen2[8], int &shown, unsigned b) {
    const uint32_t bit = 1u << (b & 31);
    const unsigned w = b >> 5;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned k = 0; k < 8; ++k) {
        const uint32_t m = w == k ? bit : 0u;
        seen2[k] |= seen1[k] & m;
        seen1[k] |= m;
    }
    shown += b != '-' && b != '?';
}

PML_TRIM_HD int trim_popcount(const uint32_t s[8]) {
    int c = 0;
    for (int k = 0; k < 8; ++k) c += __builtin_popcount(s[k]);
    return c;
}

PML_TRIM_HD unsigned trim_decide(const uint32_t seen1[8], const uint32_t seen2[8], int shown, int n) {
    constexpr uint32_t GAP = 1u << ('-' & 31), MISSING = 1u << ('?' & 31);      // both in word 1
    static_assert(('-' >> 5) == 1 && ('?' >> 5) == 1, "'-' and '?' are bytes 45 and 63");
    const int had_gap = (seen1[1] & GAP) != 0, had_missing = (seen1[1] & MISSING) != 0;
    const int occurring = trim_popcount(seen1);
    const int classes = occurring - had_gap - had_missing;         // getBipartitionsForAlignmentColumn's classes
    const int twice = trim_popcount(seen2) - ((seen2[1] & GAP) != 0);
    unsigned f = 0;
    // trimUniformColumns: getMinimumStepsPerSite != 0.  Two classes that cover all n rows are ONE bipartition (no step)
    if (classes >= 3 || (classes == 2 && shown < n)) f |= TRIM_KEEP_UNIFORM;
    // trimUniformativeColumns: two distinct bytes other than '-' ('?' is a character like any other)
    if (occurring - had_gap >= 2) f |= TRIM_KEEP_GAP_UNIFORM;
    // trimTopologicallyUninformativeColumns: two distinct bytes other than '-' that each occur at least twice
    if (twice >= 2) f |= TRIM_KEEP_TOPOLOGICAL;
    if (classes == 0) f |= TRIM_ALL_GAP;
    return f;
}

}  // namespace pml
