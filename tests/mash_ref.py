"""An independent restatement of the MinHash rule of include/peprml.h ("NeighborMasher") and of the selection routines of the
reference's util/NeighborMasher.java, for the tests: the rule in plain Python ints, the same hash vectorised over numpy uint64
(so the device tests get their reference quickly), and the Java routines line by line with their line numbers.  Nothing here calls
the library.  Parity with the mash binary is unpinned (the header says why); this file pins the library against the header's text."""
import math

import numpy as np

M64 = (1 << 64) - 1
INVALID = M64
SEED = 42
C1, C2 = 0x87c37b91114253d5, 0x4cf5ad432745937f


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def fmix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def murmur3_x64_128(data, seed=0):
    """(h1, h2) of MurmurHash3_x64_128"""
    data = bytes(data)
    n = len(data)
    h1 = h2 = seed
    for b in range(n // 16):
        k1 = int.from_bytes(data[16 * b:16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8:16 * b + 16], "little")
        k1 = (k1 * C1) & M64; k1 = rotl(k1, 31); k1 = (k1 * C2) & M64; h1 ^= k1
        h1 = rotl(h1, 27); h1 = (h1 + h2) & M64; h1 = (h1 * 5 + 0x52dce729) & M64
        k2 = (k2 * C2) & M64; k2 = rotl(k2, 33); k2 = (k2 * C1) & M64; h2 ^= k2
        h2 = rotl(h2, 31); h2 = (h2 + h1) & M64; h2 = (h2 * 5 + 0x38495ab5) & M64
    tail = data[16 * (n // 16):]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = (k2 * C2) & M64; k2 = rotl(k2, 33); k2 = (k2 * C1) & M64; h2 ^= k2
    if len(tail) > 0:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = (k1 * C1) & M64; k1 = rotl(k1, 31); k1 = (k1 * C2) & M64; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & M64; h2 = (h2 + h1) & M64
    h1 = fmix(h1); h2 = fmix(h2)
    h1 = (h1 + h2) & M64; h2 = (h2 + h1) & M64
    return h1, h2


_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def window_value(window, k):
    """the value of one window of k bytes, or None when it is not valid"""
    w = bytes(window).upper()
    if len(w) != k or any(b not in _COMP for b in w):
        return None
    rc = bytes(_COMP[b] for b in reversed(w))
    canon = rc if rc < w else w
    h1 = murmur3_x64_128(canon, SEED)[0]
    return h1 & 0xFFFFFFFF if k <= 16 else h1


def record_values_slow(record, k):
    """one entry per byte: the value of the window starting there, INVALID where there is none (plain ints)"""
    out = []
    for p in range(len(record)):
        v = window_value(record[p:p + k], k) if p + k <= len(record) else None
        out.append(INVALID if v is None else v)
    return out


# ---- the same over numpy ----
def _mul(a, b):
    return a * b            # uint64 arrays wrap


def _rotl_np(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _fmix_np(x):
    x = x ^ (x >> np.uint64(33))
    x = _mul(x, np.uint64(0xff51afd7ed558ccd))
    x = x ^ (x >> np.uint64(33))
    x = _mul(x, np.uint64(0xc4ceb9fe1a85ec53))
    x = x ^ (x >> np.uint64(33))
    return x


def murmur_h1_rows(rows, seed=SEED):
    """h1 of every row of a uint8 matrix [n][len]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, ln = rows.shape
    c1, c2 = np.uint64(C1), np.uint64(C2)
    h1 = np.full(n, seed, dtype=np.uint64)
    h2 = np.full(n, seed, dtype=np.uint64)

    def word(lo, hi):
        w = np.zeros(n, dtype=np.uint64)
        for i, col in enumerate(range(lo, hi)):
            w |= rows[:, col].astype(np.uint64) << np.uint64(8 * i)
        return w
    with np.errstate(over="ignore"):
        for b in range(ln // 16):
            k1, k2 = word(16 * b, 16 * b + 8), word(16 * b + 8, 16 * b + 16)
            k1 = _mul(_rotl_np(_mul(k1, c1), 31), c2); h1 = h1 ^ k1
            h1 = _rotl_np(h1, 27) + h2; h1 = h1 * np.uint64(5) + np.uint64(0x52dce729)
            k2 = _mul(_rotl_np(_mul(k2, c2), 33), c1); h2 = h2 ^ k2
            h2 = _rotl_np(h2, 31) + h1; h2 = h2 * np.uint64(5) + np.uint64(0x38495ab5)
        t0, t = 16 * (ln // 16), ln % 16
        if t > 8:
            k2 = word(t0 + 8, ln)
            h2 = h2 ^ _mul(_rotl_np(_mul(k2, c2), 33), c1)
        if t > 0:
            k1 = word(t0, t0 + min(t, 8))
            h1 = h1 ^ _mul(_rotl_np(_mul(k1, c1), 31), c2)
        h1 = h1 ^ np.uint64(ln); h2 = h2 ^ np.uint64(ln)
        h1 = h1 + h2; h2 = h2 + h1
        h1 = _fmix_np(h1); h2 = _fmix_np(h2)
        h1 = h1 + h2
    return h1


def record_values(record, k):
    """record_values_slow as a uint64 array"""
    rec = np.frombuffer(bytes(record), dtype=np.uint8)
    n = rec.size
    out = np.full(n, INVALID, dtype=np.uint64)
    if n < k:
        return out
    up = np.where((rec >= ord("a")) & (rec <= ord("z")), rec - 32, rec).astype(np.uint8)
    good = (up == ord("A")) | (up == ord("C")) | (up == ord("G")) | (up == ord("T"))
    nw = n - k + 1
    win = np.lib.stride_tricks.sliding_window_view(up, k)                      # [nw][k]
    valid = np.lib.stride_tricks.sliding_window_view(good, k).all(axis=1)
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in _COMP.items():
        comp[a] = b
    rc = comp[win[:, ::-1]]
    # the first place where the two differ decides which is smaller
    diff = win != rc
    first = np.argmax(diff, axis=1)
    idx = np.arange(nw)
    use_rc = diff.any(axis=1) & (rc[idx, first] < win[idx, first])
    canon = np.where(use_rc[:, None], rc, win)
    h = murmur_h1_rows(canon[valid])
    if k <= 16:
        h = h & np.uint64(0xFFFFFFFF)
    vals = np.full(nw, INVALID, dtype=np.uint64)
    vals[valid] = h
    out[:nw] = vals
    return out


def genome_values(genome, k):
    """all valid windows' values of a genome (a list of records), in order"""
    parts = []
    for rec in genome:
        rec = rec.encode("latin-1") if isinstance(rec, str) else bytes(rec)
        if len(rec) >= k:
            v = record_values(rec, k)
            up = np.frombuffer(rec.upper(), dtype=np.uint8)
            good = np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8))
            valid = np.lib.stride_tricks.sliding_window_view(good, k).all(axis=1)
            parts.append(v[:len(rec) - k + 1][valid])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def hashes(genome, k):
    """debug_mash_hashes' layout: one value per byte of every record"""
    parts = [record_values(rec.encode("latin-1") if isinstance(rec, str) else bytes(rec), k) for rec in genome]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def sketch(genome, k, s):
    """the ascending min(s, D) smallest distinct values"""
    return np.unique(genome_values(genome, k))[:s]


def pair(a, b, s):
    """(common, denom): the loop of the header, as it stands"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    i = j = common = denom = 0
    while denom < s and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            i += 1; j += 1; common += 1
        denom += 1
    if denom < s:
        denom = min(s, denom + len(a) - i + len(b) - j)
    return common, denom


def pair_fast(a, b, s):
    """the same two integers from sets (for long sketches): the s smallest of the union, and the shared values among them"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    union = np.union1d(a, b)[:s]
    return int(np.isin(union, np.intersect1d(a, b)).sum()), int(union.size)


def distance(common, denom, k, digits=None):
    if common == denom:
        d = 0.0
    elif common == 0:
        d = 1.0
    else:
        j = common / denom
        d = min(1.0, -math.log(2.0 * j / (1.0 + j)) / k)
    return float("%.*g" % (digits, d)) if digits else d


# ---- util/NeighborMasher.java ----
def _java_sorted(items, key):
    """Arrays.sort on objects is a stable merge sort; GenomeCandidate.compareTo :1064-1072 orders by distance alone"""
    return sorted(items, key=key)


def distance_from_ingroup(row):
    """getDistanceFromIngroup :360-382: an array of the distances (1.0 where none is cached), sorted, its last element"""
    distances = sorted(1.0 if x is None else x for x in row)                          # :363-378
    return distances[-1]                                                              # :380


def expand_ingroup(d, pool_is_ingroup, target):
    """expandIngroup :281-324 on a pool x ingroup table -> pool indices added, in order"""
    n_in = len(d[0]) if len(d) else 0
    candidates = [(p, distance_from_ingroup(d[p])) for p in range(len(d))]            # :292-296
    candidates = _java_sorted(candidates, key=lambda c: c[1])                         # :298
    size = n_in                                                                       # :301-304
    added = []
    i = 0
    while i < len(candidates) and size < target:                                      # :312
        p, dist = candidates[i]
        if dist < 1.0 and not pool_is_ingroup[p]:                                     # :314
            added.append(p); size += 1                                                # :316
        i += 1
    return added


def candidate_distances(d):
    """getMaxDistanceForEachOutgroupToIngroupSketch :738-783: the map keeps a query's distance when it has none yet or the new one
    is larger (:764-767); the candidates come out in the pool's order here (the Java's HashMap leaves it to the JVM)"""
    out = []
    for row in d:
        mx = None
        for x in row:
            if mx is None or x > mx:
                mx = x
        out.append(mx)
    return out


def get_mean(d):
    """StatisticsUtilities.getMean :158-173"""
    r, den = 0.0, 0
    for x in d:
        if x == x:
            r += x; den += 1
    return r / den if den else float("nan")                                           # Java: 0.0 / 0 = NaN


def get_standard_deviation(d, mean):
    """StatisticsUtilities.getStandardDeviation :831-840"""
    sos = 0.0
    for x in d:
        diff = mean - x
        sos += diff * diff
    n1 = len(d) - 1
    if n1 == 0:
        q = float("nan") if sos == 0.0 or sos != sos else math.copysign(float("inf"), sos)      # Java: x / 0
    else:
        q = sos / n1
    if q != q:
        return float("nan")
    return math.sqrt(q) if q > 0 else (q if q == 0 else float("nan"))                 # Math.sqrt(-0.0) = -0.0


def get_max(a):
    """StatisticsUtilities.getMax :938-949"""
    mx = float("nan")
    if a is not None and len(a) > 0:
        mx = a[0]
        for x in a:
            if x > mx:
                mx = x
    return mx


def ingroup_pair_distances(dff):
    """getIngroupPairDistances :855-867"""
    n = len(dff)
    return [dff[i][j] for i in range(n) for j in range(i + 1, n)]


def select_outgroup(cand, maximum_ingroup_distance, ingroup_sd, count):
    """selectOutgroupCandidates :483-568 -> candidate indices selected, in order.  Within one distance the Java's HashSet order is the
    JVM's; here it is the sorted order."""
    order = _java_sorted(list(range(len(cand))), key=lambda c: cand[c])               # :485
    minimum = maximum_ingroup_distance + (ingroup_sd * 0)                             # :486
    acceptable, too_near = {}, {}
    i = 0
    while i < len(order) and len(acceptable) < count:                                 # :493
        c = order[i]
        dist = cand[c]
        if dist < 1.0:                                                                # :495
            if dist > minimum:                                                        # :496
                acceptable.setdefault(dist, []).append(c)
            else:
                too_near.setdefault(dist, []).append(c)
        i += 1
    selected = []
    for dist in sorted(acceptable):                                                   # :521-522, :529
        for c in acceptable[dist]:
            selected.append(c)
            if len(selected) == count:                                                # :534
                break
        if len(selected) == count:                                                    # :538
            break
    if len(selected) == 0 and len(too_near) > 0:                                      # :543-563
        keys = sorted(too_near)
        selected.append(too_near[keys[-1]][0])                                        # the two unconditional breaks: one candidate
    return selected


def run(ingroup, pool, k, s, outgroup_count=3, expand=0, ingroup_only=False, outgroup_only=False, digits=6):
    """run() :112-195 on (name, genome) lists -> the final ingroup's names, the outgroup names, the taxa of the second tree
    (outgroups first, :623-635) with their distance matrix, and which trees run() builds"""
    names = [t[0] for t in ingroup] + [t[0] for t in pool]
    sk = [sketch(t[1], k, s) for t in ingroup] + [sketch(t[1], k, s) for t in pool]
    ni = len(ingroup)

    def dist(x, y):
        c, d = pair_fast(sk[x], sk[y], s)
        return distance(c, d, k, digits)
    ing = list(range(ni))
    pool_idx = list(range(ni, ni + len(pool)))
    if expand > ni:                                                                   # :116
        original = set(names[:ni])
        d = [[dist(p, i) for i in ing] for p in pool_idx]
        ing += [ni + p for p in expand_ingroup(d, [names[p] in original for p in pool_idx], expand)]
    out = {"ingroup": [names[i] for i in ing], "outgroup": [], "mean": None, "sd": None, "max": None, "candidate_distance": None}
    sel = []
    if not ingroup_only:                                                              # :148
        dff = [[dist(i, j) for j in ing] for i in ing]
        pd = ingroup_pair_distances(dff)
        mean = get_mean(pd)
        sd = get_standard_deviation(pd, mean)
        mx = get_max(pd)
        cand = candidate_distances([[dist(p, i) for i in ing] for p in pool_idx])
        sel = select_outgroup(cand, mx, sd, outgroup_count)
        out.update(outgroup=[names[ni + p] for p in sel], mean=mean, sd=sd, max=mx, candidate_distance=cand)
    taxa = [ni + p for p in sel] + ing
    T = len(taxa)
    m = np.zeros((T, T))
    for i in range(T):
        for j in range(i + 1, T):
            m[i, j] = m[j, i] = dist(taxa[i], taxa[j])                                # :656-667
    out["taxa"] = [names[t] for t in taxa]
    out["distance"] = m
    out["ingroup_tree_built"] = (not outgroup_only) and expand > 3 and len(ing) >= 4  # :128 (and NJ's own four-taxon minimum)
    out["rooted_tree_built"] = (not ingroup_only) and (not outgroup_only) and expand + len(sel) > 3 and T >= 4      # :175-181
    return out


def taxon_from_title(title):
    """FastaUtilities.getTaxonFromTitle :51-114 with stripPipeAndSuffix off"""
    last_close = -1
    for i in range(len(title) - 1, 0, -1):                                            # :61-66 (index 0 is not looked at)
        if title[i] == "]":
            last_close = i
            break
    ignore, match = 0, -1
    for i in range(last_close - 1, -1, -1):                                           # :71-82
        if title[i] == "]":
            ignore += 1
        elif title[i] == "[":
            if ignore == 0:
                match = i
                break
            ignore -= 1
    if match > -1 and last_close > -1:
        r = title[match + 1:last_close]
    else:
        r = title[1:] if title.startswith(">") else title
    r = r.replace("|", "@")                                                           # :104
    for ch in " ():,[]":                                                              # :108-111
        r = r.replace(ch, "_")
        r = _replace_all(r, "__", "_")
    return r


def _replace_all(s, a, b):
    """String.replaceAll of a literal: one left-to-right pass over non-overlapping matches"""
    return s.replace(a, b)
