"""The gene homoplasy test of the reference restated in Python, for the tests of pml_gene_steps / pml_step_thresholds.  Nothing here
calls the library.  Sources (reference tree, .../pepr/alignment/):
  ConcatenatedSequenceAlignment.java:65-103   the per-gene totals (int sums; a sequential float sum of the ratios)
  ConcatenatedSequenceAlignment.java:115-139  ratio = (float)steps / (float)(minSteps + 1); beyond = steps - minSteps
  ConcatenatedSequenceAlignment.java:141-425  the five threshold methods
  SequenceAlignment.java:673-682, :808-902    getMinimumStepsPerSite: the column's distinct Bipartitions less one
  MSAConcatenator.java:78-189                 the concatenation: sorted taxon union, genes in order, an absent taxon is '?'
The Java draws from an unseeded java.util.Random; the draws here are the rules include/peprml.h states (a counter hash, and a
Feistel permutation in place of the rejection loop), written out a second time."""
import math

import numpy as np

GAP, MISSING = ord("-"), ord("?")
M64 = (1 << 64) - 1
RAW, BEYOND_MIN, MIN_RATIO = 0, 1, 2

# ---- state sets: 20 amino acids in the order ARNDCQEGHILKMFPSTWYV, B = N|D, Z = Q|E, everything else all 20 ----
_AA = "ARNDCQEGHILKMFPSTWYV"
STATE_SET = np.full(256, (1 << 20) - 1, dtype=np.uint32)
for _i, _c in enumerate(_AA):
    STATE_SET[ord(_c)] = STATE_SET[ord(_c.lower())] = 1 << _i
STATE_SET[ord("B")] = STATE_SET[ord("b")] = (1 << _AA.index("N")) | (1 << _AA.index("D"))
STATE_SET[ord("Z")] = STATE_SET[ord("z")] = (1 << _AA.index("Q")) | (1 << _AA.index("E"))


def _bytes(row):
    return row.encode("latin-1") if isinstance(row, str) else bytes(row)


def concatenate(genes):
    """-> (sorted union of names, uint8 matrix [n][sum of columns], col_start)"""
    names = sorted({t for g in genes for t in g[0]})
    at = {t: i for i, t in enumerate(names)}
    col_start = [0]
    for g in genes:
        col_start.append(col_start[-1] + (len(g[1][0]) if g[1] else 0))
    m = np.full((len(names), col_start[-1]), MISSING, dtype=np.uint8)
    for k, (gn, rows) in enumerate(genes):
        for t, row in zip(gn, rows):
            m[at[t], col_start[k]:col_start[k + 1]] = np.frombuffer(_bytes(row), dtype=np.uint8)
    return names, m, col_start


# ---- Fitch steps per column ----
def parse_newick(text):
    """a plain Newick reader (names without quotes, optional lengths and inner labels) -> nested lists of leaf names"""
    pos = 0

    def skip_label():
        nonlocal pos
        b = pos
        while pos < len(text) and text[pos] not in ",();":
            pos += 1
        return text[b:pos].split(":")[0].strip()

    def node():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            kids = [node()]
            while text[pos] == ",":
                pos += 1
                kids.append(node())
            assert text[pos] == ")", (pos, text[pos])
            pos += 1
            skip_label()
            return kids
        return skip_label()

    return node()


def fitch_steps(tree, names, matrix):
    """Fitch's count of every column of `matrix` (rows = names) on the tree as it is rooted in its text: a node's children are
    folded in from the left, a union counts one step.  The count of a binary unrooted tree does not depend on where it is rooted."""
    at = {t: i for i, t in enumerate(names)}
    sets = STATE_SET[matrix]
    steps = np.zeros(matrix.shape[1], dtype=np.int64)

    def up(v):
        nonlocal steps
        if isinstance(v, str):
            return sets[at[v]]
        s = up(v[0])
        for k in v[1:]:
            o = up(k)
            both = s & o
            steps = steps + (both == 0)
            s = np.where(both != 0, both, s | o)
        return s

    up(tree)
    return steps.astype(np.int32)


# ---- minimum steps: the Java's class loop (SequenceAlignment.java:808-902) and the closed form ----
def _bipartition(members, n):
    """Bipartition(bitset, n): the smaller side; on a tie the side holding the lowest index.  equals compares the sides only."""
    members = frozenset(members)
    other = frozenset(range(n)) - members
    if len(other) < len(members) or (len(other) == len(members) and min(other) < min(members)):
        return other
    return members


def min_steps_loop(col):
    """getBipartitionsForAlignmentColumn(column).length - 1; None where the Java returns null (and its caller dereferences it)"""
    n = len(col)
    index = 0
    while index < n and col[index] in (GAP, MISSING):                 # :819-823
        index += 1
    if index >= n:
        return None
    cls = [-1] * n
    cls[index] = 0
    nxt = 1
    for i in range(index + 1, n):                                       # :832-851
        if col[i] != GAP and col[i] != MISSING:
            for j in range(i):
                if col[i] == col[j]:
                    cls[i] = cls[j]
            if cls[i] == -1:
                cls[i] = nxt
                nxt += 1
    sides = {_bipartition([i for i in range(n) if cls[i] == c], n) for c in range(nxt)}      # :856-882: the HashSet removes duplicates
    return len(sides) - 1


def min_steps_closed(col):
    n = len(col)
    classes = len({b for b in col if b not in (GAP, MISSING)})
    shown = sum(b not in (GAP, MISSING) for b in col)
    if classes == 0:
        return None
    return classes - 1 - (1 if classes == 2 and shown == n else 0)


def min_steps(matrix):
    """closed form over every column of a concatenation; raises on a column of only '-' and '?'"""
    out = np.zeros(matrix.shape[1], dtype=np.int32)
    for c in range(matrix.shape[1]):
        v = min_steps_closed(matrix[:, c].tolist())
        if v is None:
            raise ValueError("column %d holds nothing but '-' and '?'" % c)
        out[c] = v
    return out


# ---- tables and totals ----
def ratio_table(steps, mins):
    return np.asarray(steps, dtype=np.float32) / (np.asarray(mins, dtype=np.int32) + 1).astype(np.float32)      # :122


def table_of(statistic, steps, mins):
    steps, mins = np.asarray(steps, dtype=np.int32), np.asarray(mins, dtype=np.int32)
    return steps if statistic == RAW else steps - mins if statistic == BEYOND_MIN else ratio_table(steps, mins)


def float_chain(values):
    """r = 0f; for v in values: r += v -- the Java's sequential float sum"""
    values = np.asarray(values, dtype=np.float32)
    return np.float32(np.cumsum(values, dtype=np.float32)[-1]) if values.size else np.float32(0)


def totals(col_start, steps, mins):
    """:65-103 -> (gene_steps, gene_beyond, gene_ratio)"""
    G = len(col_start) - 1
    ratio = ratio_table(steps, mins)
    gs = [int(np.sum(steps[col_start[g]:col_start[g + 1]], dtype=np.int64)) for g in range(G)]
    gb = [int(np.sum((np.asarray(steps) - np.asarray(mins))[col_start[g]:col_start[g + 1]], dtype=np.int64)) for g in range(G)]
    gr = [float_chain(ratio[col_start[g]:col_start[g + 1]]) for g in range(G)]
    return gs, gb, gr


# ---- draws ----
def mix64(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def key_of(seed, g, reps, b):
    return ((seed + 1) * 0x9E3779B97F4A7C15 + ((g * reps + b) << 32)) & M64


def half_bits(U):
    return max(1, ((U - 1).bit_length() + 1) // 2)


def perm(K, U, x):
    h = half_bits(U)
    m = (1 << h) - 1
    while True:
        L, R = x >> h, x & m
        for r in range(4):
            L, R = R, L ^ (mix64(K + (r << 40) + R) & m)
        x = L << h | R
        if x < U:
            return x


def draw_replace(key, j, U):
    return ((mix64(key + j) >> 32) * U) >> 32


def _mix64_np(z):
    z = z.astype(np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def domain_indices(seed, g, reps, length, U, replace):
    """the same rules on numpy arrays (uint64 arithmetic wraps): -> int64 [reps][length] domain indices"""
    keys = np.array([key_of(seed, g, reps, b) for b in range(reps)], dtype=np.uint64)[:, None]
    j = np.arange(length, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        if replace:
            return (((_mix64_np(keys + j) >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64)
        K = _mix64_np(keys)
        h = np.uint64(half_bits(U))
        m = np.uint64((1 << int(h)) - 1)
        x = np.broadcast_to(j, (reps, length)).copy()
        todo = np.ones(x.shape, dtype=bool)
        Kb = np.broadcast_to(K, x.shape)
        while todo.any():
            xs = x[todo]
            L, R = xs >> h, xs & m
            for r in range(4):
                L, R = R, L ^ (_mix64_np(Kb[todo] + np.uint64(r << 40) + R) & m)
            x[todo] = L << h | R
            todo = x >= np.uint64(U)
        return x.astype(np.int64)


# ---- the thresholds: the Java's loops over that index stream ----
def domain_columns(col_start, g, mask):
    """the columns that are not masked: initialIndexMask marks gene g and every masked gene (:249-259)"""
    G = len(col_start) - 1
    cols = []
    for i in range(G):
        if i == g or (mask is not None and mask[i]):
            continue
        cols.extend(range(col_start[i], col_start[i + 1]))
    return cols


def replicate_columns(col_start, g, rep, replace, multiple, reps, seed, mask=None):
    """the concatenation columns replicate `rep` of gene g draws, in draw order; None under the -1 rule"""
    cols = domain_columns(col_start, g, mask)
    length = col_start[g + 1] - col_start[g]
    if multiple > 0 and len(cols) < length * multiple:
        return None
    key = key_of(seed, g, reps, rep)
    if replace:
        return [cols[draw_replace(key, j, len(cols))] for j in range(length)]
    K = mix64(key)
    return [cols[perm(K, len(cols), j)] for j in range(length)]


def replicate_sums(table, col_start, g, replace, multiple, reps, seed, mask=None):
    """repSteps before the sort: for i < reps, for j < alignmentLength: repSteps[i] += steps[nextIndex].  Without replacement the
    Java's indexUsed is kept and asserted: no column twice.  None under the -1 rule (unmaskedCount < alignmentLength * multiple)."""
    cols = np.array(domain_columns(col_start, g, mask), dtype=np.int64)
    length = col_start[g + 1] - col_start[g]
    U = len(cols)
    if multiple > 0 and U < length * multiple:
        return None
    if length == 0:
        return np.zeros(reps, dtype=table.dtype)
    u = domain_indices(seed, g, reps, length, U, replace)
    assert u.min() >= 0 and u.max() < U
    if not replace:
        s = np.sort(u, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()                          # indexUsed: every column at most once in a replicate
    drawn = np.asarray(table)[cols[u]]
    if drawn.dtype == np.float32:
        return np.cumsum(drawn, axis=1, dtype=np.float32)[:, -1]
    return drawn.sum(axis=1, dtype=np.int64).astype(np.int32)         # the Java's int


def threshold(table, observed, col_start, g, replace, multiple, reps, alpha, seed, mask=None):
    """-> (threshold, n_ge); (-1, -1) under the -1 rule.  :170-173: Arrays.sort(repSteps); r = repSteps[reps - (int)ceil(reps * alpha)]"""
    sums = replicate_sums(table, col_start, g, replace, multiple, reps, seed, mask)
    if sums is None:
        return -1.0, -1
    k = int(math.ceil(reps * alpha))
    assert 1 <= k <= reps
    s = np.sort(sums)
    return float(s[reps - k]), int((sums.astype(np.float64) >= float(observed)).sum())


# the five methods as option sets (statistic, replace, multiple, takes a mask)
JAVA_METHODS = {
    "getThresholdStepsForAlignment": (RAW, False, 0, False),                                   # :141-176
    "getThresholdStepsBeyondMinimumForAlignment": (BEYOND_MIN, False, 0, False),               # :178-213
    "getThresholdStepsBeyondMinimumForAlignment(mask)": (BEYOND_MIN, True, 3, True),           # :240-307, the current one
    "getThresholdStepsBeyondMinimumForAlignmentOLD": (BEYOND_MIN, False, 2, True),             # :309-365
    "getThresholdStepsToMinimumRatioForAlignment": (MIN_RATIO, False, 2, True),                # :367-425
}


def java_threshold(method, steps, mins, col_start, g, reps, alpha, seed, mask=None):
    statistic, replace, multiple, masked = JAVA_METHODS[method]
    gs, gb, gr = totals(col_start, steps, mins)
    observed = (gs, gb, gr)[statistic][g]
    return threshold(table_of(statistic, steps, mins), observed, col_start, g, replace, multiple, reps, alpha, seed, mask if masked else None)


def fake_result(lens, seed, ntax=6):
    """a gene_steps result with made-up per-column values (for the resampler's tests, which need no alignment)"""
    rng = np.random.default_rng(seed)
    col_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    steps = rng.poisson(2.0, int(col_start[-1])).astype(np.int32)
    mins = np.minimum(steps, rng.integers(0, 4, steps.size)).astype(np.int32)
    gs, gb, gr = totals(col_start, steps, mins)
    return {"names": ["t%d" % i for i in range(ntax)], "ncols": int(col_start[-1]), "col_start": col_start, "steps": steps, "min_steps": mins,
            "gene_steps": np.array(gs, dtype=np.int64), "gene_beyond": np.array(gb, dtype=np.int64), "gene_ratio": np.array(gr, dtype=np.float32)}
