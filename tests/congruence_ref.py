"""The reference's `-congruence_filter` restated in Python from the Java, for the congruence parity tests.

Read from the reference (package edu.vt.vbi.ci.pepr); taxon sets are Python ints, taxon i of the concatenation's sorted
name union = bit i.

* alignment/SequenceAlignment.java:808-882  getBipartitionsForAlignmentColumn: a column of nothing but '-' (GAP_CHAR) and
      '?' (MISSING_CHAR) returns null; otherwise every distinct char other than those two gives the set of taxa that show
      it, bytes compared by identity (no alphabet: 'a' and 'A' differ); the HashSet at :874-882 keeps equal bipartitions
      of one column once.  participatingTaxa is set but never read by equals / isCompatible
      (useParticipatingTaxonSetForEqualityCheck is false).
* tree/Bipartition.java:41-64  Bipartition(ExtendedBitSet, int): the complement over ALL size taxa; the side with fewer
      members is kept, on a tie the side whose first set bit is lower, i.e. the side that holds taxon 0.
      equals (:292-303) compares the smaller sides alone.
* alignment/SequenceAlignment.java:697-719  getBipartitionsForColumns(10000): every bipartition of every column whose
      smaller side has at least 2 members.
* tree/BipartitionSet.java:84-139  setBipartitions: counts per distinct bipartition; util/StatisticsUtilities.java:998-1011
      getDistribution: dist[c] = number of values equal to c, c in 0..max; the cutoff loop :113-118; everything with
      count >= cutoff is kept (:123-129), ties included.
      Arrays.sort with compareTo = otherHash - thisHash is only a grouping device there.  From 32 taxa upward that int
      difference can overflow, equal bipartitions may then end up apart and the Java loses counts in a way that depends on
      the JDK's sort.  This file counts per distinct split: the Java's result whenever its sort groups equal splits, which
      it always does below 32 taxa.
* tree/BipartitionSet.java:642-652  getCost, tree/Bipartition.java:125-149  isCompatible: the cost of b is the sum of the
      counts of the kept k with b & k non-empty, != b and != k.
* alignment/ConcatenatedSequenceAlignment.java:43-62  getBipartitionsForAlignment: the distinct bipartitions of a gene's
      columns, trivial ones included, each once.
* tree/pipeline/PhylogenomicPipeline2.java:429-511  filterForCongruence: topN = 4 n (:437); costSum over the gene's
      bipartitions, meanCost = costSum / length by integer division (:455-472; sums here are Python ints, the Java's int
      wherever that does not overflow); percentileIndex = (int)(G - G * p) in doubles (:485); maxCost =
      sorted[percentileIndex] (:487); gene i is kept iff i <= percentileIndex and meanCost_i <= maxCost (:497): the first
      condition compares the gene's POSITION in the input with a rank -- the Java as it stands.
      :191-195: a trim_percent of 1.0 or more is divided by 100.
A gene without columns is refused (ValueError): the Java drops it from one array and not from the other.
"""
import math

GAP, MISSING = "-", "?"


def union_names(genes):
    """MSAConcatenator's taxa: the sorted union of the genes' names"""
    return sorted({t for names, _ in genes for t in names})


def norm(a, n):
    comp = ((1 << n) - 1) & ~a
    ca, cc = bin(a).count("1"), bin(comp).count("1")
    if ca < cc:
        return a
    if ca > cc:
        return comp
    return a if a & 1 else comp


def column_splits(chars, n):
    """chars: (taxon index, char) of the taxa the gene has -> the set of the column's splits, or None (all gap / missing)"""
    classes = {}
    for t, ch in chars:
        if ch != GAP and ch != MISSING:
            classes[ch] = classes.get(ch, 0) | (1 << t)
    if not classes:
        return None
    return {norm(a, n) for a in classes.values()}


def gene_column_splits(gene, names):
    """the splits of every column of one gene over the union `names` (a repeated name: its last row, as pml_concatenate)"""
    index = {t: i for i, t in enumerate(names)}
    rows = {}
    for t, r in zip(gene[0], gene[1]):
        rows[index[t]] = r
    ncol = len(gene[1][0]) if gene[1] else 0
    return [column_splits([(t, r[c]) for t, r in rows.items()], len(names)) for c in range(ncol)]


def size(s):
    return bin(s).count("1")


def conflict(b, k):
    x = b & k
    return x != 0 and x != b and x != k


def kept_set(counts, n):
    """counts: {split: columns} of the non-trivial splits -> (cutoff, {split: count} of the kept ones)"""
    if not counts:
        return 0, {}
    top_n = 4 * n
    mx = max(counts.values())
    dist = [0] * (mx + 1)
    for c in counts.values():
        dist[c] += 1
    cutoff, included, i = 0, 0, mx
    while i >= 0 and included < top_n:
        cutoff = i
        included += dist[i]
        i -= 1
    return cutoff, {s: c for s, c in counts.items() if c >= cutoff}


def congruence_costs(genes):
    names = union_names(genes)
    n = len(names)
    per_gene = []
    counts = {}
    for g, gene in enumerate(genes):
        if not gene[0] or not gene[1] or len(gene[1][0]) == 0:
            raise ValueError("gene %d has no columns" % g)
        cols = gene_column_splits(gene, names)
        per_gene.append(cols)
        for sp in cols:
            for s in sp or ():
                if size(s) >= 2:
                    counts[s] = counts.get(s, 0) + 1
    cutoff, kept = kept_set(counts, n)
    cache = {}

    def cost(b):
        if b not in cache:
            cache[b] = sum(c for k, c in kept.items() if conflict(b, k))
        return cache[b]
    cost_sum, mean_cost, nsplits = [], [], []
    for gene, cols in zip(genes, per_gene):
        bg = set()
        for sp in cols:
            bg |= sp or set()
        cs = sum(cost(b) for b in bg)
        cost_sum.append(cs)
        mean_cost.append(cs // len(gene[1][0]))
        nsplits.append(len(bg))
    return {"names": names, "n": n, "cutoff": cutoff, "counts": counts,
            "kept": {s: (c, cost(s)) for s, c in kept.items()},
            "cost_sum": cost_sum, "mean_cost": mean_cost, "nsplits": nsplits}


def members(s, names):
    return frozenset(names[i] for i in range(len(names)) if s >> i & 1)


def kept_splits(res):
    """K as a set of (members, count, cost)"""
    return {(members(s, res["names"]), c, k) for s, (c, k) in res["kept"].items()}


def select(mean_cost, p):
    """rule 7 -> (keep flags, idx, max_cost); p <= 0, NaN or an index outside the genes raises ValueError (the Java throws)"""
    p = float(p)
    if not p > 0 or math.isnan(p):
        raise ValueError("trim_percent must be positive")
    if p >= 1.0:
        p /= 100
    g = len(mean_cost)
    idx = int(g - (g * p))
    if idx < 0 or idx >= g:
        raise ValueError("percentile index %d outside the %d genes" % (idx, g))
    max_cost = sorted(mean_cost)[idx]
    return [i <= idx and m <= max_cost for i, m in enumerate(mean_cost)], idx, max_cost


def congruence_filter(genes, p=0.1):
    res = congruence_costs(genes)
    keep, idx, max_cost = select(res["mean_cost"], p)
    res.update(keep=keep, idx=idx, max_cost=max_cost)
    return res
