"""The reference's column trimmers (`-uniform_trim` and MSATrimmer's two sibling filters) restated in Python from the Java,
for the trim parity tests.  A restatement with line citations, as congruence_ref.py: not a copy.

Read from the reference (package edu.vt.vbi.ci.pepr.alignment).  A gene is (names, rows); a row is bytes or a str of one-byte
characters; a column is the list of its bytes as ints.  n = the gene's own number of rows; bytes are compared by identity.

* MSATrimmer.java:205-253  trimUniformColumns, what `-uniform_trim` runs (HandyConstants.java:26, PhylogenomicPipeline2.java
      :205, getAlignment :788-795): column i is kept iff getMinimumStepsPerSite()[i] != 0 (:217-229).
* SequenceAlignment.java:673-682  getMinimumStepsPerSite: the size of the column's Bipartition array less one.
* SequenceAlignment.java:808-902  getBipartitionsForAlignmentColumn: null for a column of nothing but '-' (GAP_CHAR) and '?'
      (MISSING_CHAR) -- getMinimumStepsPerSite then dereferences null; here: ValueError.  Otherwise one Bipartition per
      distinct char other than those two, collected in a HashSet, so equal ones count once.
* tree/Bipartition.java:41-64, equals :292-303: a bipartition is normalised over ALL n rows and compared by its sides alone, so
      two classes that cover all n rows are ONE bipartition (a class and its complement); any other two classes differ.  Hence:
      kept iff classes >= 3, or classes == 2 and some row shows '-' or '?'.  AAAC and AACC are dropped, AAC- is kept.
* MSATrimmer.java:141-203  trimUniformativeColumns: the first char other than '-' (:157-160), then uniform while every later
      char equals it or is '-' (:167-170); '?' is a character like any other.  Kept iff not uniform; all-'-' is uniform.
* MSATrimmer.java:264-351  trimTopologicallyUninformativeColumns: the same uniform test first (:281-294); a non-uniform column
      goes through the nested loop :303-326 (topological_loop below is that loop, statement for statement); the closed form is
      "at least two distinct chars other than '-' each occur at least twice".  uninformativeCount (:297, :321) is a debug print.
* The kept columns keep their order, rows and taxa are untouched (:184-196, :234-246, :333-345); the first two set the name to
      getName() + "_ui" (:197, :247), the third sets none.
* SequenceAlignment.java:1074-1092  getProportionGapOrMissing: its numerator is the number of '-' and '?' cells.
"""
GAP, MISSING = ord("-"), ord("?")
UNIFORM, GAP_UNIFORM, TOPOLOGICAL = 0, 1, 2
KEEP_UNIFORM, KEEP_GAP_UNIFORM, KEEP_TOPOLOGICAL, ALL_GAP = 1, 2, 4, 8


def row_bytes(row):
    return row.encode("latin-1") if isinstance(row, str) else bytes(row)


def columns(gene):
    rows = [row_bytes(r) for r in gene[1]]
    return [[r[c] for r in rows] for c in range(len(rows[0]) if rows else 0)]


def bipartitions(col):
    """getBipartitionsForAlignmentColumn over the gene's own rows: a set of normalised sides, or None"""
    n = len(col)
    classes = {}
    for t, b in enumerate(col):
        if b != GAP and b != MISSING:
            classes[b] = classes.get(b, 0) | (1 << t)
    if not classes:
        return None
    full = (1 << n) - 1
    out = set()
    for a in classes.values():
        comp = full & ~a
        ca, cc = bin(a).count("1"), bin(comp).count("1")
        out.add(a if ca < cc or (ca == cc and a & 1) else comp)
    return out


def keep_uniform(col):
    b = bipartitions(col)
    if b is None:
        raise ValueError("a column of nothing but '-' and '?': the Java dereferences null")
    return len(b) - 1 != 0


def is_gap_uniform(col):
    j = 0
    while j < len(col) and col[j] == GAP:
        j += 1
    uniform = True
    if j < len(col):
        first = col[j]
        j += 1
        while j < len(col) and uniform:
            uniform = col[j] == first or col[j] == GAP
            j += 1
    return uniform


def keep_gap_uniform(col):
    return not is_gap_uniform(col)


def topological_loop(col):
    """MSATrimmer.java:296-326 for a column that has a non-'-' char: True when the column is added to the informative ones"""
    if is_gap_uniform(col):
        return False
    n = len(col)
    multiple = set()
    counts = [0] * n
    j = 0
    while j < n:
        if col[j] != GAP:
            k = 0
            while k < n:
                if col[j] == col[k]:
                    counts[j] += 1
                    if counts[j] > 1:
                        multiple.add(col[j])
                        k = n
                        if len(multiple) == 2:
                            return True
                k += 1
        j += 1
    return False


def keep_topological(col):
    """the closed form"""
    return len({b for b in col if b != GAP and col.count(b) >= 2}) >= 2


def flags(col):
    """the byte pml_debug_column_flags gives: bits 0 to 2 = kept under the three modes, bit 3 = only '-' / '?'"""
    all_gap = bipartitions(col) is None
    return ((0 if all_gap else KEEP_UNIFORM * keep_uniform(col)) | KEEP_GAP_UNIFORM * keep_gap_uniform(col) |
            KEEP_TOPOLOGICAL * keep_topological(col) | ALL_GAP * all_gap)


KEEPERS = {UNIFORM: keep_uniform, GAP_UNIFORM: keep_gap_uniform, TOPOLOGICAL: keep_topological}


def trim(gene, mode):
    """-> {"kept_cols", "rows" (the type of the input's rows), "ncols", "nkept", "gap_or_missing"}"""
    cols = columns(gene)
    kept = [c for c, col in enumerate(cols) if KEEPERS[mode](col)]
    rows = [bytes(row_bytes(r)[c] for c in kept) for r in gene[1]]
    if gene[1] and isinstance(gene[1][0], str):
        rows = [r.decode("latin-1") for r in rows]
    return {"names": list(gene[0]), "rows": rows, "kept_cols": kept, "ncols": len(cols), "nkept": len(kept),
            "gap_or_missing": sum(b in (GAP, MISSING) for r in gene[1] for b in row_bytes(r))}


def trim_genes(genes, mode=UNIFORM):
    return [trim(g, mode) for g in genes]
