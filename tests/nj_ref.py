"""The reference's `nj` tree-building method restated in Python from the Java, for the NJ parity tests.

Read from the reference line by line (package edu.vt.vbi.ci.pepr); Python floats are IEEE doubles and CPython never
contracts a multiply and an add, so every expression below, written in the Java's operand order and grouping, gives the
Java's bits.

* alignment/AlignmentUtilities.java:174-342  convertAminaAcidSequenceToInts: the switch over the 23 letters in either
      case, '-' and '?' (both GAP, :320-331).  Any other byte falls through the switch and is DROPPED (rIndex does not
      move, the array is compressed at :335-339).  The engine refuses such rows; `encode` raises ValueError for them.
* alignment/AlignmentUtilities.java:371-398  loadScoringMatrixFromResource: r = new int[24][24]; lines from the first
      that starts with "A"; cells[j + 1] -> r[i][j] for j < 23 (:387-390), for i < 23 (:392).  The file's order is
      A R N D C Q E G H I L K M F P S T W Y V B J Z X *, the codes' order (AlignmentUtilities constants) is ... V B Z X GAP:
      code Z (21) holds the J line, code X (22) the Z line, row and column 23 stay 0, the X and * lines are never read.
* alignment/SequenceAlignment.java:1042-1067 getPairwiseScores: Arrays.fill(r[i], -1f) (:1056), then r[i][j] +=
      scoreMatrix[c_i(k)][c_j(k)] for every ordered pair, the diagonal included (:1057-1064).
* tree/TreeBuilder.java:346-362  convertSimilarityToDistanceMatrix: maxSimilarity starts at 0 and looks at the diagonal
      only (:350-355); r[i][j] = max - s[i][j] for ALL i, j (:356-360): the diagonal of the distances is not zero.
* tree/TreeBuilder.java:152-344  getNJTreeString: row sums over every j, the diagonal included (:166-172);
      Q = (rMinus2 * d[i][j]) - sums[i] - sums[j] (:180-181); getMinValueCoordinates (:702-720): i < j row major, strict <,
      starting from Double.MAX_VALUE; lengths :221-229 (Math.max(x, 0): -0.0 becomes 0.0); new indices :253-262 (merged
      node at 0, the others keep their order); the copy loop :265-278 reads the UPPER triangle (j from i) and mirrors it,
      never writes [0][0]; the new node's distances :281-289 read ROWS mergeI and mergeJ; three nodes left :303-340: the
      lengths come from the row sums and are NOT clamped; n = 3 returns null (:298-303 never assigns r).
* tree/TreeBuilder.java:34-140   getNJTopology: getMaxValueCoordinates (:730-748, strict >, from -infinity) on the raw
      similarities (getMinValueCoordinates for distances), plain means (:116-124), until two nodes are left: "(x,y);".

Numbers are spelled with repr() here; the tests compare structure and the parsed doubles bit for bit, not spellings.
"""
import re
import struct

LETTERS = "ARNDCQEGHILKMFPSTWYV" + "BZX"
GAP = 23
DISTANCE, SIMILARITY = 0, 1
MAX_VALUE = 1.7976931348623157e308


def encode(row):
    out = []
    for k, ch in enumerate(row):
        u = ch.upper()
        if u in LETTERS and len(u) == 1 and u.isalpha():
            out.append(LETTERS.index(u))
        elif ch in "-?":
            out.append(GAP)
        else:
            raise ValueError("column %d: %r is dropped by the Java" % (k, ch))
    return out


def load_scoring_matrix(lines):
    """loadScoringMatrixFromResource on the lines of a BLOSUM file"""
    r = [[0] * 24 for _ in range(24)]
    it = iter(lines)
    line = next(it)
    while not line.startswith("A"):
        line = next(it)
    i = 0
    while True:
        cells = re.split(r"\s+", line.rstrip("\n"))
        for j in range(23):
            r[i][j] = int(cells[j + 1])
        i += 1
        line = next(it, None)
        if line is None or not i < 23:
            break
    return r


def pairwise_scores(rows, table):
    """getPairwiseScores -> list of lists of float"""
    codes = [encode(r) for r in rows]
    n = len(codes)
    out = [[-1.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            s = 0
            for a, b in zip(codes[i], codes[j]):
                s += table[a][b]
            out[i][j] += s          # integers: the running double of the Java is exact
    return out


def pairwise_scores_np(rows, table):
    """the same through numpy, for the larger test shapes -> int64 array of the raw sums (WITHOUT the -1)"""
    import numpy as np
    t = np.asarray(table, dtype=np.int64)
    c = np.array([encode(r) for r in rows], dtype=np.int64)
    n = c.shape[0]
    out = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        out[i] = t[c[i][None, :], c].sum(axis=1)
    return out


def _java_max0(x):
    return x if x > 0 else (x if x != x else 0.0)


def _min_coords(m):
    bi = bj = -1
    best = MAX_VALUE
    for i in range(len(m)):
        for j in range(i + 1, len(m)):
            if m[i][j] < best:
                best, bi, bj = m[i][j], i, j
    return bi, bj


def _max_coords(m):
    bi = bj = -1
    best = float("-inf")
    for i in range(len(m)):
        for j in range(i + 1, len(m)):
            if m[i][j] > best:
                best, bi, bj = m[i][j], i, j
    return bi, bj


def _new_indices(n, mi, mj):
    idx, off = [0] * n, 1
    for i in range(n):
        if i == mi or i == mj:
            off -= 1
            idx[i] = 0
        else:
            idx[i] = i + off
    return idx


def _copy_unchanged(d, mi, mj, idx):
    n = len(d)
    new = [[0.0] * (n - 1) for _ in range(n - 1)]
    for i in range(n):
        if i != mi:
            for j in range(i, n):
                if j != mj:
                    new[idx[i]][idx[j]] = d[i][j]
                    new[idx[j]][idx[i]] = d[i][j]
    return new


def nj_tree_string(nodes, matrix, matrix_type):
    nodes = list(nodes)
    d = [[float(x) for x in row] for row in matrix]
    if len(nodes) < 4:
        return None
    if matrix_type == SIMILARITY:
        mx = 0.0
        for i in range(len(d)):
            if d[i][i] > mx:
                mx = d[i][i]
        d = [[mx - x for x in row] for row in d]
    while True:
        n = len(nodes)
        sums = []
        for i in range(n):
            s = 0.0
            for j in range(n):
                s += d[i][j]
            sums.append(s)
        r2 = n - 2
        q = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1, n):
                q[i][j] = q[j][i] = (r2 * d[i][j]) - sums[i] - sums[j]
        mi, mj = _min_coords(q)
        to_i = (d[mi][mj] / 2) + ((1 / (2.0 * r2)) * (sums[mi] - sums[mj]))
        to_j = d[mi][mj] - to_i
        to_i, to_j = _java_max0(to_i), _java_max0(to_j)
        combined = "(" + nodes[mi] + ":" + repr(to_i) + "," + nodes[mj] + ":" + repr(to_j) + ")"
        idx = _new_indices(n, mi, mj)
        new = _copy_unchanged(d, mi, mj, idx)
        for i in range(n):
            if idx[i] != 0:
                mean = (d[mi][i] + d[mj][i] - d[mi][mj]) / 2
                new[0][idx[i]] = mean
                new[idx[i]][0] = mean
        nn = [None] * (n - 1)
        for i in range(n):
            nn[idx[i]] = nodes[i]
        nn[0] = combined
        nodes, d = nn, new
        if len(nodes) > 3:
            continue
        s = [0.0, 0.0, 0.0]
        for i in range(3):
            for j in range(3):
                s[i] += d[i][j]
        d0 = (d[0][1] / 2) + (0.5 * (s[0] - s[1]))
        d1 = (d[1][2] / 2) + (0.5 * (s[1] - s[2]))
        d2 = (d[2][0] / 2) + (0.5 * (s[2] - s[0]))
        return "(" + nodes[0] + ":" + repr(d0) + "," + nodes[1] + ":" + repr(d1) + "," + nodes[2] + ":" + repr(d2) + ");"


def nj_topology(nodes, matrix, matrix_type):
    nodes = list(nodes)
    d = [[float(x) for x in row] for row in matrix]
    while True:
        n = len(nodes)
        mi, mj = _min_coords(d) if matrix_type == DISTANCE else _max_coords(d)
        combined = "(" + nodes[mi] + "," + nodes[mj] + ")"
        if n == 2:
            return combined + ";"
        idx = _new_indices(n, mi, mj)
        new = _copy_unchanged(d, mi, mj, idx)
        for i in range(n):
            if idx[i] != 0:
                mean = (d[mi][i] + d[mj][i]) / 2
                new[0][idx[i]] = mean
                new[idx[i]][0] = mean
        nn = [None] * (n - 1)
        for i in range(n):
            nn[idx[i]] = nodes[i]
        nn[0] = combined
        nodes, d = nn, new


_NUM = re.compile(r":([-+0-9.eE]+|[-+]?(?:inf|nan|Infinity|NaN))")


def split_tree(newick):
    """-> (the text with every length replaced by ':#', the lengths as 8-byte patterns): two trees are the same tree with
    the same doubles iff both parts are equal.  Support labels behind ')' stay in the structure."""
    lens = [struct.pack("<d", float(m.group(1))) for m in _NUM.finditer(newick)]
    return _NUM.sub(":#", newick), lens


def strip_labels(newick):
    """the text without the support counts behind ')'"""
    return re.sub(r"\)\d+", ")", newick)


def tree_from_rows(names, rows, table, form_topology=False):
    s = pairwise_scores(rows, table)
    return nj_topology(names, s, SIMILARITY) if form_topology else nj_tree_string(names, s, SIMILARITY)


def fasta_rows(text):
    """names, rows of pml_concatenate's FASTA text"""
    names, rows = [], []
    for line in text.splitlines():
        if line.startswith(">"):
            names.append(line[1:]); rows.append("")
        elif line:
            rows[-1] += line
    return names, rows
