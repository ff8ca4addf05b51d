"""The homolog-group rule of include/peprml.h ("Homolog groups") restated in numpy and plain Python: Markov clustering of the hit
graph as `mcl --abc -I r` does it on components of up to 1100 nodes, and the Java around it (PhyloPipeline.java:357-406,
882-1024; SequenceSetProviderImpl.java; PhylogenomicPipeline2.java:564-605).  Not a test module; the tests import it."""
import numpy as np

DEFAULTS = dict(inflation=1.5, prune_inverse=10000.0, chaos_eps=1e-3, max_iter=10000)


# ---- graph ----
def parse_abc(text):
    """labels in order of first appearance (id1 before id2 on a line) and the arcs (a, b, w) as indices"""
    index, labels, arcs = {}, [], []
    for line in text.split("\n"):
        f = line.split()
        if len(f) < 2:
            continue
        for lab in f[:2]:
            if lab not in index:
                index[lab] = len(labels)
                labels.append(lab)
        arcs.append((index[f[0]], index[f[1]], float(f[2]) if len(f) > 2 else 1.0))
    return labels, arcs


def mirrored(n, arcs):
    """G with the max-combined mirror; self hits dropped; a weight that is not finite or <= 0 raises ValueError"""
    G = np.zeros((n, n))
    for a, b, w in arcs:
        if not np.isfinite(w) or w <= 0:
            raise ValueError("weight %r" % (w,))
        if a != b:
            G[a, b] = G[b, a] = max(G[a, b], w)
    return G


def components(G):
    """lists of node indices, each ascending, in order of their smallest member"""
    n = G.shape[0]
    seen, out = np.zeros(n, bool), []
    for s in range(n):
        if seen[s]:
            continue
        seen[s] = True
        todo, comp = [s], []
        while todo:
            v = todo.pop()
            comp.append(v)
            for u in np.nonzero(G[v])[0]:
                if not seen[u]:
                    seen[u] = True
                    todo.append(int(u))
        out.append(sorted(comp))
    return out


def start_matrix(G, dtype=np.float64):
    """loops = the column's largest entry (1 for an otherwise empty column), columns divided by their sums"""
    M = np.array(G, dtype=dtype)
    n = M.shape[0]
    for j in range(n):
        m = M[:, j].max() if n else 0
        M[j, j] = m if m > 0 else 1
    return (M / M.sum(axis=0, dtype=dtype)).astype(dtype)


# ---- one iteration ----
def mcl_step(M, inflation=1.5, prune_inverse=10000.0):
    """returns (the next matrix, chaos, the expanded matrix before pruning), all in M's dtype"""
    dt = M.dtype.type
    E = (M @ M).astype(M.dtype)
    P = np.where(E < dt(1.0) / dt(prune_inverse), dt(0), E)
    P = (P / P.sum(axis=0, dtype=M.dtype)).astype(M.dtype)
    chaos = float((P.max(axis=0) - (P * P).sum(axis=0, dtype=M.dtype)).max())
    Q = np.power(P, dt(inflation)).astype(M.dtype)
    Q = (Q / Q.sum(axis=0, dtype=M.dtype)).astype(M.dtype)
    return Q, chaos, E


def interpret(M):
    """clusters (lists of ascending indices, unordered) of a limit matrix"""
    n = M.shape[0]
    att = [i for i in range(n) if M[i, i] > 0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for b in att:
        for a in att:
            if M[a, b] > 0:
                parent[find(a)] = find(b)
    groups = {}
    for j in range(n):
        best = -1
        for a in att:                                  # the largest M[a, j], the lowest index of equals
            if best < 0 or M[a, j] > M[best, j]:
                best = a
        key = ("a", find(best)) if best >= 0 else ("n", j)     # no attractor at all: the node stays alone
        groups.setdefault(key, []).append(j)
    return list(groups.values())


def mcl_component(M, inflation=1.5, prune_inverse=10000.0, chaos_eps=1e-3, max_iter=10000):
    it = 0
    while it < max_iter:
        M, chaos, _ = mcl_step(M, inflation, prune_inverse)
        it += 1
        if chaos < chaos_eps:
            break
    return interpret(M), it


def order_clusters(clusters):
    """largest first, ties to the lower smallest member, members ascending"""
    cl = [sorted(c) for c in clusters]
    cl.sort(key=lambda c: (-len(c), c[0]))
    return cl


def mcl_clusters(n, arcs, dtype=np.float64, **opts):
    """(clusters in output order, components, iterations of the slowest component)"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in opts.items() if v})
    G = mirrored(n, arcs)
    clusters, iters, comps = [], 0, components(G)
    for comp in comps:
        M = start_matrix(G[np.ix_(comp, comp)], dtype)
        cl, it = mcl_component(M, o["inflation"], o["prune_inverse"], o["chaos_eps"], o["max_iter"])
        iters = max(iters, it)
        clusters += [[comp[i] for i in c] for c in cl]
    return order_clusters(clusters), len(comps), iters


def mcl_lines(text, dtype=np.float64, **opts):
    """mcl's output lines for an --abc input text"""
    labels, arcs = parse_abc(text)
    cl, _, _ = mcl_clusters(len(labels), arcs, dtype, **opts)
    return ["\t".join(labels[i] for i in c) for c in cl]


# ---- the Java around MCL ----
def _fields(line):
    f = line.split("\t")
    while f and f[-1] == "":                           # Pattern.split / String.split drop trailing empty strings
        f.pop()
    return f


def _lines(text):
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def filter_hit_pairs(text):
    """filterHitPairFile, PhyloPipeline.java:989-1024: fields 0, 1 and 11 of the lines with more than one field"""
    out = []
    for line in _lines(text):
        f = _fields(line)
        if len(f) > 1:                                 # :1008
            out.append(f[0] + "\t" + f[1] + "\t" + f[11] + "\n")     # :1009-1010 (an IndexError is the Java's exception)
    return "".join(out)


def java_float_to_string(x):
    """Float.toString of the f32 nearest x, finite values; the shortest digits that round-trip (the known JDK cases that are
    not shortest are not reproduced)"""
    with np.errstate(over="ignore"):
        v = np.float32(x)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "-Infinity" if v < 0 else "Infinity"
    if v == 0:
        return "-0.0" if np.signbit(v) else "0.0"
    s = np.format_float_scientific(v, unique=True, trim="0", exp_digits=1)     # d.dddde[+-]n
    mant, exp = s.split("e")
    sign = "-" if mant.startswith("-") else ""
    mant = mant.lstrip("-")
    e = int(exp)
    digits = mant.replace(".", "").rstrip("0") or "0"
    if 1e-3 <= abs(float(v)) < 1e7:
        if e >= 0:
            whole, frac = digits[:e + 1].ljust(e + 1, "0"), digits[e + 1:]
        else:
            whole, frac = "0", "0" * (-e - 1) + digits
        return sign + whole + "." + (frac or "0")
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(e)


def filter_bidirectional(text, score_field=11):
    """filterForBidirectional, PhyloPipeline.java:911-987"""
    stored, out = {}, []
    for line in _lines(text):
        f = _fields(line)
        if len(f) > score_field:                       # :951
            pair = (min(f[0], f[1]), max(f[0], f[1]))  # IntPair.java:12-21: unordered
            if pair not in stored:                     # :958-961
                stored[pair] = float(np.float32(float(f[score_field])))
            else:                                      # :962-973
                out.append(f[0] + "\t" + f[1] + "\t" + f[score_field] + "\n")
                out.append(f[1] + "\t" + f[0] + "\t" + java_float_to_string(stored[pair]) + "\n")
                del stored[pair]
    return "".join(out)


def select_sets(clusters, taxon_of, min_taxa, max_taxa, rep_only, target_ntax, target_min_gene):
    """indices of the kept clusters: SequenceSetProviderImpl.java:115-140, 223-247, 295-329, PhylogenomicPipeline2.java:564-605"""
    keep = [k for k, c in enumerate(clusters) if min_taxa <= len(c) <= max_taxa]          # :126-127: a sequence count
    ntax = {k: len(set(taxon_of[i] for i in clusters[k])) for k in keep}
    if rep_only:                                                                          # :575-578, :223-247
        keep = [k for k in keep if ntax[k] == len(clusters[k])]
    if len(keep) > target_min_gene:                                                       # :580
        for t in range(min_taxa + 1, target_ntax + 1):                                    # :583
            if sum(1 for k in keep if ntax[k] >= t) >= target_min_gene:                   # :584, :320-329
                keep = [k for k in keep if ntax[k] >= t]                                  # :591, :295-312
    return keep
