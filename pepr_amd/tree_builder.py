"""Host-side mirror of the reference's tree-building interface for the hot path.

Same names, argument meaning and error behaviour as the Java classes, so that the parity tests
read like the reference's own call sites; every `run()` goes through the C ABI
(include/peprml.h) to the HIP engine instead of spawning a process:

  PhylogeneticTreeBuilder  <- .../pepr/tree/pipeline/PhylogeneticTreeBuilder.java:97-129,168-196,215-338
  RAxMLRunner              <- .../pepr/tree/RAxMLRunner.java:64-152,162-213,320-336
  FastTreeRunner           <- .../pepr/tree/FastTreeRunner.java:38-135,142-199,235
  TreeComparison.runConsel <- .../pepr/tree/TreeComparison.java:812-885
  compareAllvsAll, compareSlidingWindow, rollingComparison, getBranchDistance, getDiscrepantBranchDistance
                           <- .../pepr/tree/TreeComparison.java:267-288, :241-265, :457-466, :607-747, :756-810 (pml_tree_compare)
  BasicTree.removeTaxon, pruneToCommonTaxa
                           <- .../pepr/tree/BasicTree.java:888-946, TreeComparison.java:83-128 (host text work, no device)
  NeighborJoiningRunner    <- .../pepr/tree/pipeline/PhylogeneticTreeBuilder.java:198-208 buildNeighborJoiningTree (method "nj")
  buildConcatenatedNeighborJoiningTree
                           <- .../pepr/tree/pipeline/PhylogenomicPipeline2.java:1279-1293 (the `-nj true` path: topology only)
  buildConcatenatedTreeWithGeneWiseJackKnifeSupport
                           <- .../pepr/tree/pipeline/PhylogenomicPipeline2.java:994-1126,1227-1275,1587-1633

Behaviour kept from the reference: a failed build leaves the result `None` (FastTreeRunner.java:
125-131 logs and continues; callers see a null tree string); the ML matrix is a RAxML model
string (default PROTGAMMAWAG, PhylogenomicPipeline2.java:248-250); threads/processes are accepted
and ignored (the GPU engine needs no -T).  The parsimony bootstrap (-Y -N) and buildConcatenatedTree
(PhylogenomicPipeline2.java:836-890) go through pml_bootstrap2.  Not mirrored (out of scope,
SURVEY.md 8a): nucleotide (-gtr -nt).
"""
import logging
import os

from . import engine

ML, FAST_TREE, PARSIMONY, PARSIMONY_BL, NEIGHBOR_JOINING = "ml", "FastTree", "parsimony", "parsimony_bl", "nj"
log = logging.getLogger("pepr_amd")
_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = engine.Context(0)
    return _default_ctx


class SequenceAlignment:
    """Minimal stand-in for .../pepr/alignment/SequenceAlignment.java: taxa + aligned char rows."""

    def __init__(self, taxa, rows, name=None):
        self.taxa = list(taxa)
        self.rows = list(rows)
        self.name = name

    def getName(self):
        return self.name

    def setName(self, name):
        self.name = name

    def getTaxa(self):
        return self.taxa

    def getLength(self):
        return len(self.rows[0]) if self.rows else 0

    def as_gene(self):
        return (self.taxa, self.rows)


def _model_from_matrix(matrix, ctx=None):
    """RAxML -m strings PEPR passes (RAxMLRunner.java:115-132; the 23 names of -matrix_eval,
    PhylogenomicPipeline2.java:260-284).  Built in: PROTGAMMAWAG (WAG exchangeabilities, RAxML's 3-decimal
    frequencies, Gamma4), PROTGAMMAWAGF (the same with frequencies counted from the alignment) and PROTGAMMAGTR
    (exchangeabilities estimated from the alignment).  PROTGAMMA<NAME> / PROTGAMMA<NAME>F is the matrix of the PAML file
    <name>.dat in the directory $PEPRML_MODEL_DIR, registered on the context; no table ships with the engine.  A
    likelihood is never reported under another model's name: a name whose table is not there, PROTCAT*, PROTGAMMAI*,
    PROTMIX* and the nucleotide models raise."""
    m = (matrix or "PROTGAMMAWAG").upper()
    if m == "PROTGAMMAWAGF":
        return {"ncat": 4, "pi_mode": engine.PI_EMPIRICAL}
    if m == "PROTGAMMAGTR":
        return {"ncat": 4, "pi_mode": engine.PI_GTR}
    if m == "PROTGAMMAWAG":
        return {"ncat": 4, "pi_mode": engine.PI_RAXML_3DP}
    d, name = os.environ.get("PEPRML_MODEL_DIR"), m[9:].lower() if m.startswith("PROTGAMMA") else ""
    if d and name.isalnum() and not name.startswith("i"):
        for stem, f in ((name, 0), (name[:-1], 1)) if name.endswith("f") and len(name) > 1 else ((name, 0),):
            path = os.path.join(d, stem + ".dat")
            if os.path.isfile(path):
                ex, pi = engine.parse_paml(open(path).read())
                return {"ncat": 4, "pi_mode": (ctx or default_context()).register_matrix(stem, ex, pi) + f}
    raise ValueError("the GPU engine has PROTGAMMAWAG, PROTGAMMAWAGF and PROTGAMMAGTR built in and takes PROTGAMMA<NAME>[F] "
                     "from <name>.dat in $PEPRML_MODEL_DIR; %r is not built (it would be a different likelihood function, "
                     "not a variant spelling)" % matrix)


# candidates of a prune that get the thorough insertion under setSearchSchedule("raxml") and the shim's PEPRML_SEARCH_SCHEDULE=raxml:
# DESIGN.md 9, the table of tools/search_schedule_eval.py
THOROUGH_TOP = 3


class RAxMLRunner:
    def __init__(self, threads=1, ctx=None):
        self.threads = threads
        self.ctx = ctx
        self.alignment = None
        self.matrix = "PROTGAMMAWAG"
        self.bootstrapReps = 0
        self.perSiteLL = False
        self.perSiteLLTrees = None
        self.bestTree = None
        self.perSiteLLs = None
        self.lnl = None
        self.alpha = None
        self.spr_radius = 5           # RAxML "best rearrangement setting 5" 
        self.algorithm = 0            # 1 = parsimony only, 2 = parsimony + ML lengths (RAxMLRunner.java:28-29)
        self.parsimonyTree = None
        self.parsimonyWithBLTree = None
        self.bootstrapTrees = None    # the replicate trees of a parsimony bootstrap (-Y -N)
        self.bestTreeWithSupports = None
        self.seed = 12345
        self.searchSchedule = None    # None: one fixed radius (spr_radius); "raxml": pml_search2's schedule, radius determined per gene
        self.radiusChosen = None

    def setAlignment(self, a):
        self.alignment = a

    def getAlignment(self):
        return self.alignment

    def setSearchSchedule(self, s):
        """None (default): today's search at spr_radius.  "raxml": RAxML's schedule -- the rearrangement radius is
        determined on the start tree (5, 10 ... 25), fast lazy SPR cycles at it, then the thorough phase with the
        THOROUGH_TOP best candidates of a prune (engine.Context.search2)."""
        if s not in (None, "raxml"):
            raise ValueError("search schedule must be None or \"raxml\", got %r" % (s,))
        self.searchSchedule = s

    def getRadiusChosen(self):
        return self.radiusChosen

    def setMatrix(self, m):
        self.matrix = m

    def setBootstrapReps(self, reps):
        self.bootstrapReps = reps

    def setUseTaxonNames(self, b):
        pass

    def setParsimonyOnly(self, b):          # RAxMLRunner.java:542-548
        if b:
            self.algorithm = 1

    def setParsimonyWithBL(self, b):        # RAxMLRunner.java:550-556
        if b:
            self.algorithm = 2

    def getParsimonyTree(self):             # RAxML_parsimonyTree.<run>, RAxMLRunner.java:338-359
        return self.parsimonyTree

    def getParsimonyWithBLTree(self):       # RAxML_result.<run>BL, RAxMLRunner.java:361-383
        return self.parsimonyWithBLTree

    def setPerSiteLogLikelihoods(self, b):
        self.perSiteLL = b

    def setPerSiteLLTrees(self, trees):
        self.perSiteLLTrees = list(trees)

    def run(self):
        """-f d (ML search) or, with setPerSiteLogLikelihoods(true), -f g on the given trees."""
        mdl = _model_from_matrix(self.matrix, self.ctx)          # an unbuilt model name is refused, loudly, before any device work
        ctx = self.ctx or default_context()
        try:
            gene = self.alignment.as_gene()
            if self.perSiteLL:
                self.perSiteLLs = []
                for nw in self.perSiteLLTrees:
                    if mdl["pi_mode"] == engine.PI_GTR:             # the estimated matrix lives in the batch that estimated it
                        b = engine.Batch(ctx, [gene], [nw], **mdl)
                        b.optimize()
                        self.perSiteLLs.append(b.site_lnl(0, len(gene[1][0])))
                        b.close()
                        continue
                    o = ctx.optimize([gene], [nw], **mdl)[0]        # RAxML -f g optimises model + lengths first
                    r = ctx.score([gene], [o["newick"]], alpha=o["alpha"], site_lnl=True, **mdl)[0]
                    self.perSiteLLs.append(r["site_lnl"])
                return
            if self.algorithm in (1, 2):
                if self.bootstrapReps:                                         # -Y -N reps (RAxMLRunner.java:134-137): pml_bootstrap2
                    method = engine.TREE_PARSIMONY if self.algorithm == 1 else engine.TREE_PARSIMONY_BL
                    r = ctx.bootstrap2([gene], reps=self.bootstrapReps, seed=self.seed, method=method, parsimony_radius=20, **mdl)
                    self.bootstrapTrees = r["replicates"]
                    if self.algorithm == 1:
                        self.parsimonyTree = r["newick"]
                    else:
                        self.parsimonyWithBLTree, self.lnl, self.alpha = r["newick"], r["lnl"], r["alpha"]
                    return
                p = ctx.parsimony([gene], seed=self.seed)[0]                  # -f d -y
                self.parsimonyTree = p["newick"]
                if self.algorithm == 2:                                        # -f e -t RAxML_parsimonyTree.<run>
                    o = ctx.optimize([gene], [p["newick"]], **mdl)[0]
                    self.parsimonyWithBLTree, self.lnl, self.alpha = o["newick"], o["lnl"], o["alpha"]
                return
            if self.bootstrapReps:                                                # -f a -x <odd seed> -N reps
                r = ctx.bootstrap(gene, reps=self.bootstrapReps, seed=self.seed | 1, spr_radius=self.spr_radius, **mdl)
                self.bestTreeWithSupports, self.lnl, self.alpha = r["newick"], r["lnl"], r["alpha"]
                self.bestTree = None                                              # -f a writes no RAxML_result
                return
            if self.searchSchedule == "raxml":
                res, tr = ctx.search2([gene], None, radius="auto", thorough=True, thorough_top=THOROUGH_TOP, seed=self.seed, trace=True, **mdl)
                r, self.radiusChosen = res[0], tr[0]["radius_chosen"]
            else:
                r = ctx.search([gene], None, spr_radius=self.spr_radius, seed=self.seed, **mdl)[0]      # parsimony start, as -f d
            self.bestTree, self.lnl, self.alpha = r["newick"], r["lnl"], r["alpha"]
        except Exception as e:          # reference: rc logged, result stays null
            log.error("RAxMLRunner failed: %s", e)
            self.bestTree = self.parsimonyTree = self.parsimonyWithBLTree = None

    def getBestTree(self):
        return self.bestTree

    def getBestTreeWithSupports(self):      # RAxML_bipartitions.<run>, RAxMLRunner.java:302-318
        return self.bestTreeWithSupports

    def getPerSiteLLs(self):
        return self.perSiteLLs


class FastTreeRunner:
    def __init__(self, ctx=None):
        self.ctx = ctx
        self.alignment = None
        self.result = None
        self.useRaxmlBranchLengths = False
        self.bootstrapReps = 0
        self.lnl = None
        self.constraints = None

    def setAlignment(self, a):
        self.alignment = a

    def getAlignment(self):
        return self.alignment

    def setConstraints(self, fasta_text):
        """FASTA text of 0/1/- rows, one column per constrained split (FastTreeRunner.java:220-222)."""
        self.constraints = fasta_text

    def setConstraintTree(self, treeString):
        """One column per node of the tree: 1 = leaf below the node (FastTreeRunner.java:224-229,243-273)."""
        if treeString is not None:
            names, rows = engine.constraints_from_tree(treeString)
            self.setConstraints("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, rows)))

    def _constraint_matrix(self):
        if self.constraints is None:
            return None
        names, rows = [], []
        for line in self.constraints.splitlines():
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:]); rows.append("")
            elif line and names:
                rows[-1] += line
        return names, rows

    def setUseRaxmlBranchLengths(self, b):
        self.useRaxmlBranchLengths = b

    def getUseRaxmlBranchLengths(self):
        return self.useRaxmlBranchLengths

    def setBootstrapReps(self, reps):
        self.bootstrapReps = reps

    def setRunName(self, n):
        self.runName = n

    def setThreadCount(self, n):
        pass

    def setNucleoide(self, nuc):
        if nuc:
            raise ValueError("nucleotide models are not on the GPU path")

    def run(self):
        """`FastTree_WAG -gamma [-nosupport]` (FastTreeRunner.java:67-86): NJ start + NNI hill climbing under WAG+Gamma, then
        FastTree's Gamma20 step -- the tree PEPR reads from stdout carries the lengths multiplied by the fitted rescale."""
        import re
        ctx = self.ctx or default_context()
        try:
            # FastTree_WAG carries the full-precision WAG frequencies, RAxML the 3-decimal ones
            gene = self.alignment.as_gene()
            r = ctx.search([gene], None, nni=True, spr_radius=0, pi_mode=engine.PI_WAG_FULL,
                           constraints=self._constraint_matrix())[0]
            g20 = ctx.gamma20([gene], [r["newick"]], pi_mode=engine.PI_WAG_FULL)[0]
            self.lnl, self.gamma20LogLk, self.gamma20Alpha, self.rescale = r["lnl"], g20["lnl"], g20["alpha"], g20["rescale"]
            self.result = g20["newick"]
            if self.bootstrapReps > 0 and len(self.alignment.getTaxa()) > 3:   # FastTreeRunner.java:67-70: no -nosupport -> SH-like supports
                s = ctx.sh_support([gene], [r["newick"]], alpha=r["alpha"], pi_mode=engine.PI_WAG_FULL)[0]
                self.result = re.sub(r":([0-9.eE+-]+)", lambda m: ":%.10f" % (float(m.group(1)) * g20["rescale"]), s["newick"])
        except Exception as e:
            log.error("FastTreeRunner failed: %s", e)
            self.result = None

    def getResult(self):
        return self.result


class NeighborJoiningRunner:
    """The reference's `nj` method (PhylogeneticTreeBuilder.buildNeighborJoiningTree, :198-208): BLOSUM62 pair scores of the
    alignment (SequenceAlignment.getPairwiseScores, on the device) and TreeBuilder.getNJTreeString on them -- the Java's
    doubles bit for bit.  An alignment with a byte outside the 24 codes, which the Java drops, is refused: the result stays
    None and the reason is logged, as for the other runners."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.alignment = None
        self.scoreMatrix = None           # None = BLOSUM62 as AlignmentUtilities.loadScoringMatrixFromResource leaves it
        self.result = None
        self.scores = None

    def setAlignment(self, a):
        self.alignment = a

    def getAlignment(self):
        return self.alignment

    def setScoreMatrix(self, m):
        """a 24 x 24 table of ints in [-128, 127] over the codes ARNDCQEGHILKMFPSTWYV, B, Z, X, gap; None = BLOSUM62 as loaded"""
        self.scoreMatrix = m

    def run(self):
        ctx = self.ctx or default_context()
        try:
            self.result = ctx.nj_tree(self.alignment.as_gene(), table=self.scoreMatrix, form=engine.NJ_TREE)
        except Exception as e:
            log.error("NeighborJoiningRunner failed: %s", e)
            self.result = None

    def getResult(self):
        return self.result


def buildConcatenatedNeighborJoiningTree(genes, ctx=None):
    """PhylogenomicPipeline2.buildConcatenatedNeighborJoiningTree (:1279-1293), the `-nj true` path: the concatenation's BLOSUM62
    pair scores (every gene scored once on the device, summed over the sorted taxon union) and TreeBuilder.getNJTopology on
    them -> "(x,y);" without lengths."""
    ctx = ctx or default_context()
    pairs = [g.as_gene() if hasattr(g, "as_gene") else g for g in genes]
    return ctx.nj_replicates(pairs, None, form=engine.NJ_TOPOLOGY)[0]


def filterForCongruence(genes, percentileToRemove=0.1, ctx=None):
    """PhylogenomicPipeline2.filterForCongruence (:429-511), the `-congruence_filter` step: the genes that stay in the
    concatenation, in input order.  Nothing is printed; Context.congruence_filter returns the costs behind the choice."""
    ctx = ctx or default_context()
    pairs = [g.as_gene() if hasattr(g, "as_gene") else g for g in genes]
    keep = ctx.congruence_filter(pairs, percentileToRemove)["keep"]
    return [g for g, k in zip(genes, keep) if k]


class MSATrimmer:
    """.../pepr/alignment/MSATrimmer.java's three column filters (:141-203, :205-253, :264-351) and its Gblocks step (trim, :41-126)
    on the device (Context.trim_columns, Context.gblocks_trim; the rules are in include/peprml.h).  Each returns a new
    SequenceAlignment with the same taxa.  The first two filters append "_ui" to the alignment's name (:197, :247: the Java
    concatenates, so a null name reads "null_ui"); the third sets none; trim appends "_trim" (:46).  trim applies the published
    block selection with PEPR's parameters; its parity with the Gblocks binary is unpinned (include/peprml.h)."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def _trim(self, alignment, mode, suffix):
        ctx = self.ctx or default_context()
        t = ctx.trim_columns([alignment.as_gene()], mode)[0]
        name = alignment.getName()
        return SequenceAlignment(alignment.getTaxa(), t["rows"], None if suffix is None else ("null" if name is None else name) + suffix)

    def trim(self, alignment):
        ctx = self.ctx or default_context()
        t = ctx.gblocks_trim([alignment.as_gene()])[0]
        name = alignment.getName()
        return SequenceAlignment(alignment.getTaxa(), t["rows"], ("null" if name is None else name) + "_trim")

    def trimUniformativeColumns(self, alignment):
        return self._trim(alignment, engine.TRIM_GAP_UNIFORM, "_ui")

    def trimUniformColumns(self, alignment):
        return self._trim(alignment, engine.TRIM_UNIFORM, "_ui")

    def trimTopologicallyUninformativeColumns(self, alignment):
        return self._trim(alignment, engine.TRIM_TOPOLOGICAL, None)


class NeighborMasher:
    """util/NeighborMasher.java with the Java's setter names: run() (:112-195) picks the ingroup's expansion and the outgroups from
    a pool and builds the two NJ trees, from MinHash sketches and Mash distances computed on the device (Context.neighbor_masher;
    the rule is in include/peprml.h and its parity with the mash binary is unpinned).  Genomes are given as (taxon name, records)
    instead of file names; tools/pepr_neighbor_masher.py reads the files.  The second tree is the unrooted NJ tree with the
    outgroup taxa first: rooting (:637-640) is not built.  digits = 6 feeds the selection and NJ the distance as the Java reads it
    from mash's text, None the double."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.mashKmerLength, self.mashSketchSize = 21, 100000        # :45, :49
        self.outgroupCount, self.expandedIngroupSize = 3, 0          # :53, :57
        self.ingroupOnly = self.outgroupOnly = False
        self.runName = None
        self.ingroup, self.pool = [], []
        self.digits = 6
        self.result = None

    def setMashKmerLength(self, k):
        self.mashKmerLength = int(k)

    def setMashSketchSize(self, s):
        self.mashSketchSize = int(s)

    def setOutgroupCount(self, n):
        self.outgroupCount = int(n)

    def setExpandedIngroupSize(self, n):
        self.expandedIngroupSize = int(n)

    def setIngroupTreeOnly(self, b):          # the Java's name for -ingroup_only (:873)
        self.ingroupOnly = bool(b)

    def setOutgroupOnly(self, b):
        self.outgroupOnly = bool(b)

    def setRunName(self, name):
        self.runName = name

    def getRunName(self):
        return self.runName

    def setIngroupGenomes(self, named_genomes):
        """[(taxon name, records)] in place of setIngroupGenomeFileNames"""
        self.ingroup = list(named_genomes)

    def setOutgroupGenomes(self, named_genomes):
        """[(taxon name, records)] in place of setOutgroupGenomeFileNames: the pool of candidates"""
        self.pool = list(named_genomes)

    def setDistanceDigits(self, digits):
        self.digits = digits

    def run(self):
        ctx = self.ctx or default_context()
        self.result = ctx.neighbor_masher(self.ingroup, self.pool, k=self.mashKmerLength, s=self.mashSketchSize, outgroup_count=self.outgroupCount,
                                          expand_ingroup=self.expandedIngroupSize, ingroup_only=self.ingroupOnly, outgroup_only=self.outgroupOnly,
                                          digits=self.digits)
        return self.result

    def getIngroupTaxa(self):
        return list(self.result["ingroup"])

    def getSelectedOutgroupTaxa(self):
        return list(self.result["outgroup"])

    def getIngroupTree(self):
        return self.result["ingroup_tree"]

    def getRootedTree(self):
        return self.result["rooted_tree"]


def readFastaRecords(path):
    """[(id token, [the record's lines])] of a FASTA file; the id token is FastaSequenceFile.getIDToken's (:192-204): the title up
    to its first blank, without the '>'"""
    out = []
    with open(path) as fh:
        for line in fh.read().split("\n"):
            if line.startswith(">"):
                sp = line.find(" ", 1)
                out.append((line[1:sp if sp >= 0 else len(line)], [line]))
            elif line and out:
                out[-1][1].append(line)
    return out


class HomologySearch:
    """BlastRunner (alignment/BlastRunner.java) for proteins, as PhyloPipeline.runBlast (:1061-1077) drives it: every protein of
    every genome file against every genome, the best subject per query and target genome, as an exhaustive Smith-Waterman search
    on the device (Context.sw_search; the rule, and that parity with blastall is unpinned, are in include/peprml.h).  Genome
    files are read as createConcatenatedSet reads them (:199-208): lines of length <= 1 are dropped.  run() computes,
    getResults() writes the combined table (result_file_name, else <run_name>_all_blast.out in out_dir, :427-478) and returns its path."""

    def __init__(self, genome_files, evalue=0.1, run_name="run", ctx=None, out_dir=".", traceback=False, result_file_name=None):
        self.genome_files, self.evalue, self.run_name, self.ctx = list(genome_files), float(evalue), run_name, ctx
        self.out_dir, self.traceback, self.result_file_name = out_dir, bool(traceback), result_file_name
        self.result, self.result_file = None, None

    @staticmethod
    def readGenome(path):
        """[(title without '>', residues)] in file order"""
        out = []
        with open(path) as fh:
            for line in fh.read().split("\n"):
                line = line.rstrip("\r")
                if len(line) <= 1:
                    continue
                if line.startswith(">"):
                    out.append([line[1:], []])
                elif out:
                    out[-1][1].append(line.strip())
        return [(t, "".join(r)) for t, r in out]

    def setEvalueCutoff(self, evalue):
        self.evalue = float(evalue)

    def setRunName(self, name):
        self.run_name = name

    def run(self):
        ctx = self.ctx or default_context()
        self.result = ctx.sw_search([self.readGenome(p) for p in self.genome_files], evalue=self.evalue, traceback=self.traceback)
        self.result_file = None
        return self.result

    def getResults(self):
        if self.result is None:
            self.run()
        if self.result_file is None:
            path = self.result_file_name or os.path.join(self.out_dir, self.run_name + "_all_blast.out")      # getResultFile :427-439
            with open(path, "wb") as fh:
                fh.write(self.result["table"])
            self.result_file = path
        return self.result_file


ALIGNMENT_FILE_SUFFIX = "_align"        # HandyConstants.ALIGNMENT_FILE_SUFFIX


class MultipleSequenceAligner:
    """.../pepr/alignment/MultipleSequenceAligner.java: getMSA (:90-141, `muscle -fasta -stable -quiet`) and getProfileMSA
    (:143-218, `muscle -profile -in1 -in2`) as the progressive profile alignment of include/peprml.h ("Multiple alignment") on the
    device (Context.msa_align, Context.msa_profile_align); parity with muscle is unpinned.  Sequences are (title, residues) pairs
    or a SequenceAlignment of unaligned rows; the result's rows are in input order (-stable) and it is named as the Java names
    it: the input's name + "_align" (a null name reads "null_align").  getMSAs aligns many sets in ONE batched call.  host=True
    runs the host twin (no device)."""

    def __init__(self, ctx=None, host=False, **opts):
        self.ctx, self.host, self.opts = ctx, bool(host), dict(opts)

    @staticmethod
    def _unpack(sequences):
        if isinstance(sequences, SequenceAlignment):
            return sequences.getTaxa(), list(sequences.rows), sequences.getName()
        return [t for t, _ in sequences], [r for _, r in sequences], getattr(sequences, "name", None)

    @staticmethod
    def _named(name):
        return ("null" if name is None else name) + ALIGNMENT_FILE_SUFFIX

    def getMSAs(self, list_of_sets, names=None):
        sets = [self._unpack(s) for s in list_of_sets]
        rows = [r for _, r, _ in sets]
        res = engine.msa_align_host(rows, **self.opts) if self.host else (self.ctx or default_context()).msa_align(rows, **self.opts)
        return [SequenceAlignment(taxa, r["rows"], self._named(names[k] if names else name)) for k, ((taxa, _, name), r) in enumerate(zip(sets, res))]

    def getMSA(self, sequences):
        return self.getMSAs([sequences])[0]

    def getProfileMSA(self, a, b):
        f = engine.msa_profile_align_host if self.host else (self.ctx or default_context()).msa_profile_align
        r = f(list(a.rows), list(b.rows), **self.opts)
        return SequenceAlignment(list(a.getTaxa()) + list(b.getTaxa()), r["rows"], self._named(a.getName()))


class HomologGroups:
    """PhyloPipeline.java:357-406 between the all-vs-all search and the trees: filterHitPairFile or filterForBidirectional,
    `mcl --abc -I inflation` (runMCL :882-909) and SequenceSetExtractor's set files, with the clustering on the device
    (Context.homolog_groups; the rule and what is pinned are in include/peprml.h).  run() writes <hits>_filtered or <hits>_bidir,
    <...>_mclOut and hg_<run>/set_<k>.faa for every line k of mcl's output, members in the line's order.  A sequence's taxon is
    the text of the last [...] of its title, or its file where the title has none; min_taxa .. target_min_gene are
    createInputSequenceSetProvider's parameters (PhylogenomicPipeline2.java:564-605) and decide getSelectedSetFiles()."""

    def __init__(self, hit_file, genome_files=(), ctx=None, run_name="run", out_dir=None, bidirectional=False, inflation=1.5, min_taxa=0,
                 max_taxa=2 ** 31 - 1, rep_only=False, target_ntax=0, target_min_gene=0):
        self.ctx, self.hit_file, self.genome_files = ctx, hit_file, list(genome_files)
        self.run_name, self.out_dir = run_name, out_dir if out_dir is not None else os.path.dirname(os.path.abspath(hit_file))
        self.bidirectional, self.inflation = bool(bidirectional), float(inflation)
        self.min_taxa, self.max_taxa, self.rep_only, self.target_ntax, self.target_min_gene = min_taxa, max_taxa, rep_only, target_ntax, target_min_gene
        self.result = None
        self.set_files = []

    def run(self):
        ctx = self.ctx or default_context()
        with open(self.hit_file, "rb") as fh:
            table = fh.read()
        records, taxon_names, taxon_of = {}, {}, {}
        for fi, path in enumerate(self.genome_files):
            for token, lines in readFastaRecords(path):
                records[token] = lines                                # SequenceSetExtractor.buildSequenceIndexMap :379-392: the last file wins
                title = lines[0]
                lb, rb = title.rfind("["), title.rfind("]")
                name = title[lb + 1:rb] if 0 <= lb < rb else "file %d" % fi
                taxon_of[token] = taxon_names.setdefault(name, len(taxon_names))
        r = ctx.homolog_groups(table, score_field=11, bidirectional=self.bidirectional, inflation=self.inflation, taxon_of=taxon_of or None,
                               min_taxa=self.min_taxa, max_taxa=self.max_taxa, rep_only=self.rep_only, target_ntax=self.target_ntax,
                               target_min_gene=self.target_min_gene)
        self.result = r
        filtered = self.hit_file + ("_bidir" if self.bidirectional else "_filtered")          # :919-920, :1002-1003
        with open(filtered, "w") as fh:
            fh.write(r["filtered_text"])
        self.mcl_file = filtered + "_mclOut"                                                    # :889
        with open(self.mcl_file, "w") as fh:
            fh.write(r["mcl_text"])
        hg = os.path.join(self.out_dir, "hg_" + self.run_name)                                  # :400-402
        os.makedirs(hg, exist_ok=True)
        self.set_files = []
        for k, cluster in enumerate(r["clusters"]):                                             # SequenceSetExtractor.processSequenceSets :158-198
            path = os.path.join(hg, "set_%d.faa" % k)
            with open(path, "w") as fh:
                for i in cluster:
                    for line in records.get(r["labels"][i], ()):
                        fh.write(line + "\n")
            self.set_files.append(path)
        return r

    def getSetFiles(self):
        return list(self.set_files)

    def getSelectedSetFiles(self):
        return [self.set_files[k] for k in self.result["kept"]]


class ConcatenatedSequenceAlignment:
    """.../pepr/alignment/ConcatenatedSequenceAlignment.java's gene homoplasy test (:65-425) on the device (Context.gene_steps,
    Context.step_thresholds; the rules are in include/peprml.h).  In the reference nothing ever calls setStepsPerSite
    (SequenceAlignment.java:1033), so these methods have no input there; here `tree`, the tree of the concatenation, supplies
    the per-site steps through the engine's Fitch pass.  Every method answers for one alignmentIndex as the Java does, but all
    genes are computed in one call and cached per option set.  The Java draws from an unseeded java.util.Random; here the
    draws are the library's own, a function of `seed`.  alignmentMask: one boolean per gene."""

    def __init__(self, genes, tree, ctx=None, seed=0):
        self.genes = [g.as_gene() if hasattr(g, "as_gene") else g for g in genes]
        self.tree, self.ctx, self.seed = tree, ctx, seed
        self._steps, self._thresholds = None, {}

    def _result(self):
        if self._steps is None:
            self._steps = (self.ctx or default_context()).gene_steps(self.genes, self.tree)
        return self._steps

    def getStepsPerSite(self):
        return self._result()["steps"]

    def getMinimumStepsPerSite(self):
        return self._result()["min_steps"]

    def getStepsForAlignment(self, alignmentIndex):
        return int(self._result()["gene_steps"][alignmentIndex])

    def getTotalStepsBeyondMinimumForAlignment(self, alignmentIndex):
        return int(self._result()["gene_beyond"][alignmentIndex])

    def getTotalStepsToMinimumRatioForAlignment(self, alignmentIndex):
        return float(self._result()["gene_ratio"][alignmentIndex])

    def _threshold(self, alignmentIndex, statistic, replace, multiple, reps, alpha, mask):
        key = (statistic, replace, multiple, int(reps), float(alpha), None if mask is None else tuple(bool(m) for m in mask))
        if key not in self._thresholds:
            ctx = self.ctx or default_context()
            self._thresholds[key] = ctx.step_thresholds(self._result(), statistic, replace, multiple, reps, alpha, self.seed, mask)
        return self._thresholds[key]["threshold"][alignmentIndex]

    def getThresholdStepsForAlignment(self, alignmentIndex, reps, alpha):
        return int(self._threshold(alignmentIndex, engine.STEPS_RAW, False, 0, reps, alpha, None))

    def getThresholdStepsBeyondMinimumForAlignment(self, alignmentIndex, reps, alpha, alignmentMask=None):
        """without a mask :178-213 (no replacement); with one :240-307, the current rule (replacement, multiple 3)"""
        if alignmentMask is None:
            return int(self._threshold(alignmentIndex, engine.STEPS_BEYOND_MIN, False, 0, reps, alpha, None))
        return int(self._threshold(alignmentIndex, engine.STEPS_BEYOND_MIN, True, 3, reps, alpha, alignmentMask))

    def getThresholdStepsBeyondMinimumForAlignmentOLD(self, alignmentIndex, reps, alpha, alignmentMask):
        return int(self._threshold(alignmentIndex, engine.STEPS_BEYOND_MIN, False, 2, reps, alpha, alignmentMask))

    def getThresholdStepsToMinimumRatioForAlignment(self, alignmentIndex, reps, alpha, alignmentMask):
        return float(self._threshold(alignmentIndex, engine.STEPS_MIN_RATIO, False, 2, reps, alpha, alignmentMask))


class TreeComparison:
    """.../pepr/tree/TreeComparison.java:812-885 runConsel: `raxmlHPC -f g` on the trees, then `makermt -b 10 --puzzle`, `consel`
    and `catpv -v` on its per-site lnL -- here one engine call (pml_tree_tests, or pml_tree_tests_weighted).  weighted=True returns
    the whole table of `catpv -v`, the weighted tests wKH / wSH after sh; the default leaves the two columns out, as ever."""

    REPS = 100000          # makermt's 10 000 replicates per scale times the -b 10 of the reference's command line

    def __init__(self, ctx=None, reps=None, seed=0, weighted=False):
        self.ctx, self.reps, self.seed, self.weighted = ctx, reps or self.REPS, seed, weighted
        self.result = None

    def runConsel(self, alignment, trees, processors=None, matrix="PROTGAMMAWAG"):
        """alignment: SequenceAlignment; trees: Newick strings; processors is accepted and ignored; matrix is resolved as
        RAxMLRunner resolves it (an unbuilt model name raises before anything touches a device).
        -> the lines of a `catpv -v`-shaped table, one row per tree sorted by rank (item = 1-based index into trees):
           # rank item obs au np | bp pp kh sh |            or, weighted (the lines of pml_catpv_table),
           # rank item obs au np | bp pp kh sh wkh wsh |"""
        mdl = _model_from_matrix(matrix, self.ctx)
        ctx = self.ctx or default_context()
        r = ctx.tree_tests(alignment.as_gene(), [str(t) for t in trees], reps=self.reps, seed=self.seed, weighted=self.weighted, **mdl)
        self.result = r
        lines = ["# reading per-site lnL of %d trees x %d sites, %d scales x %d replicates" % (r["ntrees"], r["nsites"], r["nscales"], r["reps"])]
        if self.weighted:
            return lines + engine.catpv_table(r)
        lines.append("# %4s %4s %8s %6s %6s | %6s %6s %6s %6s |" % ("rank", "item", "obs", "au", "np", "bp", "pp", "kh", "sh"))
        for t in sorted(range(r["ntrees"]), key=lambda i: r["rank"][i]):
            lines.append("# %4d %4d %8.1f %6.3f %6.3f | %6.3f %6.3f %6.3f %6.3f |" % (
                r["rank"][t], t + 1, r["obs"][t], r["au"][t], r["np"][t], r["bp"][t], r["pp"][t], r["kh"][t], r["sh"][t]))
        return lines


# ---- TreeComparison's -rf / -tree_dist legs: every value comes from one pml_tree_compare call on the device ----
def compareAllvsAll(trees, ctx=None, useLengths=True):
    """TreeComparison.compareAllvsAll(TreeI[]) (:267-288) on Newick strings over one leaf set -> the dict of Context.tree_compare:
    rf_legacy is the int[][] the Java returns, branch_dist / discrepant_dist the two values it prints per pair"""
    return (ctx or default_context()).tree_compare(list(trees), use_lengths=useLengths)


def compareSlidingWindow(trees, windowSize, ctx=None):
    """TreeComparison.compareSlidingWindow (:241-265): for i >= windowSize the legacy RF of tree i against each of the windowSize
    trees before it -> [(i, [(j, distance), ...], min, max, mean)] as the Java prints them (mean = sum / count in doubles)"""
    rf = (ctx or default_context()).tree_compare(list(trees), window=windowSize, want=["rf_legacy"])["rf_legacy"]
    out = []
    for i in range(windowSize, len(trees)):
        d = [(j, int(rf[i, j])) for j in range(i - windowSize, i)]
        v = [x for _, x in d]
        out.append((i, d, min(v), max(v), float(sum(v)) / len(v)))
    return out


def rollingComparison(trees, ctx=None):
    """TreeComparison.rollingComparison (:457-466): r[i] = legacy RF between trees i + 1 and i"""
    rf = (ctx or default_context()).tree_compare(list(trees), window=1, want=["rf_legacy"])["rf_legacy"]
    return [int(rf[i + 1, i]) for i in range(len(trees) - 1)]


def getBranchDistance(tree1, tree2, ctx=None, useLengths=True):
    """TreeComparison.getBranchDistance (:607-747) of two Newick strings; tree1 is the Java's tree1"""
    return float((ctx or default_context()).tree_compare_one(tree1, [tree2], use_lengths=useLengths, want=["branch_dist"])["branch_dist"][0])


def getDiscrepantBranchDistance(tree1, tree2, ctx=None, useLengths=True):
    """TreeComparison.getDiscrepantBranchDistance (:756-810)"""
    return float((ctx or default_context()).tree_compare_one(tree1, [tree2], use_lengths=useLengths, want=["discrepant_dist"])["discrepant_dist"][0])


def compressTaxonNameForComparison(name):
    """TreeUtils.compressTaxonNameForComparison (TreeUtils.java:48-73)"""
    import re
    r = name
    if re.fullmatch(r".*\.f.+", r, re.S):
        r = r[:r.rindex(".")]
    if r.endswith(".PATRIC"):
        r = r[:r.rindex(".")]
    return re.sub(r"[\._,\s]", "", r).lower()


class BasicTree:
    """The part of BasicTree that TreeComparison's pruning uses, for well-formed Newick text: the node arrays of
    parseNewickTreeString (BasicTree.java:131-409: leaves in text order, then inner nodes in the order of their ')'; a branch
    without a length has length 0.0; the text between ')' and ':' is the node's support string), populateChildPointers
    (:411-448: children in ascending node index), removeTaxon (:888-946) and getTreeString (:450-520)."""
    NO_PARENT = -1

    def __init__(self, treeString):
        s = treeString.strip()
        if s.endswith(";"):
            s = s[:-1]
        self.leaves, inner = [], []            # inner: (children as ("l" | "i", index), length, support), in the order of ')'
        leaf_len = []
        pos = 0

        def sub():
            nonlocal pos
            kids = []
            if s[pos] == "(":
                pos += 1
                while True:
                    kids.append(sub())
                    if s[pos] == ",":
                        pos += 1
                        continue
                    if s[pos] == ")":
                        pos += 1
                        break
                    raise ValueError("expected , or ) at %d" % pos)
            b = pos
            while pos < len(s) and s[pos] not in ",():":
                pos += 1
            label = s[b:pos]
            length = 0.0
            if pos < len(s) and s[pos] == ":":
                pos += 1
                b = pos
                while pos < len(s) and s[pos] not in ",()":
                    pos += 1
                length = float(s[b:pos])
            if kids:
                inner.append((kids, length, label or None))
                return ("i", len(inner) - 1)
            self.leaves.append(label)
            leaf_len.append(length)
            return ("l", len(self.leaves) - 1)

        sub()
        if pos != len(s):
            raise ValueError("text after the tree at %d" % pos)
        nl = len(self.leaves)
        n = nl + len(inner)
        self.nodeStrings = list(self.leaves) + [None] * len(inner)
        self.parent = [self.NO_PARENT] * n
        self.branchLengths = leaf_len + [x[1] for x in inner]
        self.branchSupports = [None] * nl + [x[2] for x in inner]
        for k, (kids, _, _) in enumerate(inner):
            for kind, idx in kids:
                self.parent[idx if kind == "l" else nl + idx] = nl + k
        self.children = [[c for c in range(n) if self.parent[c] == v] for v in range(n)]      # ascending index (:438-447)

    def getLeaves(self):
        """the leaves still in the tree, in node order"""
        top = self.getTopLevelNode()
        out = []

        def walk(v):
            if not self.children[v]:
                out.append(self.nodeStrings[v])
            for c in self.children[v]:
                walk(c)
        if top >= 0:
            walk(top)
        return out

    def removeTaxon(self, taxon):
        idx = -1
        for i, leaf in enumerate(self.leaves):                                  # :891-895: the LAST match
            if taxon.lower() == leaf.lower() or compressTaxonNameForComparison(taxon) == compressTaxonNameForComparison(leaf):
                idx = i
        if idx < 0 or self.parent[idx] == self.NO_PARENT:                       # :897-903
            return
        parent = self.parent[idx]
        self.children[parent].remove(idx)                                       # removeChildNode :815-829
        self.parent[idx] = self.NO_PARENT
        if len(self.children[parent]) == 1:                                     # :910-935
            rest = self.children[parent][0]
            if self.parent[parent] == self.NO_PARENT:
                self.parent[rest] = self.NO_PARENT
                self.children[parent] = []
            else:
                grand = self.parent[parent]
                self.branchLengths[rest] += self.branchLengths[parent]
                self.children[grand][self.children[grand].index(parent)] = rest
                self.parent[rest] = grand

    def getTopLevelNode(self):
        r = -1
        for i in range(len(self.parent)):                                       # :466-472: the last node without a parent that has children
            if self.parent[i] == self.NO_PARENT and self.children[i]:
                r = i
        return r

    def getTreeString(self, includeLengths=True, includeSupports=True):
        top = self.getTopLevelNode()
        if top < 0:
            return None

        def node(v):                                                            # getNodeString :480-520
            kids = self.children[v]
            if not kids:
                return self.nodeStrings[v]
            parts = []
            for c in kids:
                parts.append(node(c) + (":" + engine.format_double(self.branchLengths[c]) if includeLengths else ""))
            r = ",".join(parts)
            if len(kids) > 1:
                r = "(" + r + ")"
            if includeSupports and self.branchSupports[v] is not None:
                r += self.branchSupports[v]
            return r
        return node(top) + ";"


def pruneToCommonTaxa(treeStrings, outgroupTaxa=(), useLengths=True):
    """What TreeComparison.main does to its trees before it compares them: every outgroup taxon (sorted, :88) is removed from
    every tree (:89-96), then every taxon that is not in all trees (:101-127); after each removal the tree is rebuilt from its
    own text, as the Java rebuilds it (:94, :124) -> (the pruned Newick strings, [(tree index, removed taxon)])"""
    trees = [BasicTree(t) for t in treeStrings]
    removed = []
    for taxon in sorted(outgroupTaxa):
        for j in range(len(trees)):
            trees[j].removeTaxon(taxon)
            trees[j] = BasicTree(trees[j].getTreeString(useLengths, True))
    common = set(trees[0].getLeaves()) if trees else set()
    for t in trees[1:]:
        common &= set(t.getLeaves())
    for i in range(len(trees)):
        for taxon in trees[i].getLeaves():                                      # :118: the leaves before any removal
            if taxon not in common:
                removed.append((i, taxon))
                trees[i].removeTaxon(taxon)
                trees[i] = BasicTree(trees[i].getTreeString(useLengths, True))
    return [t.getTreeString(useLengths, True) for t in trees], removed


class PhylogeneticTreeBuilder:
    def __init__(self, ctx=None):
        self.ctx = ctx
        self.alignment = None
        self.treeBuildingMethod = ML
        self.mlMatrix = "PROTGAMMAWAG"
        self.treeString = None
        self.processes = 1
        self.bootstrapReps = 0
        self.runName = None
        self._useRaxmlBL = False
        self.constraintTree = None

    def setAlignment(self, a):
        self.alignment = a

    def getAlignment(self):
        return self.alignment

    def setTreeBuildingMethod(self, m):
        self.treeBuildingMethod = m

    def setMLMatrix(self, m):
        self.mlMatrix = m

    def setProcesses(self, n):
        self.processes = n

    def setBootstrapReps(self, reps):
        self.bootstrapReps = reps

    def getBootstrapReps(self):
        return self.bootstrapReps

    def setRunName(self, n):
        self.runName = n

    def getRunName(self):
        return self.runName

    def useRaxmlBranchLengths(self, b):
        self._useRaxmlBL = b

    def setConstraintTree(self, t):
        self.constraintTree = t

    def setNucleotide(self, nuc):
        if nuc:
            raise ValueError("nucleotide models are not on the GPU path")

    def setTreeString(self, s):
        self.treeString = s

    def getTreeString(self):
        return self.treeString

    def run(self):
        if self.treeBuildingMethod == ML:
            r = RAxMLRunner(self.processes, self.ctx)
            r.setBootstrapReps(self.bootstrapReps); r.setAlignment(self.alignment); r.setMatrix(self.mlMatrix)
            r.run()
            self.setTreeString(r.getBestTree() if self.bootstrapReps == 0 else r.getBestTreeWithSupports())
        elif self.treeBuildingMethod in (PARSIMONY, PARSIMONY_BL):        # PhylogeneticTreeBuilder.java:136-161
            r = RAxMLRunner(self.processes, self.ctx)
            if self.treeBuildingMethod == PARSIMONY:
                r.setParsimonyOnly(True)
            else:
                r.setParsimonyWithBL(True)
            r.setBootstrapReps(self.bootstrapReps); r.setAlignment(self.alignment)
            r.run()
            self.setTreeString(r.getParsimonyTree() if self.treeBuildingMethod == PARSIMONY else r.getParsimonyWithBLTree())
        elif self.treeBuildingMethod == FAST_TREE:
            f = FastTreeRunner(self.ctx)
            f.setAlignment(self.alignment); f.setRunName(self.runName); f.setBootstrapReps(self.bootstrapReps)
            f.setUseRaxmlBranchLengths(self._useRaxmlBL)
            if self.constraintTree is not None:             # PhylogeneticTreeBuilder.java:190-192
                f.setConstraintTree(self.constraintTree)
            f.run()
            self.setTreeString(f.getResult())
        else:
            # NEIGHBOR_JOINING is built (NeighborJoiningRunner, buildConcatenatedNeighborJoiningTree, and both tree methods of
            # buildConcatenatedTreeWithGeneWiseJackKnifeSupport), but this dispatch keeps refusing it: callers and the mirror test
            # (tests/test_tree_builder_mirror.py::test_dispatch_and_errors_cpu) rely on the refusal, so it is not changed here
            raise ValueError("tree building method %r is outside the GPU path (ml, FastTree, parsimony, parsimony_bl)" % self.treeBuildingMethod)


def buildConcatenatedTree(genes, bootstraps=100, concatenatedTreeMethod=ML, mlMatrix="PROTGAMMAWAG", ctx=None, seed=1, details=False):
    """PhylogenomicPipeline2.buildConcatenatedTree (:836-890; reached from :395-402 with `-concatenated true` and no
    `-gene_wise_jackknife`, bootstraps = support_reps, default 100) as one engine call (pml_bootstrap2): the tree of the
    concatenation of `genes` under "ml" (`-f a -x -N`), "parsimony" or "parsimony_bl" (`-Y -N`), with the column bootstrap's
    percent supports when bootstraps > 0.  The genes are encoded once and every replicate is built on the device.  "FastTree"
    and "nj" are refused: their bootstraps are not built.  -> the tree string (the reference's return value), or with details
    the dict of Context.bootstrap2."""
    if concatenatedTreeMethod in (FAST_TREE, NEIGHBOR_JOINING):
        raise ValueError("concatenated tree method %r has no bootstrap on the GPU path (ml, parsimony, parsimony_bl)" % concatenatedTreeMethod)
    if concatenatedTreeMethod not in (ML, PARSIMONY, PARSIMONY_BL):
        raise ValueError("concatenated tree method %r is not built here (ml, parsimony, parsimony_bl)" % concatenatedTreeMethod)
    mdl = _model_from_matrix(mlMatrix, ctx)                         # an unbuilt model name is refused before any device work
    ctx = ctx or default_context()
    pairs = [g.as_gene() if hasattr(g, "as_gene") else g for g in genes]
    methods = {ML: engine.TREE_ML, PARSIMONY: engine.TREE_PARSIMONY, PARSIMONY_BL: engine.TREE_PARSIMONY_BL}
    r = ctx.bootstrap2(pairs, reps=int(bootstraps), seed=seed, method=methods[concatenatedTreeMethod], spr_radius=5, parsimony_radius=20,
                       pi_mode=mdl["pi_mode"], ncat=mdl["ncat"])
    return r if details else r["newick"]


def buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, reps=100, supportTreeMethod=FAST_TREE, mlMatrix="PROTGAMMAWAG",
                                                      ctx=None, seed=1, support_rule=engine.SUPPORT_DECORATOR, fullTreeMethod=ML):
    """PhylogenomicPipeline2.java:994-1126 as one engine call (pml_jackknife2).  genes: SequenceAlignments (or (taxa, rows)
    pairs) of the single-copy families.  mlMatrix goes to the full tree (buildConcatenatedTree, :855-858) and, when the
    support trees are ML trees too, to every gene-subset tree (GeneSubsetTreeRunnable.setMatrix, :1247, :1619-1620);
    FastTree support trees (the default method, :335-338) stay WAG with FastTree_WAG's frequencies.  The supports are what
    TreeSupportDecorator.addSupportValues counts on the returned support trees unless another rule is asked for.
    supportTreeMethod "nj" (`-support_tree_method nj`): the full tree is built as ever, the support trees are NJ trees
    (pml_nj_replicates) of the very gene subsets the seeded draw gives the other methods, and the supports are counted under
    support_rule.  fullTreeMethod "nj" (`-full_tree_method nj`, with "nj" support trees): the whole loop is pml_nj_jackknife,
    and "newick" is the NJ tree's own text with the counts behind its inner nodes; with ML or FastTree support trees it is
    refused (that loop would search a full ML tree only to drop it).
    supportTreeMethod "parsimony" and fullTreeMethod "parsimony" / "parsimony_bl" (`raxmlHPC -y`, and `-y` then `-f e -t`,
    PhylogeneticTreeBuilder.java:104-115,136-161) go through pml_jackknife3: parsimony trees of the genes resident in HBM,
    topology only (RAxML's radius 20); "parsimony_bl" optimises the full tree's lengths and alpha under mlMatrix.  A
    "parsimony_bl" support tree is refused (nothing reads a support tree's lengths), as is a "FastTree" full tree (its Gamma20
    rescale is not built into the loop).  These calls also return "mp_lengths" (Context.jackknife3).
    -> the dict of Context.jackknife2: "newick" carries the supports, "support_trees" the replicate trees (the NJ loop
    returns these two keys alone: an NJ tree has no likelihood)."""
    if supportTreeMethod == PARSIMONY_BL:
        raise ValueError("support tree method 'parsimony_bl' is not built: nothing reads a support tree's branch lengths (use 'parsimony')")
    if supportTreeMethod not in (ML, FAST_TREE, PARSIMONY, NEIGHBOR_JOINING):
        raise ValueError("support tree method %r is outside the GPU path (ml, FastTree, parsimony, nj)" % supportTreeMethod)
    if fullTreeMethod not in (ML, PARSIMONY, PARSIMONY_BL, NEIGHBOR_JOINING):
        raise ValueError("full tree method %r is not built here (ml, parsimony, parsimony_bl, nj)" % fullTreeMethod)
    if fullTreeMethod == NEIGHBOR_JOINING and supportTreeMethod != NEIGHBOR_JOINING:
        raise ValueError("an nj full tree takes nj support trees (support tree method %r would search a full ML tree to drop it)" % supportTreeMethod)
    if fullTreeMethod in (PARSIMONY, PARSIMONY_BL) and supportTreeMethod == NEIGHBOR_JOINING:
        raise ValueError("nj support trees under a %s full tree are not built (nj support trees take an ml or nj full tree)" % fullTreeMethod)
    full = _model_from_matrix(mlMatrix, ctx)                        # an unbuilt model name is refused before any device work
    support_pi = full["pi_mode"] if supportTreeMethod == ML else engine.PI_WAG_FULL
    ctx = ctx or default_context()
    pairs = [g.as_gene() if hasattr(g, "as_gene") else g for g in genes]
    if fullTreeMethod == NEIGHBOR_JOINING:
        return ctx.nj_jackknife(pairs, reps=reps, seed=seed, support_rule=support_rule)
    if supportTreeMethod == NEIGHBOR_JOINING:
        r = ctx.jackknife2(pairs, reps=0, seed=seed, spr_radius_full=5, pi_mode=full["pi_mode"], ncat=full["ncat"], support_rule=support_rule)
        sel = engine.jackknife_draw(len(pairs), reps, 0, seed)
        r["support_trees"] = ctx.nj_replicates(pairs, sel, form=engine.NJ_TREE) if reps > 0 else []
        r["newick"] = engine.support_tree_rule(r["newick"], r["support_trees"], support_rule)
        return r
    if PARSIMONY in (supportTreeMethod, fullTreeMethod) or fullTreeMethod == PARSIMONY_BL:
        methods = {ML: engine.TREE_ML, FAST_TREE: engine.TREE_ML, PARSIMONY: engine.TREE_PARSIMONY, PARSIMONY_BL: engine.TREE_PARSIMONY_BL}
        return ctx.jackknife3(pairs, reps=reps, seed=seed, spr_radius_full=5, pi_mode=full["pi_mode"], ncat=full["ncat"],
                              support_pi_mode=support_pi, support_rule=support_rule, full_method=methods[fullTreeMethod],
                              support_method=methods[supportTreeMethod], parsimony_radius=20)
    return ctx.jackknife2(pairs, reps=reps, seed=seed, spr_radius_full=5, pi_mode=full["pi_mode"], ncat=full["ncat"],
                          support_pi_mode=support_pi, support_rule=support_rule)
