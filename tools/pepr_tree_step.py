#!/usr/bin/env python
"""PEPR's tree-building step as one command on the GPU engine.

Reads a directory of per-gene protein alignments (FASTA, one file per single-copy family, titles =
taxon names, as PhylogenomicPipeline2 holds them after muscle+Gblocks) and writes what
buildConcatenatedTreeWithGeneWiseJackKnifeSupport writes (PhylogenomicPipeline2.java:994-1126):
    <run>.nwk   full ML tree of the concatenation with integer jackknife supports as node labels
    <run>.sup   the support trees, one Newick per line
usage: pepr_tree_step.py -run_name X -alignment_dir DIR [-support_reps 100] [-seed 1] [-device 0]
                         [--matrix NAME] [--support-matrix NAME] [--support-rule N]
                         [--full-tree-method ml|parsimony|parsimony_bl|nj] [--support-tree-method ml|FastTree|parsimony|nj]
                         [-gblocks_trim] [-uniform_trim] [-congruence_filter] [-trim_percent 0.1] [-gene_steps [REPS ALPHA]] [-concatenated]
(flag style and names follow .../util/HandyConstants.java: run_name, support_reps)
--matrix          RAxML model name of the full tree (what -matrix_eval chose; PROTGAMMAWAG, PROTGAMMAWAGF, PROTGAMMAGTR or
                  PROTGAMMA<NAME>[F] from <name>.dat in $PEPRML_MODEL_DIR, resolved as the raxmlHPC shim resolves -m)
--support-matrix  the same for the support trees (default: the full tree's; FastTree supports are PROTGAMMAWAG)
--support-rule    0 = only replicates over the full taxon set count, 1 = TreeSupportDecorator.addSupportValues on the support
                  trees as written to <run>.sup, 2 = main split restricted to the replicate's taxa (include/peprml.h)
--full-tree-method, --support-tree-method   PEPR's -full_tree_method / -support_tree_method; the value nj builds the trees by
                  neighbor joining on BLOSUM62 pair scores, as the reference's TreeBuilder does (supports under --support-rule,
                  default 1); nj for the full tree takes nj support trees (the default support method then); --support-matrix is
                  refused with these two flags (ml support trees use --matrix, FastTree ones are WAG, nj has no model).
                  The value parsimony builds the trees by maximum parsimony (`raxmlHPC -y`: stepwise addition + SPR radius 20)
                  from the genes resident on the device; they are written topology only, so a parsimony full tree has supports
                  but no lengths and no likelihood.  parsimony_bl (full tree only) then optimises branch lengths and alpha under
                  --matrix (`-f e -t`).  parsimony_bl support trees and a FastTree full tree are refused
-congruence_filter, -trim_percent P   PEPR's flags of the same names (HandyConstants.java:86, :92): before any tree is built the
                  genes are filtered as PhylogenomicPipeline2.filterForCongruence filters them (column bipartition costs, the
                  genes of the highest mean cost go; P of 1.0 or more is a percentage).  Prints the reference's two messages and
                  writes <run>.congruence.tsv: file, columns, cost_sum, mean_cost, kept -- one row per gene
-uniform_trim     PEPR's flag of the same name (HandyConstants.java:26): every gene goes through MSATrimmer.trimUniformColumns first,
                  as getAlignment (PhylogenomicPipeline2.java:788-795) precedes filterForCongruence; the rule is in
                  include/peprml.h (PML_TRIM_UNIFORM).  Writes <run>.trim.tsv: file, columns, kept -- one row per gene; a gene trimmed
                  to 0 columns is dropped with a message.  With -congruence_filter the genes are uploaded once and trimmed and
                  filtered in one call (pml_trim_congruence_filter)
-gblocks_trim     PEPR's flag of the same name (the default track sets it, PhyloPipeline.java:1121): every gene goes through the block
                  selection of MSATrimmer.trim (Gblocks -b1=ceil(0.8 n) -b3=8 -b5=h) first, before -uniform_trim and
                  -congruence_filter, as PhylogenomicPipeline2.getAlignment orders them.  The rule is the published one, residues
                  counted by identity; its parity with the Gblocks binary is unpinned (include/peprml.h pml_gblocks_trim).  Writes
                  <run>.gblocks.tsv: file, columns, kept -- one row per gene; a gene trimmed to 0 columns is dropped with a message.
                  With -uniform_trim and / or -congruence_filter the genes are uploaded once and all stages run in one call
                  (pml_trim_pipeline)
-gene_steps [REPS ALPHA]   the gene homoplasy test of ConcatenatedSequenceAlignment.java (include/peprml.h pml_gene_steps) on the full
                  tree just built: per gene the Fitch steps of its columns, the steps beyond the minimum, the steps-to-minimum
                  ratio, and the threshold of the Java's current rule (steps beyond the minimum, REPS samples with replacement from
                  the other genes' columns, the ceil(REPS * ALPHA)-th largest; -1 when the others hold fewer than three times the
                  gene's columns) with n_ge, the samples at or above the gene's own total.  Defaults 1000 and 0.05; the draws take
                  -seed.  Writes <run>.steps.tsv: gene, columns, steps, beyond, ratio, threshold, n_ge -- one row per gene
-concatenated     PEPR's `-concatenated true` without -gene_wise_jackknife (PhylogenomicPipeline2.java:395-402, buildConcatenatedTree
                  :836-890): ONE tree of the concatenation under --full-tree-method ml | parsimony | parsimony_bl and --matrix, with
                  the column bootstrap's percent supports from -support_reps replicates (`-f a -x -N`, `-Y -N`; include/peprml.h
                  pml_bootstrap2).  The genes are encoded once; every replicate is built on the device.  <run>.sup holds the
                  replicate trees.  FastTree and nj are refused
Without these flags the step runs as it always did (pml_jackknife: PROTGAMMAWAG, rule 0).
"""
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine


def read_fasta(path):
    names, rows = [], []
    for line in open(path):
        line = line.strip()
        if not line:
            continue
        if line.startswith(">"):
            names.append(line[1:].split()[0]); rows.append([])
        else:
            rows[-1].append(line)
    return names, ["".join(r) for r in rows]


def main(argv):
    args = {}
    gene_steps_vals = None
    i = 0
    while i < len(argv):                       # CommandLineProperties style: -flag value
        if argv[i].startswith("-"):
            key = argv[i].lstrip("-").replace("-", "_"); vals = []
            i += 1
            while i < len(argv) and not argv[i].startswith("-"):
                vals.append(argv[i]); i += 1
            args[key] = vals[0] if vals else "true"
            if key == "gene_steps":
                gene_steps_vals = vals
        else:
            i += 1
    if "run_name" not in args or "alignment_dir" not in args:
        raise SystemExit(__doc__)
    files = sorted(glob.glob(os.path.join(args["alignment_dir"], "*")))
    files = [f for f in files if os.path.isfile(f)]
    genes = [read_fasta(f) for f in files]
    files = [f for f, g in zip(files, genes) if len(g[0]) >= 3]
    genes = [g for g in genes if len(g[0]) >= 3]
    reps = int(args.get("support_reps", 100))
    ctx = engine.Context(int(args.get("device", 0)))
    filtering = args.get("congruence_filter", "false").lower() == "true"
    r = None
    uniform = args.get("uniform_trim", "false").lower() == "true"
    trimmed = None
    if args.get("gblocks_trim", "false").lower() == "true":
        staged = None
        if uniform or filtering:                # one upload: every stage reads the matrices the stage before left in HBM
            try:
                staged = ctx.trim_pipeline(genes, True, None, engine.TRIM_UNIFORM if uniform else None, float(args.get("trim_percent", 0.1)) if filtering else 0)
            except engine.PmlError as e:        # a gene trimmed to nothing: it is dropped below and the steps run one after the other
                if e.code != -2 or "no columns left" not in str(e):
                    raise
        blocks = staged["gblocks"] if staged else ctx.gblocks_trim(genes)
        with open(args["run_name"] + ".gblocks.tsv", "w") as f:
            f.write("file\tcolumns\tkept\n")
            for name, t in zip(files, blocks):
                f.write("%s\t%d\t%d\n" % (os.path.basename(name), t["ncols"], t["nkept"]))
                if not t["nkept"]:
                    print("dropping set %s: no column left after -gblocks_trim" % os.path.basename(name))
        files = [f for f, t in zip(files, blocks) if t["nkept"]]
        genes = [(t["names"], t["rows"]) for t in blocks if t["nkept"]]
        if staged:
            trimmed = staged.get("trimmed")
            r = staged if filtering else None
    if uniform:
        if filtering and trimmed is None:       # one upload: trimmed in HBM, the congruence stage runs on the trimmed matrices
            try:
                r = ctx.trim_congruence_filter(genes, engine.TRIM_UNIFORM, float(args.get("trim_percent", 0.1)))
                trimmed = r["trimmed"]
            except engine.PmlError as e:        # a gene trimmed to nothing: it is dropped below and the two steps run one after the other
                if e.code != -2 or "no columns left" not in str(e):
                    raise
        if trimmed is None:
            trimmed = ctx.trim_columns(genes, engine.TRIM_UNIFORM)
        with open(args["run_name"] + ".trim.tsv", "w") as f:
            f.write("file\tcolumns\tkept\n")
            for name, t in zip(files, trimmed):
                f.write("%s\t%d\t%d\n" % (os.path.basename(name), t["ncols"], t["nkept"]))
                if not t["nkept"]:
                    print("dropping set %s: no column left after -uniform_trim" % os.path.basename(name))
        files = [f for f, t in zip(files, trimmed) if t["nkept"]]
        genes = [(t["names"], t["rows"]) for t in trimmed if t["nkept"]]
    if filtering:
        if r is None:
            r = ctx.congruence_filter(genes, float(args.get("trim_percent", 0.1)))
        with open(args["run_name"] + ".congruence.tsv", "w") as f:
            f.write("file\tcolumns\tcost_sum\tmean_cost\tkept\n")
            for name, g, cs, mc, k in zip(files, genes, r["cost_sum"], r["mean_cost"], r["keep"]):
                f.write("%s\t%d\t%d\t%d\t%d\n" % (os.path.basename(name), len(g[1][0]), cs, mc, int(k)))
                if not k:
                    print("discarding set %s cost: %d" % (os.path.basename(name), mc))
        genes = [g for g, k in zip(genes, r["keep"]) if k]
        print("Discarded: %d\tKept: %d" % (len(files) - len(genes), len(genes)))
        files = [f for f, k in zip(files, r["keep"]) if k]
    t0 = time.time()
    if args.get("concatenated", "false").lower() == "true":
        from pepr_amd import tree_builder
        if {"support_tree_method", "support_matrix", "support_rule"} & set(args):
            raise SystemExit("-concatenated builds one tree with column-bootstrap supports: --support-tree-method, --support-matrix and "
                             "--support-rule belong to the gene-wise jackknife")
        r = tree_builder.buildConcatenatedTree(genes, reps, args.get("full_tree_method", tree_builder.ML), args.get("matrix", "PROTGAMMAWAG"),
                                               ctx=ctx, seed=int(args.get("seed", 1)), details=True)
        r["support_trees"] = r["replicates"]
    elif {"full_tree_method", "support_tree_method"} & set(args):
        from pepr_amd import tree_builder
        if "support_matrix" in args:
            raise SystemExit("--support-matrix does not go with --full-tree-method / --support-tree-method: ml support trees take --matrix, "
                             "FastTree support trees are WAG, nj trees have no model")
        full_method = args.get("full_tree_method", tree_builder.ML)
        r = tree_builder.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(
            genes, reps=reps, supportTreeMethod=args.get("support_tree_method", tree_builder.NEIGHBOR_JOINING if full_method == tree_builder.NEIGHBOR_JOINING else tree_builder.FAST_TREE),
            mlMatrix=args.get("matrix", "PROTGAMMAWAG"),
            ctx=ctx, seed=int(args.get("seed", 1)), support_rule=int(args.get("support_rule", 1)), fullTreeMethod=full_method)
    elif {"matrix", "support_matrix", "support_rule"} & set(args):
        from pepr_amd import tree_builder
        full = tree_builder._model_from_matrix(args.get("matrix"), ctx)
        sup = tree_builder._model_from_matrix(args["support_matrix"], ctx) if "support_matrix" in args else full
        r = ctx.jackknife2(genes, reps=reps, seed=int(args.get("seed", 1)), spr_radius_full=5, pi_mode=full["pi_mode"], ncat=full["ncat"],
                           support_pi_mode=sup["pi_mode"], support_rule=int(args.get("support_rule", 0)))
    else:
        r = ctx.jackknife(genes, reps=reps, seed=int(args.get("seed", 1)), spr_radius_full=5)
    dt = time.time() - t0
    run = args["run_name"]
    open(run + ".nwk", "w").write(r["newick"] + "\n")
    open(run + ".sup", "w").write("\n".join(r["support_trees"]) + "\n")
    if gene_steps_vals is not None:             # the gene homoplasy test on the tree just built
        g_reps = int(gene_steps_vals[0]) if len(gene_steps_vals) > 0 else 1000
        g_alpha = float(gene_steps_vals[1]) if len(gene_steps_vals) > 1 else 0.05
        gs = ctx.gene_steps(genes, r["newick"])
        th = ctx.step_thresholds(gs, engine.STEPS_BEYOND_MIN, True, 3, g_reps, g_alpha, int(args.get("seed", 1)))
        with open(run + ".steps.tsv", "w") as f:
            f.write("gene\tcolumns\tsteps\tbeyond\tratio\tthreshold\tn_ge\n")
            for k, name in enumerate(files):
                f.write("%s\t%d\t%d\t%d\t%s\t%d\t%d\n" % (os.path.basename(name), gs["col_start"][k + 1] - gs["col_start"][k], gs["gene_steps"][k],
                                                         gs["gene_beyond"][k], repr(float(gs["gene_ratio"][k])), int(th["threshold"][k]), th["n_ge"][k]))
    if "lnl" not in r:                          # the NJ loop: no likelihood
        print("%s: %d genes, neighbor joining, %d support trees, %.2f s -> %s.nwk %s.sup" % (run, len(genes), reps, dt, run, run))
        return
    if r.get("mp_lengths") and r["mp_lengths"][0] >= 0 and ":" not in r["newick"]:      # a parsimony full tree: a Fitch length, no likelihood
        print("%s: %d genes, %d columns, parsimony length %d, %d support trees, %.2f s -> %s.nwk %s.sup" % (
            run, len(genes), r["nsites"], r["mp_lengths"][0], reps, dt, run, run))
        return
    print("%s: %d genes, %d columns, lnL %.3f, alpha %.4f, %d support trees, %.2f s -> %s.nwk %s.sup" % (
        run, len(genes), r["nsites"], r["lnl"], r["alpha"], reps, dt, run, run))


if __name__ == "__main__":
    main(sys.argv[1:])
