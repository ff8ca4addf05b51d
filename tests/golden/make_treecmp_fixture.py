"""Writes tests/golden/treecmp_cases.json: pairs of small trees whose three RF values and two distances were worked BY HAND
(the arithmetic is in each case's "why"), so that tests/treecmp_ref.py is not its own judge, and hand-worked prunings for the
mirror of BasicTree.removeTaxon.  A distance is stored as the two numbers the hand calculation ends with, r and den =
sumOfSquaresTree1 + sumOfSquaresTree2 (all exact in binary: the lengths are dyadic), and as the double sqrt(r) / sqrt(den).
Nothing here calls the restatement.  Run from the repository root: python tests/golden/make_treecmp_fixture.py"""
import json
import math
import os


def dist(r, den):
    if r != r or den != den or (r == 0 and den == 0):
        return {"r": None, "den": None, "value": "nan"}
    return {"r": r, "den": den, "value": (math.sqrt(r) / math.sqrt(den)).hex()}


NAN = float("nan")
CASES = [
    {"name": "quartet_nni", "tree1": "((A:1,B:1):1,C:1,D:1);", "tree2": "((A:1,C:1):1,B:1,D:1);",
     "why": "Both trees have 5 branches of length 1 (4 pendant, 1 inner), maximum 1, so normalised lengths are 1. Clade sets: 10 "
            "sets each (4 singletons, 4 triples, and AB,CD against AC,BD); 8 shared, union 12: (12-8)/4 = 1. Bipartitions: AB|CD "
            "against AC|BD, union 2, intersection 0: 2/2 = 1. Branch distance: the 4 pendant branches match with difference 0, AB "
            "has no counterpart: r = 1; ss1 = 5; second loop: ss2 = 5, AC unmatched: r = 2. sqrt(2)/sqrt(10). Discrepant: AB and AC "
            "unmatched, 1 + 1 = 2, raw sums 5 + 5.",
     "rf_legacy": 1, "rf_bipartition": 1, "rf_splits": 1, "branch_dist": dist(2.0, 10.0), "discrepant_dist": dist(2.0, 10.0)},
    {"name": "bifurcating_root_is_one_branch", "tree1": "((A:0.5,B:0.5):0.25,((C:1,D:1):0.5,E:2):0.75);", "tree2": "(A:0.5,B:0.5,((C:1,D:1):0.5,E:2):1.0);",
     "why": "tree1's two top-level nodes (AB) and (CDE) become ONE branch AB|CDE of length 0.25 + 0.75 = 1.0: 7 = 2n-3 branches, "
            "not 8. tree2 is the same unrooted tree with that branch written as (CDE):1.0. Every split and every length agrees: all "
            "RF values 0, r = 0. Maximum 2; normalised squares: A,B 0.0625 each, C,D 0.25 each, E 1, CD 0.0625, AB|CDE 0.25: "
            "ss = 1.9375 per tree, den 3.875; 0/sqrt(3.875) = 0. Raw: 0.25+0.25+1+1+4+0.25+1 = 7.75 per tree.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(0.0, 3.875), "discrepant_dist": dist(0.0, 15.5)},
    {"name": "bifurcating_root_sum_differs", "tree1": "((A:0.5,B:0.5):0.25,((C:1,D:1):0.5,E:2):0.75);", "tree2": "(A:0.5,B:0.5,((C:1,D:1):0.5,E:2):0.5);",
     "why": "As above but tree2's AB|CDE branch is 0.5 against the summed 1.0: normalised 0.25 against 0.5, r = 0.0625. ss1 = 1.9375, "
            "ss2 = 1.9375 - 0.25 + 0.0625 = 1.75. sqrt(0.0625)/sqrt(3.6875). If the root's two halves were two branches, tree1 "
            "would hold the split twice and the value would differ. Discrepant: every branch has a counterpart, r = 0; raw sums "
            "7.75 + 7.0.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(0.0625, 3.6875), "discrepant_dist": dist(0.0, 14.75)},
    {"name": "multifurcation", "tree1": "((A:1,B:1,C:1):1,D:1,(E:1,F:1):1);", "tree2": "(((A:1,B:1):1,C:1):1,D:1,(E:1,F:1):1);",
     "why": "tree1 has 8 branches (6 pendant, ABC, EF), tree2 has 9 (also AB). Clade sets 16 and 18, 16 shared, union 18: (18-16)/4 = "
            "2/4 = 0 in integers. Bipartitions {ABC,EF} and {AB,ABC,EF}: (3-2)/2 = 0. rf_splits: the project's parser resolves "
            "(A,B,C) into ((A,B),C), which IS tree2: 0. All lengths 1: tree1's branches all match, r = 0, ss1 = 8; ss2 = 9 and AB is "
            "unmatched: r = 1. 1/sqrt(17), the same for the discrepant distance.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(1.0, 17.0), "discrepant_dist": dist(1.0, 17.0)},
    {"name": "missing_length_is_zero", "tree1": "((A,B:2):1,C:1,D:1);", "tree2": "((A:1,B:2):1,C:1,D:1);",
     "why": "A has no length in tree1: 0.0, not TreeBranch's default 1. Maximum 2 in both. tree1 normalised: A 0, B 1, AB, C, D 0.5: "
            "ss1 = 1 + 3*0.25 = 1.75. tree2: A 0.5: ss2 = 2.0. Only A differs: r = 0.25. sqrt(0.25)/sqrt(3.75). With the default 1 "
            "r would be 0. Discrepant: all matched, r = 0, raw sums (4+1+1+1) + (1+4+1+1+1) = 7 + 8.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(0.25, 3.75), "discrepant_dist": dist(0.0, 15.0)},
    {"name": "all_lengths_zero", "tree1": "((A:0,B:0):0,C:0,D:0);", "tree2": "((A:1,B:1):1,C:1,D:1);",
     "why": "tree1's maximum is 0: every normalised length is 0/0 = NaN, so r and ss1 are NaN and the branch distance is NaN. "
            "Discrepant uses raw lengths: all branches match, r = 0, ss1 = 0, ss2 = 5: 0/sqrt(5) = 0.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(NAN, NAN), "discrepant_dist": dist(0.0, 5.0)},
    {"name": "all_lengths_zero_against_itself", "tree1": "((A:0,B:0):0,C:0,D:0);", "tree2": "((A:0,B:0):0,C:0,D:0);",
     "why": "Branch distance NaN as above; discrepant: sqrt(0)/sqrt(0 + 0) = 0/0 = NaN.",
     "rf_legacy": 0, "rf_bipartition": 0, "rf_splits": 0, "branch_dist": dist(NAN, NAN), "discrepant_dist": dist(NAN, NAN)},
    {"name": "no_lengths_used", "tree1": "((A:1,B:1):1,C:1,D:1);", "tree2": "((A:1,C:1):1,B:1,D:1);", "use_lengths": False,
     "why": "Without -use_lengths getTreeString prints no length and every length reads 0: both distances NaN, RF as quartet_nni.",
     "rf_legacy": 1, "rf_bipartition": 1, "rf_splits": 1, "branch_dist": dist(NAN, NAN), "discrepant_dist": dist(NAN, NAN)},
    {"name": "eight_taxa_one_nni",
     "tree1": "(((A:1,B:1):1,C:1):1,D:1,(E:1,(F:1,(G:1,H:1):1):1):1);", "tree2": "(((A:1,C:1):1,B:1):1,D:1,(E:1,(F:1,(G:1,H:1):1):1):1);",
     "why": "13 = 2n-3 branches each, all of length 1: 8 pendant and AB (AC in tree2), ABC, GH, FGH, EFGH. 12 shared splits: clade "
            "sets 26 and 26 with 24 shared, union 28: 4/4 = 1. Bipartitions 5 and 5 with 4 shared: (6-4)/2 = 1. r = 1 (AB) + 1 (AC) = 2, "
            "ss1 = ss2 = 13: sqrt(2)/sqrt(26) for both distances.",
     "rf_legacy": 1, "rf_bipartition": 1, "rf_splits": 1, "branch_dist": dist(2.0, 26.0), "discrepant_dist": dist(2.0, 26.0)},
]

# a repeated split: no text gives one (a node with one child is refused), so the trees are given as branch lists
AB, CD = ["A", "B"], ["C", "D"]
PEND = [(["A"], ["B", "C", "D"], 1), (["B"], ["A", "C", "D"], 1), (["C"], ["A", "B", "D"], 1), (["D"], ["A", "B", "C"], 1)]
REPEATED = [
    {"name": "repeated_split_in_tree2", "leaves": ["A", "B", "C", "D"],
     "branches1": [list(b) for b in PEND] + [[AB, CD, 2]], "branches2": [list(b) for b in PEND] + [[AB, CD, 1], [AB, CD, 2]],
     "why": "tree2 holds AB|CD twice, lengths 1 then 2; HashMap.put keeps the LATER one as the counterpart. Maximum 2 in both. tree1 "
            "normalised: pendant 0.5, AB 1; its AB meets the later AB (1): every difference 0, r = 0, ss1 = 4*0.25 + 1 = 2. Second "
            "loop: ss2 = 5*0.25 + 1 = 2.25; the EARLIER AB (0.5) is not in checkedBranches: r = 0.25. sqrt(0.25)/sqrt(4.25). "
            "Discrepant: first loop adds nothing, the earlier AB adds 1*1: r = 1, raw sums (4+4) + (5+4) = 17. RF: equal clade sets, 0.",
     "rf_legacy": 0, "branch_dist": dist(0.25, 4.25), "discrepant_dist": dist(1.0, 17.0)},
    {"name": "repeated_split_in_tree1", "leaves": ["A", "B", "C", "D"],
     "branches1": [list(b) for b in PEND] + [[AB, CD, 1], [AB, CD, 2]], "branches2": [list(b) for b in PEND] + [[AB, CD, 2]],
     "why": "The same two trees the other way round: both ABs of tree1 meet tree2's AB (1): differences 0.5 and 0, r = 0.25, ss1 = 2.25; "
            "every branch of tree2 is checked, ss2 = 2. sqrt(0.25)/sqrt(4.25). Discrepant: nothing unmatched, r = 0, raw 9 + 8.",
     "rf_legacy": 0, "branch_dist": dist(0.25, 4.25), "discrepant_dist": dist(0.0, 17.0)},
]

# BasicTree.removeTaxon (BasicTree.java:888-946) followed by getTreeString(true, true): node indices are leaves in text order,
# then inner nodes by ')'; a node's children are listed in ascending index
PRUNE = [
    {"name": "parent_left_with_one_child", "tree": "((A:1,B:2):3,C:4,D:5);", "remove": "B", "expect": "(C:4.0,D:5.0,A:4.0);",
     "why": "(A,B) keeps only A: A takes the parent's place among the root's children [C, D, (AB)] and its length 1 + 3 = 4 (:919-934)."},
    {"name": "top_level_leaf", "tree": "((A:1,B:2):3,C:4,D:5);", "remove": "D", "expect": "(C:4.0,(A:1.0,B:2.0):3.0);",
     "why": "The root keeps two children: nothing collapses (:936-943); children print leaves first."},
    {"name": "root_left_with_one_child", "tree": "((A:1,B:2):3,C:4);", "remove": "C", "expect": "(A:1.0,B:2.0);",
     "why": "The root keeps only (AB), which becomes the new root (:912-917); its own length 3 is not printed for a root."},
    {"name": "absent_taxon", "tree": "((A:1,B:2):3,C:4,D:5);", "remove": "Z", "expect": "(C:4.0,D:5.0,(A:1.0,B:2.0):3.0);",
     "why": "No leaf matches: the tree is unchanged (:897) and prints in child-index order."},
    {"name": "case_insensitive_match", "tree": "((A:1,b:2):3,C:4,D:5);", "remove": "B", "expect": "(C:4.0,D:5.0,A:4.0);",
     "why": "removeTaxon matches with equalsIgnoreCase (:892)."},
]

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "treecmp_cases.json")
    with open(out, "w") as f:
        json.dump({"cases": CASES, "repeated": REPEATED, "prune": PRUNE}, f, indent=1)
        f.write("\n")
    print("wrote", out)
