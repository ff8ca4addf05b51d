"""tests/wide_harness.py over the small cases of tests/test_gpu_step_path.py: the same three legs (recorded score, replay, stored
traversal) and the same JSON, for tile occupancies and tree shapes at which a wave of the scoring kernel waits for its staged
fragments or reads back a CLV it has just stored.  The test runs it once per PML_CHAIN_VARIANT, as test_gpu_score_wide.py does."""
import wide_harness
from pepr_amd import synth

# rooted at t0, operations in depth-first order:
#   ((t1,t2),t3) a pitchfork and ((t4,t5),(t6,t7)) a double cherry, joined in A;
#   (((t8,t9),t10),t11) a ladder: every result is the chained input of the very next operation;
#   the last operation joins A -- stored five operations earlier and read back from memory -- with the ladder in registers
TREE = ("(t0:0.1,((((t1:0.2,t2:0.13):0.07,t3:0.3):0.09,((t4:0.05,t5:0.21):0.12,(t6:0.17,t7:0.08):0.1):0.06):0.11,"
        "(((t8:0.1,t9:0.2):0.05,t10:0.15):0.07,t11:0.09):0.13):0.1);")
# the same taxa as one ladder from t11 down to t1: eleven operations, each reading its predecessor's result
LADDER = ("(t0:0.1,(t1:0.2,(t2:0.13,(t3:0.3,(t4:0.05,(t5:0.21,(t6:0.17,(t7:0.08,(t8:0.1,(t9:0.2,(t10:0.15,t11:0.09)"
          ":0.04):0.06):0.05):0.12):0.07):0.03):0.09):0.11):0.08):0.1);")
NPAT = {"one_chunk": 30, "mpad_288": 270, "mpad_544": 530}      # padded to multiples of 32: 32, 288 = 256 + one wave, 544 = 512 + one wave


def cases():
    names, rows, _ = synth.simulate_alignment(12, 1500, 606, 0.8)
    out = {}
    for name, n in NPAT.items():
        gene = wide_harness._first_patterns(names, rows, n)
        out[name] = ([gene, gene], [TREE, LADDER], 0.8, None)
    return out


if __name__ == "__main__":
    wide_harness.cases = cases
    wide_harness.main()
