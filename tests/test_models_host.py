"""pml_matrix_parse_paml: the host-side reader of PAML .dat rate-matrix files (190 lower-triangle exchangeabilities by rows,
then 20 frequencies, state order ARNDCQEGHILKMFPSTWYV) that `raxmlHPC -m PROTGAMMA<NAME>` and Context.register_matrix feed on."""
import json
import os

import numpy as np
import pytest

from pepr_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PML_EPARSE = -2


def _wag():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "wag_constants.json")))
    return np.array(d["S_lower"]), np.array(d["pi_full"])


def paml_text(ex, pi, tail=""):
    lines, k = [], 0
    for i in range(1, 20):
        lines.append(" ".join(repr(float(x)) for x in ex[k:k + i]))
        k += i
    lines += ["", " ".join(repr(float(x)) for x in pi), tail]
    return "\n".join(lines)


def test_paml_round_trip_and_trailing_text():
    ex, pi = _wag()
    for tail in ("", "\n A R N D C Q E G H I L K M F P S T W Y V\nAla Arg 12 3.5 not a number\n"):
        e2, p2 = engine.parse_paml(paml_text(ex, pi, tail))
        assert np.array_equal(e2, ex) and np.array_equal(p2, pi)


@pytest.mark.parametrize("bad", ["short", "negative", "nan", "inf", "word"])
def test_paml_rejects(bad):
    ex, pi = _wag()
    nums = [repr(float(x)) for x in np.concatenate([ex, pi])]
    if bad == "short":
        nums = nums[:209]
    elif bad == "negative":
        nums[57] = "-0.25"
    elif bad == "nan":
        nums[3] = "nan"
    elif bad == "inf":
        nums[200] = "inf"
    else:
        nums[100] = "abc"
    with pytest.raises(engine.PmlError) as e:
        engine.parse_paml(" ".join(nums))
    assert e.value.code == PML_EPARSE
