"""A replayed scoring plan visits only the genes whose branch lengths or rates moved since its descriptors were last
refreshed.  Lengths and alpha changed by an optimisation between two scoring passes must reach the next replay, a replay
with nothing changed must repeat the bits, and an untouched gene must keep its score."""
import numpy as np
import pytest

from pepr_amd import engine, synth

pytestmark = pytest.mark.gpu


def test_replay_picks_up_moved_lengths_and_rates(gpu_ctx):
    shapes = [(50, 1000), (12, 30), (20, 1400), (50, 1000), (7, 20), (16, 700)]
    genes = [synth.simulate_alignment(nt, ns, 400 + i, missing_frac=0.1 * (i % 3)) for i, (nt, ns) in enumerate(shapes)]
    b = engine.Batch(gpu_ctx, [(g[0], g[1]) for g in genes], [g[2] for g in genes], alpha=0.8)
    first = b.score()                       # records the plan
    assert all(np.array_equal(b.score(), first) for _ in range(3))
    b.set_alpha(0.5, 2)                     # one gene's rates
    one = b.score()
    assert one[2] != first[2] and np.array_equal(np.delete(one, 2), np.delete(first, 2)) and np.array_equal(b.score(), one)
    opt, _ = b.optimize()                   # every gene's lengths and alpha
    after = b.score()
    assert np.array_equal(b.score(), after) and np.array_equal(b.score(stored=True), after)
    assert np.all(after > one) and np.allclose(after, opt, rtol=1e-6, atol=0)
    # the same trees and rates scored without a cached plan
    fresh = np.array([b.site_lnl(g, shapes[g][1]).sum() for g in range(len(genes))])
    assert np.allclose(after, fresh, rtol=1e-11, atol=0)
    b.close()
