"""CPU: one scripted step on the oracle from each of tests/flat_fuse_states.py's states ends with the
in-window counts tests/test_gpu_flat_fuse.py's threshold walk relies on: one below, at and one above
flat_obs.hip's gather threshold, 99, 100, 101 and more than 128, entities on datastore rows
257..384 among the rows shown, and agents whose count crosses either threshold in both directions
from one state to the next."""

import numpy as np

from tests import flat_fuse_states as fs
from tests import obs_scenarios as sc


def test_post_step_counts_cross_the_thresholds():
    orc = sc.make_oracle(sc.config())
    seen, high = set(), 0
    prev = [None, None]
    cross = {(t, d): 0 for t in (fs.K_GATHER, 100) for d in ("up", "down")}
    for name, blob in fs.states():
        orc.set_state(blob)
        orc.step(orc.scripted_actions(fs.ACTION_SEED))
        post = orc.get_state()
        for e, c in enumerate(sc.counts(post)):
            iw = np.where(c["nv"] >= 0, c["in_window"], 0)
            seen.update(iw[iw > 0].tolist())
            if prev[e] is not None:
                both = (iw > 0) & (prev[e] > 0)
                for t in (fs.K_GATHER, 100):
                    cross[t, "up"] += int((both & (prev[e] <= t) & (iw > t)).sum())
                    cross[t, "down"] += int((both & (prev[e] > t) & (iw <= t)).sum())
            prev[e] = iw
        high += fs.high_rows_seen(post)
    print(sorted(seen), cross, high)
    assert all(k in seen for k in fs.NEED), sorted(seen)
    assert max(seen) > 128
    assert high > 0
    assert all(v > 0 for v in cross.values()), cross
