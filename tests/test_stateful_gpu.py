"""GPU: random interleavings of every mutator with every query, the engine against the host model after each operation
(tests/stateful_model.py: Model, draw_ops, run; tests/test_stateful.py proves the driver on the CPU).

What a snapshot carries beyond S19's list of copied segments (read off snapshot_segments() and VecPogema.save_state, and
modelled so): the slots' generation counters `epoch`, `map_index` where a pool is installed, and the seed of the last
reset(seed); nothing of the distance-field cache, of the output sets or of their held-zeros records.

One test per committed (profile, seed).  A failure prints the profile, the seed, the operation's index, the operation, the
first differing element and the JSON of the operations so far; PGX_STATEFUL_SEED shifts the seeds, PGX_STATEFUL_OPS=N cuts
a sequence to its first N operations (tools/stateful_campaign.sh runs a range of seeds)."""
import pytest

from stateful_model import PROFILES, Model, committed_seeds, draw_ops, make_engine, profile_config, run

pytestmark = pytest.mark.gpu

CASES = [(p, s) for p in PROFILES for s in committed_seeds(p)]


@pytest.mark.parametrize("profile,seed", CASES)
def test_random_sequence_tracks_the_model(profile, seed):
    cfg = profile_config(profile, seed)
    ops = draw_ops(profile, seed)
    env = make_engine(cfg)
    try:
        assert env.held_zeros["enabled"] == bool(cfg["held"]), env.held_zeros
        run(env, Model(cfg), ops, label=f"{profile} seed {seed} ({cfg['collision']}, {cfg['semantics']})")
    finally:
        env.close()
