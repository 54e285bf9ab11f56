"""What the cases of tests/persist_cases.py reach, asserted on their inputs and the oracle alone (no GPU): every consumer a case is
for gets more tiles (entries) than one pass of its grid covers -- one full round more and a partial one --, both kinds of tile lie
beyond the first pass, and the frame cuts the tiles at the right and at the bottom.  tests/test_gpu_persist.py holds the library to
the oracle's bytes on these cases; this file is why a pass there means something."""
import numpy as np
import pytest

import flat_cases as F
import persist_cases as P


def test_limits_restate_the_launchers():
    """The first-pass sizes at 256 compute units, as the issue's table states them."""
    assert P.CUS == 256 and P.VERDICT_TILE == (64, 16) and P.SITE_TILE == (64, 64)
    assert {k: v[1] for k, v in P.LIMITS.items()} == {"tube": 256, "detail_plan": 1024, "detail_retile": 2048,
                                                       "detail_fill": 4096, "fix2": 32768, "site_tiles": 256, "site_fix": 262144}


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_edge_tile_shape(name):
    k = P.CASES[name]
    assert k["w"] % 64 and k["w"] % 16 and k["w"] % 4 and k["h"] % 16 and k["h"] % 4, k
    assert -(-k["w"] // 64) == 2 and k["w"] - 64 < 4        # the second tile column is narrower than one dword of samples


def test_band_period_mixes_the_tall_tiles_only():
    assert P.PERIOD % 64 and P.PERIOD != 16 and 0 < P.NATURAL_ROWS < P.PERIOD
    # a photograph-like band and a noise band each hold a whole 16-row tile at some phase; no 64-row tile is of one kind
    natural = (np.arange(16 * P.PERIOD) % P.PERIOD) < P.NATURAL_ROWS
    t16, t64 = natural.reshape(-1, 16), natural[:(len(natural) // 64) * 64].reshape(-1, 64)
    assert t16.all(1).any() and (~t16).all(1).any()
    assert not t64.all(1).any() and not (~t64).all(1).any()


def test_images_of_a_batch_differ():
    for name, k in P.CASES.items():
        if k["n"] > 1:
            x = P.case_frames(name)
            assert (x[0] != x[1]).mean() > 0.4, name


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_every_consumer_runs_past_its_first_pass(name):
    k = P.CASES[name]
    for consumer in k["consumers"]:
        what, limit = P.LIMITS[consumer]
        for stage in P.stages_of(name, consumer):
            r = P.reach(name, stage)
            count = r[what]
            print("%s stage %d %s: %s %d, first pass %d (%.2f rounds); verdict tiles %d, 64 x 64 tiles %d, dirty samples %d of %d" % (
                name, stage, consumer, what, count, limit, count / limit, r["verdict_tiles"], r["site_tiles"], r["entries"],
                P.stage_inputs(name)[stage - 1].size))
            if consumer in P.ONE_ROUND_MORE:
                assert count > limit and count % limit, (name, consumer, count)
            else:
                assert count > 2 * limit and count % limit, (name, consumer, count)
            if what == "entries":
                continue
            clean, heavy = P.kinds_beyond(P.dirty(name, stage), P.tile_of(consumer), limit)
            print("    tiles beyond the first pass: %d without a dirty sample, %d more than half dirty" % (clean, heavy))
            assert clean >= 1 and heavy >= 1, (name, consumer, stage, clean, heavy)
            # and as the device walks them: in round 1 or later of the consumer's own order
            clean, heavy = P.kinds_beyond(P.dirty(name, stage), P.tile_of(consumer), limit, consumer)
            print("    tiles in round >= 1 of the walk: %d without a dirty sample, %d more than half dirty" % (clean, heavy))
            assert clean >= 1 and heavy >= 1, (name, consumer, stage, clean, heavy, "by walk round")


def test_tile_measures_on_a_small_frame():
    """kinds_beyond and tile_index against a frame worked out by hand: 2 images of 20 x 70 x 1, tiles of 64 x 16 -> 2 x 2 tiles each."""
    d = np.zeros((2, 20, 70, 1), bool)
    d[0, :16, :64] = True               # tile 0 of image 0: all dirty
    d[1, 16:, 64:] = True               # the corner tile of image 1 (4 x 6 samples): all dirty
    d[1, 0, 0] = True                   # tile 0 of image 1: one sample of 1024
    dirty_per, size_per = P.tile_dirty_share(d, (64, 16))
    assert dirty_per.tolist() == [1024, 0, 0, 0, 1, 0, 0, 24] and size_per.tolist() == [1024, 96, 256, 24] * 2
    assert P.kinds_beyond(d, (64, 16), 0) == (5, 2) and P.kinds_beyond(d, (64, 16), 5) == (2, 1)
    assert P.kinds_beyond(d, (64, 16), 5, "detail_plan") == (0, 0)      # 8 tiles: all in the first pass of a 1,024-thread grid
    assert P.tile_count(2, 20, 70, (64, 16)) == 8
    assert P.tile_index(1, 17, 65, 20, 70, (64, 16)) == 7 and P.tile_index(0, 15, 63, 20, 70, (64, 16)) == 0


def test_walk_rounds():
    """4,142 tiles: the persistent walkers' 8 ranges hold 518 tiles, 32 workgroups stride over each; a fixed grid strides over all."""
    idx = np.array([0, 31, 32, 517, 518, 549, 550, 4141])
    assert P.walk_round(idx, 4142, "tube").tolist() == [0, 0, 1, 16, 0, 0, 1, 16]
    assert P.walk_round(idx, 4142, "detail_plan").tolist() == [0, 0, 0, 0, 0, 0, 0, 4]
    got, want = np.zeros((1, 40, 280, 1), np.uint8), np.zeros((1, 40, 280, 1), np.uint8)
    got[0, 39, 279, 0] = 1
    assert "1 bytes differ" in P.describe_difference(got, want, "x4_final_c1", "tube") and "(0, 39, 279, 0)" in P.describe_difference(got, want, "x4_final_c1", "tube")


def test_dirty_tiles_agree_with_flat_cases():
    """The tile predicate here, at the wave tile of flat_cases (16 x 4), is flat_cases.dirty_tiles."""
    img = P.frames(1, 203, 67, 3, seed=99)[0]
    per, _ = P.tile_dirty_share(F.dirty_mask(img)[None], (F.TW, F.TH))
    assert np.array_equal(per.reshape(-(-203 // F.TH), -(-67 // F.TW)) > 0, F.dirty_tiles(img).any(2))
