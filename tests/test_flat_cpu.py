"""The cases of tests/flat_cases.py do what they claim -- asserted on the NumPy reference alone (no GPU, no oracle)."""
import numpy as np
import pytest

import flat_cases as F

CASES = F.small_cases()


def test_reference_dirty_mask_is_the_pass_by_pass_definition():
    """dirty_mask against a direct loop over sites, passes and clamped neighbours on a small random image."""
    rng = np.random.default_rng(3)
    img = rng.integers(96, 160, (9, 11, 2)).astype(np.uint8)
    h = img >> 4
    H, W, C = h.shape
    want = np.zeros(h.shape, bool)
    for y in range(H):
        for x in range(W):
            for m in "sdy":
                for r in range(4):
                    pts = [(0, 0)] + [F._rot(r, di, dj) for di, dj in F.PAT[m]]
                    k = np.stack([h[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)] for dy, dx in pts]).astype(int)
                    want[y, x] |= (k.max(0) - k.min(0)) > 1
    assert np.array_equal(F.dirty_mask(img), want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_case_does_what_it_claims(name):
    img, chans, expect = CASES[name]
    H, W, C = img.shape
    assert (H, W) == (F.H0, F.W0) and W % 4 == 0
    dirty, flat, dt = F.dirty_mask(img), F.flat_tiles(img), F.dirty_tiles(img)
    # exact-dirty implies not flat, for every tile
    assert not (dt & flat).any()
    # only the outlier's channels hold dirty samples, and only within a window's reach of it
    for ch in range(C):
        if ch not in chans:
            assert not dirty[:, :, ch].any() and flat[:, :, ch].all(), (name, ch)
    if name == "two_level":
        assert not dirty.any() and flat.all()
        assert set(np.unique(img >> 4).tolist()) == {F.LEVEL, F.LEVEL + 1}
        return
    oy, ox = F.OUTLIER_AT[name]
    ys, xs, cs = np.nonzero(dirty)
    assert len(ys) > 0 and set(cs.tolist()) == set(chans), name
    assert (np.abs(ys - oy) <= F.HALO).all() and (np.abs(xs - ox) <= F.HALO).all()
    assert dirty[oy, ox, list(chans)].all()
    ty, tx = F.TILE
    if expect == "dirty":
        # the tile at (16, 4) holds dirty samples of exactly these channels and is not flat there
        assert [bool(dt[ty, tx, ch]) for ch in range(C)] == [ch in chans for ch in range(C)], name
        assert not flat[ty, tx, list(chans)].any()
    elif expect == "flat":
        # just outside what the tile's windows read: the tile stays flat and clean, its neighbour is not
        assert flat[ty, tx].all() and not dt[ty, tx].any(), name
        assert not flat[oy // F.TH, ox // F.TW].any()
    else:
        # borders: the clamped windows of the tile that holds the outlier see it
        assert dt[oy // F.TH, ox // F.TW].all() and not flat[oy // F.TH, ox // F.TW].any()


def test_halo_positions_lie_outside_the_tile_and_inside_its_windows():
    for name, (oy, ox) in F.OUTLIER_AT.items():
        inside = F.Y0 <= oy < F.Y0 + F.TH and F.X0 <= ox < F.X0 + F.TW
        reach = F.Y0 - F.HALO <= oy < F.Y0 + F.TH + F.HALO and F.X0 - F.HALO <= ox < F.X0 + F.TW + F.HALO
        if name.startswith("halo"):
            assert reach and not inside, name
        if name.startswith("outside"):
            assert not reach, name
            # one step further in and the windows would read it
            assert min(abs(oy - (F.Y0 - F.HALO)), abs(oy - (F.Y0 + F.TH + F.HALO - 1)), abs(ox - (F.X0 - F.HALO)),
                       abs(ox - (F.X0 + F.TW + F.HALO - 1))) == 1, name


@pytest.mark.parametrize("shape", F.PARTIAL_SHAPES)
def test_ridged_field_loads_the_edge_tiles_and_their_neighbours(shape):
    n, h, w, c = shape
    assert w % F.TW != 0 or h % F.TH != 0
    assert n * (-(-h // 16)) * (-(-w // 64)) > 256          # more verdict tiles than the device has compute units
    img = F.ridged(*shape)
    for f in range(n):
        dt, flat = F.dirty_tiles(img[f]), F.flat_tiles(img[f])
        assert not (dt & flat).any()
        # every tile of the right and of the bottom edge carries entries, and so do most of the full tiles beside them
        assert dt[:, -1].any(-1).all() and dt[-1, :].any(-1).all()
        assert dt[:, -2].any(-1).mean() > 0.5 and dt[-2, :].any(-1).mean() > 0.5
        # ... while the field is smooth enough that flat tiles and clean samples are common too: both paths run
        share = flat.mean()
        assert 0.1 < share < 0.9, share
        assert 0.02 < F.dirty_mask(img[f]).mean() < 0.5
