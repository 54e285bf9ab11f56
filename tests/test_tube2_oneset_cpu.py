"""stage_tube2_kernel's one-set form on the CPU (no GPU): the rotation-closed placement of the 16 fields of a band row
(mulut_core.h tube4r_*, compiled with g++ from tests/host_emul/emul_oneset.cpp) and the arithmetic of one wrapping 16-bit accumulator
set against the two-set form the kernel had and against plain integers.  Bar: bit-exact."""
import ctypes

import numpy as np
import pytest

from host_emul_lib import load_emul


@pytest.fixture(scope="module")
def lib():
    L = load_emul("emul_oneset", ["mulut_core.h"])
    ip = ctypes.POINTER(ctypes.c_int)
    L.oneset_place.argtypes = [ctypes.c_int, ip]
    L.oneset_rot.argtypes = [ctypes.c_int, ctypes.c_int, ip]
    L.oneset_from_plain.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.oneset_from_plain.restype = None
    L.oneset_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.oneset_run.restype = None
    return L


def place(lib, p):
    out = (ctypes.c_int * 3)()
    lib.oneset_place(p, out)
    return tuple(out)


def rot(lib, r, plane):
    out = (ctypes.c_int * 2)()
    lib.oneset_rot(r, plane, out)
    return tuple(out)


def test_placement_is_a_bijection_with_its_inverse(lib):
    places = [place(lib, p) for p in range(16)]
    assert sorted(places) == [(pl, d, h) for pl in range(2) for d in range(4) for h in range(2)]
    for p, (pl, d, h) in enumerate(places):
        assert lib.oneset_pos(pl, d, h) == p
    # a position shares its dword with its 180-degree partner, and the other plane holds the two quarter turns
    for p, (pl, d, h) in enumerate(places):
        assert places[15 - p] == (pl, d, 1 - h)
        q = [x for x in range(16) if lib.oneset_row_elem(1, x >> 2, x & 3) == p][0]
        assert places[q][0] == 1 - pl and places[q][1] == d


@pytest.mark.parametrize("r", range(4))
def test_every_rotation_maps_dwords_onto_dwords(lib, r):
    """Row field (plane, dword, half) holds element e; rotation r adds it to the block position p with row_elem(r, p) == e.  Every
    position is reached exactly once, p sits in the same dword of plane acc_plane(r, plane), and the half swap is one per plane."""
    reached = []
    for plane in range(2):
        acc_plane, swap = rot(lib, r, plane)
        for d in range(4):
            for h in range(2):
                e = lib.oneset_pos(plane, d, h)
                hits = [p for p in range(16) if lib.oneset_row_elem(r, p >> 2, p & 3) == e]
                assert len(hits) == 1
                assert place(lib, hits[0]) == (acc_plane, d, h ^ swap), (r, plane, d, h)
                reached.append(hits[0])
    assert sorted(reached) == list(range(16))
    assert rot(lib, r, 0)[0] != rot(lib, r, 1)[0]
    if r == 0:
        assert [rot(lib, 0, pl) for pl in range(2)] == [(0, 0), (1, 0)]
    if r == 2:
        assert [rot(lib, 2, pl) for pl in range(2)] == [(0, 1), (1, 1)]
    if r in (1, 3):       # the planes cross, exactly one of them swaps, and rotation 3 takes the opposite choice
        assert rot(lib, r, 0)[0] == 1 and rot(lib, r, 0)[1] != rot(lib, r, 1)[1]
        assert [rot(lib, r, pl)[1] for pl in range(2)] == [1 - rot(lib, 4 - r, pl)[1] for pl in range(2)]


def test_staging_reorders_a_plain_slot(lib):
    """The kernel stages the plain band (lo_k = e(4k) | e(4k+2) << 16, hi_k = e(4k+1) | e(4k+3) << 16) in the rotation-closed order:
    every dword of the result holds the fields the placement names, for distinct and for 16-bit-wide values."""
    for e in (np.arange(16) * 7 + 78, np.random.default_rng(9).integers(0, 65536, 16)):
        e = np.ascontiguousarray(e.astype(np.uint16))
        out = np.zeros(8, np.uint32)
        lib.oneset_from_plain(e.ctypes.data, out.ctypes.data)
        for plane in range(2):
            for d in range(4):
                want = int(e[lib.oneset_pos(plane, d, 0)]) | (int(e[lib.oneset_pos(plane, d, 1)]) << 16)
                assert int(out[4 * plane + d]) == want, (plane, d)


def test_generated_blocks_use_the_same_placement(lib):
    """tools/gen_tube2_asm.py derives the table of its one-set blocks on its own; the generated file static_asserts it against the header
    when the kernel is compiled -- here the two are compared directly."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("gen_tube2_asm", os.path.join(ROOT, "tools", "gen_tube2_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert [[tuple(x) for x in m] for m in gen.ONESET] == [[rot(lib, r, pl) for pl in range(2)] for r in range(4)]


N_CASES = 10000


def weights(rng, n):
    """n x 12 x 5 weights, each 5-tuple non-negative with sum 16 (the differences of four sorted cuts of 0..16, as the simplex's are)"""
    cuts = np.sort(rng.integers(0, 17, (n, 12, 4)), axis=-1)
    edges = np.concatenate([np.zeros((n, 12, 1), int), cuts, np.full((n, 12, 1), 16)], axis=-1)
    w = np.diff(edges, axis=-1)
    assert (w.sum(-1) == 16).all() and (w >= 0).all()
    return w.astype(np.uint8)


@pytest.mark.parametrize("table", ["random", "all_max", "all_min"])
@pytest.mark.parametrize("M", [3, 4])
def test_one_set_gives_the_bytes_of_two_sets(lib, M, table):
    """10^4 seeded cases of 12 passes.  M = 4 is the list sdys: pattern s counts twice, its fields are 2-fold.  With the all-+127 table
    the fields pass 2^16 on the way and end at K = 32512 (M = 4); with all -128 they end at K = -32768: both sides wrap."""
    rng = np.random.default_rng(20240 + M)
    if table == "random":
        v = rng.integers(0, 256, (N_CASES, 12, 5, 16))
    else:
        v = np.full((N_CASES, 12, 5, 16), 255 if table == "all_max" else 0)
    fold = np.ones(12, int)
    if M == 4:
        fold[0:4] = 2
    rows = np.ascontiguousarray((v * fold[None, :, None, None]).astype(np.uint16))
    w = np.ascontiguousarray(weights(rng, N_CASES))
    two, one, ref = (np.zeros((N_CASES, 16), np.uint8) for _ in range(3))
    lib.oneset_run(rows.ctypes.data, w.ctypes.data, N_CASES, M, two.ctypes.data, one.ctypes.data, ref.ctypes.data)
    # the integer reference once more in NumPy, from row_elem alone
    elem = np.array([[lib.oneset_row_elem(r, p >> 2, p & 3) for p in range(16)] for r in range(4)])
    k = np.zeros((N_CASES, 16), np.int64)
    for ps in range(12):
        k += (w[:, ps, :, None].astype(np.int64) * rows[:, ps][:, :, elem[ps % 4]].astype(np.int64)).sum(1)
    k -= 128 * 16 * 4 * M
    assert np.abs(k).max() <= 8192 * M
    want = np.clip(np.round(k / (16 * M)), 0, 255).astype(np.uint8)       # np.round: half to even
    print(M, table, "K range", int(k.min()), int(k.max()), "one != two:", int((one != two).sum()), "one != ref:", int((one != want).sum()))
    assert np.array_equal(ref, want)
    assert np.array_equal(two, want)
    assert np.array_equal(one, two)
    if table == "all_max":
        assert (one == 255).all() and int(k.max()) == 127 * 16 * 4 * M
    if table == "all_min":
        assert (one == 0).all() and int(k.min()) == -128 * 16 * 4 * M
