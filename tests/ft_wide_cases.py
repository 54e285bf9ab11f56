"""Exact cases for fine-tuning the 4 x 4 patterns e, h, o (test infrastructure, shared by test_ft_wide_cpu.py and
test_gpu_ft_wide.py), on top of tests/ft_exact_cases.py, which is used as it is.

The reference's differentiable module implements s, d, y only ("more sampling modes can be implemented similarly",
sr/model.py:119-121), and so does the oracle pinned to it, oracle/ft_torch.py -- which knows a pattern only through its
module-level PATTERNS (key offsets) and PAD (edge pad).  wide_oracle() adds the taps of e, h, o (common/network.py:173-215;
tests/golden/gen_golden_wide.py:TAPS) with pad 3 to both for the duration of a `with` block and restores them afterwards;
nothing under oracle/ is edited.  tests/test_ft_wide_cpu.py holds the oracle so extended to the NumPy restatement of a pass
(reach_cases.pass_q_np, itself held to c_oracle.pass_q), for all six patterns.

The exact-integer argument of ft_exact_cases carries over unchanged: integer x, integer tables and grad_out = avg * k make every
term an integer over q, and while the sum of magnitudes stays below 2^24 / q float32 sums are exact in any order -- the kernels
must give the extended oracle's bytes.  The cases below are the smallest shapes at which the halo-3 geometry of the backward
kernels' input-gradient tiles can go wrong.
"""
import contextlib

import ft_exact_cases as fx
from ft_exact_cases import CAP, Case, run_oracle      # noqa: F401  (re-exported for the tests)
from oracle import ft_torch

WIDE_PATTERNS = {
    "e": ((0, 0), (0, 3), (3, 0), (3, 3)),
    "h": ((0, 0), (2, 2), (2, 3), (3, 2)),
    "o": ((0, 0), (2, 2), (1, 3), (3, 1)),
}
WIDE_PAD = {"e": 3, "h": 3, "o": 3}
INTERVALS = (4, 5, 6)


@contextlib.contextmanager
def wide_oracle():
    """oracle.ft_torch with e, h, o added to its PATTERNS and PAD; both are put back on exit."""
    patterns, pad = ft_torch.PATTERNS, ft_torch.PAD
    ft_torch.PATTERNS, ft_torch.PAD = dict(patterns, **WIDE_PATTERNS), dict(pad, **WIDE_PAD)
    try:
        yield ft_torch
    finally:
        ft_torch.PATTERNS, ft_torch.PAD = patterns, pad


def reference(case, **kw):
    """ft_exact_cases.reference (integrality, the exactness cap and the case's reach asserted on the oracle alone) under wide_oracle()"""
    with wide_oracle():
        return fx.reference(case, **kw)


class WideCase(Case):
    """A Case whose name -- and so its seed -- can carry a draw number: the two smallest images need a draw that reaches what they are for"""

    def __init__(self, *a, **k):
        draw = k.pop("draw", 0)
        super(WideCase, self).__init__(*a, **k)
        if draw:
            self.name += "_draw%d" % draw


# First draw per interval at which the case reaches what it is for, found on the CPU with the oracle alone (the cases' reach= keeps it so):
# the 1 x 1 image needs pred inside the clamp at one block position at least (draw 0 clamps the only site at interval 6), the 2 x 2
# planes of five grey levels need a 255 next to a 0 (draw 0 has no vertex on the upper rim at interval 4)
ONE_PIXEL_DRAW = {4: 0, 5: 0, 6: 1}
TWO_BY_TWO_DRAW = {4: 1, 5: 0, 6: 0}


def _cases():
    out = []

    def add(*a, **k):
        out.append(WideCase(*a, **k))

    for iv in INTERVALS:
        band = iv in (4, 5)          # a band with rows outside it: the tube band (interval 4), the 121-row band (interval 5, u = 4)
        # every halo position folds onto the one pixel
        add(iv, 4, 1, "e", (1, 1, 1, 1), "noise", reach=("inside",), draw=ONE_PIXEL_DRAW[iv])
        # H and W smaller than the halo; three planes: the plane stride of the padded stack
        add(iv, 2, 1, "ho", (1, 3, 2, 2), "extreme", reach=("rim_lo", "rim_hi"), draw=TWO_BY_TWO_DRAW[iv])
        add(iv, 1, 0, "sdyeho", (1, 2, 9, 11), "noise", reach=("inside",))             # mixed reach in one list, two planes in one wave
        add(iv, 4, 1, "eho", (2, 1, 13, 10), "noise", reach=("below", "inside"))       # ragged 4 x 4 blocks
        add(iv, 3, 1, "oeh", (1, 1, 5, 6), "noise")                                    # interval 5, u = 3: the non-resident route
        add(iv, 4, 1, "sdyehoeh", (2, 1, 5, 6), "noise")                               # eight modes
        add(iv, 1, 0, "eho", (1, 2, 3, 300), "noise")                                  # the wave tile's memory fallback
        add(iv, 2, 1, "ho", (1, 1, 4, 260), "noise")
        add(iv, 4, 1, "eho", (1, 2, 3, 300), "noise")
        add(iv, 1, 0, "eho", (1, 1, 2, 120), "noise")                                  # still fits at halo 3: (2 + 6) * 126 = 1008 <= 1024
        # many workgroups flushing, band rows outside the tube / the 121-row band, evictions
        add(iv, 4, 1, "eho", (16, 1, 48, 48), "noise", reach=("rim_lo", "rim_hi", "below", "inside", "evict") + (("band_out",) if band else ()))
        add(iv, 1, 0, "eho", (16, 1, 48, 48), "noise", reach=("rim_lo", "rim_hi") + (("band_out",) if iv == 4 else ()))
        # the band-resident path on the content it was built for (thinned at the coarser grids: the exactness cap)
        thin = {4: None, 5: 0.5, 6: 0.15}[iv]
        add(iv, 4, 1, "eho", (64, 1, 48, 48), "natural", reach=("band_in", "evict", "below", "inside"), density=thin)
        add(iv, 1, 0, "eho", (64, 1, 48, 48), "natural", reach=("band_in",), density=thin)
        # the clamp's closed ends with an e in the list (a pass over constant tables gives the constant, whatever its pattern)
        add(iv, 4, 1, "sdye", (2, 1, 6, 7), "noise", tables=(64, 64, 64, 63), reach=("at_hi",))      # pred = 1020 = 255 * 4 at every site
        add(iv, 2, 1, "sdye", (2, 1, 6, 7), "noise", tables=(64, 64, 64, 64), reach=("above",))      # 1024: just outside
        add(iv, 1, 1, "ed", (2, 1, 6, 7), "noise", tables=(0, 0), reach=("at_lo",))
        add(iv, 1, 0, "edy", (2, 1, 6, 7), "noise", tables=(-127, -127, -127), reach=("at_lo",))     # -127 * 12 / 12 + 127 = 0
    assert len(set(c.name for c in out)) == len(out)
    return out


CASES = _cases()
