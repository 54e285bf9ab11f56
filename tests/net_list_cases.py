"""What tests/test_net_list_cpu.py and tests/test_gpu_net_list.py share: the lists of the list form of the cascade (mulut_net_plan_*,
mulut_amd/csrc/mulut_net_list.hip), a restatement of the plan's tables, and the pools a GPU test lays a list out in.

The shapes are the smallest at which the kernel can go wrong, h x w of the LR image.  A workgroup serves 128 sites of one item and a
site is (channel, y, x), the channel slowest; with ch = 3:
    1 x 1      3 sites: every tap of every pattern is the pixel itself
    2 x 3      18 sites: smaller than the pad of e / h / o (3), so every tap is clamped in some rotation
    5 x 7      105 sites: less than one workgroup, plane boundaries at sites 35 and 70 inside a wave
    6 x 7      126 sites: two short of a workgroup
    43 x 1     129 sites: one more than a workgroup; a single column
    11 x 12    396 sites: four workgroups, the plane boundaries 132 and 264 inside the second and third
    1 x 43     a single row
"""
import numpy as np

SITES = 128          # kNetSites
MIXED = [(1, 1), (2, 3), (5, 7), (6, 7), (43, 1), (11, 12), (1, 43)]
MANY = [(6 + i % 4, 7 + (i // 4) % 5) for i in range(328)]      # 328 small items of 126 .. 297 sites, 1 to 3 workgroups each: a map of more than 512 entries (a page)

# the models of the GPU tests: seeded (net_cases.seeded_model), nf 8 and 33 for the two M-tile instances, nf 64 once
MODELS = {
    "x4_sdy_nf8": dict(nf=8, scale=4, modes="sdy", stages=2, seed=11),
    "x4_sdy_nf33": dict(nf=33, scale=4, modes="sdy", stages=2, seed=12),
    "x2_one_stage_nf8": dict(nf=8, scale=2, modes="sd", stages=1, seed=13),
    "x2_one_stage_nf33": dict(nf=33, scale=2, modes="y", stages=1, seed=14),
    "x3_eho_nf8": dict(nf=8, scale=3, modes="eho", stages=3, seed=15),
    "x3_eho_nf33": dict(nf=33, scale=3, modes="eho", stages=3, seed=16),
    "x4_sdy_nf64": dict(nf=64, scale=4, modes="sdy", stages=2, seed=17),
}


def tables(shapes, ch, stages, scale):
    """The plan of images of `shapes` packed back to back in both pools, restated: (items, map, workspace bytes, copied bytes), items
    as (in_off, out_off, mid, h, w) and the map as (item, first site) per workgroup."""
    items, wg_map, in_off, out_off, mid = [], [], 0, 0, 0
    for i, (h, w) in enumerate(shapes):
        sites = ch * h * w
        items.append((in_off, out_off, mid, h, w))
        wg_map += [(i, first) for first in range(0, sites, SITES)]
        in_off, out_off, mid = in_off + sites, out_off + sites * scale * scale, mid + sites
    sets = 0 if stages == 1 else 1 if stages == 2 else 2
    copied = 32 * len(items) + 8 * len(wg_map)
    return items, wg_map, copied + sets * mid, copied


class Pools:
    """A list laid out in two byte pools for the GPU tests: image k's input at an odd offset of the input pool, its result's slot at
    an odd offset of the output pool, the slots in ANOTHER order than the inputs (reversed), and a guard band of `guard` bytes of
    GUARD in front of, between and behind the slots of either pool."""
    GUARD = 0xA5

    def __init__(self, shapes, ch, scale, seed=0, guard=37):
        rng = np.random.default_rng(seed)
        self.shapes, self.ch, self.scale = list(shapes), ch, scale
        self.images = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for h, w in self.shapes]
        self.in_off, self.out_off = [0] * len(self.shapes), [0] * len(self.shapes)
        at = guard
        for k, im in enumerate(self.images):
            at += (at + 1) % 2      # odd
            self.in_off[k] = at
            at += im.size + guard
        self.in_bytes = at
        at = guard
        for k in reversed(range(len(self.shapes))):
            at += (at + 1) % 2
            self.out_off[k] = at
            at += self.images[k].size * scale * scale + guard
        self.out_bytes = at
        self.in_pool = np.full(self.in_bytes, self.GUARD, np.uint8)
        for k, im in enumerate(self.images):
            self.in_pool[self.in_off[k]:self.in_off[k] + im.size] = im.reshape(-1)

    def items(self):
        return [(self.in_off[k], self.out_off[k], h, w, self.in_bytes, self.out_bytes) for k, (h, w) in enumerate(self.shapes)]

    def fresh_out(self):
        return np.full(self.out_bytes, self.GUARD, np.uint8)

    def result(self, out_pool, k):
        h, w = self.shapes[k]
        n = h * w * self.ch * self.scale * self.scale
        return out_pool[self.out_off[k]:self.out_off[k] + n].reshape(h * self.scale, w * self.scale, self.ch)

    def outside(self, out_pool):
        """The bytes of an output pool that belong to no item."""
        mask = np.ones(self.out_bytes, bool)
        for k, (h, w) in enumerate(self.shapes):
            mask[self.out_off[k]:self.out_off[k] + h * w * self.ch * self.scale * self.scale] = False
        return out_pool[mask]
