"""The reach of tests/abi_sequences.py, asserted on the generator alone (no GPU): what test_gpu_abi_state.py runs on the device is
a tour that really visits every reconfiguration, every form of mulut_set_lut per table slot, every error code the header names and
every operation -- and it is the same tour on every run."""
import itertools

import numpy as np
import pytest

import abi_sequences as A


@pytest.fixture(scope="module")
def seqs():
    return A.sequences()


def test_every_ordered_pair_of_families_is_a_reconfiguration_with_a_checked_call(seqs):
    pairs = set()
    for ops in seqs:
        confs = A.configurations(ops)
        for fam, i, checked in confs:
            assert checked, "no checked compute call after configure #%d (%s)" % (i, fam)
        pairs.update((a[0], b[0]) for a, b in zip(confs, confs[1:]))
    want = set(itertools.permutations(A.FAMILIES, 2))
    assert want <= pairs, sorted(want - pairs)


def test_every_table_slot_sees_the_three_forms_of_set_lut(seqs):
    forms = {}
    for ops in seqs:
        m = A.Model()
        for op in ops:          # replay the set-up calls through a fresh model: the forms follow from the state alone
            a = op.args
            if op.name == "configure":
                m.configure(a["stages"], a["modes"], a["scale"], a["interval"])
            elif op.name == "set_lut":
                m.set_lut(a["stage"], a["mode"], a["table"])
        for slot, form in m.forms:
            forms.setdefault(slot, set()).add(form)
    assert len(forms) >= 4 * 3 + 2 * 3      # stages 1..4 of s, d, y; stages 1..2 of e, h, o
    for slot, seen in sorted(forms.items()):
        assert seen == {"new", "rewrite", "vnum"}, (slot, seen)


def test_every_error_code_and_every_operation_occurs(seqs):
    ops = [op for s in seqs for op in s]
    errors = {(op.name, op.value) for op in ops if op.kind == "error"}
    for name, code in (("pipeline", A.ENOTCONFIGURED), ("pass_q", A.ENOTCONFIGURED), ("pipeline", A.ENOLUT), ("pipeline", A.ESHAPE),
                       ("set_lut", A.ESHAPE), ("set_lut", A.EMODE), ("configure", A.EMODE), ("pass_q", A.EMODE),
                       ("configure", A.EUNSUPPORTED), ("set_tuning", A.EINVAL)):
        assert (name, code) in errors, (name, code)
    checked = {op.name for op in ops if op.kind == "bytes"}
    assert checked == {"pipeline", "pipeline_rows", "stage", "pass_q"}
    assert {op.name for op in ops} >= {"configure", "set_lut", "set_tuning", "reserve", "set_stage_timing", "last_stage_ms",
                                       "last_kernel_ms", "last_detail_counters"}
    # ENOLUT after an interval change in particular: the configure before it moved to another interval
    cleared = 0
    for s in seqs:
        iv = 4
        for a, b in zip(s, s[1:]):
            if a.name == "configure" and a.kind == "ok":
                cleared += a.args["interval"] != iv and b.kind == "error" and b.value == A.ENOLUT
                iv = a.args["interval"]
    assert cleared >= 12
    # both layouts for every compute call that has one, a stage chained through the buffer the previous stage wrote
    for name in ("pipeline", "pipeline_rows", "stage"):
        assert {op.args["layout"] for op in ops if op.name == name and op.kind == "bytes"} == {A.CHW, A.HWC}, name
    assert {op.args["out_layout"] for op in ops if op.name == "stage" and op.kind == "bytes"} == {A.CHW, A.HWC}
    assert sum(1 for op in ops if op.name == "stage" and op.args["from_prev"] and op.kind == "bytes") >= 3
    # every accepted tuning key; timing queries that return the stage count and ones that return nothing
    assert {op.args["key"] for op in ops if op.name == "set_tuning" and op.kind == "ok"} == set(A.TUNING)
    counts = {op.value for op in ops if op.name == "last_stage_ms"}
    assert 0 in counts and len(counts) >= 3


def test_images_are_small_mixed_and_of_every_channel_count_and_width_class(seqs):
    imgs = [op.args["img"] for s in seqs for op in s if op.name in ("pipeline", "stage") and op.args.get("img") is not None]
    assert all(im.shape[1] <= 150 and im.shape[2] <= 200 for im in imgs)
    assert {im.shape[3] for im in imgs} == {1, 2, 3, 4, 5}
    assert {im.shape[2] % 4 == 0 for im in imgs} == {True, False}
    big = [im for im in imgs if im.shape[2] >= 64]
    for im in big[:20]:         # left half smooth, right half noise (mean step of uniform bytes: 85)
        W = im.shape[2]
        step = lambda z: float(np.abs(np.diff(z.astype(np.int32), axis=2)).mean())  # noqa: E731
        assert 3 * step(im[:, :, : W // 2]) < step(im[:, :, W // 2:]) and step(im[:, :, W // 2:]) > 60, (im.shape, step(im[:, :, : W // 2]), step(im[:, :, W // 2:]))


def test_the_same_seed_gives_the_same_operations_and_the_same_expected_bytes(seqs):
    again = A.build_sequences()
    assert [len(s) for s in again] == [len(s) for s in seqs]
    assert A.digest(again) == A.digest(seqs)
    other = A.build_sequences(seed=7, contexts=2, fill=1)
    assert A.digest(other) != A.digest(seqs)


def test_references_agree_where_both_apply():
    """the host emulators against the C oracle on s / d / y lists (the model uses the oracle there and the emulators for e, h, o)"""
    rng = np.random.default_rng(3)
    for interval in (4, 5, 6):
        for u, last in ((1, False), (4, True), (3, True)):
            luts = [A.make_table(rng, interval, u * u, bool(k % 2)) for k in range(3)]
            img = A.natural_noise(1, 21, 30, 4, seed=interval)[0]
            assert np.array_equal(A._emul_stage(luts, "sdy", last, img, u, interval), A.ref_stage(luts, "sdy", last, img, u, interval))
