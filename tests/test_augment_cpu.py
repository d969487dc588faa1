"""building_detection_amd.augment's host half (no GPU): the plan of data_enhancement.py's variants against the test-side
restatement (tests/_data_enhance_ref.py), the file order train_data_gen reads, refused name collisions, the rescale geometry."""
import random

import pytest

from building_detection_amd import _lib
from building_detection_amd import augment as A

import _data_enhance_ref as R

NAMES = ["1.png", "10.png", "2.tif", "7.png", "11.png"]


@pytest.mark.parametrize("seed", [0, 1, 5, 42, 1234])
def test_plan_matches_the_restated_draws(seed):
    names = list(NAMES)
    random.Random(99).shuffle(names)          # the plan draws in sorted order whatever order it is given
    got = A.plan(names, seed)
    want = R.enhance([(n, None, None) for n in names], random.Random(seed))
    assert [e.name for e in got] == sorted(want)
    for e in got:
        s, ud, lr, swap = want[e.name][2]
        assert A._stem(names[e.source]) + e.variant.suffix + ".png" == e.name
        assert (e.variant.scale, e.variant.flip_ud, e.variant.flip_lr, e.variant.swap_rb) == (s, ud, lr, swap)
    assert A.plan(names, seed) == got          # a seed fixes the plan


def test_plan_continues_one_random_sequence():
    """redraw=True's cycles: successive passes over one Random, as the restatement continued."""
    rng_a, rng_b = random.Random(3), random.Random(3)
    for _ in range(3):
        got = A._draw(NAMES, rng_a)
        want = R.enhance([(n, None, None) for n in NAMES], rng_b)
        assert [e.name for e in got] == sorted(want)
        assert [e.variant.scale for e in got] == [want[e.name][2][0] for e in got]


def test_virtual_names_sort_as_strings_and_interleave_sources():
    seen = 0
    for seed in range(20):
        p = A.plan(["1.png", "10.png"], seed)
        names = [e.name for e in p]
        assert names == sorted(names)
        assert names[:2] == ["1.png", "10.png"]            # '.' < '0' < '_': 1.png, 10.png, 10_*.png, 1_*.png
        if any(e.source == 0 for e in p[2:]):
            seen += 1
            first_1 = names.index(next(e.name for e in p[2:] if e.source == 0))
            assert all(e.source == 1 for e in p[1:first_1])  # a variant of "1" only after every entry of "10"
    assert seen > 0


@pytest.mark.parametrize("names", [["a.tif", "a.png"], ["a.png", "a_1.png"], ["x/a.b.png", "y/a.c.png"], ["b_4.png", "b.tif"]])
def test_colliding_virtual_names_raise(names):
    with pytest.raises(ValueError, match="augmented file name"):
        A.plan(names, 0)


def test_rescale_geometry():
    table = {0.6: (307, -102), 0.9: (460, -26), 1.0: (512, 0), 1.1: (563, 24), 1.5: (768, 127), 2.0: (1024, 255)}
    for s, want in table.items():
        assert A.scale_geometry(s) == want
    for k in range(6, 21):
        s = k / 10
        n, shift = A.scale_geometry(s)
        assert n == int(512 * s)
        assert n != 256 and 512 != 2 * n             # no factor reaches the exact-2x INTER_AREA path
        if s < 1:
            assert -shift + n <= 512 and shift < 0    # the pad leaves the resized tile inside the canvas
        else:
            assert 0 <= shift and shift + 512 <= n    # the crop window inside the resized tile


def test_items_of_each_variant():
    V = A.Variant
    assert A.item(V("", None, False, False, False), False, 3) == (3, 512, 0, 0)
    assert A.item(V("_1", None, True, False, False), True) == (0, 512, 0, _lib.SG_AUG_FLIP_UD)
    assert A.item(V("_2", None, False, True, False), False) == (0, 512, 0, _lib.SG_AUG_FLIP_LR)
    assert A.item(V("_3", 1.0, False, True, False), True) == (0, 512, 0, _lib.SG_AUG_FLIP_LR | _lib.SG_AUG_THRESHOLD)
    assert A.item(V("_3", 0.6, True, False, False), False) == (0, 307, -102, _lib.SG_AUG_FLIP_UD)
    assert A.item(V("_4", None, False, False, True), False) == (0, 512, 0, _lib.SG_AUG_SWAP_RB)
    assert A.item(V("_4", None, False, False, True), True) == (0, 512, 0, 0)   # the label of _4 is the source's
