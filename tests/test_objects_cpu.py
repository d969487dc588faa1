"""objects.match / ObjectScores (pure host code, exact integers) against the plain-loop restatement of tests/_objects_ref.py and
against answers worked out by hand.  The restatement itself is checked on a map small enough to read."""
import math
from fractions import Fraction

import numpy as np
import pytest

from _objects_ref import label_ref, match_ref, overlaps_ref, scores_ref
from building_detection_amd import objects as OB


def table(*objs):
    """objs: (area, value) -> table rows; only area and value matter to the matching."""
    return np.array([[k, a, 0, 0, 0, 0, v, 0] for k, (a, v) in enumerate(objs)], np.int32).reshape(-1, 8)


def both(pairs, tp, tt, **kw):
    """The product's answer, after holding it to the restatement's."""
    pairs = np.array(pairs, np.int32).reshape(-1, 3)
    got_m, got_c = OB.match(pairs, tp, tt, **kw)
    ref_m, ref_c = match_ref(pairs, tp, tt, **kw)
    assert [tuple(r) for r in got_m.tolist()] == ref_m
    assert got_c == ref_c
    return [tuple(r) for r in got_m.tolist()], got_c


def test_restatement_on_a_readable_map():
    m = np.array([[1, 1, 0, 2],
                  [0, 1, 2, 2],
                  [3, 0, 0, 1]], np.uint8)
    lab, tab = label_ref(m, 8)
    assert lab.tolist() == [[0, 0, -1, 1], [-1, 0, 1, 1], [2, -1, -1, 3]]
    assert tab.tolist() == [[0, 3, 0, 0, 1, 1, 1, 0], [3, 3, 2, 0, 3, 1, 2, 0], [8, 1, 0, 2, 0, 2, 3, 0], [11, 1, 3, 2, 3, 2, 1, 0]]
    d = np.array([[255, 0], [0, 255]], np.uint8)                      # a diagonal: one object at 8, two at 4
    assert len(label_ref(d, 8)[1]) == 1 and len(label_ref(d, 4)[1]) == 2
    assert label_ref(d.astype(np.float32) / 255, 8)[1][0, 6] == 255   # not uint8: binary
    assert label_ref(np.zeros((3, 4), np.uint8))[1].shape == (0, 8)
    other = np.array([[1, 0, 0, 2], [1, 1, 2, 0], [0, 0, 0, 0]], np.uint8)
    assert overlaps_ref(lab, label_ref(other, 8)[0]).tolist() == [[0, 0, 2], [1, 1, 2]]
    assert overlaps_ref(lab, np.full_like(lab, -1)).shape == (0, 3)


def test_iou_exactly_one_half_matches_and_three_of_six_does_not():
    tp, tt = table((6, 255)), table((6, 255))
    m, c = both([(0, 0, 4)], tp, tt, iou=0.5)          # 4 / (6 + 6 - 4) = 1/2: '>=' is inclusive
    assert m == [(0, 0, 4, 8)] and (c["tp"], c["fp"], c["fn"]) == (1, 0, 0)
    m, c = both([(0, 0, 3)], tp, tt, iou=0.5)          # 3 / 9
    assert m == [] and (c["tp"], c["fp"], c["fn"]) == (0, 1, 1)
    # a threshold that binary floating point cannot hold is still taken at its decimal value: 1/10 >= 0.1, and 3/10 >= 0.3
    assert both([(0, 0, 1)], table((5, 255)), table((6, 255)), iou=0.1)[1]["tp"] == 1
    assert both([(0, 0, 3)], table((6, 255)), table((7, 255)), iou=0.3)[1]["tp"] == 1
    assert both([(0, 0, 3)], table((6, 255)), table((7, 255)), iou=Fraction(3, 10))[1]["tp"] == 1
    with pytest.raises(ValueError):
        OB.match(np.zeros((0, 3)), tp, tt, iou=0)
    with pytest.raises(ValueError):
        OB.match(np.zeros((0, 3)), tp, tt, iou=1.5)


def test_greedy_one_prediction_over_two_truths():
    tp, tt = table((100, 255)), table((60, 255), (50, 255))
    # IoU 55/105 against truth 0, 45/105 against truth 1: at 0.3 both qualify, the better one wins, truth 1 is a miss
    m, c = both([(0, 0, 55), (0, 1, 45)], tp, tt, iou=0.3)
    assert m == [(0, 0, 55, 105)] and (c["tp"], c["fp"], c["fn"]) == (1, 0, 1)
    # equal IoU: the tie goes to the smaller (p, t)
    m, c = both([(0, 1, 50), (0, 0, 50)], table((100, 255)), table((50, 255), (50, 255)), iou=0.3)
    assert m == [(0, 0, 50, 100)]


def test_two_predictions_compete_for_one_truth_at_0_3():
    tp, tt = table((40, 255), (50, 255)), table((80, 255))
    # 30/90 = 1/3 and 45/85: both above 0.3, prediction 1 takes the truth, prediction 0 becomes a false positive
    m, c = both([(0, 0, 30), (1, 0, 45)], tp, tt, iou=0.3)
    assert m == [(1, 0, 45, 85)] and (c["tp"], c["fp"], c["fn"]) == (1, 1, 0)
    # the loser may still take another truth further down the list
    tt2 = table((80, 255), (40, 255))
    m, c = both([(0, 0, 30), (1, 0, 45), (0, 1, 10)], table((40, 255), (50, 255)), tt2, iou=0.1)
    assert m == [(1, 0, 45, 85), (0, 1, 10, 70)] and (c["tp"], c["fp"], c["fn"]) == (2, 0, 0)


def test_small_truths_are_ignored_with_their_matches():
    tp = table((12, 255), (200, 255), (9, 255), (300, 255))
    tt = table((10, 255), (210, 255), (8, 255))
    pairs = [(0, 0, 9), (1, 1, 190)]
    m, c = both(pairs, tp, tt, iou=0.5, min_area_truth=50, min_area_pred=50)
    assert m == [(1, 1, 190, 220), (0, 0, 9, 13)]              # the small truth still takes part in the matching ...
    assert (c["tp"], c["fp"], c["fn"]) == (1, 1, 0)             # ... but neither it nor its match counts; truth 2 (8 px) is
    #                                                             no miss, prediction 2 (9 px, unmatched) no false alarm,
    #                                                             prediction 3 (300 px, unmatched) is one
    m, c = both(pairs, tp, tt, iou=0.5)
    assert (c["tp"], c["fp"], c["fn"]) == (2, 2, 1)
    # a small prediction matched to a counted truth counts
    m, c = both([(0, 0, 30)], table((30, 255)), table((60, 255)), iou=0.5, min_area_pred=50)
    assert (c["tp"], c["fp"], c["fn"]) == (1, 0, 0)


def test_pairs_of_different_value_never_match():
    tp, tt = table((80, 1), (80, 2)), table((80, 2), (80, 1), (20, 3))
    m, c = both([(0, 0, 50), (1, 1, 50), (0, 1, 30), (1, 0, 30)], tp, tt, iou=0.2)
    assert m == [(0, 1, 30, 130), (1, 0, 30, 130)]              # the larger overlaps are of the wrong class
    assert c["per_class"] == {1: {"tp": 1, "fp": 0, "fn": 0}, 2: {"tp": 1, "fp": 0, "fn": 0}, 3: {"tp": 0, "fp": 0, "fn": 1}}
    assert (c["tp"], c["fp"], c["fn"]) == (2, 0, 1)


def test_empty_sides_give_nan_ratios_and_right_counts():
    none = np.zeros((0, 8), np.int32)
    for tp, tt, want in ((none, table((30, 255), (40, 255)), (0, 0, 2)), (table((30, 255)), none, (0, 1, 0)), (none, none, (0, 0, 0))):
        m, c = both([], tp, tt)
        assert m == [] and (c["tp"], c["fp"], c["fn"]) == want
        s = OB.ObjectScores()
        s.add(m, c, tt)
        r = s.result()
        assert (r["tp"], r["fp"], r["fn"]) == want
        assert math.isnan(r["mean_iou"])
        assert math.isnan(r["precision"]) == (want[0] + want[1] == 0)
        assert math.isnan(r["recall"]) == (want[0] + want[2] == 0)
        assert math.isnan(r["f1"]) == (sum(want) == 0)
        if not math.isnan(r["f1"]):
            assert r["f1"] == 0.0
    assert "per_class" not in r


def test_object_scores_over_three_updates():
    rng = np.random.default_rng(5)
    scenes = []
    s = OB.ObjectScores(iou=0.4, min_area_truth=120)
    for _ in range(3):
        n_p, n_t = int(rng.integers(5, 30)), int(rng.integers(5, 30))
        tp = table(*[(int(a), int(v)) for a, v in zip(rng.integers(100, 20000, n_p), rng.integers(1, 3, n_p))])
        tt = table(*[(int(a), int(v)) for a, v in zip(rng.integers(100, 20000, n_t), rng.integers(1, 3, n_t))])
        seen, pairs = set(), []
        for _ in range(60):
            p, t = int(rng.integers(0, n_p)), int(rng.integers(0, n_t))
            if (p, t) in seen:
                continue
            seen.add((p, t))
            pairs.append((p, t, int(rng.integers(1, min(tp[p, 1], tt[t, 1]) + 1))))
        m, c = both(pairs, tp, tt, iou=0.4, min_area_truth=120)
        s.add(m, c, tt)
        scenes.append((m, c, tt))
    r, want = s.result(), scores_ref(scenes, 0.4, OB.AREA_BINS, 120)
    assert r["tp"] > 0 and r["fp"] > 0 and r["fn"] > 0, "the case is meant to have all three"
    for k in ("tp", "fp", "fn", "precision", "recall", "f1", "mean_iou"):
        assert r[k] == want[k], k
    assert [b["tp"] for b in r["bins"]] == want["bin_tp"] and [b["fn"] for b in r["bins"]] == want["bin_fn"]
    assert sum(want["bin_tp"]) == r["tp"] and sum(want["bin_fn"]) == r["fn"]
    assert [(b["lo"], b["hi"]) for b in r["bins"]] == [(0, 150), (150, 300), (300, 3000), (3000, 8000), (8000, 15000), (15000, None)]
    for b in r["bins"]:
        n = b["tp"] + b["fn"]
        assert (math.isnan(b["recall"]) and n == 0) or b["recall"] == b["tp"] / n
    assert set(r["per_class"]) == {1, 2} and sum(v["tp"] for v in r["per_class"].values()) == r["tp"]
    assert r["scenes"] == 3
    # the sum of the three scenes' counts is all the accumulator knows: one scene holding all of them says the same
    one = OB.ObjectScores(iou=0.4, min_area_truth=120)
    shift_t, all_m, all_t = 0, [], []
    for m, c, tt in scenes:
        all_m += [(p, t + shift_t, i, u) for p, t, i, u in m]
        all_t.append(tt)
        shift_t += len(tt)
    total = {k: sum(c[k] for _, c, _ in scenes) for k in ("tp", "fp", "fn")}
    total["per_class"] = {v: {k: sum(c["per_class"].get(v, {}).get(k, 0) for _, c, _ in scenes) for k in ("tp", "fp", "fn")}
                          for v in (1, 2)}
    one.add(all_m, total, np.concatenate(all_t))
    r1 = one.result()
    r1.pop("scenes"), r.pop("scenes")
    assert repr(r1) == repr(r)                                  # repr: an empty bin's recall is nan, which equals nothing


def test_bins_edges_are_inclusive_below():
    s = OB.ObjectScores(bins=(150, 300))
    tt = table((149, 255), (150, 255), (299, 255), (300, 255))
    m, c = OB.match(np.array([(0, 1, 150)]), table((150, 255)), tt)
    s.add(m, c, tt)
    r = s.result()
    assert [(b["tp"], b["fn"]) for b in r["bins"]] == [(0, 1), (1, 1), (0, 1)]
    assert r["mean_iou"] == 1.0 and r["recall"] == 0.25 and r["precision"] == 1.0
    with pytest.raises(ValueError):
        OB.ObjectScores(bins=(300, 150))


def test_objects_module_has_no_host_labeller():
    import os
    src = open(os.path.join(os.path.dirname(OB.__file__), "objects.py")).read()
    assert "scipy" not in src and "ndimage" not in src
