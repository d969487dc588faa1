"""The host definition of the separation weight (data.separation_term, the generators' `separation` keyword) against the
brute force of tests/_separation_ref.py.  No GPU."""
import numpy as np
import pytest

from _separation_ref import INF, distances_ref, label8, weight_ref


def small_maps():
    rng = np.random.default_rng(11)
    maps = {"empty": np.zeros((9, 12), bool), "full": np.ones((7, 5), bool)}
    one = np.zeros((10, 10), bool)
    one[3:6, 2:5] = True
    maps["one_object"] = one
    two = np.zeros((8, 11), bool)
    two[2:6, 1:5] = True
    two[2:6, 6:10] = True                    # a one-pixel alley at column 5
    maps["one_pixel_apart"] = two
    diag = np.zeros((8, 8), bool)
    diag[1:4, 1:4] = True
    diag[4:7, 4:7] = True                    # touching diagonally: ONE object under 8-connectivity
    maps["diagonal_touch"] = diag
    for dens in (0.05, 0.2, 0.5):
        for k in range(3):
            h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
            maps[f"random_{dens}_{k}_{h}x{w}"] = rng.random((h, w)) < dens
    return maps


MAPS = small_maps()


def test_reference_knows_its_answers():
    """The brute force on hand-checked maps (everything else is held to it)."""
    d1, d2 = distances_ref(label8(MAPS["one_pixel_apart"]))
    assert d1[3, 5] == 1 and d2[3, 5] == 1            # the alley: both buildings one pixel away
    assert d1[3, 0] == 1 and d2[3, 0] == 36           # left of the left building: the other is 6 columns away
    assert d1[3, 2] == 0 and d2[3, 2] == 16           # on a building: d2 = the nearest OTHER building
    d1, d2 = distances_ref(label8(MAPS["one_object"]))
    assert (d2 == INF).all() and d1[0, 0] == 9 + 4
    d1, d2 = distances_ref(label8(MAPS["empty"]))
    assert (d1 == INF).all() and (d2 == INF).all()
    assert label8(MAPS["diagonal_touch"]).max() == 0 and label8(MAPS["diagonal_touch"], 4).max() == 1
    w = weight_ref(*distances_ref(label8(MAPS["one_pixel_apart"])), 10.0, 5.0)
    assert w[3, 2] == 0.0 and abs(w[3, 5] - 10.0 * np.exp(-4.0 / 50.0)) < 1e-15


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (7, 1), (9, 13), (5, 65), (4, 64), (3, 63), (12, 130)])
def test_two_candidates_per_row_suffice(h, w):
    """The kernels' algorithm (tests/_separation_port.py) against the all-pairs brute force: random maps with ties, object numbers
    that are anything but 0 ... n-1, both connectivities, with and without the second object."""
    from _separation_port import run
    rng = np.random.default_rng(h * 1000 + w)
    for dens in (0.0, 0.05, 0.2, 0.5, 1.0):
        for conn in (8, 4):
            lab = label8(rng.random((h, w)) < dens, conn)
            lab = np.where(lab >= 0, (lab.astype(np.int64) * 2654435761 + 3) % 0x7fffffff, -1)
            r1, r2 = distances_ref(lab)
            g1, g2 = run(lab, True)
            assert np.array_equal(g1, r1) and np.array_equal(g2, r2), (dens, conn)
            assert np.array_equal(run(lab, False)[0], r1), (dens, conn)


@pytest.mark.parametrize("w0,sigma", [(10.0, 5.0), (1.0, 0.5), (0.0, 3.0)])
@pytest.mark.parametrize("name", list(MAPS))
def test_separation_term_equals_the_brute_force(name, w0, sigma):
    from building_detection_amd.data import separation_term
    m = MAPS[name]
    ref = weight_ref(*distances_ref(label8(m)), w0, sigma)
    got = separation_term(m.astype(np.float32), w0, sigma)
    assert got.dtype == np.float64 and got.shape == m.shape
    # scipy's distance transform returns sqrt of the exact integer in float64, as the reference takes it: a few ulp of exp
    assert np.abs(got - ref).max() <= 1e-13 * (1.0 + w0), np.abs(got - ref).max()
    assert (got[m] == 0).all()
    if label8(m).max() < 1:
        assert (got == 0).all()


@pytest.mark.parametrize("bad", [(-1.0, 5.0), (10.0, 0.0), (10.0, -2.0), (float("nan"), 5.0), (10.0, float("inf")),
                                 (float("inf"), 1.0), (1.0,), "ab", 3.0])
def test_bad_parameters_are_refused(bad, tmp_path):
    from building_detection_amd import input_pipeline as IP
    from building_detection_amd.data import check_separation, separation_term
    with pytest.raises(ValueError, match="separation"):
        check_separation(bad)
    if isinstance(bad, tuple) and len(bad) == 2:
        with pytest.raises(ValueError, match="separation"):
            separation_term(np.zeros((4, 4)), *bad)
    with pytest.raises(ValueError, match="separation"):
        IP.train_data_gen([], [], 1, separation=bad)
    with pytest.raises(ValueError, match="separation"):
        IP.val_data_gen([], [], 1, separation=bad)


def test_separation_needs_the_edge_loss_channels():
    from building_detection_amd import input_pipeline as IP
    with pytest.raises(ValueError, match="separation"):
        IP.train_data_gen([], [], 1, loss="focal_loss", separation=(10.0, 5.0))


def test_host_generator_channel_2_with_and_without_separation(tmp_path):
    """train_data_gen without `separation` yields what it always did; with it, channel 2 gains the brute-force term on the
    background between the two buildings of the tile and nothing else changes."""
    from PIL import Image
    from building_detection_amd import input_pipeline as IP
    rng = np.random.default_rng(5)
    lab = np.zeros((512, 512), np.uint8)
    lab[100:140, 60:120] = 255
    lab[100:140, 124:180] = 255              # a 4-pixel alley
    lab[300:330, 300:340] = 255
    lab[200, 200] = 128                      # grey: not a building
    pi, pl = tmp_path / "i0.png", tmp_path / "l0.png"
    Image.fromarray(rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8)).save(pi)
    Image.fromarray(lab).save(pl)
    x0, y0 = next(IP.train_data_gen([str(pi)], [str(pl)], 1))
    x1, y1 = next(IP.train_data_gen([str(pi)], [str(pl)], 1, separation=None))
    x2, y2 = next(IP.train_data_gen([str(pi)], [str(pl)], 1, separation=(10.0, 5.0)))
    assert y0.dtype == y2.dtype == np.float64 and y2.shape == (1, 512, 512, 4)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(x0, x2)
    assert np.array_equal(y0[..., [0, 1, 3]], y2[..., [0, 1, 3]])
    # the reference on a crop that holds everything within reach (the term is below 1e-300 beyond): the two near buildings
    crop = (slice(60, 180), slice(20, 220))
    ref = weight_ref(*distances_ref(label8(lab[crop] == 255)), 10.0, 5.0)
    term = (y2 - y0)[0, ..., 2]
    assert (term >= 0).all() and (term[lab == 255] == 0).all()
    assert abs(term[120, 121] - 10.0 * np.exp(-((2 + 3) ** 2) / 50.0)) < 1e-12      # in the alley: 2 px and 3 px away
    # far from the crop's edge the third building (200 px away) cannot be second-nearest: the crop's answer is the tile's
    inner = (slice(80, 160), slice(40, 200))
    got_in = term[inner]
    ref_in = ref[20:100, 20:180]
    assert np.abs(got_in - ref_in).max() <= 1e-12, np.abs(got_in - ref_in).max()
    assert term.max() > 5.0 and y2[0, ..., 2].max() > 2.0
