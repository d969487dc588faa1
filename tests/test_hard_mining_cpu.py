"""Hard-pixel mining without a GPU: what losses.hard_mining takes and refuses, the min_kept arithmetic, what the resolve_*
functions and compile() make of a mined loss, the float64 reference (tests/_hard_mining_ref.py) against a full sort and against
central differences, and the binding's table."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _hard_mining_ref as HR
import _multiclass_ref as MR

FD_BOUND = 1e-7   # of max |grad|, as tests/test_region_loss_cpu.py: h = 1e-6 in float64, p >= 0.012


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_hard_mining_arguments():
    from building_detection_amd import losses as LS
    m = LS.hard_mining(LS.edge_focal_loss)
    assert (m.thresh, m.min_kept, m.__name__) == (0.7, 0.1, "hard_mining(edge_focal_loss)") and m.pointwise is LS.edge_focal_loss
    w = LS.focal_loss.with_alpha([0.2, 0.3, 0.5])
    m = LS.hard_mining(w, thresh=0, min_kept=100)
    assert (m.thresh, m.min_kept, m.__name__) == (0.0, 100, "hard_mining(focal_loss)") and m.pointwise is w
    assert isinstance(m.min_kept, int) and isinstance(LS.hard_mining(LS.focal_loss, min_kept=np.int64(3)).min_kept, int)
    assert LS.hard_mining(LS.binary_crossentropy, thresh=1, min_kept=1.0).min_kept == 1.0
    assert isinstance(LS.hard_mining(LS.binary_crossentropy, min_kept=1.0).min_kept, float)      # 1.0 is the whole batch, 1 one pixel
    assert isinstance(LS.hard_mining(LS.binary_crossentropy, min_kept=np.float32(0.5)).min_kept, float)
    with pytest.raises(RuntimeError, match="compile"):
        m(None, None)
    for bad in ("focal_loss", LS.dice_loss, LS.PA, None, m, LS.compound(LS.focal_loss, LS.dice_loss)):
        with pytest.raises(ValueError, match="pointwise"):
            LS.hard_mining(bad)
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="thresh"):
            LS.hard_mining(LS.focal_loss, thresh=bad)
    for bad in (0, -1, 0.0, -0.5, 1.5, 2.0, float("nan"), float("inf"), "x", None, True, [1]):
        with pytest.raises(ValueError, match="min_kept"):
            LS.hard_mining(LS.focal_loss, min_kept=bad)


@pytest.mark.parametrize("rows", (1, 7, 1000))
def test_min_kept_fraction_and_count(rows):
    from building_detection_amd import losses as LS
    for f in (1e-9, 0.001, 0.1, 1 / 3, 0.5, 0.999, 1.0):
        k = LS.mined_rows(f, rows)
        assert k == min(rows, max(1, math.ceil(f * rows))) and 1 <= k <= rows, (f, rows, k)
    assert LS.mined_rows(1.0, rows) == rows and LS.mined_rows(1e-9, rows) == 1
    assert LS.mined_rows(0.1, rows) == {1: 1, 7: 1, 1000: 100}[rows]
    assert LS.mined_rows(1 / 3, rows) == {1: 1, 7: 3, 1000: 334}[rows]
    for n in (1, 2, 7, 999, 1000, 1001, 10 ** 12):
        assert LS.mined_rows(n, rows) == min(rows, n)
    assert LS.mined_rows(1, rows) == 1                                     # the int 1 is one pixel, not the whole batch


def test_resolve_functions_for_two_and_three_classes():
    from building_detection_amd import losses as LS
    from building_detection_amd._lib import SG_LOSS_CE2, SG_LOSS_FOCAL, SG_LOSS_EDGE_FOCAL
    for l in (LS.binary_crossentropy, LS.focal_loss, LS.edge_focal_loss, "focal_loss", LS.dice_loss,
              LS.compound(LS.focal_loss, LS.dice_loss)):
        assert LS.resolve_mining(l, 2) is None
    m = LS.hard_mining(LS.edge_focal_loss, 0.6, 0.25)
    assert LS.resolve_loss(m) == SG_LOSS_EDGE_FOCAL and LS.resolve_region(m, 2) is None and LS.resolve_alpha(m, 2) is None
    assert LS.resolve_mining(m, 2) == dict(kind=SG_LOSS_EDGE_FOCAL, alpha=(0.35, 0.65), thresh=0.6, min_kept=0.25)
    m = LS.hard_mining(LS.focal_loss, min_kept=500)
    assert LS.resolve_loss(m) == SG_LOSS_FOCAL
    assert LS.resolve_mining(m, 2) == dict(kind=SG_LOSS_FOCAL, alpha=(0.5, 0.5), thresh=0.7, min_kept=500)
    assert LS.resolve_mining(m, 3)["alpha"] == (0.5,) * 3 == LS.resolve_alpha(m, 3)
    m = LS.hard_mining(LS.binary_crossentropy)
    assert LS.resolve_loss(m) == SG_LOSS_CE2 and LS.resolve_alpha(m, 3) is None
    assert LS.resolve_mining(m, 3) == dict(kind=SG_LOSS_CE2, alpha=None, thresh=0.7, min_kept=0.1)
    w3 = (0.2, 0.3, 0.5)
    m = LS.hard_mining(LS.edge_focal_loss.with_alpha(w3), thresh=1.0)
    assert LS.resolve_mining(m, 3) == dict(kind=SG_LOSS_EDGE_FOCAL, alpha=w3, thresh=1.0, min_kept=0.1) and LS.resolve_alpha(m, 3) == w3
    with pytest.raises(ValueError, match="class weights"):
        LS.resolve_mining(m, 2)
    with pytest.raises(ValueError, match="with_alpha"):
        LS.resolve_mining(LS.hard_mining(LS.edge_focal_loss), 3)


def test_compound_refuses_a_mined_term():
    from building_detection_amd import losses as LS
    with pytest.raises(ValueError, match="mined pointwise term inside a compound is not implemented"):
        LS.compound(LS.hard_mining(LS.focal_loss), LS.dice_loss)


def test_compile_stores_the_mining_fields():
    from building_detection_amd import losses as LS, zoo
    m = zoo.HRNet((32, 32, 3), num_classes=3)
    m.compile(loss=LS.hard_mining(LS.focal_loss, 0.5, 64), metrics=[LS.MIoU])
    assert m.loss_kind == 1 and m.loss_region is None
    assert m.loss_mining == dict(kind=1, alpha=(0.5,) * 3, thresh=0.5, min_kept=64) and m.last_hard_mining() is None
    m.compile(loss=LS.focal_loss)
    assert m.loss_mining is None and m.last_hard_mining() is None
    m2 = zoo.HRNet((32, 32, 3))
    m2.compile(loss=LS.hard_mining(LS.edge_focal_loss))
    assert m2.loss_mining["alpha"] == (0.35, 0.65) and m2.loss_alpha is None


def test_descriptor_binding():
    from building_detection_amd import losses as LS
    from building_detection_amd import _lib
    from building_detection_amd.ops import Engine
    assert ctypes.sizeof(_lib.MineDesc) == 4 * 4 + 2 * 8 + 4 + 4 * _lib.SG_MAX_CLASSES + 4     # 4 bytes of tail padding
    names = _lib.exported_symbols()
    for s in ("sg_loss_mined_ws_bytes", "sg_loss_mined_fwd", "sg_loss_mined_bwd"):
        assert s in names
    p, y6, y3 = torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 6), torch.zeros(2, 8, 8, 3)
    r = LS.resolve_mining(LS.hard_mining(LS.edge_focal_loss.with_alpha([0.2, 0.3, 0.5]), 0.25, 0.1), 3)
    d = Engine.mine_desc(r, p, y6)
    assert (d.C, d.y_cols, d.kind, d.reserved, d.rows, d.min_kept, d.thresh) == (3, 6, 2, 0, 128, 13, 0.25)
    assert [round(v, 6) for v in list(d.alpha)[:4]] == [0.2, 0.3, 0.5, 0.0]
    with pytest.raises(ValueError, match="edge_focal_loss needs"):
        Engine.mine_desc(r, p, y3)
    r = LS.resolve_mining(LS.hard_mining(LS.binary_crossentropy, min_kept=1000), 3)
    assert Engine.mine_desc(r, p, y3).min_kept == 128
    with pytest.raises(ValueError, match="does not go with"):
        Engine.mine_desc(r, p, torch.zeros(2, 8, 8, 4))


@pytest.mark.parametrize("C", (2, 5))
def test_reference_against_a_full_sort(C):
    rows = 501
    g = gen(7 + C)
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, 2 * C)
    p[::9] = p[3]                                                   # ties
    keys = HR.keys_ref(p, yt, C)
    t = yt[:, :C].argmax(1)
    assert np.array_equal(keys, p[torch.arange(rows), t].numpy())   # in (0, 1): the clamp changes nothing
    order = np.sort(keys, kind="stable")
    for k in (1, 2, rows // 3, rows - 1, rows):
        for thresh in (0.0, 0.3, float(order[k - 1]), 0.9, 1.0):
            T, keep = HR.select_ref(keys, thresh, k)
            assert T == max(np.float32(thresh), order[k - 1]) and T.dtype == np.float32
            n = int(np.searchsorted(order, T, side="right"))        # every key <= T, ties included
            assert keep.sum() == n >= k and np.array_equal(keep, keys <= T)
            for kind in (0, 1, 2):
                alpha = None if kind == 0 else tuple(0.2 + 0.1 * c for c in range(C))
                r = HR.mined_ref(kind, p, yt, alpha, thresh, k)
                l = HR.row_terms(kind, p.double(), yt.double(), alpha)
                srt = torch.from_numpy(np.argsort(keys, kind="stable"))[:n]
                assert r["n_kept"] == n and r["T_bits"] == HR.bits(T)
                assert abs(r["loss"].item() - l[srt].sum().item() / n) <= 1e-12 * abs(r["loss"].item())
    full = HR.mined_ref(2, p, yt, (0.35,) * C, 1.0, 1)              # thresh = 1: the plain loss
    assert full["n_kept"] == rows
    assert abs(full["loss"].item() - MR.loss_ref(2, p.double(), yt.double(), (0.35,) * C).item()) <= 1e-12
    # the clamp and the NaN rule
    pz = p.clone()
    pz[0, t[0]], pz[1, t[1]], pz[2, t[2]], pz[3, t[3]] = float("nan"), -0.0, 1.5, -2.0
    kz = HR.keys_ref(pz, yt, C)
    assert [HR.bits(v) for v in kz[:4]] == [0, 0, 0x3F800000, 0]


def test_reference_gradient_against_central_differences():
    rows, C, k, thresh = 50, 3, 17, 0.2
    g = gen(50)
    p32, yt = MR.class_probs(g, rows, C, -1.5, 1.5), MR.class_labels(g, rows, C, 2 * C)
    alpha = (0.2, 0.5, 0.8)
    for kind in (0, 1, 2):
        r = HR.mined_ref(kind, p32, yt, alpha, thresh, k)
        assert k <= r["n_kept"] < rows
        p = p32.double()
        h, fd = 1e-6, torch.zeros(rows, C, dtype=torch.float64)
        for i in range(rows):
            for c in range(C):
                hi, lo = p.clone(), p.clone()
                hi[i, c] += h
                lo[i, c] -= h
                fd[i, c] = (HR.mined_ref(kind, p32, yt, alpha, thresh, k, p64=hi)["loss"]
                            - HR.mined_ref(kind, p32, yt, alpha, thresh, k, p64=lo)["loss"]).item() / (2 * h)
        err, scale = (r["grad"] - fd).abs().max().item(), r["grad"].abs().max().item()
        print(f"kind={kind}: max |grad - fd| = {err:.3e} = {err / scale:.2e} of max |grad| {scale:.3e}")
        assert err <= FD_BOUND * scale
        assert (r["grad"][~r["kept"]] == 0).all() and (fd[~r["kept"]] == 0).all()
        assert torch.allclose(HR.mined_ref(kind, p32, yt, alpha, thresh, k, scale=0.25)["grad"], 0.25 * r["grad"], rtol=1e-15, atol=0)
