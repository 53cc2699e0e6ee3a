"""tests/lpips_ref.py (the float64 restatement of LPIPS-VGG that tests/test_gpu_lpips.py measures against) and the weight
loading of coponerf_amd.lpips, on the CPU.

The seeded defects calibrate the end-to-end bar of the GPU test: |d| <= 5e-5 (half a unit of the fourth decimal test.py:300
prints).  Every plausible mistake in the implementation must cost at least 100 x that on the shapes the GPU test uses, or the
bar could not tell it from rounding."""
import pytest
import torch

from coponerf_amd import lpips as cl
from tests import lpips_ref as lr

E2E_BAR = 5e-5
SEED = 3


def test_identical_images_give_exactly_zero():
    p, t = lr.make_images(2, 16, 20, seed=1)
    d, layers, _ = lr.lpips64(t.clone(), t, SEED)           # in range: the clamp is the identity
    assert d.tolist() == [0.0, 0.0] and bool((layers == 0).all())
    d, _, _ = lr.lpips64(p, t, SEED)
    assert bool((d > 1e-3).all()) and bool(torch.isfinite(d).all())


def test_zero_feature_vectors():
    w = torch.tensor([0.5, 0.25, 2.0], dtype=torch.float64)
    fp = torch.zeros(1, 3, 2, 2, dtype=torch.float64)
    ft = torch.zeros(1, 3, 2, 2, dtype=torch.float64)
    d, _ = lr.head64(fp, ft, w)
    assert d.tolist() == [0.0]                              # zero in both maps: 0 / (0 + 1e-10) = 0, no NaN
    ft[0, :, 0, 1] = torch.tensor([3.0, 0.0, 4.0])          # zero in one map: sum_c w_c b_c^2 of that pixel, over 4 pixels
    d, _ = lr.head64(fp, ft, w)
    b = torch.tensor([3.0, 0.0, 4.0], dtype=torch.float64) / (5.0 + 1e-10)
    assert d.item() == pytest.approx(float((w * b * b).sum()) / 4, rel=1e-14)


def _full_layout(tv):
    """torchvision + lin keys -> the key layout of lpips.LPIPS(net='vgg').state_dict()."""
    full = {"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)}
    for key, v in tv.items():
        if key.startswith("features."):
            i = int(key.split(".")[1])
            full[f"net.slice{cl._slice_of(i)}.{i}.{key.split('.')[2]}"] = v
        else:
            full[key] = v
            full["lins." + key[3:]] = v                     # lin0.model.1.weight is also lins.0.model.1.weight
    return full


def test_both_key_layouts_load_identical_tensors(tmp_path):
    tv = cl.synthetic_state_dict(SEED)
    want = cl.parse_state_dict(tv)
    assert [tuple(w.shape) for w in want[0]] == [(co, ci, 3, 3) for ci, co in cl.CONV_CHANNELS]
    assert [tuple(l.shape) for l in want[2]] == [(c,) for c in cl.TAP_CHANNELS]
    vgg = {k: v for k, v in tv.items() if k.startswith("features.")}
    lin = {k: v for k, v in tv.items() if k.startswith("lin")}
    assert all(tuple(v.shape) == (1, c, 1, 1) for v, c in zip(lin.values(), cl.TAP_CHANNELS))
    full = _full_layout(tv)
    assert [cl._slice_of(i) for i in cl.CONV_INDICES] == [1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5]
    assert "net.slice3.14.bias" in full and "lins.4.model.1.weight" in full
    flat = {k: v.reshape(-1) for k, v in lin.items()}                      # (C,) is accepted as well
    for got in (cl.parse_state_dict(vgg, lin), cl.parse_state_dict(full), cl.parse_state_dict(vgg, flat)):
        for a, b in zip(sum(want, []), sum(got, [])):
            assert torch.equal(a, b)
    # through files, and into the module's buffers
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    torch.save(full, tmp_path / "full.pth")
    mods = [cl.LPIPS.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")), cl.LPIPS.from_files(str(tmp_path / "full.pth")),
            cl.LPIPS.synthetic(SEED)]
    for m in mods[1:]:
        assert list(m.state_dict()) == list(mods[0].state_dict())
        for a, b in zip(m.state_dict().values(), mods[0].state_dict().values()):
            assert torch.equal(a, b)
    assert torch.equal(mods[0].w14, want[0][6]) and torch.equal(mods[0].lin4, want[2][4])
    assert not any(p.requires_grad for p in mods[0].parameters())


def test_missing_and_misshaped_keys_are_named():
    tv = cl.synthetic_state_dict(SEED)
    with pytest.raises(ValueError, match=r"features\.17\.bias"):
        cl.LPIPS.from_state_dict({k: v for k, v in tv.items() if k != "features.17.bias"})
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        cl.LPIPS.from_state_dict({k: v for k, v in tv.items() if k != "lin2.model.1.weight"})
    with pytest.raises(ValueError, match=r"net\.slice4\.19\.weight"):
        full = _full_layout(tv)
        del full["net.slice4.19.weight"]
        cl.LPIPS.from_state_dict(full)
    bad = dict(tv)
    bad["features.5.weight"] = bad["features.5.weight"][:, :32]
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 3, 3\)"):
        cl.LPIPS.from_state_dict(bad)
    with pytest.raises(RuntimeError, match="HIP device only"):             # no CPU path
        cl.LPIPS.synthetic(SEED)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_synthetic_weights_are_a_function_of_the_seed():
    a, b, c = cl.synthetic_state_dict(5), cl.synthetic_state_dict(5), cl.synthetic_state_dict(6)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["features.0.weight"], c["features.0.weight"])
    w = a["features.10.weight"]
    assert abs(float(w.std()) - (2.0 / (9 * 128)) ** 0.5) < 0.02 * (2.0 / (9 * 128)) ** 0.5
    assert float(a["lin3.model.1.weight"].min()) >= 0.0 and float(a["lin3.model.1.weight"].max()) < 1.0


def test_round_trip_is_done_in_fp32():
    x = torch.tensor([0.3333333, -0.7777777, 1.0, -1.0, 1e-8], dtype=torch.float32)
    got = lr.round_trip32(x)
    want = ((x.double() + 1.0) * 0.5).float()               # the one rounding that matters; - 0.5 and * 2 are then exact
    assert torch.equal(got, ((want.double() - 0.5) * 2.0).float()) and got[4].item() == 0.0      # 1 + 1e-8 rounds to 1


# defect -> the end-to-end case of the GPU test it is seeded on (without that test's identical pair: every image must move)
DEFECT_CASES = {"pad_before_scale": "16x16", "shift_sign": "16x16", "tap_early": "16x16", "channel_mean": "16x16", "mis_split": "16x16",
                "ceil_pool": "20x28", "clamp_target": "20x28"}


@pytest.mark.parametrize("defect", lr.DEFECTS)
def test_seeded_defects_move_the_distance_far_beyond_the_bar(defect):
    H, W, kw = lr.CASES[DEFECT_CASES[defect]]
    p, t = lr.make_images(3, H, W, seed=11, **kw)
    clean, _, _ = lr.lpips64(p, t, SEED)
    broken, _, _ = lr.lpips64(p, t, SEED, defect=defect)
    moved = (broken - clean).abs()
    print(f"{defect}: 3 x {H} x {W}  lpips {[round(v, 4) for v in clean.tolist()]}  moved {[f'{v:.2e}' for v in moved.tolist()]}"
          f"  = {[round(v) for v in (moved / E2E_BAR).tolist()]} bars")
    assert bool((moved >= 100 * E2E_BAR).all()), (defect, moved.tolist())
