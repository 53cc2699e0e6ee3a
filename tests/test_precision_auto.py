"""precision = "auto" on the host side (no GPU, no library load): the setting, its threshold, what a copied engine keeps and the
binding of the four new entries (tests/test_cabi.py checks them against the built library)."""
import copy
import math

from coponerf_amd import _hip
from coponerf_amd.render import RenderEngine


def test_precision_auto_from_the_environment(monkeypatch):
    monkeypatch.setenv("COPONERF_PRECISION", "auto")
    eng = RenderEngine()
    assert eng.precision == "auto"
    assert "auto" in RenderEngine.PRECISIONS and {"f16", "f32"} <= set(RenderEngine.PRECISIONS)
    monkeypatch.delenv("COPONERF_PRECISION")
    assert RenderEngine().precision == "f16"               # the default is unchanged


def test_auto_threshold_default_and_deepcopy():
    eng = RenderEngine()
    assert eng.auto_threshold == RenderEngine.AUTO_THRESHOLD
    assert 0 < RenderEngine.AUTO_THRESHOLD < math.inf
    assert eng.last_exact_rays is None
    eng.precision, eng.auto_threshold = "auto", 0.125
    new = copy.deepcopy(eng)
    assert new.precision == "auto" and new.auto_threshold == 0.125
    eng.auto_threshold = math.inf
    assert copy.deepcopy(eng).auto_threshold == math.inf


def test_deepcopy_keeps_every_setting():
    eng = RenderEngine(chunk_rays=1300, lanes=3)
    eng.grad_scale_target, eng.call_lanes, eng.lazy_pixel_val = 64.0, 3, False
    eng.precision, eng.f32_chunk_rays, eng.auto_threshold = "f32", 1000, 0.25
    new = copy.deepcopy(eng)
    for name in ("chunk_rays", "lanes", "grad_scale_target", "call_lanes", "lazy_pixel_val", "precision", "f32_chunk_rays",
                 "auto_threshold"):
        assert getattr(new, name) == getattr(eng, name), name
    assert new._t32 is None and not new._ws and not new._w                 # caches are not copied


def test_guard_entries_are_bound():
    for name in ("cpn_logit_guard", "cpn_select_rays", "cpn_encode_hidden_f32_rays", "cpn_attend_hidden_f32_rays"):
        assert name in _hip.SIGNATURES and name in _hip.declared_symbols()
    assert len(_hip.SIGNATURES["cpn_encode_hidden_f32_rays"]) == len(_hip.SIGNATURES["cpn_encode_hidden_f32"]) + 1
    assert len(_hip.SIGNATURES["cpn_attend_hidden_f32_rays"]) == len(_hip.SIGNATURES["cpn_attend_hidden_f32"]) + 1
