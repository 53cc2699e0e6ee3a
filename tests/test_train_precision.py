"""train_precision on the host side (no GPU): the setting, its environment variable, its check in render_train, what a copied
engine keeps, and the binding of the two backward entries of the f32 training mode (tests/test_gpu_train_f32.py runs them)."""
import copy
import inspect

import pytest
import torch

from coponerf_amd import _hip
from coponerf_amd.render import RenderEngine


def test_train_precision_default_and_environment(monkeypatch):
    monkeypatch.delenv("COPONERF_TRAIN_PRECISION", raising=False)
    assert RenderEngine().train_precision == "f16"
    assert RenderEngine.TRAIN_PRECISIONS == ("f16", "f32")
    monkeypatch.setenv("COPONERF_TRAIN_PRECISION", "f32")
    eng = RenderEngine()
    assert eng.train_precision == "f32"
    assert eng.precision == "f16"                          # the inference setting is a separate one


def test_bad_train_precision_is_rejected_before_device_work():
    eng = RenderEngine()
    eng.train_precision = "auto"
    B, R, S, H = 1, 4, 8, 16
    eye = torch.eye(4).expand(B, 2, 4, 4)
    z = [torch.zeros(2 * B, 8, H, H) for _ in range(4)]
    with pytest.raises(ValueError, match="train_precision"):
        eng.render_train({}, eye, eye, eye[:, :1], eye[:, :1], torch.zeros(B, 1, R, 2), z, eye[:, :1], False, S, H, H)
    assert not eng._ws and eng._w == {}


def test_deepcopy_keeps_train_precision():
    eng = RenderEngine()
    eng.train_precision, eng.precision = "f32", "auto"
    new = copy.deepcopy(eng)
    assert new.train_precision == "f32" and new.precision == "auto"
    assert "train_precision" in RenderEngine.SETTINGS


def test_f32_training_entries_are_bound_and_declared():
    declared = _hip.declared_symbols()
    for name in ("cpn_attend_hidden_bwd_f32", "cpn_gemm_f16_combine_hs"):
        assert name in _hip.SIGNATURES and name in declared, name
    # the hs form of the combine takes exactly the arguments of the hid form
    assert _hip.SIGNATURES["cpn_gemm_f16_combine_hs"] == _hip.SIGNATURES["cpn_gemm_f16_combine"]
    # the f32 attention backward: the fp16 form's arguments without dhid
    assert len(_hip.SIGNATURES["cpn_attend_hidden_bwd_f32"]) == len(_hip.SIGNATURES["cpn_attend_hidden_bwd"]) - 1
    assert _hip.ABI_VERSION == 12
    with open(_hip.HEADER_PATH) as f:
        head = f.read()
    at = head.index("int cpn_attend_hidden_bwd_f32(")
    assert "CoPoNeRF.py:450-461" in head[at - 1200:at] and "475-485" in head[at - 1200:at]
    at = head.index("int cpn_gemm_f16_combine_hs(")
    assert "CoPoNeRF.py:404-408" in head[at - 1200:at]


def test_render_train_docstring_names_train_precision():
    doc = inspect.getdoc(RenderEngine.render_train)
    assert "train_precision" in doc and "render() only" in doc
