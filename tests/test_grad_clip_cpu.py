"""Host side of gradient clipping (Lightning's gradient_clip_val / gradient_clip_algorithm) that needs no GPU: what is read from a
recipe, what the optimizers carry, and what they refuse."""
import os

import pytest
import torch
import yaml

from grad_clip_common import tiny_dc_flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lightning.trainer of the other recipes, restated (the reference tree is absent on the GPU box): none of them clips
COGVIDEOX_2B = """
lightning:
  trainer:
    benchmark: True
    num_nodes: 1
    accumulate_grad_batches: 2
    max_epochs: 2000
    precision: 32
"""
VC2_FLOW_STYLE = """
train:
  lightning:
    trainer:
      benchmark: True
      num_nodes: 1
      accumulate_grad_batches: 2
      max_epochs: 2000
      precision: bf16
"""
STDIT = """
lightning:
  trainer:
    benchmark: True
    num_nodes: 1
    accumulate_grad_batches: 1
    max_epochs: 2000
    precision: bf16
"""


def test_trainer_options_of_the_recipes():
    from vt355.config import load_yaml, trainer_options
    dc = trainer_options(load_yaml(os.path.join(ROOT, "tests", "golden", "dc_i2v_1024.yaml")))
    assert dc == dict(accumulate_grad_batches=2, gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    assert isinstance(dc["gradient_clip_val"], float) and isinstance(dc["accumulate_grad_batches"], int)
    dflt = dict(accumulate_grad_batches=1, gradient_clip_val=None, gradient_clip_algorithm="norm")
    for cfg in ({}, None, {"model": {"target": "x"}}, {"lightning": {"callbacks": {}}}, {"lightning": {"trainer": None}}):
        assert trainer_options(cfg) == dflt, cfg
    for text, acc in ((COGVIDEOX_2B, 2), (VC2_FLOW_STYLE, 2), (STDIT, 1)):
        o = trainer_options(yaml.safe_load(text))
        assert o["gradient_clip_val"] is None and o["gradient_clip_algorithm"] == "norm" and o["accumulate_grad_batches"] == acc
    o = trainer_options({"lightning": {"trainer": {"gradient_clip_val": 1, "gradient_clip_algorithm": "value", "max_steps": 7}}})
    assert o == dict(accumulate_grad_batches=1, gradient_clip_val=1.0, gradient_clip_algorithm="value")          # other keys stay ignored


def test_dc_flow_optimizers_carry_the_clip_settings():
    from vt355.config import load_yaml, trainer_options
    from vt355.lvdm import _JointOptimizer
    from vt355.optim import FusedAdamW
    _, flow = tiny_dc_flow()
    opt = flow.configure_optimizers(gradient_clip_val=0.5)
    assert isinstance(opt, _JointOptimizer) and len(opt.optimizers) == 2
    for o in [opt] + opt.optimizers:
        assert o.gradient_clip_val == 0.5 and o.gradient_clip_algorithm == "norm"
    for o in opt.optimizers:
        g = o.state_dict()["param_groups"][0]
        assert g["gradient_clip_val"] == 0.5 and g["gradient_clip_algorithm"] == "norm" and g["lr"] == 1e-3
    # the documented way to train the recipe as written
    opts = trainer_options(load_yaml(os.path.join(ROOT, "tests", "golden", "dc_i2v_1024.yaml")))
    opt = flow.configure_optimizers(**{k: v for k, v in opts.items() if k.startswith("gradient_clip")})
    assert opt.gradient_clip_val == 0.5 and opt.gradient_clip_algorithm == "norm"
    # without arguments: what it returned before the option existed
    opt = flow.configure_optimizers()
    assert opt.gradient_clip_val is None and opt.grad_norm is None
    assert all(o.gradient_clip_val is None and o._clip_mode() is None for o in opt.optimizers)
    uts, rts = flow.model.train_state, flow.image_proj_model.train_state
    mk = lambda ts, **k: FusedAdamW(ts.params, lr=1e-3, fullft_state=ts, **k)
    with pytest.raises(ValueError, match="same gradient_clip_val"):
        _JointOptimizer([mk(uts, gradient_clip_val=0.5), mk(rts, gradient_clip_val=1.0)])
    with pytest.raises(ValueError, match="same gradient_clip_val"):
        _JointOptimizer([mk(uts, gradient_clip_val=0.5), mk(rts, gradient_clip_val=0.5, gradient_clip_algorithm="value")])
    with pytest.raises(ValueError, match="same gradient_clip_val"):
        _JointOptimizer([mk(uts, gradient_clip_val=0.5), mk(rts)])
    _JointOptimizer([mk(uts, gradient_clip_val=0), mk(rts)])             # 0 and None both mean off
    with pytest.raises(ValueError):
        flow.configure_optimizers(gradient_clip_val=-0.5)
    with pytest.raises(ValueError):
        flow.configure_optimizers(gradient_clip_val=float("nan"))
    with pytest.raises(ValueError):
        flow.configure_optimizers(gradient_clip_val=0.5, gradient_clip_algorithm="l2")
    with pytest.raises(ValueError):
        flow.configure_optimizers(gradient_clip_algorithm="l2")          # checked even while clipping is off, as Lightning does


def test_every_flow_takes_the_clip_options():
    import inspect
    from vt355.hunyuan import HunyuanVideoFlow
    from vt355.lvdm import LatentVisualDiffusionFlow, LVDMFlow
    from vt355.stdit import OpenSoraFlow
    from vt355.workflow import CogVideoXWorkFlow
    for cls in (CogVideoXWorkFlow, LVDMFlow, LatentVisualDiffusionFlow, OpenSoraFlow, HunyuanVideoFlow):
        p = inspect.signature(cls.configure_optimizers).parameters
        assert p["gradient_clip_val"].default is None and p["gradient_clip_algorithm"].default == "norm", cls


def test_fused_adamw_settings_round_trip_and_ops_refuse_cpu_tensors():
    from vt355 import ops
    from vt355.optim import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(8))
    a = FusedAdamW([p], gradient_clip_val=2.0, gradient_clip_algorithm="value")
    b = FusedAdamW([p])
    assert b.gradient_clip_val is None and b.gradient_clip_algorithm == "norm" and b._clip_mode() is None
    b.load_state_dict(a.state_dict())
    assert b.gradient_clip_val == 2.0 and b._clip_mode() == "value" and b.grad_norm is None
    with pytest.raises(ValueError):                                      # no CPU path, no fallback
        ops.grad_sqnorm(torch.zeros(8), torch.zeros(4096))
    with pytest.raises(ValueError):
        ops.clip_finalize(torch.zeros(4096), 1, 1.0, 0.5, torch.zeros(2))
