"""lora_dropout for the CogVideoX DiT, host side: LoraConfig's range, the YAML path, the new C symbols, and the CPU restatement
(tests/lora_dropout_ref.py) against peft's formula; the three deliberately wrong restatements must be far from the right one."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import lora_dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["to_k", "to_q", "to_v", "to_out.0"]
NEW_SYMBOLS = ("vt_lora_down_drop", "vt_skinny_tn_drop", "vt_lora_up_add_drop", "vt_lora_down_wide_drop_fits", "vt_lora_down_wide_drop",
               "vt_lora_tn_wide_drop", "vt_lora_up_add_wide_drop")


def test_lora_config_accepts_dropout():
    from vt355.lora import LoraConfig
    cfg = LoraConfig(r=4, lora_alpha=1.0, target_modules=TARGETS, lora_dropout=0.1)
    assert cfg.lora_dropout == 0.1
    assert LoraConfig(r=4).lora_dropout == 0.0


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
def test_lora_config_refuses_dropout_outside_0_1(p):
    from vt355.lora import LoraConfig
    with pytest.raises(ValueError):
        LoraConfig(r=4, lora_dropout=p)


def test_yaml_node_with_lora_dropout_instantiates_and_reaches_the_state():
    """a CogVideoX recipe's adapter_config node with lora_dropout: 0.05 (restated inline) through the target remap, then into LoraState"""
    import cogvideox_oracle as O
    from selfcheck import CFG_KEYS
    from vt355.config import instantiate_from_config
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    node = {"target": "peft.LoraConfig", "params": {"r": 4, "lora_alpha": 1.0, "init_lora_weights": True, "lora_dropout": 0.05,
                                                    "target_modules": TARGETS}}
    cfg = instantiate_from_config(node)
    assert isinstance(cfg, LoraConfig) and cfg.lora_dropout == 0.05
    tiny = O.tiny_config(num_layers=1, num_attention_heads=2)
    model = CogVideoXTransformer3DModel(**{k: getattr(tiny, k) for k in CFG_KEYS})
    peft = get_peft_model(model, cfg)
    assert peft._lora_state.p == 0.05
    assert model.lora_dropout_seed is None and model.last_lora_dropout_seed is None


def test_new_symbols_are_declared_and_in_the_ctypes_table():
    from vt355 import _lib
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    table = open(_lib.__file__).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), f"{name} is not declared in include/vt355.h"
        assert f'"{name}":' in table, f"{name} is not in the ctypes table"
    assert "currently 2" in header          # new symbols only: the ABI version stays


def test_patched_lin_is_pefts_formula_with_autograd():
    """one adapted Linear: the patched _lin against result + lora_B(lora_A(dropout(x))) * scaling written out with the site's mask, values
    and gradients of x, A and B"""
    g = torch.Generator().manual_seed(5)
    Bt, S, d, r, p, scale = 2, 6, 8, 4, 0.25, 0.5
    name = "transformer_blocks.3.attn1.to_v"
    P = {name + ".weight": torch.randn(d, d, generator=g, dtype=torch.float64), name + ".bias": torch.randn(d, generator=g, dtype=torch.float64)}

    def leaves():
        gg = torch.Generator().manual_seed(6)
        return [torch.randn(s, generator=gg, dtype=torch.float64).requires_grad_(True) for s in ((Bt, S, d), (r, d), (d, r))]
    x, A, Bm = leaves()
    lo = {name + ".lora_A.default.weight": A, name + ".lora_B.default.weight": Bm}
    y = R.dropped_lin(p, R.SEED, "right")(x, P, name, lo, scale)
    x2, A2, B2 = leaves()
    keep = R.keep_mask(Bt * S, d, p, R.SEED, 4 * 3 + 2).view(Bt, S, d)
    assert 0 < keep.sum().item() < keep.numel()
    y2 = F.linear(x2, P[name + ".weight"], P[name + ".bias"]) + F.linear(F.linear(x2 * keep / (1 - p), A2), B2) * scale
    tol = dict(rtol=1e-12, atol=1e-12)          # fp64; the two spellings round x / (1 - p) and the scaling at different points
    assert torch.allclose(y, y2, **tol)
    w = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * w).sum().backward(); (y2 * w).sum().backward()
    for a, b in ((x, x2), (A, A2), (Bm, B2)):
        assert torch.allclose(a.grad, b.grad, **tol)
    # the hand-written dA: (1 / (1 - p)) dT^T (keep * x)
    dT = (w @ Bm.detach()) * scale
    dA = dT.reshape(-1, r).T @ (keep * x.detach()).reshape(-1, d) / (1 - p)
    assert torch.allclose(A.grad, dA, **tol)


def test_sites_get_different_masks_at_the_stated_rate():
    M, d, p = 64, 128, 0.1
    m = [R.keep_mask(M, d, p, R.SEED, s) for s in (0, 1, 2, 3, R.SITE0)]
    for i in range(len(m)):
        assert abs(1 - m[i].mean().item() - p) < 0.02
        for j in range(i):
            assert not torch.equal(m[i], m[j])


@pytest.mark.parametrize("r", [4, 20])
def test_wrong_references_are_far_from_the_right_one(r, monkeypatch):
    """The tiny model and settings of the GPU test (selfcheck.build_tiny, B = 2, lora_b_random, p = 0.5, the pinned seed): each wrong
    restatement must be at least 3 x the model-level gradient bar (rel-L2 6e-2) away from the right one on at least one adapter
    gradient, and the overall figure of tiny_train_step_check must reject it too."""
    from selfcheck import build_tiny
    import cogvideox_oracle as O
    cfg, model, peft, st = build_tiny(torch.device("cpu"), lora_r=r)
    x0, text, noise, t = R.tiny_inputs(cfg)
    ab = O.alphas_cumprod_cogvideox()[t].view(-1, 1, 1, 1, 1).float()          # the scheduler's add_noise (a device kernel), restated
    noisy = (ab.sqrt() * x0 + (1 - ab).sqrt() * noise).to(torch.bfloat16).double()
    _, right = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, 0.5, R.SEED)
    for variant in R.VARIANTS[1:]:
        _, wrong = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, 0.5, R.SEED, variant)
        per = {k: ((wrong[k] - right[k]).norm() / right[k].norm()).item() for k in right}
        rel, cos = R.overall(R.flat(wrong), R.flat(right))
        print(f"r={r} {variant}: worst adapter rel-L2 {max(per.values()):.3f}, overall rel-L2 {rel:.3f} cos {cos:.4f}")
        assert max(per.values()) >= 3 * 6e-2, (variant, max(per.values()))
        assert not (rel < 6e-2 and cos > 0.995), (variant, rel, cos)
