"""LoRA on the CogVideoX feed-forward pair ff.net.0.proj / ff.net.2, host side: peft's target rule, key names, flat layout and init,
the checkpoint round trip, the unchanged attention dispatch, and the CPU restatement of tests/lora_ff_ref.py (at p = 0 against the
oracle's block on merged weights; at p > 0 the three deliberately wrong restatements must be far from the right one)."""
import inspect
import json
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import cogvideox_oracle as O
import lora_ff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN = ["to_k", "to_q", "to_v", "to_out.0"]
SIX = ATTN + ["ff.net.0.proj", "ff.net.2"]
NEW_SYMBOLS = ("vt_lora_up_add_dgelu_drop", "vt_lora_up_add_wide_dgelu_drop")


def tiny_peft(targets, r=4, layers=2, seed=0):
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    m = CogVideoXTransformer3DModel(num_layers=layers, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(seed)
    m.requires_grad_(False)
    return get_peft_model(m, LoraConfig(r=r, lora_alpha=1.0, target_modules=list(targets)))


def test_six_targets_give_pefts_keys_shapes_and_count():
    """get_peft_model with the six targets: exactly peft's key names and shapes, L (8 r d + 10 r d) trainable parameters, the base weight
    under .base_layer., everything else frozen"""
    r, L, d = 4, 2, 128
    peft = tiny_peft(SIX, r=r, layers=L)
    sd = peft.state_dict()
    want = {}
    for i in range(L):
        pre = f"base_model.model.transformer_blocks.{i}."
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            want[pre + f"attn1.{n}.lora_A.default.weight"] = (r, d)
            want[pre + f"attn1.{n}.lora_B.default.weight"] = (d, r)
        want[pre + "ff.net.0.proj.lora_A.default.weight"] = (r, d)
        want[pre + "ff.net.0.proj.lora_B.default.weight"] = (4 * d, r)
        want[pre + "ff.net.2.lora_A.default.weight"] = (r, 4 * d)
        want[pre + "ff.net.2.lora_B.default.weight"] = (d, r)
        assert tuple(sd[pre + "ff.net.0.proj.base_layer.weight"].shape) == (4 * d, d)
        assert tuple(sd[pre + "ff.net.2.base_layer.weight"].shape) == (d, 4 * d)
        assert pre + "ff.net.2.weight" not in sd and pre + "ff.net.0.proj.weight" not in sd
    got = {k: tuple(v.shape) for k, v in sd.items() if "lora" in k}
    assert got == want
    tr, _ = peft.get_nb_trainable_parameters()
    assert tr == L * (8 * r * d + 10 * r * d)
    assert all(p.requires_grad == ("lora" in n) for n, p in peft.named_parameters())
    st = peft._lora_state
    assert sorted({j for (_, _, j) in st._index}) == [0, 1, 2, 3, 4, 5]
    for p, (layer, kind, j) in zip(st.params, st._index):
        assert p.data_ptr() == st.view(st.flat, layer, kind, j).data_ptr() and p.grad.data_ptr() == st.view(st.grad, layer, kind, j).data_ptr()
    assert st.flat.numel() == tr
    # every flat element belongs to exactly one adapter
    cover = torch.zeros_like(st.flat)
    for (layer, kind, j) in st._index:
        st.view(cover, layer, kind, j).add_(1)
    assert (cover == 1).all()


def test_targets_resolve_by_pefts_suffix_rule():
    from vt355.lora import LoraConfig, LoraState
    st = tiny_peft(["to_q", "net.2"])._lora_state
    assert st.targets == ["to_q", "ff.net.2"] and st.ff2 and not st.ff1
    st = tiny_peft(["net.0.proj", "attn1.to_v"])._lora_state
    assert st.targets == ["to_v", "ff.net.0.proj"] and st.ff1 and not st.ff2
    keys = [k for k in tiny_peft(["net.2"], layers=1).state_dict() if "lora" in k]
    assert keys == ["base_model.model.transformer_blocks.0.ff.net.2.lora_A.default.weight",
                    "base_model.model.transformer_blocks.0.ff.net.2.lora_B.default.weight"]
    # "proj" also matches patch_embed.proj (a convolution); "linear" the adaLN Linears outside the supported set; "net" a container
    for bad in ("proj", "linear", "net", "ff", "norm_q", "to_out", "bogus", "proj_out"):
        with pytest.raises(ValueError, match="unsupported LoRA target"):
            tiny_peft(["to_q", bad])
    # a model that is not an nn.Module (tests/test_lora_dispatch_cpu.py's): same rule on the DiT's module paths, ff_mult defaults to 4
    bare = SimpleNamespace(inner_dim=64, config=SimpleNamespace(num_layers=2), device="cpu")
    assert LoraState(bare, LoraConfig(r=4)).flat.numel() == 2 * 8 * 4 * 64
    st = LoraState(bare, LoraConfig(r=4, target_modules=["to_q", "net.2", "ff.net.0.proj"]))
    assert st.dff == 256 and st.flat.numel() == 2 * 18 * 4 * 64
    with pytest.raises(ValueError, match="unsupported LoRA target"):
        LoraState(bare, LoraConfig(r=4, target_modules=["proj"]))


@pytest.mark.parametrize("r", [4, 20])
def test_init_bounds_follow_in_features_and_attention_init_is_independent_of_the_target_list(r):
    d = 128
    a = tiny_peft(ATTN, r=r)._lora_state
    b = tiny_peft(SIX, r=r)._lora_state
    assert torch.equal(b.flat[:a.flat.numel()], a.flat), "the attention slabs differ with feed-forward targets present"
    for (layer, kind, j) in b._index:
        v = b.view(b.flat, layer, kind, j)
        if kind == "B":
            assert (v == 0).all()
            continue
        fin = 4 * d if j == 5 else d
        bound = 1.0 / math.sqrt(fin)
        assert v.shape == (r, fin) and v.abs().max().item() <= bound
        assert v.abs().max().item() > 0.9 * bound, "kaiming-uniform(a = sqrt 5) reaches close to 1 / sqrt(in_features)"
    only2 = tiny_peft(["ff.net.2"], r=r)._lora_state
    assert only2.flat[:a.flat.numel()].abs().max().item() == 0 and only2.flat.numel() == a.flat.numel() + 2 * 5 * r * d


def test_lora_only_checkpoint_round_trips(tmp_path):
    from vt355 import checkpoint as C
    from vt355.workflow import CogVideoXWorkFlow
    src = tiny_peft(SIX, seed=0)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if "lora_B" in n:
                p.copy_(torch.randn(p.shape) * 0.01)
    wf = SimpleNamespace(model=src, global_step=5)
    wf.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf, ck)
    path = C.save_checkpoint(wf, str(tmp_path / "last.ckpt"), epoch=1)
    sd = C.load_checkpoint_file(path)["state_dict"]
    assert len(sd) == 2 * 12 and all(k.startswith("model.base_model.model.") and "lora" in k for k in sd)
    assert sum(".ff.net." in k for k in sd) == 2 * 4
    dst = tiny_peft(SIX, seed=1)
    v0 = dst._lora_state.version
    assert C.load_lora_from_ckpt(dst, path) == 24
    assert dst._lora_state.version > v0
    assert torch.equal(dst._lora_state.flat, src._lora_state.flat) and dst._lora_state.flat.abs().sum().item() > 0
    with pytest.raises(RuntimeError, match="was not copied"):          # an attention-only model refuses the longer file
        C.load_lora_from_ckpt(tiny_peft(ATTN), path)


def test_recipe_with_the_longer_target_list_loads_through_config():
    from vt355.config import instantiate_from_config
    from vt355.lora import LoraConfig
    node = {"target": "peft.LoraConfig", "params": {"r": 4, "lora_alpha": 1.0, "init_lora_weights": True, "target_modules": SIX}}
    cfg = instantiate_from_config(node)
    assert isinstance(cfg, LoraConfig) and list(cfg.target_modules) == SIX


def test_new_symbols_are_declared_and_in_the_ctypes_table():
    from vt355 import _lib
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    table = open(_lib.__file__).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), f"{name} is not declared in include/vt355.h"
        assert f'"{name}":' in table, f"{name} is not in the ctypes table"
    assert "currently 2" in header


def test_saved_bytes_count_the_kept_feed_forward_inputs():
    from vt355.engine import saved_bytes_per_block
    M, d = 1000, 128
    a, b = tiny_peft(ATTN), tiny_peft(SIX)
    only2 = tiny_peft(["ff.net.2"])
    ext = b._lora_state.ext_ff
    assert ext == 64
    assert saved_bytes_per_block(b, M) - saved_bytes_per_block(a, M) == 2 * M * (d + ext + 4 * d + ext)
    assert saved_bytes_per_block(only2, M) - saved_bytes_per_block(a, M) == 2 * M * (4 * d + ext)


# ------------------------------------------------------------------------------------------------------------------ dispatch
PRODUCTS = ("lora_down", "skinny_tn", "lora_up_add", "lora_down_wide", "lora_tn_wide", "lora_up_add_wide")


@pytest.mark.parametrize("drop", [None, (0.1, 1234567)], ids=["nodrop", "drop"])
@pytest.mark.parametrize("r", [4, 6, 20, 128])
def test_attention_dispatch_is_unchanged_by_feed_forward_targets(monkeypatch, r, drop):
    """the calls engine._lora_down / _lora_da / _lora_dx record for the qkv and out projections, under tests/test_lora_dispatch_cpu.py's
    recorders (function name, scalars, [storage_offset, shape, stride] of tensors), with and without the feed-forward targets"""
    from vt355 import engine, ops
    from vt355.lora import LoraConfig, LoraState
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    D, M, LAYER = 64, 8, 1
    log = []

    def recorder(name, sig):
        def rec(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            log.append([name] + [[v.storage_offset(), list(v.shape), list(v.stride())] if isinstance(v, torch.Tensor) else v
                                 for v in ba.arguments.values()])
        return rec
    for name in [p + s for p in PRODUCTS for s in ("", "_drop")]:
        monkeypatch.setattr(ops, name, recorder(name, inspect.signature(getattr(ops, name))))
    monkeypatch.setattr(ops, "lora_down_wide_drop_fits", lambda n, rp: n * (64 + rp) * 72 * 2 <= 65536 and n * rp <= 384)
    seqs = []
    for targets in (ATTN, SIX):
        model = SimpleNamespace(inner_dim=D, config=SimpleNamespace(num_layers=2), device="cpu")
        st = LoraState(model, LoraConfig(r=r, lora_alpha=float(r), target_modules=targets))
        bf = dict(dtype=torch.bfloat16)
        x1, dx1 = torch.empty(M, D + st.ext_qkv, **bf), torch.empty(M, D + st.ext_qkv, **bf)
        o, dO = torch.empty(M, D + st.ext_o, **bf), torch.empty(M, D + st.ext_o, **bf)
        engine._lora_down(st, LAYER, "qkv", x1, D, drop)
        engine._lora_down(st, LAYER, "out", o, D, drop)
        for proj, x, dxe in (("qkv", x1, dx1), ("out", o, dO)):
            engine._lora_da(st, LAYER, proj, x, dxe, D, drop)
            engine._lora_dx(st, LAYER, proj, dxe, D, drop)
        seqs.append(json.loads(json.dumps(log)))
        log.clear()
    assert len(seqs[0]) >= 6 and seqs[0] == seqs[1]


# ------------------------------------------------------------------------------------------------------------------ the restated block
def _tiny_setup(r=4, p=0.0, scaling=0.25):
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), lora_r=r, p=p, scaling=scaling)
    x0, text, noise, t = R.tiny_inputs(cfg)
    ab = O.alphas_cumprod_cogvideox()[t].view(-1, 1, 1, 1, 1).float()          # the scheduler's add_noise (a device kernel), restated
    noisy = (ab.sqrt() * x0 + (1 - ab).sqrt() * noise).to(torch.bfloat16).double()
    return cfg, model, st, x0, text, t, noisy


@pytest.mark.parametrize("rope", [False, True])
def test_restated_block_equals_the_oracle_on_merged_weights(rope, monkeypatch):
    """fp64, p = 0: the helper's block with adapters on all six Linears against cogvideox_oracle.dit_block on W + s B A, to 1e-10"""
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), use_rotary_positional_embeddings=rope)
    P, Lo = R.oracle_params(model, st)
    assert sum(R.is_ff(k) for k in Lo) == 8 and len(Lo) == 24
    merged = dict(P)
    for k in [k for k in Lo if "lora_A" in k]:
        base = k.replace(".lora_A.default.weight", "")
        merged[base + ".weight"] = P[base + ".weight"] + st.scaling * Lo[k.replace("lora_A", "lora_B")] @ Lo[k]
    g = torch.Generator().manual_seed(3)
    B, St, Sv, d = 2, 10, 24, cfg.inner_dim
    h_txt, h_vid = torch.randn(B, St, d, generator=g, dtype=torch.float64), torch.randn(B, Sv, d, generator=g, dtype=torch.float64)
    emb = torch.randn(B, cfg.time_embed_dim, generator=g, dtype=torch.float64)
    tabs = R.rope_tables(cfg, rope)
    rp = None if tabs is None else (tabs[0].double(), tabs[1].double())
    for i in range(cfg.num_layers):
        pre = f"transformer_blocks.{i}."
        want = O.dit_block(h_txt, h_vid, emb, merged, pre, cfg, None, st.scaling, rope=rp)
        got = R.make_block()(h_txt, h_vid, emb, P, pre, cfg, Lo, st.scaling, rope=rp)
        plain = O.dit_block(h_txt, h_vid, emb, P, pre, cfg, None, st.scaling, rope=rp)
        for a, b, c in zip(got, want, plain):
            assert (a - b).abs().max().item() < 1e-10
            assert (a - c).abs().max().item() > 1e-4, "the adapters do not reach the output"


@pytest.mark.parametrize("r", [4, 20])
def test_wrong_references_are_far_from_the_right_one(r, monkeypatch):
    """The tiny model and inputs of the GPU test (B = 2, random B as build_tiny draws it, p = 0.5, the pinned seed): on the feed-forward
    adapter gradients alone, the right restatement and each wrong one must differ by more than the step bars (rel-L2 >= 6e-2 or cosine
    <= 0.995), in either direction of the comparison.  lora_alpha = 4 r (R.WRONG_SCALING): at build_tiny's alpha / r = 0.25 the ff.net.2
    correction is 1-3 % of du and "dgelu_outside" stays inside the bars (rel-L2 0.014 at r = 4, 0.031 at r = 20), so the inputs, not the
    bar, were changed; the GPU test's p = 0.5 cases use the same scaling."""
    cfg, model, st, x0, text, t, noisy = _tiny_setup(r, 0.5, R.WRONG_SCALING)
    _, right, _ = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, 0.5, R.SEED)
    ff = R.ff_names(right)
    assert len(ff) == 8
    for variant in R.VARIANTS[1:]:
        _, wrong, _ = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, 0.5, R.SEED, variant)
        rel, cos = R.overall(R.flat(wrong, ff), R.flat(right, ff))
        rel2, _ = R.overall(R.flat(right, ff), R.flat(wrong, ff))
        print(f"r={r} {variant}: feed-forward group rel-L2 {rel:.3f} / {rel2:.3f} cos {cos:.4f}")
        assert (rel >= 6e-2 and rel2 >= 6e-2) or cos <= 0.995, (variant, rel, rel2, cos)


def test_dropped_reference_is_pefts_formula_on_the_feed_forward_sites():
    """ff.net.2 of layer 1 of 2: the helper's Linear against result + lora_B(lora_A(dropout(x))) * scaling written out with the mask of
    site 4 L + 2 layer + 1 over the [M, 4 d] input"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    Bt, S, k, n, r, p, scale, L = 2, 6, 32, 8, 4, 0.25, 0.5, 2
    name = "transformer_blocks.1.ff.net.2"
    P = {name + ".weight": torch.randn(n, k, generator=g, dtype=torch.float64), name + ".bias": torch.randn(n, generator=g, dtype=torch.float64)}
    x, A, Bm = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((Bt, S, k), (r, k), (n, r)))
    lo = {name + ".lora_A.default.weight": A, name + ".lora_B.default.weight": Bm}
    y = R.make_lin(p, R.SEED, L)(x, P, name, lo, scale)
    keep = R.keep_mask(Bt * S, k, p, R.SEED, 4 * L + 2 * 1 + 1).view(Bt, S, k)
    assert 0 < keep.sum().item() < keep.numel()
    y2 = F.linear(x, P[name + ".weight"], P[name + ".bias"]) + F.linear(F.linear(x * keep / (1 - p), A), Bm) * scale
    assert torch.allclose(y, y2, rtol=1e-12, atol=1e-12)
    assert R.site_of(name, L) == 11 and R.site_of("transformer_blocks.1.ff.net.0.proj", L) == 10
    assert R.site_of("transformer_blocks.1.attn1.to_out.0", L) == 7 and R.site_of(name, L, "attn_sites") == 5
