"""DoRA adapters (LoraConfig.use_dora) for the CogVideoX DiT, host side: the config surface, the flat layout with the magnitudes behind
every A / B slab, peft's key names, the checkpoint round trip, the declared entry points, and the CPU restatement of tests/dora_ref.py
(against the oracle's block on merged weights diag(c) (W + s B A); its three wrong variants must leave the GPU step's bars at the GPU
step's inputs)."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import cogvideox_oracle as O
import dora_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN = ["to_k", "to_q", "to_v", "to_out.0"]
SIX = ATTN + ["ff.net.0.proj", "ff.net.2"]
NEW_SYMBOLS = ("vt_dora_norm", "vt_dora_scale", "vt_dora_transpose_scale", "vt_dora_db_add", "vt_dora_dm")
# the step cases of tests/test_dora_gpu.py: (rank, targets, rope)
STEP_CASES = [(4, ATTN, False), (4, SIX, False), (16, SIX, False), (20, SIX, False), (40, SIX, False), (128, SIX, False), (4, SIX, True),
              (4, ["ff.net.2"], False)]
# the group of gradients on which a wrong variant must leave the bars: the one it touches
GROUP = {"norm_attached": R.adapter_names, "bias_scaled": R.mag_names, "norm_of_w": R.adapter_names}


def tiny_peft(targets, r=4, layers=2, seed=0, **kw):
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    m = CogVideoXTransformer3DModel(num_layers=layers, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(seed)
    m.requires_grad_(False)
    return get_peft_model(m, LoraConfig(r=r, lora_alpha=1.0, target_modules=list(targets), **kw))


# ------------------------------------------------------------------------------------------------------------------ the config surface
def test_recipe_node_with_use_dora_instantiates():
    from vt355.config import instantiate_from_config
    from vt355.lora import LoraConfig
    node = {"target": "peft.LoraConfig", "params": {"r": 4, "lora_alpha": 1.0, "init_lora_weights": True, "target_modules": ATTN,
                                                    "use_dora": True}}
    cfg = instantiate_from_config(node)
    assert isinstance(cfg, LoraConfig) and cfg.use_dora is True and cfg.use_rslora is False
    assert LoraConfig(r=4).use_dora is False


@pytest.mark.parametrize("r", [4, 16, 20])
def test_use_rslora_scales_by_sqrt_r(r):
    from vt355.lora import LoraConfig, LoraState
    bare = SimpleNamespace(inner_dim=64, config=SimpleNamespace(num_layers=2), device="cpu")
    assert LoraState(bare, LoraConfig(r=r, lora_alpha=3.0, use_rslora=True)).scaling == 3.0 / math.sqrt(r)
    assert LoraState(bare, LoraConfig(r=r, lora_alpha=3.0)).scaling == 3.0 / r


def test_use_dora_with_lora_dropout_is_refused():
    from vt355.lora import LoraConfig
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        LoraConfig(r=4, use_dora=True, lora_dropout=0.1)
    LoraConfig(r=4, use_dora=True, lora_dropout=0.0)
    LoraConfig(r=4, use_dora=False, lora_dropout=0.1)


# ------------------------------------------------------------------------------------------------------------------ layout, keys, init
@pytest.mark.parametrize("targets", [ATTN, SIX, ["to_q", "ff.net.2"]], ids=["attn", "six", "q_ff2"])
@pytest.mark.parametrize("r", [4, 20])
def test_magnitudes_lie_behind_every_adapter_slab(targets, r):
    """numel grows by L (4 d + the targeted feed-forward widths); every A / B view has the offset, shape and init of the state without
    DoRA; the magnitude views tile the tail; Parameters and .grad are views of flat / grad"""
    L, d = 2, 128
    plain, dora = tiny_peft(targets, r=r)._lora_state, tiny_peft(targets, r=r, use_dora=True)._lora_state
    ff1, ff2 = "ff.net.0.proj" in targets, "ff.net.2" in targets
    assert dora.numel == dora.flat.numel() == plain.numel + L * (4 * d + (4 * d if ff1 else 0) + (d if ff2 else 0))
    assert dora.grad.numel() == dora.numel and dora.flat_bf16.numel() == dora.numel
    assert torch.equal(dora.flat[:plain.numel], plain.flat)
    for (layer, kind, j) in plain._index:
        a, b = plain.view(plain.flat, layer, kind, j), dora.view(dora.flat, layer, kind, j)
        assert a.storage_offset() == b.storage_offset() and a.shape == b.shape
    cover = torch.zeros_like(dora.flat)
    for p, (layer, kind, j) in zip(dora.params, dora._index):
        v = dora.view(dora.flat, layer, kind, j)
        assert p.data_ptr() == v.data_ptr() and p.grad.data_ptr() == dora.view(dora.grad, layer, kind, j).data_ptr() and p.dtype == torch.float32
        if kind == "M":
            assert v.storage_offset() >= plain.numel and v.shape == (4 * d if j == 4 else d,)
        v2 = dora.view(cover, layer, kind, j)
        v2.add_(1)
    assert sorted({k for (_, k, _) in dora._index}) == ["A", "B", "M"]
    assert cover[:plain.numel].max().item() <= 1 and cover[plain.numel:].max().item() <= 1
    n_mag = sum(1 for (_, k, _) in dora._index if k == "M")
    assert n_mag == L * len(dora.targets)
    assert torch.equal(dora.mag_qkv(dora.flat, 1), torch.cat([dora.view(dora.flat, 1, "M", j) for j in range(3)]))


def test_state_dict_has_pefts_magnitude_keys():
    r, L, d = 4, 2, 128
    peft = tiny_peft(SIX, r=r, layers=L, use_dora=True)
    sd = peft.state_dict()
    want = {}
    for i in range(L):
        pre = f"base_model.model.transformer_blocks.{i}."
        for path, fin, fout in [("attn1.to_q", d, d), ("attn1.to_k", d, d), ("attn1.to_v", d, d), ("attn1.to_out.0", d, d),
                                ("ff.net.0.proj", d, 4 * d), ("ff.net.2", 4 * d, d)]:
            want[pre + path + ".lora_A.default.weight"] = (r, fin)
            want[pre + path + ".lora_B.default.weight"] = (fout, r)
            want[pre + path + ".lora_magnitude_vector.default.weight"] = (fout,)
    got = {k: tuple(v.shape) for k, v in sd.items() if "lora" in k}
    assert got == want
    assert all("lora" in n for n, p in peft.named_parameters() if p.requires_grad)
    tr, _ = peft.get_nb_trainable_parameters()
    assert tr == peft._lora_state.numel == L * (18 * r * d + 9 * d)
    assert not any("magnitude" in k for k in tiny_peft(SIX).state_dict())


def test_cpu_init_is_the_fp32_row_norm_of_the_base_weight():
    peft = tiny_peft(SIX, use_dora=True)
    st = peft._lora_state
    sd = peft.state_dict()
    for k, v in sd.items():
        if "lora_magnitude_vector" in k:
            w = sd[k.replace("lora_magnitude_vector.default.weight", "base_layer.weight")]
            assert torch.equal(v, torch.linalg.norm(w.float(), dim=1)) and v.min().item() > 0
    assert st.version > 0


def test_lora_only_checkpoint_round_trips_the_magnitudes(tmp_path):
    from vt355 import checkpoint as C
    from vt355.workflow import CogVideoXWorkFlow
    src = tiny_peft(SIX, seed=0, use_dora=True)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if "lora_B" in n or "magnitude" in n:
                p.add_(torch.randn(p.shape) * 0.01)
    wf = SimpleNamespace(model=src, global_step=5)
    wf.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf, ck)
    path = C.save_checkpoint(wf, str(tmp_path / "last.ckpt"), epoch=1)
    sd = C.load_checkpoint_file(path)["state_dict"]
    assert len(sd) == 2 * 18 and all("lora" in k for k in sd) and sum("lora_magnitude_vector" in k for k in sd) == 12
    dst = tiny_peft(SIX, seed=1, use_dora=True)
    assert C.load_lora_from_ckpt(dst, path) == 36
    assert torch.equal(dst._lora_state.flat, src._lora_state.flat)
    with pytest.raises(RuntimeError, match="was not copied"):          # a model without DoRA refuses the file with magnitudes
        C.load_lora_from_ckpt(tiny_peft(SIX), path)


def test_new_symbols_are_declared_and_in_the_ctypes_table():
    from vt355 import _lib, ops
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    table = open(_lib.__file__).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), f"{name} is not declared in include/vt355.h"
        assert f'"{name}":' in table, f"{name} is not in the ctypes table"
        assert hasattr(ops, name[3:]), f"vt355.ops has no wrapper {name[3:]}"


def test_saved_bytes_count_the_kept_branch_outputs():
    from vt355.engine import saved_bytes_per_block
    M, d = 1000, 128
    for targets, extra in ((ATTN, d), (SIX, 2 * d), (["ff.net.2"], d), (["to_q"], 0)):
        a, b = tiny_peft(targets), tiny_peft(targets, use_dora=True)
        assert saved_bytes_per_block(b, M) - saved_bytes_per_block(a, M) == 2 * M * extra


# ------------------------------------------------------------------------------------------------------------------ the restated block
def _tiny_setup(r, targets, rope=False):
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), targets, lora_r=r, use_rotary_positional_embeddings=rope)
    x0, text, noise, t = R.tiny_inputs(cfg)
    ab = O.alphas_cumprod_cogvideox()[t].view(-1, 1, 1, 1, 1).float()          # the scheduler's add_noise (a device kernel), restated
    noisy = (ab.sqrt() * x0 + (1 - ab).sqrt() * noise).to(torch.bfloat16).double()
    return cfg, model, st, x0, text, t, noisy


@pytest.mark.parametrize("rope", [False, True])
def test_restated_block_equals_the_oracle_on_merged_weights(rope):
    """fp64: the helper's block with DoRA on all six Linears against cogvideox_oracle.dit_block on diag(c) (W + s B A) with the bias
    unchanged, to 1e-10; c is far from 1 (the step's perturbed magnitudes)"""
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), use_rotary_positional_embeddings=rope)
    P, Lo = R.oracle_params(model, st)
    assert len(Lo) == 36 and len(R.mag_names(Lo)) == 12
    merged, cs = dict(P), []
    for k in [k for k in Lo if "lora_A" in k]:
        base = k.replace(".lora_A.default.weight", "")
        w = P[base + ".weight"] + st.scaling * Lo[k.replace("lora_A", "lora_B")] @ Lo[k]
        c = Lo[base + ".lora_magnitude_vector.default.weight"] / torch.linalg.norm(w, dim=1)
        merged[base + ".weight"] = c[:, None] * w
        cs.append(c)
    assert (torch.cat(cs) - 1).abs().mean().item() > 0.03
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


def test_restatement_at_pefts_init_is_the_base_model(monkeypatch):
    """B = 0 and untouched magnitudes: c = 1 and the prediction is the base model's (fp64: to rounding)"""
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), b_std=0.0, m_std=0.0)
    x0, text, noise, t = R.tiny_inputs(cfg)
    noisy = noise.to(torch.bfloat16).double()
    _, g, out = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t)
    P, _ = R.oracle_params(model, st)
    base = O.dit_forward(P, cfg, noisy, text.double(), t, None, st.scaling)
    assert (out - base).abs().max().item() < 1e-5          # m is the fp32 norm of the fp64 weights: c = 1 to fp32 rounding
    assert all(v.abs().max().item() == 0 for k, v in g.items() if "lora_A" in k)
    assert all(v.abs().max().item() > 0 for k, v in g.items() if "lora_A" not in k)


@pytest.mark.parametrize("r,targets,rope", STEP_CASES, ids=[f"r{r}_{len(tg)}targets{'_rope' if rp else ''}" for r, tg, rp in STEP_CASES])
def test_wrong_references_are_far_from_the_right_one(r, targets, rope, monkeypatch):
    """At the inputs of every GPU step case (dora_ref.STEP_*: alpha / r = 4, B ~ 0.1 / sqrt(r) randn, m perturbed by 10 %, biases x 10) each
    wrong restatement differs from the right one by more than the step's bars (rel-L2 >= 6e-2 in both directions, or cosine <= 0.995) on
    the group of gradients it touches: the adapters for "norm_attached" and "norm_of_w", the magnitudes for "bias_scaled"."""
    cfg, model, st, x0, text, t, noisy = _tiny_setup(r, targets, rope)
    tabs = R.rope_tables(cfg, rope)
    _, right, _ = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, rope_tabs=tabs)
    assert all(v.abs().max().item() > 0 for v in right.values())
    for variant in R.VARIANTS[1:]:
        _, wrong, _ = R.reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, variant, tabs)
        names = GROUP[variant](right)
        rel, cos = R.overall(R.flat(wrong, names), R.flat(right, names))
        rel2, _ = R.overall(R.flat(right, names), R.flat(wrong, names))
        print(f"r={r} targets={len(targets)} rope={rope} {variant}: rel-L2 {rel:.3f} / {rel2:.3f} cos {cos:.4f}")
        assert (rel >= 6e-2 and rel2 >= 6e-2) or cos <= 0.995, (variant, rel, rel2, cos)
