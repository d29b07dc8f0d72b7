"""CPU checks of the VideoCrafter1 layout (use_relative_position=True): parameter layout against the reference module's list, the
restatements of tests/relpos_ref.py against the reference's own modules (tests/golden/vc1_*.npz, tests/golden/make_golden_vc1.py), the
recipe yaml, the C-ABI table, and that the GPU test's inputs tell every likely-wrong kernel apart."""
import os
import re

import numpy as np
import pytest
import torch

import golden_io
import relpos_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vt_attn_relpos_fwd", "vt_attn_relpos_bwd", "vt_attn_relpos_workspace_bytes")


def _unet(cfg, rel=True, **kw):
    from vt355.unet import UNetModel
    args = dict(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
                num_head_channels=64, transformer_depth=1, context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True,
                temporal_conv=cfg.temporal_conv, temporal_attention=True, temporal_selfatt_only=True, use_relative_position=rel,
                use_causal_attention=False, temporal_length=cfg.temporal_length, addition_attention=True, fps_cond=True)
    args.update(kw)
    return UNetModel(**args)


def test_relative_position_unet_has_the_reference_parameter_list():
    """UNetModel(use_relative_position=True) constructs; named_parameters() equals the reference module's list stored in the fixture (two
    tables per temporal CrossAttention, right after its to_out.0.bias), so a VideoCrafter1 / LVDM state dict loads with strict=True"""
    cfg = RR.vc1_tiny_config()
    m = _unet(cfg)
    names = [str(n) for n in golden_io.load("vc1_unet_tiny")["names"]]
    assert [n for n, _ in m.named_parameters()] == names
    assert m.config.use_relative_position
    tables = [n for n in names if n.endswith(".embeddings_table")]
    assert len(tables) == 32 and tables == RR.vc1_table_names(cfg)
    for n in tables:
        assert m.shapes[n] == (2 * cfg.temporal_length + 1, 64), n
        assert names[names.index(n) - (1 if "position_k" in n else 2)].endswith(".to_out.0.bias")
    P = RR.vc1_init_params(cfg, seed=17, dtype=torch.bfloat16)
    m.load_state_dict(P, strict=True)
    k = "middle_block.2.transformer_blocks.0.attn2.relative_position_v.embeddings_table"
    assert torch.equal(dict(m.named_parameters())[k], P[k])
    # init_weights draws the tables at xavier_uniform_'s scale (bound 0.29 for [9, 64]: standard deviation 0.166), nothing left at zero
    t0 = dict(_unet(cfg).init_weights(3).named_parameters())[k].detach().float()
    assert 0.12 < t0.std().item() < 0.21 and float(t0.abs().min()) > 0
    # to_q | to_k | to_v stay adjacent in the flat buffer (one fused projection)
    pre = "input_blocks.1.2.transformer_blocks.0.attn1"
    assert m.span(m.flat_bf16, pre + ".to_q.weight", pre + ".to_v.weight").shape == (3 * 64, 64)
    for bad in (dict(use_causal_attention=True), dict(tempspatial_aware=True)):
        with pytest.raises(NotImplementedError):
            _unet(cfg, **bad)
    # openaimodel3d_dc-style nets share the temporal path: the combination is not refused
    assert _unet(cfg, img_cross_attention=True, fps_cond=False, fs_condition=True, in_channels=8).config.use_relative_position


def test_option_off_leaves_the_flat_layout_unchanged():
    """with use_relative_position=False the shape dict, and therefore every flat offset, is what it was before the option existed: numel
    and offsets of the tiny VideoCrafter2 configuration, pinned as literals taken from the parent commit"""
    import unet_oracle as U
    cfg = U.tiny_config()
    m = _unet(cfg, rel=False)
    assert list(m.shapes) == list(U.param_shapes(cfg)) and not any("relative_position" in n for n in m.shapes)
    assert m.numel == 12460552 and len(m.shapes) == 626
    assert m.offsets["time_embed.0.weight"] == 0
    assert m.offsets["input_blocks.1.2.transformer_blocks.0.attn1.to_out.0.bias"] == 419840
    assert m.offsets["input_blocks.1.2.transformer_blocks.0.ff.net.0.proj.weight"] == 419904
    assert m.offsets["init_attn.0.norm.weight"] == 1698624
    assert m.offsets["middle_block.2.transformer_blocks.0.attn2.to_q.weight"] == 8170112
    assert m.offsets["out.2.bias"] == 12460544
    assert not m.config.use_relative_position


def test_relpos_entry_points_are_declared_and_exported():
    import vt355
    from vt355._lib import PROTOTYPES
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    declared = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", header))
    lib = vt355.load_library()
    for name in ENTRY_POINTS:
        assert name in declared and name in PROTOTYPES and hasattr(lib, name), name
    ws = lib.vt_attn_relpos_workspace_bytes()
    assert 0 < ws <= 4 << 20 and ws % 16 == 0              # a constant: it does not grow with the number of rows
    # a refused call needs no device: T = 3 does not divide the 32-row tile
    assert lib.vt_attn_relpos_fwd(None, None, None, None, None, None, None, 96, 1, 3, 16, 64, 64, 64, 64, 0.125, None) == -1


@pytest.mark.parametrize("T,P", [(16, 16), (8, 4)])
def test_relpos_restatement_equals_the_reference_attention_module(T, P):
    """relpos_ref.relpos_attention (variant "exact", hand-written backward) around the module's four Linears vs the reference's
    CrossAttention(relative_position=True) run as self-attention: output, input gradient and both table gradients (float64 against the
    reference's fp32 module: 1e-5 of the tensor's largest element)"""
    g = golden_io.load("vc1_attn")
    tag = f"T{T}P{P}."
    A = lambda k: torch.from_numpy(g[tag + k]).double()
    x, gy = A("x"), A("gy")
    n = x.shape[0]
    W = {k: A("w." + k) for k in ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias")}
    ek, ev = A("w.relative_position_k.embeddings_table"), A("w.relative_position_v.embeddings_table")
    assert ek.shape == (2 * P + 1, 64)
    x2 = x.reshape(n * T, 128)
    q, k, v = x2 @ W["to_q.weight"].t(), x2 @ W["to_k.weight"].t(), x2 @ W["to_v.weight"].t()
    do = gy.reshape(n * T, 128) @ W["to_out.0.weight"]
    r = RR.relpos_attention(q, k, v, ek, ev, do, T, 2, 0.125)
    y = r["o"] @ W["to_out.0.weight"].t() + W["to_out.0.bias"]
    gx = r["dq"] @ W["to_q.weight"] + r["dk"] @ W["to_k.weight"] + r["dv"] @ W["to_v.weight"]
    for got, ref, what in ((y, A("y").reshape(n * T, 128), "output"), (gx, A("gx").reshape(n * T, 128), "input gradient"),
                           (r["d_rel_k"], A("g.relative_position_k.embeddings_table"), "k table gradient"),
                           (r["d_rel_v"], A("g.relative_position_v.embeddings_table"), "v table gradient")):
        assert (got - ref).abs().max().item() < 1e-5 * ref.abs().max().item(), what
    if T <= P:
        assert r["d_rel_k"][[0, 2 * P]].abs().max().item() == 0.0 and r["d_rel_v"][[0, 2 * P]].abs().max().item() == 0.0


def test_relpos_restatement_backward_is_the_derivative():
    """the hand-written backward against autograd of the written-out formula, with the clamp live (T = 8 > P = 3)"""
    T, P, H, R = 8, 3, 2, 32
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(R, H * 64, generator=g, dtype=torch.float64) for _ in range(4))
    ek, ev = (torch.randn(2 * P + 1, 64, generator=g, dtype=torch.float64) * 0.25 for _ in range(2))
    leaves = [t.requires_grad_(True) for t in (q, k, v, ek, ev)]
    sp = lambda t: t.view(R // T, T, H, 64).permute(0, 2, 1, 3)
    idx, _ = RR.rel_index(T, P)
    s = (torch.einsum("nhid,nhjd->nhij", sp(q), sp(k)) + torch.einsum("nhid,ijd->nhij", sp(q), ek[idx])) * 0.125
    p = s.softmax(-1)
    o = (torch.einsum("nhij,nhjd->nhid", p, sp(v)) + torch.einsum("nhij,ijd->nhid", p, ev[idx])).permute(0, 2, 1, 3).reshape(R, H * 64)
    (o * do).sum().backward()
    r = RR.relpos_attention(q.detach(), k.detach(), v.detach(), ek.detach(), ev.detach(), do, T, H, 0.125)
    assert torch.allclose(r["o"], o.detach(), rtol=1e-10, atol=1e-12)
    for name, leaf in zip(("dq", "dk", "dv", "d_rel_k", "d_rel_v"), leaves):
        assert torch.allclose(r[name], leaf.grad, rtol=1e-9, atol=1e-12), name


def test_vc1_unet_restatement_matches_reference_unet():
    """relpos_ref.vc1_unet_forward (unet_oracle with the relative-position CrossAttention) vs the reference's UNetModel(use_relative_position=
    True, temporal_conv=False): output, loss, checksums of ALL parameter gradients and the kept gradients in full, four tables among them"""
    cfg = RR.vc1_tiny_config()
    P = RR.vc1_init_params(cfg, seed=17, dtype=torch.float64)
    g = golden_io.load("vc1_unet_tiny")
    assert list(P) == [str(n) for n in g["names"]]
    for v in P.values():
        v.requires_grad_(True)
    A = lambda k: torch.from_numpy(g[k])
    out = RR.vc1_unet_forward(P, cfg, A("x").double(), A("t"), A("context").double(), fps=A("fps"))
    ref = A("out").double()
    assert (out - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    loss = ((out - A("noise").double()) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * float(g["loss"])
    loss.backward()
    names = list(P)
    gs = np.array([P[n].grad.sum().item() for n in names]); ga = np.array([P[n].grad.abs().sum().item() for n in names])
    assert np.allclose(ga, g["grad_abs_sum"], rtol=2e-4, atol=1e-7), np.abs(ga - g["grad_abs_sum"]).max()
    assert np.allclose(gs, g["grad_sum"], rtol=0, atol=2e-4 * np.abs(g["grad_abs_sum"]).max())
    full = [k[5:] for k in g.files if k.startswith("grad.")]
    tables = [n for n in full if n.endswith(".embeddings_table")]
    assert len(full) == 15 and len(tables) == 4 and len({n.split(".transformer_blocks.")[0] for n in tables}) == 4
    assert any("attn1.relative_position_k" in n for n in tables) and any("attn2.relative_position_v" in n for n in tables)
    for n in full:
        r = torch.from_numpy(g["grad." + n]).double()
        assert r.abs().max().item() > 0 and (P[n].grad - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-9, n


def _reference_yaml():
    """the recipe as the reference ships it, as test_dc_cpu._reference_yaml reads its own: the settings-only copy under tests/golden/,
    checked byte for byte against the reference tree where that is present (the fixture generators' REF)"""
    import sys
    sys.path.insert(0, golden_io.GOLDEN)
    import make_golden as MG
    ref = os.path.join(MG.REF, "configs", "000_videocrafter", "vc1_t2v_1024.yaml")
    local = os.path.join(golden_io.GOLDEN, "vc1_t2v_1024.yaml")
    if os.path.exists(ref):
        assert open(ref, "rb").read() == open(local, "rb").read(), "tests/golden/vc1_t2v_1024.yaml is no longer the reference's file"
    return local


def test_vc1_recipe_yaml_loads_unchanged():
    """configs/000_videocrafter/vc1_t2v_1024.yaml, whole (its top-level linear_start / linear_end / timesteps included): LVDMFlow + UNetModel
    with relative-position tables [33, 64], no temporal convolutions, the 1000-entry scale table of fix_scale_bug"""
    from vt355.config import instantiate_from_config, load_yaml
    from vt355.lvdm import LVDMFlow
    from vt355.unet import UNetModel
    cfg = load_yaml(_reference_yaml())
    assert cfg["model"]["target"] == "videotuna.models.lvdm.ddpm3d.LVDMFlow"
    assert cfg["model"]["params"]["unet_config"]["params"]["use_relative_position"] is True
    with torch.device("meta"):
        flow = instantiate_from_config(cfg["model"])
    assert type(flow) is LVDMFlow and isinstance(flow.model, UNetModel)
    m = flow.model
    assert m.config.use_relative_position and not m.config.temporal_conv and m.config.fps_cond and m.config.temporal_length == 16
    tables = [n for n in m.shapes if n.endswith(".embeddings_table")]
    assert len(tables) == 4 * 17 and all(m.shapes[n] == (33, 64) for n in tables)          # 16 temporal transformers + init_attn
    assert not any("temopral_conv" in n for n in m.shapes)
    assert flow.use_scale and flow.scale_arr.shape == (1000,) and flow.parameterization == "eps" and flow.num_timesteps == 1000


def test_add_lora_freezes_the_tables():
    """the tables are base weights: add_lora() freezes them with the rest, and the adapters are those of the same net without tables"""
    cfg = RR.vc1_tiny_config()
    m, plain = _unet(cfg).add_lora(4, 1.0), _unet(cfg, rel=False).add_lora(4, 1.0)
    P = dict(m.named_parameters())
    tables = [n for n in P if n.endswith(".embeddings_table")]
    assert len(tables) == 32 and not any(P[n].requires_grad for n in tables)
    assert sorted(n for n in P if "lora" in n) == sorted(n for n, _ in plain.named_parameters() if "lora" in n)
    assert all(p.requires_grad == ("lora" in n) for n, p in P.items())
    assert list(m.lora.shapes) == list(plain.lora.shapes)


DISCRIMINATION_CASES = [(256, 16, 2, 16), (160, 32, 2, 16), (264, 8, 1, 4), (72, 4, 8, 16), (130, 2, 1, 1)]


@pytest.mark.parametrize("case", DISCRIMINATION_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gpu_inputs_tell_the_wrong_variants_apart(case):
    """a condition on the GPU test's INPUTS (tests/test_vc1_gpu.py uses relpos_ref.case_inputs): in float64, every wrong variant puts at
    least 10 % of o outside the output bar (rtol 2e-2, atol 1e-2) and at least 10 % of at least one table gradient outside its bar
    (rtol 3e-2, atol 2e-2 max|ref|).  Measured: 49-97 % of o, 14-99 % of a table gradient; "unclamped" (T > P only) 66 % / 17 % at
    (160, 32, 2, 16) and 49 % / 28 % at (264, 8, 1, 4)"""
    assert case in RR.CASES
    R, T, H, P = case
    ref = RR.case_reference(*case)
    variants = ["transposed", "no_k", "no_v", "unscaled"] + (["unclamped"] if case in ((160, 32, 2, 16), (264, 8, 1, 4)) else [])
    for variant in variants:
        bad = RR.case_reference(*case, variant=variant)
        f_o = RR.outside(bad["o"], ref["o"], 2e-2, 1e-2)
        f_t = max(RR.outside(bad[n], ref[n], 3e-2, 2e-2 * ref[n].abs().max().item()) for n in ("d_rel_k", "d_rel_v"))
        print(f"{case} {variant}: {100 * f_o:.1f}% of o, {100 * f_t:.1f}% of a table gradient outside")
        assert f_o >= 0.10 and f_t >= 0.10, (variant, f_o, f_t)
