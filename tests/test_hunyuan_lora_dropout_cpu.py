"""HunyuanVideo lora_dropout without a device: the arguments and refusals, the layout switch, adapter site numbering, the new entry
points' declarations, and the reference pair (tests/hunyuan_lora_dropout_ref.py) -- the fp64 shim reference equals lora_effective's at
p = 0, and at p = 0.3 the bars of the device tests pass the bf16 restatement with the right masks and fail each wrong variant."""
import functools
import os
import re
import sys

import pytest
import torch

from hunyuan_lora_dropout_ref import VARIANTS, adapter_sites, keep_mask, local_row_index, reference_step, verdict
from hunyuan_lora_ff_ref import ALL, ATTN, FF, blocks_loss, init_adapters, lora_effective
from parity import rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import hunyuan_oracle as HO              # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
BF = torch.bfloat16
D, H, M4 = 256, 2, 1024
B, LI, LT, VALID = 2, 160, 32, (32, 19)
KW = dict(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_alpha=2.0)
P_DROP, SEED, SCALING = 0.3, 1234, 2.0 / 24


def _blocks(**kw):
    from vt355.hunyuan import HunyuanBlocks
    return HunyuanBlocks(**{**KW, **kw})


# ---------------------------------------------------------------------------------------------------------------- the interface
def test_arguments_and_refusals():
    from vt355.hunyuan import HYVideoDiffusionTransformer
    m = _blocks(lora_rank=4)
    assert m.lora_dropout == 0.0 and m.lora.p == 0.0 and m.lora_dropout_seed is None and m.last_lora_dropout_seed is None
    m = _blocks(lora_rank=4, lora_dropout=0.3)
    assert m.lora_dropout == pytest.approx(0.3) and m.lora.p == pytest.approx(0.3) and m.lora_dropout_seed is None
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lora_dropout"):
            _blocks(lora_rank=4, lora_dropout=bad)
    with pytest.raises(ValueError, match="lora_rank"):
        _blocks(lora_rank=0, lora_dropout=0.1)
    _blocks(lora_rank=0, lora_dropout=0.0)
    # fp8_dgrad together with dropout: refused at construction, with the reason; either alone is fine
    with pytest.raises(NotImplementedError, match=r"d\(u\)") as ei:
        _blocks(lora_rank=4, lora_dropout=0.1, fp8="mfma", fp8_dgrad=True)
    assert "masked adapter term" in str(ei.value)
    _blocks(lora_rank=4, lora_dropout=0.1, fp8="mfma")
    m = _blocks(lora_rank=4, lora_dropout=0.1, fp8="mfma")
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        m.fp8_dgrad = "e4m3"
    _blocks(lora_rank=4, fp8="mfma", fp8_dgrad=True)
    # the whole model takes the argument under the same rules
    kw = dict(in_channels=4, hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, text_states_dim=64,
              text_states_dim_2=32)
    w = HYVideoDiffusionTransformer(lora_rank=4, lora_dropout=0.25, **kw)
    assert w.lora_dropout == 0.25 and w.lora.p == 0.25 and w.lora.wide and w.lora_dropout_seed is None
    with pytest.raises(ValueError, match="lora_dropout"):
        HYVideoDiffusionTransformer(lora_rank=4, lora_dropout=1.0, **kw)
    with pytest.raises(ValueError, match="lora_rank"):
        HYVideoDiffusionTransformer(lora_dropout=0.5, **kw)


def test_flow_passes_lora_dropout_through_the_denoiser_config():
    from vt355.hunyuan import HunyuanVideoFlow
    cfg = {"target": "vt355.hunyuan.HYVideoDiffusionTransformer",
           "params": dict(in_channels=4, hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, text_states_dim=64,
                          text_states_dim_2=32, lora_rank=8, lora_dropout=0.1)}
    flow = HunyuanVideoFlow(denoiser_config=cfg)
    assert flow.model.lora_dropout == pytest.approx(0.1) and flow.model.lora.wide


def test_layout_is_wide_at_every_rank_under_dropout(monkeypatch):
    from vt355.hunyuan import lora_layout
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    assert lora_layout(4) == (4, 64, 64, False)                        # existing callers keep their meaning
    assert lora_layout(4, wide=True) == (16, 64, 64, True)
    assert lora_layout(24) == lora_layout(24, wide=True)
    assert not _blocks(lora_rank=4).lora.wide and not _blocks(lora_rank=4, lora_dropout=0.0).lora.wide
    m = _blocks(lora_rank=4, lora_dropout=0.3, lora_target_modules=list(ALL))
    assert m.lora.wide and (m.lora.rp, m.lora.ext_qkv, m.lora.ext_proj, m.lora.ext_ff) == (16, 64, 64, 64)
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    assert lora_layout(4) == (16, 64, 64, True)


def test_dropout_changes_no_parameter():
    """dropout has no parameters: names, shapes and the flat order are those of the undropped model (no checkpoint change)"""
    a, b = _blocks(lora_rank=24, lora_target_modules=list(ALL)), _blocks(lora_rank=24, lora_target_modules=list(ALL), lora_dropout=0.3)
    assert list(a.lora.shapes.items()) == list(b.lora.shapes.items()) and a.lora.offsets == b.lora.offsets
    assert list(a.state_dict()) == list(b.state_dict())


def test_site_numbering():
    """site s = the adapter's position among the lora_A entries of model.lora.shapes; q, k, v of a module are consecutive"""
    m = _blocks(lora_rank=4, lora_dropout=0.3, lora_target_modules=list(ALL), mm_double_blocks_depth=2, mm_single_blocks_depth=2)
    names = [n for n in m.lora.shapes if ".lora_A" in n]
    assert len(names) == 22 and m.lora.site_of == {n: i for i, n in enumerate(names)}
    so = m.lora.site_of
    for mod in ("double_blocks.0.img_attn_qkv", "double_blocks.1.img_attn_qkv", "single_blocks.0.linear1", "single_blocks.1.linear1"):
        q = so[f"{mod}.lora_A.q.weight"]
        assert (so[f"{mod}.lora_A.k.weight"], so[f"{mod}.lora_A.v.weight"]) == (q + 1, q + 2)
    assert so["double_blocks.0.img_attn_qkv.lora_A.q.weight"] == 0 and so["double_blocks.0.img_attn_proj.lora_A.weight"] == 3
    assert so["single_blocks.0.linear1.lora_A.q.weight"] == 8 and so["double_blocks.0.img_mlp.fc1.lora_A.weight"] == 14
    assert so["single_blocks.1.linear2.lora_A.weight"] == 21
    # the reference numbers them the same way
    ref = adapter_sites(ALL, D, M4, 2, 2)
    assert [(s, f"{mod}.lora_A{'.' + t if t else ''}.weight") for s, mod, t, *_ in ref] == list(enumerate(names))
    one = _blocks(lora_rank=4, lora_dropout=0.3, lora_target_modules=["proj_out"])
    assert one.lora.site_of == {"single_blocks.0.linear2.lora_A.weight": 0}
    ff = _blocks(lora_rank=4, lora_dropout=0.3, lora_target_modules=list(FF))
    assert list(ff.lora.site_of.values()) == [0, 1, 2, 3]
    assert list(ff.lora.site_of)[2] == "single_blocks.0.linear1.lora_A.mlp.weight"


AT = ("vt_lora_down_wide_drop_at", "vt_lora_tn_wide_drop_at", "vt_lora_up_add_wide_drop_at", "vt_lora_up_add_wide_dgelu_drop_at")


def test_entry_points_are_declared():
    """the four _at entry points: in the header, in the ctypes table (sibling's arguments + five row and two column integers) and as ops"""
    import ctypes as C
    from vt355 import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "vt355.h")).read()
    for name in AT:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        sib = _lib.PROTOTYPES[name[:-3]]
        assert _lib.PROTOTYPES[name] == sib[:-1] + [C.c_longlong] * 5 + [C.c_int] * 2 + [sib[-1]], name
        assert callable(getattr(ops, name[3:]))
    assert "mask convention" in hdr.lower() and "unsharded" in hdr


def test_local_row_index_is_the_rank_local_row():
    idx = local_row_index(2, 8, 3, True, 2)                             # per sample: 4 + 4 image rows, 3 text rows; local segment 4 + 3
    assert idx.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6] + [7, 8, 9, 10, 7, 8, 9, 10, 11, 12, 13]
    assert local_row_index(2, 8, 3, False, 2).tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 4, 5, 6, 7]
    assert local_row_index(2, 8, 3, True, 1).tolist() == list(range(22))


# ---------------------------------------------------------------------------------------------------------------- the reference pair
@functools.lru_cache(maxsize=None)
def _setup(r=24):
    gen = torch.Generator().manual_seed(31)
    img, txt, vec = torch.randn(B, LI, D, generator=gen).to(BF), torch.randn(B, LT, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    ang = torch.rand(LI, 64, generator=gen) * 6.28
    cos, sin = torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()
    tv = torch.tensor(VALID)
    dout = torch.randn(B, LI + LT, D, generator=gen).to(BF)
    for i in range(B):
        dout[i, LI + int(tv[i]):] = 0
    base = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
    base = {k: v.to(BF).double() for k, v in base.items()}
    ad = {k: v.to(BF).double() for k, v in init_adapters(ALL, D, M4, r).items()}
    return (img, txt, vec, tv, cos, sin, dout), base, ad


@functools.lru_cache(maxsize=None)
def _step(variant, dtype, p=P_DROP):
    inputs, base, ad = _setup()
    return reference_step(HO, base, ad, ALL, SCALING, D, M4, H, inputs, p, SEED, variant, dtype)


def test_keep_mask_is_philox_at_the_site_offset():
    import philox
    m = keep_mask(8, 16, 0.3, SEED, 5)
    assert torch.equal(m, torch.from_numpy(philox.dropout_keep_mask(8, 16, float(torch.tensor(0.3).item()), SEED, 5 << 36).astype("float64")))
    assert not torch.equal(m, keep_mask(8, 16, 0.3, SEED, 6)) and not torch.equal(m, keep_mask(8, 16, 0.3, SEED + 1, 5))
    big = keep_mask(512, 256, 0.3, SEED, 0)
    assert abs(big.mean().item() - 0.7) < 0.01


def test_shim_reference_at_p0_is_lora_effectives():
    """p = 0: the shim's W x + s B (A x) against the effective weights (W + s B A) x of hunyuan_lora_ff_ref, both fp64"""
    inputs, base, ad = _setup()
    got = _step("right", torch.float64, 0.0)
    assert got["hits"] == 11
    img, txt, vec, tv, cos, sin, dout = inputs
    a = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
    ri, rt, rv = [t.double().requires_grad_(True) for t in (img, txt, vec)]
    xo, loss = blocks_loss(HO, lora_effective(base, a, ALL, SCALING, D, M4), ri, rt, rv, tv, cos.double(), sin.double(), dout, H)
    loss.backward()
    assert rel_l2(got["out"], xo) < 1e-12 and rel_l2(got["dimg"], ri.grad) < 1e-12 and rel_l2(got["dtxt"], rt.grad) < 1e-12
    for n in ad:
        assert rel_l2(got["grads"][n], a[n].grad) < 1e-11, n


def _verdict(dev_like, ref, noisy):
    return verdict(dev_like, ref, noisy, VALID, LI)


def test_bars_pass_the_right_masks_and_fail_every_wrong_variant():
    """p = 0.3.  The stand-in for a correct device is the bf16 restatement with the right masks, which also gives the floor (so the
    floor-derived bars hold by construction; the fixed ones -- forward 1e-2, input gradients 3e-2, cosine 0.98 -- are met on their own
    merits).  Each wrong variant's fp64 run is then the 'reference' that the same result must fail."""
    right64, right16 = _step("right", torch.float64), _step("right", BF)
    ok, fig = _verdict(right16, right64, right16)
    print(f"[hunyuan lora dropout ref] right masks: {fig}")
    assert ok, fig
    for v in VARIANTS[1:]:
        wrong = _step(v, torch.float64)
        ok, fig = _verdict(right16, wrong, right16)
        print(f"[hunyuan lora dropout ref] {v}: fwd {fig['fwd']:.3e} overall {fig['overall']:.3e} worst {fig['worst']:.3e} bad {len(fig['bad'])}")
        assert not ok and fig["bad"], (v, fig)
    # the two effects the choice p = 0.3 rests on: a missing 1 / (1 - p) is a 0.3 relative error in dB, a wrong mask a cosine ~0.7 in dA
    ns = _step("no_scale", torch.float64)
    nb = "double_blocks.0.img_attn_proj.lora_B.weight"
    assert 0.25 < rel_l2(ns["grads"][nb], right64["grads"][nb]) < 0.35
    nx = _step("next_site", torch.float64)
    na = "double_blocks.0.img_attn_proj.lora_A.weight"
    a, b = nx["grads"][na].flatten(), right64["grads"][na].flatten()
    assert 0.55 < (a @ b / (a.norm() * b.norm())).item() < 0.85
