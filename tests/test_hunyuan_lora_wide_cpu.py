"""HunyuanVideo LoRA ranks 22..128, host side: the K-extension layout per rank (vt355.hunyuan.lora_layout), the rank range, and the
adapter names / shapes of a wide-rank model.  No GPU."""
import pytest
import torch


@pytest.mark.parametrize("r,want", [(21, (21, 64, 64, False)), (22, (32, 128, 64, True)), (24, (32, 128, 64, True)),
                                    (64, (64, 192, 64, True)), (128, (128, 384, 128, True))])
def test_layout_table(monkeypatch, r, want):
    """(rp, ext_qkv, ext_proj, wide): 3 r <= 64 keeps the narrow 64-column extension, above it rp = ceil16(r) and the extensions are
    ceil64(3 rp) / ceil64(rp) columns"""
    from vt355.hunyuan import _HYLora, lora_layout
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    assert lora_layout(r) == want
    L = _HYLora(256, 1, 1, r, 1.0)
    assert (L.rp, L.ext_qkv, L.ext_proj, L.wide) == want
    assert L.ext_of("double_blocks.0.img_attn_qkv") == want[1] and L.ext_of("single_blocks.0.linear1") == want[1]
    assert L.ext_of("double_blocks.0.img_attn_proj") == want[2]
    # adapter j's columns [j rp, j rp + r) fit the extension
    assert 2 * L.rp + r <= L.ext_qkv and r <= L.ext_proj


def test_wide_knob_selects_the_wide_layout_at_any_rank(monkeypatch):
    from vt355.hunyuan import lora_layout
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    assert lora_layout(4) == (16, 64, 64, True)
    assert lora_layout(21) == (32, 128, 64, True)
    monkeypatch.setenv("VT355_LORA_WIDE", "0")
    assert lora_layout(4) == (4, 64, 64, False)


@pytest.mark.parametrize("r", [0, 129, -1])
def test_ranks_outside_1_128_are_refused(r):
    from vt355.hunyuan import HunyuanBlocks, _HYLora, lora_layout
    with pytest.raises(ValueError, match="128"):
        lora_layout(r)
    with pytest.raises(ValueError, match="128"):
        _HYLora(256, 1, 1, r, 1.0)
    if r != 0:                      # lora_rank=0 is the constructor's "no adapters"
        with pytest.raises(ValueError, match="128"):
            HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r)


def test_rank_64_constructs_with_the_adapter_shapes():
    """the reference's own HunyuanVideo recipe carries lora_rank 64: the constructor takes it; names and shapes are those of rank 4"""
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=64)
    assert m.lora.wide and (m.lora.rp, m.lora.ext_qkv, m.lora.ext_proj) == (64, 192, 64)
    sd = m.state_dict()
    want = {}
    for mod, tags in (("double_blocks.0.img_attn_qkv", "qkv"), ("double_blocks.0.img_attn_proj", ""), ("single_blocks.0.linear1", "qkv")):
        for dot in ([f".{t}" for t in tags] or [""]):
            want[f"lora.{mod}.lora_A{dot}.weight"] = (64, 256)
            want[f"lora.{mod}.lora_B{dot}.weight"] = (256, 64)
    got = {k: tuple(v.shape) for k, v in sd.items() if "lora_" in k}
    assert got == want
    m4 = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=4)
    assert sorted(k for k in m4.state_dict() if "lora_" in k) == sorted(want)
    assert not m4.lora.wide


def test_whole_model_and_flow_take_rank_128():
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=128, lora_alpha=2.0, fp8="mfma", fp8_dgrad=True)
    assert (m.lora.rp, m.lora.ext_qkv, m.lora.ext_proj) == (128, 384, 128)
    assert tuple(m.state_dict()["lora.single_blocks.0.linear1.lora_B.v.weight"].shape) == (256, 128)
    assert HunyuanVideoFlow(model=m, learning_rate=1e-3).model is m
