"""LoRA ranks 17..128 for the CogVideoX DiT, host side: LoraConfig's rank range, peft's keys / shapes at rank 64, the K-extension
layout (LoraState.rp / ext_qkv / ext_o) and the activation accounting that follows it.  No GPU."""
import pytest
import torch

PREFIX = "base_model.model."
TARGETS = ["to_k", "to_q", "to_v", "to_out.0"]


def _tiny(layers=2):
    from vt355.dit import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_layers=layers, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(0)
    m.requires_grad_(False)
    return m


@pytest.mark.parametrize("r", [17, 64, 128])
def test_lora_config_accepts_wide_ranks(r):
    from vt355.lora import LoraConfig
    assert LoraConfig(r=r, lora_alpha=float(r)).r == r


@pytest.mark.parametrize("r", [0, 129])
def test_lora_config_refuses_ranks_outside_1_128(r):
    from vt355.lora import LoraConfig
    with pytest.raises(NotImplementedError, match="128"):
        LoraConfig(r=r)


def test_rank_64_keys_shapes_and_trainable_count():
    from vt355.lora import LoraConfig, get_peft_model
    L, r = 2, 64
    m = _tiny(L)
    d = m.inner_dim
    n_base = sum(p.numel() for p in m.parameters())
    peft = get_peft_model(m, LoraConfig(r=r, lora_alpha=16.0, target_modules=TARGETS))
    sd = peft.state_dict()
    keys = [k for k in sd if "lora" in k]
    assert len(keys) == 2 * 4 * L and all(k.startswith(PREFIX) for k in keys)
    for k in keys:
        assert tuple(sd[k].shape) == ((r, d) if "lora_A.default.weight" in k else (d, r)), k
        assert k.endswith("lora_A.default.weight") or k.endswith("lora_B.default.weight")
    tr, al = peft.get_nb_trainable_parameters()
    assert tr == L * 8 * r * d and al == n_base + tr
    st = peft._lora_state
    assert (st.rp, st.ext_qkv, st.ext_o) == (64, 192, 64)
    assert st.flat.numel() == tr and st.grad.numel() == tr          # one flat master / gradient buffer at any rank


@pytest.mark.parametrize("r", [1, 4, 5, 16, 17, 24, 32, 100, 128])
def test_extension_layout_invariants(r, monkeypatch):
    from vt355.lora import LoraConfig, LoraState
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    st = LoraState(_tiny(1), LoraConfig(r=r, target_modules=TARGETS))
    if r <= 16:
        assert st.ext_qkv == 64 and st.ext_o == 64 and st.rp == r and not st.wide
    else:
        assert st.wide
        assert st.rp >= r and st.rp % 8 == 0
        assert st.ext_qkv % 64 == 0 and st.ext_qkv >= 3 * st.rp
        assert st.ext_o % 64 == 0 and st.ext_o >= st.rp
        # no more than one GEMM K-step of slack
        assert st.ext_qkv < 3 * st.rp + 64 and st.ext_o < st.rp + 64 and st.rp < r + 16


def test_wide_knob_forces_the_wide_layout_at_low_rank(monkeypatch):
    from vt355.lora import LoraConfig, LoraState
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    st = LoraState(_tiny(1), LoraConfig(r=16, target_modules=TARGETS))
    assert st.wide and (st.rp, st.ext_qkv, st.ext_o) == (16, 64, 64)
    st = LoraState(_tiny(1), LoraConfig(r=4, target_modules=TARGETS))
    assert st.wide and (st.rp, st.ext_qkv, st.ext_o) == (16, 64, 64)
    monkeypatch.setenv("VT355_LORA_WIDE", "0")
    assert not LoraState(_tiny(1), LoraConfig(r=4, target_modules=TARGETS)).wide


def test_saved_bytes_follow_the_extension_width():
    from vt355.engine import saved_bytes_per_block
    from vt355.lora import LoraConfig, get_peft_model
    M = 1000
    m16, m64 = _tiny(1), _tiny(1)
    get_peft_model(m16, LoraConfig(r=16, target_modules=TARGETS))
    get_peft_model(m64, LoraConfig(r=64, target_modules=TARGETS))
    st = m64.lora
    assert (m16.lora.ext_qkv, m16.lora.ext_o) == (64, 64)
    assert saved_bytes_per_block(m64, M) - saved_bytes_per_block(m16, M) == 2 * M * (st.ext_qkv + st.ext_o - 128)
    assert st.ext_qkv + st.ext_o - 128 == 128
