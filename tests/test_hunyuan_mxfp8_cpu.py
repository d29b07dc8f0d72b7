"""CPU: the fp8="mfma" mode's host contract -- the modes HunyuanBlocks accepts, the widths the MX-fp8 GEMM needs, the activation sites."""
import pytest


def test_mfma_mode_construction():
    from vt355.hunyuan import HunyuanBlocks, HYVideoDiffusionTransformer
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=3, mm_single_blocks_depth=5, fp8="mfma", fp8_amax_history=8)
    assert m.fp8 == "mfma" and m.n_fp8_sites == 8 * 3 + 2 * 5 and m.fp8_amax_history == 8
    with pytest.raises(ValueError, match="multiple of 128"):                     # MLP width 1088: fc2 / linear2 inputs not 128-aligned
        HunyuanBlocks(hidden_size=256, heads_num=2, mlp_width_ratio=4.25, mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="mfma")
    with pytest.raises(ValueError, match="multiple of 128"):
        m2 = HunyuanBlocks(hidden_size=256, heads_num=2, mlp_width_ratio=4.25, mm_double_blocks_depth=1, mm_single_blocks_depth=1)
        m2.fp8 = "mfma"
    with pytest.raises(ValueError):
        HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="int8")
    w = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=2,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=4, fp8="mfma", fp8_amax_history=4)
    assert w.n_fp8_sites == 12 and w.fp8_amax_history == 4


def test_mfma_state_resets_on_load_and_mode_change():
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="mfma")
    st = m.fp8_state()
    assert st.amax.shape == (10,) and st.history.shape == (10, 16) and not st.seeded
    st.seeded = True
    m.load_state_dict(m.state_dict())
    assert not m.fp8_state().seeded
    m.fp8_state().seeded = True
    m.fp8 = "mfma"
    assert not m.fp8_state().seeded
