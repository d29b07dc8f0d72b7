"""CPU: the host contract of fp8="mfma" with fp8_dgrad -- the values the keyword accepts, that it belongs to fp8="mfma", the gradient sites
and their delayed-scaling state, what resets it, and the new entry points in the C-ABI table."""
import pytest

KW = dict(hidden_size=256, heads_num=2)


def test_dgrad_constructor_contract():
    from vt355.hunyuan import HunyuanBlocks, HYVideoDiffusionTransformer
    m = HunyuanBlocks(mm_double_blocks_depth=3, mm_single_blocks_depth=5, fp8="mfma", **KW)
    assert m.fp8_dgrad is False and m.fp8_grad_format is None                  # default: today's behaviour
    for value, fmt in ((True, "e5m2"), ("e5m2", "e5m2"), ("e4m3", "e4m3")):
        m = HunyuanBlocks(mm_double_blocks_depth=3, mm_single_blocks_depth=5, fp8="mfma", fp8_dgrad=value, fp8_amax_history=8, **KW)
        assert m.fp8_dgrad == value and m.fp8_grad_format == fmt
        assert m.n_fp8_grad_sites == 8 * 3 + 3 * 5 and m.n_fp8_sites == 8 * 3 + 2 * 5
    with pytest.raises(ValueError):
        HunyuanBlocks(mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="mfma", fp8_dgrad="int8", **KW)
    for mode in (False, True, "weights", "matmul"):
        with pytest.raises(ValueError, match="mfma"):
            HunyuanBlocks(mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8=mode, fp8_dgrad=True, **KW)
    m = HunyuanBlocks(mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="weights", **KW)
    with pytest.raises(ValueError, match="mfma"):
        m.fp8_dgrad = "e4m3"                                                     # settable afterwards, under the same rule
    m.fp8 = "mfma"
    m.fp8_dgrad = "e4m3"
    assert m.fp8_grad_format == "e4m3"
    with pytest.raises(ValueError, match="fp8_dgrad"):
        m.fp8 = "weights"                                                        # the dX products cannot outlive fp8="mfma"
    m.fp8_dgrad = False
    m.fp8 = "weights"
    w = HYVideoDiffusionTransformer(in_channels=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2, text_states_dim=64, text_states_dim_2=32,
                                    lora_rank=4, fp8="mfma", fp8_dgrad=True, fp8_amax_history=4, **KW)
    assert w.fp8_grad_format == "e5m2" and w.n_fp8_grad_sites == 8 + 6
    with pytest.raises(ValueError, match="mfma"):
        HYVideoDiffusionTransformer(in_channels=4, mm_double_blocks_depth=1, mm_single_blocks_depth=1, text_states_dim=64, text_states_dim_2=32,
                                    fp8_dgrad=True, **KW)


def test_dgrad_state_shape_and_resets():
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8="mfma", fp8_dgrad=True, fp8_amax_history=5, **KW)
    st = m.fp8_grad_state()
    assert st.amax.shape == (11,) and st.history.shape == (11, 5) and st.scale.shape == (11,) and not st.seeded
    assert m.fp8_grad_state() is st and m.fp8_state() is not st and m.fp8_state().history.shape == (10, 5)

    def seeded_then(action):
        m.fp8_grad_state().seeded = True
        m.fp8_state().seeded = True
        action()
        assert not m.fp8_grad_state().seeded and not m.fp8_state().seeded

    seeded_then(lambda: m.load_state_dict(m.state_dict()))
    seeded_then(lambda: setattr(m, "fp8", "mfma"))
    seeded_then(lambda: setattr(m, "fp8_dgrad", "e4m3"))
    seeded_then(m.fp8_reset)


def test_dgrad_entry_points_declared():
    """the four new entry points are in the ctypes table and in the header; the version stays 2's ABI (new symbols only)"""
    import os
    import re
    from vt355._lib import PROTOTYPES
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "vt355.h")).read()
    for name, nargs in (("vt_gemm_mxfp8_dx", 28), ("vt_cast_fp8_fmt", 15), ("vt_gate_mul_fp8", 17), ("vt_fp8_scale_update_fmax", 7)):
        assert len(PROTOTYPES[name]) == nargs
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl is not None and len(decl.group(1).split(",")) == nargs
    assert len(PROTOTYPES["vt_gemm_mxfp8"]) == 32 and len(PROTOTYPES["vt_cast_fp8_scaled"]) == 14 and len(PROTOTYPES["vt_fp8_scale_update"]) == 6
